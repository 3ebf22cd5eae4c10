// st_scene.cpp — host engine of libstrolle_hip.so: the scene stores of st_stores.h — lights (lights.rs, light.rs), the image atlas (images.rs), materials (materials.rs, material.rs), meshes, instances and the triangle slots they are baked into (instances.rs, mesh_triangle.rs, triangle.rs) — and the tick's phases that connect them to the tree, the copies and the deformer. See st_engine.h.
#include "st_engine.h"

namespace st {

// ---- lights (lights.rs:49-172, light.rs:25-79)
LightStore::LightStore() {
    GpuLight sun{};
    sun.d0 = make_float4(0, 0, 0, 25.0f); sun.d1 = make_float4(0, 0, 0, INFINITY); sun.d2 = make_float4(b2f(1u), 0, 0, 0);
    buffer_.push_back(sun);
    slot_[-1] = 0;
}

void LightStore::overwrite(uint32_t slot, int64_t key, GpuLight g) {
    const GpuLight old = buffer_[slot];
    g.prev_d0 = old.d0; g.prev_d1 = old.d1; g.prev_d2 = old.d2;
    note(updated_, key);
    buffer_[slot] = g;
}

void LightStore::insert(uint64_t id, const StLight& l) {
    GpuLight g{};
    g.d0 = make_float4(l.position[0], l.position[1], l.position[2], l.radius);
    g.d1 = make_float4(l.color[0], l.color[1], l.color[2], l.range);
    if (l.kind == ST_LIGHT_POINT) g.d2 = make_float4(b2f(1u), 0, 0, 0);
    else {
        V3 n = v3(l.direction[0], l.direction[1], l.direction[2]);  // Normal::encode (normal.rs:9-24)
        n = n / (fabsf(n.x) + fabsf(n.y) + fabsf(n.z));
        V2 e = n.z >= 0.0f ? v2(n.x, n.y) : v2(copysignf(1.0f - fabsf(n.y), n.x), copysignf(1.0f - fabsf(n.x), n.y));
        e = e * 0.5f + 0.5f;
        g.d2 = make_float4(b2f(2u), e.x, e.y, l.angle);
    }
    const int64_t key = (int64_t)id;
    auto it = slot_.find(key);
    if (it != slot_.end()) { overwrite(it->second, key, g); return; }
    if (next_id_ < buffer_.size()) { buffer_[next_id_] = g; slot_[key] = next_id_; }
    else { slot_[key] = (uint32_t)buffer_.size(); buffer_.push_back(g); }
    note(created_, key);
    next_id_ += 1;
}

void LightStore::remove(uint64_t id) {
    const int64_t key = (int64_t)id;
    auto it = slot_.find(key);
    if (it == slot_.end()) return;
    const uint32_t slot = it->second;
    slot_.erase(it);
    buffer_.erase(buffer_.begin() + slot);
    buffer_.push_back(GpuLight{});
    created_.erase(std::remove(created_.begin(), created_.end(), key), created_.end());
    updated_.erase(std::remove(updated_.begin(), updated_.end(), key), updated_.end());
    remapped_.erase(key);
    if (std::find(killed_.begin(), killed_.end(), slot) == killed_.end()) killed_.push_back(slot);
    next_id_ -= 1;
    for (auto& kv : slot_)
        if (kv.second > slot) { if (!remapped_.count(kv.first)) remapped_[kv.first] = kv.second; kv.second -= 1; }
}

void LightStore::snapshot() {
    count_ = next_id_;
    for (uint32_t s : killed_) buffer_[s].d3.x = b2f(0xcafebabeu);
    for (auto& kv : remapped_) buffer_[kv.second].d3.x = b2f(slot_[kv.first] + 1u);
    gpu_ = buffer_; slot_uploaded_ = slot_;
    auto commit = [&](int64_t k) { GpuLight& l = buffer_[slot_[k]]; l.prev_d0 = l.d0; l.prev_d1 = l.d1; l.prev_d2 = l.d2; };
    for (int64_t k : created_) commit(k);
    for (int64_t k : updated_) commit(k);
    for (uint32_t s : killed_) buffer_[s].d3.x = b2f(0u);
    for (auto& kv : remapped_) buffer_[kv.second].d3.x = b2f(0u);
    created_.clear(); updated_.clear(); remapped_.clear(); killed_.clear();
}

// ---- images (images.rs)
bool ImageAtlas::release(uint64_t id) {
    auto it = rects_.find(id);
    if (it == rects_.end()) return false;
    shelves_.release(it->second.x, it->second.y, it->second.w);
    rects_.erase(it);
    device_.erase(id);
    rects_dirty = true;
    return true;
}
void ImageAtlas::remove(uint64_t id) { (void)release(id); }

// finds the rectangle for image `id` and makes the host copy of the atlas tall enough
int ImageAtlas::place(uint64_t id, uint32_t w, uint32_t h, Rect* out) {
    if (w > kW) return fail(ST_ERR_ATLAS_FULL, "image wider than the atlas");
    auto it = rects_.find(id);
    Rect rec;
    if (it != rects_.end() && it->second.w == w && it->second.h == h) rec = it->second;  // same size: rewritten in place (images.rs:61-63)
    else {
        (void)release(id);  // another size: the old rectangle is given back first (images.rs:64-66)
        rec = {0, 0, w, h};
        if (!shelves_.allocate(w, h, &rec.x, &rec.y)) return fail(ST_ERR_ATLAS_FULL, "no more space in the atlas");
    }
    const uint32_t need_h = rec.y + h;
    if (w_ == 0) w_ = kW;
    if (need_h > h_) {
        // grow in 256-row steps; rects are stored in texels, so existing materials stay valid after a rebuild
        h_ = (need_h + 255u) & ~255u;
        texels_.resize((size_t)w_ * h_ * 4, 0);
    }
    rects_[id] = rec;
    dirty = true; rects_dirty = true;
    *out = rec;
    return ST_OK;
}

int ImageAtlas::insert_rgba8(uint64_t id, uint32_t w, uint32_t h, const uint8_t* rgba) {
    Rect rec;
    if (int rc = place(id, w, h, &rec)) return rc;
    device_.erase(id);
    for (uint32_t y = 0; y < h; y++) memcpy(texel(rec.x, rec.y + y), rgba + (size_t)y * w * 4, (size_t)w * 4);
    return ST_OK;
}
int ImageAtlas::insert_device(uint64_t id, uint32_t w, uint32_t h, const void* pixels, size_t pitch, bool dynamic) {
    Rect rec;
    if (int rc = place(id, w, h, &rec)) return rc;
    device_[id] = DeviceImage{pixels, pitch, dynamic, true};
    return ST_OK;
}

float4 ImageAtlas::rect_uv(uint64_t id) const {
    const Rect* r = id ? rect_texels(id) : nullptr;
    if (!r || w_ == 0) return make_float4(0, 0, 0, 0);
    return make_float4((float)r->x / (float)w_, (float)r->y / (float)h_, (float)r->w / (float)w_, (float)r->h / (float)h_);
}

// ---- materials (materials.rs:33-96, material.rs:29-50)
void MaterialStore::insert(uint64_t id, const StMaterial& m) {
    auto it = slot_.find(id);
    if (it != slot_.end()) materials_[it->second] = m;
    else {
        size_t b, end_;
        uint32_t slot;
        if (free_.take(1, &b, &end_)) slot = (uint32_t)b;  // materials.rs:48-50 (the slot keeps its previous contents)
        else { materials_.push_back(m); slot = (uint32_t)materials_.size() - 1u; }
        slot_[id] = slot;
    }
    dirty = true;
}
void MaterialStore::remove(uint64_t id) {
    auto it = slot_.find(id);
    if (it == slot_.end()) return;
    free_.give(it->second, it->second);  // `give(id..id)`: an empty range, as in materials.rs:74
    slot_.erase(it);
    dirty = true;
}
void MaterialStore::rebuild(const ImageAtlas& images) {
    gpu_.resize(materials_.size()); base_packed_.resize(materials_.size());
    any_normal_map = false;
    for (size_t i = 0; i < materials_.size(); i++) {
        const StMaterial& m = materials_[i]; GpuMaterial& g = gpu_[i];
        g.base_color = make_float4(m.base_color[0], m.base_color[1], m.base_color[2], m.base_color[3]);
        g.base_color_texture = images.rect_uv(m.base_color_texture);
        g.emissive = make_float4(m.emissive[0], m.emissive[1], m.emissive[2], m.emissive[3]);
        g.emissive_texture = images.rect_uv(m.emissive_texture);
        g.roughness = pow2_(m.perceptual_roughness);
        g.metallic = m.metallic; g.reflectance = m.reflectance; g.ior = m.ior;
        g.metallic_roughness_texture = images.rect_uv(m.metallic_roughness_texture);
        g.normal_map_texture = images.rect_uv(m.normal_map_texture);
        any_normal_map = any_normal_map || !is_zero(g.normal_map_texture);
        base_packed_[i] = gbuffer_pack_base_color(g.base_color);  // st_math.h routines are bit-identical on host and device
    }
}

// ---- meshes
void MeshStore::insert(uint64_t id, const StMeshTriangle* t, size_t count) { meshes_[id].assign(t, t + count); version_[id] = next_version_++; }
void MeshStore::remove(uint64_t id) { meshes_.erase(id); version_.erase(id); }
std::pair<size_t, size_t> MeshStore::device_range(uint64_t id, uint64_t version, const std::vector<StMeshTriangle>& tris) {
    auto dm = device_.find(id);
    if (dm == device_.end() || dm->second.version != version) {
        const DeviceRec rec{store_host_.size() / kTriangleFloats, tris.size(), version};
        store_host_.resize(kTriangleFloats * (rec.first + rec.count));
        for (size_t i = 0; i < rec.count; i++) pack_triangle(tris[i], &store_host_[kTriangleFloats * (rec.first + i)]);
        dm = device_.insert_or_assign(id, rec).first;
    }
    return {dm->second.first, dm->second.count};
}
int MeshStore::upload(hipStream_t up, StagingRing& ring, bool* pageable) {
    if (store_uploaded_ == store_host_.size()) return ST_OK;
    const size_t bytes = store_host_.size() * sizeof(float);
    if (bytes > d_store_.capacity) {   // a new allocation: everything again (hipFree waits for the kernels that read the old one)
        if (int rc = d_store_.upload(store_host_.data(), bytes, up, ring, pageable)) return rc;
    } else if (int rc = d_store_.upload_range(store_host_.data(), store_uploaded_ * sizeof(float), (store_host_.size() - store_uploaded_) * sizeof(float), up, ring, pageable)) return rc;
    store_uploaded_ = store_host_.size();
    return ST_OK;
}

// ---- instances (instances.rs:69-99)
void InstanceStore::insert(uint64_t id, uint64_t mesh, uint64_t material, const Affine& x) {
    dirty = true;
    if (InstanceRec* r = find(id)) { r->prev_xform = r->xform; r->mesh = mesh; r->material = material; r->xform = x; r->xform_inv = affine_inverse(x); r->dirty = true; return; }
    uint32_t xslot;
    if (!xslot_free_.empty()) { xslot = xslot_free_.back(); xslot_free_.pop_back(); }
    else { xslot = (uint32_t)(xforms.size() / 8u); xforms.resize(xforms.size() + 8u, make_float4(0, 0, 0, 0)); }
    records.push_back({id, mesh, material, x, affine_inverse(x), x, true, xslot});
}
void InstanceStore::remove(uint64_t id) {
    for (size_t i = 0; i < records.size(); i++)
        if (records[i].id == id) { xslot_free_.push_back(records[i].xslot); records.erase(records.begin() + i); dirty = true; removed = true; break; }
}
void InstanceStore::fill_xforms() {
    for (const auto& inst : records) {
        float4* x = xforms.data() + 8u * inst.xslot;
        const Affine* src[2] = {&inst.xform_inv, &inst.prev_xform};
        for (int k = 0; k < 2; k++) { x[4 * k] = f4(src[k]->x, 0.0f); x[4 * k + 1] = f4(src[k]->y, 0.0f); x[4 * k + 2] = f4(src[k]->z, 0.0f); x[4 * k + 3] = f4(src[k]->t, 0.0f); }
    }
}

// ---- triangle slots (triangles.rs)
void TriangleSlots::reserve(size_t want) { triangles_.reserve(want); prims_.reserve(want); alive_.reserve(want); geo_.reserve(3 * want); attr_.reserve(4 * want); bounds_.reserve(2 * want); }
void TriangleSlots::grow_to(size_t end) { triangles_.resize(end); prims_.resize(end); alive_.resize(end, 0); geo_.resize(3 * end); attr_.resize(4 * end); bounds_.resize(2 * end); }
void TriangleSlots::take(uint64_t instance, size_t count, size_t* b, size_t* e, bool* appended) {
    *appended = false;
    if (range_of(instance, b, e)) return;
    if (!free_.take(count, b, e)) { *b = size(); *e = *b + count; grow_to(*e); *appended = true; }
    live_ += count;   // (the bake that follows sets alive() for the whole range)
    ranges_[instance] = {*b, *e};
}
bool TriangleSlots::drop(uint64_t instance, size_t* b, size_t* e) {
    auto it = ranges_.find(instance);
    if (it == ranges_.end()) return false;
    *b = it->second.first; *e = it->second.second;
    free_.give(*b, *e);
    for (size_t i = *b; i < *e; i++) { live_ -= alive_[i]; alive_[i] = 0; }
    ranges_.erase(it);
    return true;
}
void TriangleSlots::write(size_t slot, const StMeshTriangle& t, const InstanceRec& inst, uint32_t material) {
    // normals use transpose(inverse(xform)) (Mat4::transform_vector3 order); tangents follow the forward matrix
    const Affine& inv = inst.xform_inv;
    const V3 r0 = v3(inv.x.x, inv.y.x, inv.z.x), r1 = v3(inv.x.y, inv.y.y, inv.z.y), r2 = v3(inv.x.z, inv.y.z, inv.z.z);
    const float det = dot(inst.xform.z, cross(inst.xform.x, inst.xform.y));
    const float sign = (f2b(det) >> 31) ? -1.0f : 1.0f;
    V3 p[3], n[3]; float4 tg[3];
    for (int i = 0; i < 3; i++) {
        p[i] = affine_point(inst.xform, v3(t.positions[i][0], t.positions[i][1], t.positions[i][2]));
        const V3 nn = v3(t.normals[i][0], t.normals[i][1], t.normals[i][2]);
        // transpose(inverse): columns are the inverse's rows; the 4th row of the transposed matrix carries the
        // inverse translation in .w only, which transform_vector3 drops
        V3 acc = r0 * nn.x; acc = r1 * nn.y + acc; acc = r2 * nn.z + acc;
        n[i] = normalize(acc);
        const V3 tt = normalize(affine_vec(inst.xform, v3(t.tangents[i][0], t.tangents[i][1], t.tangents[i][2])));
        tg[i] = make_float4(tt.x, tt.y, tt.z, t.tangents[i][3] * sign);
    }
    HostTriangle h;
    h.d0 = f4(p[0], t.uvs[0][0]); h.d1 = f4(n[0], t.uvs[0][1]); h.d2 = tg[0];
    h.d3 = f4(p[1], t.uvs[1][0]); h.d4 = f4(n[1], t.uvs[1][1]); h.d5 = tg[1];
    h.d6 = f4(p[2], t.uvs[2][0]); h.d7 = f4(n[2], t.uvs[2][1]); h.d8 = tg[2];
    triangles_[slot] = h;
    BuildPrim bp;
    bp.triangle_id = (uint32_t)slot; bp.material_id = material;
    bp.center = (((v3s(0.0f) + p[0]) + p[1]) + p[2]) / 3.0f;
    bp.bounds = Aabb(); bp.bounds.grow(p[0]); bp.bounds.grow(p[1]); bp.bounds.grow(p[2]);
    prims_[slot] = bp; alive_[slot] = 1;
    geo_[3 * slot] = f4(p[0], 0.0f); geo_[3 * slot + 1] = f4(p[1] - p[0], 0.0f); geo_[3 * slot + 2] = f4(p[2] - p[0], 0.0f);
    bounds_[2 * slot] = f4(bp.bounds.lo, 0.0f); bounds_[2 * slot + 1] = f4(bp.bounds.hi, 0.0f);
    attr_[4 * slot] = f4(n[0], t.uvs[0][0]); attr_[4 * slot + 1] = f4(n[1], t.uvs[0][1]); attr_[4 * slot + 2] = f4(n[2], t.uvs[1][0]);
    attr_[4 * slot + 3] = make_float4(t.uvs[1][1], t.uvs[2][0], t.uvs[2][1], b2f(inst.xslot));
}

// ---- the engine's entry points over more than one owner
void Engine::insert_mesh(uint64_t id, const StMeshTriangle* t, size_t count) {
    deform.drop_skin(id);   // skinned meshes: a new mesh drops the skin and the poses of its instances
    deform.drop_morph(id);  // morph targets: likewise the targets and the weights
    meshes.insert(id, t, count);
}
void Engine::remove_mesh(uint64_t id) { deform.drop_skin(id); deform.drop_morph(id); meshes.remove(id); }
void Engine::insert_instance(uint64_t id, uint64_t mesh, uint64_t material, const Affine& x) {
    if (const InstanceRec* r = instances.find(id)) if (r->mesh != mesh) deform.drop_instance(id, false);
    instances.insert(id, mesh, material, x);
}
void Engine::remove_instance(uint64_t id) {
    instances.remove(id);
    drop_instance_triangles(id);
    deform.drop_instance(id, false);
}
void Engine::drop_instance_triangles(uint64_t id) {
    size_t b, e;
    if (slots.drop(id, &b, &e)) tree.slots_changed(b, e);
}

// ---- instances -> world-space triangles (instances.rs:100-139)
// Baking writes disjoint slots and reads nothing it writes, so once every range is assigned — the arrays
// do not move any more — large refreshes are spread over the BVH builder's worker pool in chunks.
void Engine::bake_jobs_on_host(const std::vector<BakeJob>& jobs, size_t total) {
    const auto tb0 = TickClock::now();
    constexpr size_t kChunk = 2048, kParallelFrom = 16384;
    unsigned threads = std::thread::hardware_concurrency();
    if (threads > 16u) threads = 16u;
    if (total < kParallelFrom || threads < 2u) {
        for (const BakeJob& j : jobs)
            for (size_t i = 0; i < j.count; i++) slots.write(j.first + i, (*j.mesh)[i], *j.inst, j.material);
    } else {
        TaskPool pool(threads);
        for (const BakeJob& j : jobs)
            for (size_t at = 0; at < j.count; at += kChunk) {
                const size_t end = std::min(j.count, at + kChunk);
                pool.push([this, j, at, end] { for (size_t i = at; i < end; i++) slots.write(j.first + i, (*j.mesh)[i], *j.inst, j.material); });
            }
        pool.finish();
    }
    if (tuning.tick_timing) fprintf(stderr, "[bake] %zu triangles in %zu jobs: %.2f ms\n", total, jobs.size(), ms_between(tb0, TickClock::now()));
}

// Instances the device has moved (StTuning::device_bake) are baked on the host only when the host arrays are needed again: a rebuild
// (its primitives), a host refit or a debug read of the stream (the bounds), a full upload. Both device copies then receive those slots from
// the host like any other baked range, and their lists of pending device moves are void.
void Engine::bake_stale_on_host() {
    // posed instances bake from their posed regions (st_deform.cpp); a failed read-back is reported by the next st_tick or debug read
    if (int rc = deform.read_back()) deferred_status = rc;
    std::vector<BakeJob> jobs; size_t total = 0;
    for (auto& inst : instances.records) {
        if (!inst.host_stale) continue;
        inst.host_stale = false;
        const std::vector<StMeshTriangle>* mesh = meshes.find(inst.mesh);
        size_t b, e;
        if (!mesh || !slots.range_of(inst.id, &b, &e) || e - b != mesh->size()) continue;  // the next refresh re-bakes it as dirty
        jobs.push_back({deform.bake_source(inst.id, *mesh), &inst, inst.baked_material, b, mesh->size()});
        total += mesh->size();
        copies.owe_slots(b, e);
    }
    copies.void_pending_moves();
    if (!jobs.empty()) bake_jobs_on_host(jobs, total);
}

bool Engine::refresh_instances() {
    moved_on_device = false;
    if (!instances.dirty) return false;
    instances.dirty = false;
    // Device bake: when every dirty instance only MOVED — same mesh (and version of it), same material, its slots already assigned —
    // under ST_BVH_REFIT_DEVICE with the tree's topology on record, the host bakes nothing: the device copies do (Engine::bake_on_device).
    const bool removed = instances.removed; instances.removed = false;
    const bool tree_follows = tree.moves_stay_on_device();
    if (tuning.device_bake && tree_follows && !materials_changed_this_tick && !removed) {
        bool only_moves = true; size_t moved = 0;
        for (const auto& inst : instances.records) {
            if (!inst.dirty) continue;
            moved++;
            const std::vector<StMeshTriangle>* mesh = meshes.find(inst.mesh);
            uint32_t mat; size_t b, e;
            if (!inst.baked || !mesh || !materials.slot_of(inst.material, &mat) || !slots.range_of(inst.id, &b, &e) ||
                inst.baked_mesh != inst.mesh || inst.baked_mesh_version != meshes.version_of(inst.mesh) || inst.baked_material != mat ||
                e - b != mesh->size()) { only_moves = false; break; }
        }
        if (only_moves && moved) {
            for (auto& inst : instances.records) {
                if (!inst.dirty) continue;
                inst.dirty = false; inst.host_stale = true;
                copies.instance_moved(inst.id);
            }
            moved_on_device = true;
            return true;
        }
    }
    // the host bakes this refresh: posed instances from their posed regions, read back in one batch (st_deform.cpp)
    if (int rc = deform.read_back()) deferred_status = rc;
    // instances the device moved earlier and that are not dirty now must catch up first (a rebuild reads every primitive)
    if (instances.any_host_stale()) {
        // re-baked below anyway — but only those whose bake job WILL be queued: an instance whose mesh or material is missing is retried at a
        // later tick, and until then its host arrays must still count as stale (debug reads catch up through bake_stale_on_host)
        for (auto& inst : instances.records)
            if (inst.host_stale && inst.dirty && meshes.find(inst.mesh) && materials.has(inst.material)) inst.host_stale = false;
        bake_stale_on_host();
    }
    std::vector<BakeJob> jobs; size_t total = 0;
    {   // one reallocation at most for everything this refresh appends (a scene load appends every instance)
        size_t fresh = 0, b, e;
        for (const auto& inst : instances.records) {
            if (!inst.dirty || slots.range_of(inst.id, &b, &e)) continue;
            if (const std::vector<StMeshTriangle>* mesh = meshes.find(inst.mesh)) fresh += mesh->size();
        }
        // (geometric: reserve(size + fresh) at EVERY spawn reallocated and copied all the arrays — 60 MB at 208 k triangles, 7 ms of a spawn tick
        // that otherwise costs 0.2 ms, profiles/r06_spawn_cost.txt — although the free list usually serves the new instance)
        if (fresh && slots.size() + fresh > slots.capacity()) slots.reserve(std::max(slots.size() + fresh, slots.capacity() + slots.capacity() / 2));
    }
    for (auto& inst : instances.records) {
        if (!inst.dirty) continue;
        inst.dirty = false;
        const std::vector<StMeshTriangle>* mesh = meshes.find(inst.mesh);
        uint32_t mat;
        if (!mesh || !materials.slot_of(inst.material, &mat)) { inst.dirty = true; instances.dirty = true; continue; }  // retry next tick
        const size_t count = mesh->size();
        size_t b, e; bool appended;
        if (slots.range_of(inst.id, &b, &e) && e - b != count) drop_instance_triangles(inst.id);
        slots.take(inst.id, count, &b, &e, &appended);
        if (appended) copies.owe_whole_arrays();
        jobs.push_back({deform.bake_source(inst.id, *mesh), &inst, mat, b, count});
        total += count;
        copies.owe_slots(b, e);
        tree.slots_changed(b, e);
        inst.baked = true; inst.baked_mesh = inst.mesh; inst.baked_mesh_version = meshes.version_of(inst.mesh); inst.baked_material = mat; inst.host_stale = false;
    }
    bake_jobs_on_host(jobs, total);
    return true;
}

// The device half of a tick whose instances only moved: object-space meshes this copy's pending instances need (appended to the
// device mesh store once), one 128-B job per instance with its CURRENT transform, one launch of k_bvh_bake (which also patches the
// leaf entries). PCIe per tick: 128 B + 4 B per moved instance (and the instance-transform table st_tick sends anyway).
int Engine::bake_on_device(SceneSet& t, hipStream_t up, bool* pageable) {
    if (t.pending_moves.empty()) return ST_OK;
    std::unordered_map<uint64_t, const InstanceRec*> by_id;
    for (const auto& inst : instances.records) by_id[inst.id] = &inst;
    struct Job { float4 x, y, z, t, r0, r1, r2; uint32_t mesh_first, count, slot_first, xslot; };
    static_assert(sizeof(Job) == 128, "k_bvh.hip BakeJobDevice");
    std::vector<Job> jobs; std::vector<uint32_t> starts{0u};
    bool reads_posed = false;
    for (uint64_t id : t.pending_moves) {
        auto it = by_id.find(id);
        if (it == by_id.end()) continue;   // removed since: that tick rebuilt the tree and voided the lists
        const InstanceRec& inst = *it->second;
        const std::vector<StMeshTriangle>* mesh = meshes.find(inst.mesh);
        size_t b, e;
        if (!slots.range_of(id, &b, &e) || !mesh) continue;
        // a posed instance (skinned mesh) reads its region of the posed store, which this tick's skin launch brought up to date (st_deform.cpp)
        size_t posed_first = 0;
        const bool posed = deform.bake_region(id, e - b, &posed_first);
        const std::pair<size_t, size_t> range = posed ? std::make_pair(posed_first, e - b) : meshes.device_range(inst.mesh, inst.baked_mesh_version, *mesh);
        const Affine& inv = inst.xform_inv;
        Job j;
        j.x = f4(inst.xform.x, 0.0f); j.y = f4(inst.xform.y, 0.0f); j.z = f4(inst.xform.z, 0.0f); j.t = f4(inst.xform.t, 0.0f);
        j.r0 = make_float4(inv.x.x, inv.y.x, inv.z.x, 0.0f); j.r1 = make_float4(inv.x.y, inv.y.y, inv.z.y, 0.0f); j.r2 = make_float4(inv.x.z, inv.y.z, inv.z.z, 0.0f);
        j.mesh_first = (uint32_t)range.first; j.count = (uint32_t)range.second; j.slot_first = (uint32_t)b; j.xslot = inst.xslot;
        if (posed) { j.x.w = b2f(1u); reads_posed = true; }
        jobs.push_back(j); starts.push_back(starts.back() + j.count);
    }
    t.pending_moves.clear();
    if (jobs.empty()) return ST_OK;
    int rc;
    if ((rc = meshes.upload(up, staging, pageable))) return rc;
    if ((rc = t.bake_jobs.upload(jobs.data(), jobs.size() * sizeof(Job), up, staging, pageable))) return rc;
    if ((rc = t.bake_starts.upload(starts.data(), starts.size() * sizeof(uint32_t), up, staging, pageable))) return rc;
    if (reads_posed) if ((rc = deform.wait_skinned(up))) return rc;   // the skin launch (skin stream) wrote the posed regions
    // the EXACT build's kernel, whatever arithmetic the frames use: the baked arrays are the host's bits
    launchers_exact().launch_bvh_bake(t.bake_jobs.ptr, static_cast<const uint32_t*>(t.bake_starts.ptr), (uint32_t)jobs.size(), starts.back(), meshes.device_store(),
                                      deform.posed_store(), static_cast<float4*>(t.tri_geo.ptr), static_cast<float4*>(t.tri_bounds.ptr), static_cast<float4*>(t.tri_attr.ptr),
                                      t.tree.patch_stream(), t.tree.patch_index(), up);
    // the next skin launch overwrites the regions after this bake — and after an earlier one still pending on another stream:
    // the event is re-recorded here behind a wait for its previous recording, so that it covers both (the bake itself is not delayed)
    if (reads_posed) if ((rc = deform.posed_read_by(up))) return rc;
    device_bakes++; device_baked_triangles += starts.back();
    return ST_OK;
}

}  // namespace st
