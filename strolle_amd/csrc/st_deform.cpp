// st_deform.cpp — host engine of libstrolle_hip.so: mesh deformation, the Deformer of st_deform.h (include/strolle_hip.h "skinned meshes",
// "morph targets"; k_skin.hip). See st_engine.h.
//
// A tick deforms before it refreshes the scene (Deformer::tick): on the skin stream one launch of k_skin (the instances with a pose and no
// active morph target) and one of k_morph (those with active targets, skinned behind the morph where they have a pose too) write the posed
// triangles of every instance whose pose or weights changed into its region of the posed store. A posed instance then takes the path of a
// moved one — its bake job reads the posed region instead of the mesh store (k_bvh.hip k_bvh_bake), and the tree is refitted or rebuilt as
// for moves. Where the host bakes (host refresh modes, observers of the contract stream, debug reads), the regions it lacks are read back in
// one batch first.
#include "st_engine.h"

#include <cmath>

namespace st {

namespace {

using DeformRec = Deformer::DeformRec;
using MorphRec = Deformer::MorphRec;
using SkinRec = Deformer::SkinRec;

// what st_mesh_set_skin and st_mesh_set_morph_targets ask of their mesh: it exists, and `corner_count` is its corners
int mesh_triangles(const Engine& e, uint64_t mesh, size_t corner_count, size_t* triangles) {
    const std::vector<StMeshTriangle>* m = e.meshes.find(mesh);
    if (!m) return fail(ST_ERR_INVALID_ARGUMENT, "no such mesh");
    if (corner_count != 3u * m->size()) return fail(ST_ERR_INVALID_ARGUMENT, "corner_count is not 3 x the mesh's triangles");
    *triangles = m->size();
    return ST_OK;
}

// the deformation of this instance, created if absent
DeformRec& record_of(Deformer& d, const InstanceRec& inst) {
    auto it = d.deforms.find(inst.id);
    if (it == d.deforms.end()) {
        it = d.deforms.emplace(inst.id, DeformRec{}).first;
        it->second.mesh = inst.mesh; it->second.count = d.e.meshes.at(inst.mesh).size();
    }
    return it->second;
}

// the next tick computes `r` again; xform and prev_xform stay: a deformation that changes is a "move" (refresh_instances)
void mark(Engine& e, DeformRec& r, InstanceRec* inst) { r.reskin = true; r.changed = true; e.instances.mark_dirty(inst); }

// The one release path of a deformation's regions (frames still reading a second region: deform_read). The second region goes with what it was
// computed from; `whole`: the current one goes too.
void release(Deformer& d, DeformRec& r, bool whole) {
    if (whole) { d.posed.give(r.first, r.count); r.first = SIZE_MAX; }
    d.posed.give(r.other, r.count); r.other = SIZE_MAX;
    r.has_previous = false; r.recorded = false;
    std::vector<float>().swap(r.skinned); std::vector<float>().swap(r.previous); std::vector<float>().swap(r.skinned_w); std::vector<float>().swap(r.previous_w);
}

// One part of a deformation goes; the deformation itself goes when nothing is left. forget: what the part was made for is gone (a skin or target
// set replaced): the previous positions and what they were computed from go too.
void drop_part(Deformer& d, uint64_t instance, bool palette, bool weights, bool forget) {
    auto it = d.deforms.find(instance);
    if (it == d.deforms.end()) return;
    DeformRec& r = it->second;
    if (palette) r.palette.clear();
    if (weights) r.weights.clear();
    if (r.palette.empty() && r.weights.empty()) { d.drop_instance(instance, true); return; }   // back to the base mesh
    if (forget) release(d, r, false);
    mark(d.e, r, d.e.instances.find(instance));
}

uint32_t padded_to_block(size_t triangles) { return (uint32_t)((triangles + kSkinBlock - 1u) / kSkinBlock * kSkinBlock); }

}  // namespace

int Deformer::set_skin(uint64_t mesh, const StSkinVertex* corners, size_t corner_count, uint32_t joint_count) {
    if (!corners) return fail(ST_ERR_INVALID_ARGUMENT, "null skin corners");
    size_t triangles;
    if (int rc = mesh_triangles(e, mesh, corner_count, &triangles)) return rc;
    if (joint_count < 1u || joint_count > kSkinMaxJoints) return fail(ST_ERR_INVALID_ARGUMENT, "joint_count is 1 ... 256");
    for (size_t i = 0; i < corner_count; i++) {
        const StSkinVertex& c = corners[i];
        bool any = false;
        for (int s = 0; s < 4; s++) {
            if (c.joints[s] >= joint_count) return fail(ST_ERR_INVALID_ARGUMENT, "corner " + std::to_string(i) + ": joint index >= joint_count");
            if (!std::isfinite(c.weights[s]) || c.weights[s] < 0.0f) return fail(ST_ERR_INVALID_ARGUMENT, "corner " + std::to_string(i) + ": weight negative or not finite");
            any |= c.weights[s] > 0.0f;
        }
        if (!any) return fail(ST_ERR_INVALID_ARGUMENT, "corner " + std::to_string(i) + ": all weights are zero");
    }
    drop_skin(mesh);   // a new skin replaces the old one and the poses made for it
    SkinRec& r = skins[mesh];
    r.corners.assign(corners, corners + corner_count); r.joints = joint_count;
    return ST_OK;
}

int Deformer::set_pose(uint64_t instance, const float* joint_xforms, uint32_t joint_count) {
    if (!e.has_device) return fail(ST_ERR_NO_DEVICE, "skinning runs on the device: a host-only engine has no poses");
    InstanceRec* inst = e.instances.find(instance);
    if (!inst) return fail(ST_ERR_INVALID_ARGUMENT, "no such instance");
    auto skin = skins.find(inst->mesh);
    if (skin == skins.end()) return fail(ST_ERR_INVALID_ARGUMENT, "the instance's mesh has no skin");
    if (!joint_xforms || joint_count == 0u) {   // back to the bind pose
        auto had = deforms.find(instance);
        if (had != deforms.end() && !had->second.palette.empty()) drop_part(*this, instance, true, false, false);   // (morph weights stay)
        return ST_OK;
    }
    if (joint_count != skin->second.joints) return fail(ST_ERR_INVALID_ARGUMENT, "joint_count differs from the skin's");
    for (size_t i = 0; i < 12u * (size_t)joint_count; i++) if (!std::isfinite(joint_xforms[i])) return fail(ST_ERR_INVALID_ARGUMENT, "a joint matrix element is not finite");
    DeformRec& p = record_of(*this, *inst);
    p.palette.assign(joint_xforms, joint_xforms + 12u * (size_t)joint_count);
    mark(e, p, inst);
    return ST_OK;
}

void Deformer::drop_instance(uint64_t instance, bool make_dirty) {
    auto it = deforms.find(instance);
    if (it == deforms.end()) return;
    release(*this, it->second, true);   // (deformation motion: the previous positions go with the deformation)
    deforms.erase(it);
    if (make_dirty) e.instances.mark_dirty(instance);
}

void Deformer::drop_skin(uint64_t mesh) {
    auto it = skins.find(mesh);
    if (it == skins.end()) return;
    binds.give(it->second.first, it->second.corners.size() / 3u);
    skins.erase(it);
    std::vector<uint64_t> ids;   // the poses made for it, and what earlier ticks computed from such poses (morph weights stay)
    for (const auto& kv : deforms) if (kv.second.mesh == mesh && (!kv.second.palette.empty() || !kv.second.skinned.empty() || !kv.second.previous.empty())) ids.push_back(kv.first);
    for (uint64_t id : ids) drop_part(*this, id, true, false, true);
}

// ---- morph targets
int Deformer::set_morph_targets(uint64_t mesh, const StMorphDelta* deltas, size_t corner_count, uint32_t target_count) {
    if (!deltas) return fail(ST_ERR_INVALID_ARGUMENT, "null morph deltas");
    size_t triangles;
    if (int rc = mesh_triangles(e, mesh, corner_count, &triangles)) return rc;
    if (target_count < 1u || target_count > kMorphMaxTargets) return fail(ST_ERR_INVALID_ARGUMENT, "target_count is 1 ... 64");
    for (size_t i = 0; i < corner_count * target_count; i++)
        for (int c = 0; c < 3; c++)
            if (!std::isfinite(deltas[i].position[c]) || !std::isfinite(deltas[i].normal[c]))
                return fail(ST_ERR_INVALID_ARGUMENT, "target " + std::to_string(i / corner_count) + ", corner " + std::to_string(i % corner_count) + ": a delta is not finite");
    drop_morph(mesh);   // new targets replace the old ones and the weights made for them
    MorphRec& r = morphs[mesh];
    r.targets = target_count; r.count = triangles;
    r.padded = padded_to_block(r.count);
    // the device layout (st_kernels.h MorphJob): per target four planes of float4 and one of float2 over `padded` triangles
    r.planes.assign((size_t)target_count * r.padded * kMorphUnitFloats, 0.0f);
    for (uint32_t k = 0; k < target_count; k++) {
        float* base = r.planes.data() + (size_t)k * r.padded * kMorphUnitFloats;
        for (size_t t = 0; t < r.count; t++) {
            float f[18];
            for (int v = 0; v < 3; v++) {
                const StMorphDelta& d = deltas[(size_t)k * corner_count + 3u * t + (size_t)v];
                for (int c = 0; c < 3; c++) { f[3 * v + c] = d.position[c]; f[9 + 3 * v + c] = d.normal[c]; }
            }
            for (int q = 0; q < 4; q++) memcpy(base + 4u * ((size_t)q * r.padded + t), f + 4 * q, 4 * sizeof(float));
            memcpy(base + 16u * r.padded + 2u * t, f + 16, 2 * sizeof(float));
        }
    }
    return ST_OK;
}

int Deformer::set_morph_weights(uint64_t instance, const float* weights, uint32_t target_count) {
    if (!e.has_device) return fail(ST_ERR_NO_DEVICE, "morphing runs on the device: a host-only engine has no morph weights");
    InstanceRec* inst = e.instances.find(instance);
    if (!inst) return fail(ST_ERR_INVALID_ARGUMENT, "no such instance");
    auto morph = morphs.find(inst->mesh);
    if (morph == morphs.end()) return fail(ST_ERR_INVALID_ARGUMENT, "the instance's mesh has no morph targets");
    bool active = false;
    if (weights && target_count != 0u) {
        if (target_count != morph->second.targets) return fail(ST_ERR_INVALID_ARGUMENT, "target_count differs from the mesh's");
        for (uint32_t k = 0; k < target_count; k++) {
            if (!std::isfinite(weights[k])) return fail(ST_ERR_INVALID_ARGUMENT, "a weight is not finite");
            active |= weights[k] != 0.0f;
        }
    }
    if (!active) {   // back to the base shape (a joint pose stays)
        auto had = deforms.find(instance);
        if (had != deforms.end() && !had->second.weights.empty()) drop_part(*this, instance, false, true, false);
        return ST_OK;
    }
    DeformRec& p = record_of(*this, *inst);
    p.weights.assign(weights, weights + target_count);
    mark(e, p, inst);
    return ST_OK;
}

void Deformer::drop_morph(uint64_t mesh) {
    auto it = morphs.find(mesh);
    if (it == morphs.end()) return;
    targets.give(it->second.first, (size_t)it->second.targets * it->second.padded);
    binds.give(it->second.bind_first, it->second.count);
    morphs.erase(it);
    std::vector<uint64_t> ids;
    for (const auto& kv : deforms) if (kv.second.mesh == mesh && (!kv.second.weights.empty() || !kv.second.skinned_w.empty() || !kv.second.previous_w.empty())) ids.push_back(kv.first);
    for (uint64_t id : ids) drop_part(*this, id, false, true, true);
}

int Deformer::morphing_stats(uint64_t* ticks, uint64_t* triangles, uint64_t* delta_bytes) const {
    uint64_t bytes = 0;
    for (const auto& kv : morphs) if (kv.second.first != SIZE_MAX) bytes += (uint64_t)kv.second.targets * kv.second.padded * kMorphUnitFloats * sizeof(float);
    *ticks = morph_ticks; *triangles = morphed_triangles; *delta_bytes = bytes;
    return ST_OK;
}

const std::vector<StMeshTriangle>* Deformer::bake_source(uint64_t instance, const std::vector<StMeshTriangle>& mesh) const {
    auto it = deforms.find(instance);
    if (it != deforms.end() && it->second.host_current && it->second.host.size() == mesh.size()) return &it->second.host;
    return &mesh;   // (a pose that no tick has skinned yet: the instance still shows the bind pose)
}

const uint4* Deformer::deform_table() const { return live ? static_cast<const uint4*>(e.copies.scene.current().instance_table.ptr) : nullptr; }

// Deformation motion: what the last tick left is forgotten before this one deforms — an instance has a previous pose for the frames of the tick
// that deformed it again, no longer. With the switch off the second regions go back to the store.
void Deformer::begin_tick() {
    live = 0;
    for (auto& kv : deforms) {
        kv.second.has_previous = false;
        if (!motion_on) release(*this, kv.second, false);
    }
}

int Deformer::deformation_stats(uint64_t* instances_with_previous, uint64_t* previous_bytes) const {
    if (!e.has_device) return fail(ST_ERR_NO_DEVICE, "deformation motion reads the posed store: a host-only engine has none");
    uint64_t bytes = 0;
    for (const auto& kv : deforms) if (kv.second.other != SIZE_MAX) bytes += (uint64_t)kv.second.count * kTriangleFloats * sizeof(float);
    *instances_with_previous = live; *previous_bytes = bytes;
    return ST_OK;
}

// ------------------------------------------------------------------ the tick, in phases
namespace {

struct DeformTick {   // one Deformer::tick: what its phases hand on
    Deformer& d;
    bool grown = false;      // the posed store is a new allocation: every region is computed again, previous ones included
    bool pageable = false;   // an upload went straight from the vectors below
    std::vector<std::pair<size_t, size_t>> fresh_binds;   // (first, triangles) of the bind ranges placed now
    std::vector<MorphRec*> fresh_targets;
    std::vector<SkinJob> jobs; std::vector<uint32_t> starts{0u}; std::vector<float> palettes;
    std::vector<MorphJob> mjobs; std::vector<uint32_t> mstarts{0u}; std::vector<MorphActive> actives;
    size_t skin_triangles = 0, morph_triangles = 0;

    void rotate_previous();
    int place_regions();
    size_t place_bind(uint64_t mesh, const SkinRec* skin);
    int place_sources();
    void add_job(const DeformRec& p, size_t region, const std::vector<float>& palette, const std::vector<float>& weights);
    void build_jobs();
    int upload_jobs();
    int launch(hipStream_t stream);
};

// 1. Deformation motion: a deformation that changed while its region holds what an earlier tick computed with the switch on (`recorded`; `skinned`
// and `skinned_w` are that tick's palette and weights) is computed into its second region, which becomes the current one — the bake, read-backs
// and st_debug_read_posed follow `first` — and the old one keeps the previous positions for this tick's frames. The first tick of a deformation
// has no earlier positions and takes no second region.
void DeformTick::rotate_previous() {
    for (auto& kv : d.deforms) {
        DeformRec& p = kv.second;
        if (!d.motion_on || !p.changed || p.first == SIZE_MAX || !p.recorded) continue;
        if (p.other == SIZE_MAX) p.other = d.posed.take(p.count);
        std::swap(p.first, p.other);
        p.previous.swap(p.skinned); p.previous_w.swap(p.skinned_w);
        p.has_previous = true; d.live++;
    }
}

// 2. A region of the posed store for every deformation that has none; a store that has to grow is a new allocation: everything is computed again —
// every previous region this tick's frames will read too, from the palette and weights it was computed with.
int DeformTick::place_regions() {
    for (auto& kv : d.deforms) if (kv.second.first == SIZE_MAX) kv.second.first = d.posed.take(kv.second.count);
    // (earlier bakes and frames may still read the old allocation)
    if (int rc = grow_store(d.d_posed, d.posed.size * kTriangleFloats * sizeof(float), &grown, {&d.posed_read, &d.deform_read})) return rc;
    if (grown) for (auto& kv : d.deforms) kv.second.reskin = true;   // (the deformations themselves are unchanged: host images stay current)
    return ST_OK;
}

// the mesh's triangles (and the skin's corners) into a range of the bind store's host images
size_t DeformTick::place_bind(uint64_t mesh, const SkinRec* skin) {
    const std::vector<StMeshTriangle>& tris = d.e.meshes.at(mesh);
    bool appended;
    const size_t b = d.binds.take(tris.size(), &appended);
    if (appended) { d.bind_host.resize(kTriangleFloats * d.binds.size); d.corner_host.resize(3u * d.binds.size); }
    for (size_t i = 0; i < tris.size(); i++) pack_triangle(tris[i], &d.bind_host[kTriangleFloats * (b + i)]);
    if (skin) std::copy(skin->corners.begin(), skin->corners.end(), d.corner_host.begin() + 3u * b);
    fresh_binds.push_back({b, tris.size()});
    return b;
}

// 3. What these deformations need on the device, once each: a skin's bind-pose triangles and corners in the bind store, a target set in the target
// store, and for a mesh with targets and no skin its base triangles in the bind store (no corners). Each goes into a range a dropped one gave
// back, or is appended; a store that outgrows its device allocation is sent whole into a larger one (the skin stream's earlier launches read
// the old one: hipFree waits for them).
int DeformTick::place_sources() {
    for (auto& kv : d.deforms) {
        DeformRec& p = kv.second;
        if (!p.reskin) continue;
        auto skin = d.skins.find(p.mesh);
        if (skin != d.skins.end() && skin->second.first == SIZE_MAX) skin->second.first = place_bind(p.mesh, &skin->second);
        auto morph = d.morphs.find(p.mesh);
        if (morph == d.morphs.end()) continue;
        MorphRec& m = morph->second;
        if (skin == d.skins.end() && m.bind_first == SIZE_MAX) m.bind_first = place_bind(p.mesh, nullptr);
        if (m.first == SIZE_MAX && (!p.weights.empty() || (grown && p.has_previous && !p.previous_w.empty()))) {
            m.first = d.targets.take((size_t)m.targets * m.padded);
            fresh_targets.push_back(&m);
        }
    }
    if (fresh_binds.empty() && fresh_targets.empty()) return ST_OK;
    // (rare: a new skin or target set) straight from the host images, then wait for the copies
    int rc; bool fresh_bind, fresh_corners, fresh_store;
    if ((rc = grow_store(d.d_bind, d.bind_host.size() * sizeof(float), &fresh_bind)) || (rc = grow_store(d.d_corners, d.corner_host.size() * sizeof(StSkinVertex), &fresh_corners))) return rc;
    if (fresh_bind || fresh_corners) fresh_binds.assign(1, {0, d.binds.size});
    for (const auto& [b, n] : fresh_binds) {
        ST_HIP(hipMemcpyAsync(d.d_bind.as<float>() + kTriangleFloats * b, d.bind_host.data() + kTriangleFloats * b, n * kTriangleFloats * sizeof(float), hipMemcpyHostToDevice, d.skin_stream));
        ST_HIP(hipMemcpyAsync(d.d_corners.as<StSkinVertex>() + 3u * b, d.corner_host.data() + 3u * b, n * 3u * sizeof(StSkinVertex), hipMemcpyHostToDevice, d.skin_stream));
    }
    if ((rc = grow_store(d.d_targets, d.targets.size * kMorphUnitFloats * sizeof(float), &fresh_store))) return rc;
    if (fresh_store) {   // every set that has a place is sent again
        fresh_targets.clear();
        for (auto& kv : d.morphs) if (kv.second.first != SIZE_MAX) fresh_targets.push_back(&kv.second);
    }
    for (const MorphRec* m : fresh_targets)
        ST_HIP(hipMemcpyAsync(d.d_targets.as<float>() + kMorphUnitFloats * m->first, m->planes.data(), m->planes.size() * sizeof(float), hipMemcpyHostToDevice, d.skin_stream));
    ST_HIP(hipStreamSynchronize(d.skin_stream));
    return ST_OK;
}

// One job for `region` of `p`, padded to a whole workgroup, computed from `palette` and `weights` (its current ones, or those of its previous
// region): k_skin's for a palette alone, k_morph's where a weight is not zero (the host compacts those into the tick's (target, weight) list).
void DeformTick::add_job(const DeformRec& p, size_t region, const std::vector<float>& palette, const std::vector<float>& weights) {
    const uint32_t padded = padded_to_block(p.count);
    const auto skin = d.skins.find(p.mesh);
    const uint32_t palette_first = (uint32_t)(palettes.size() / 12u), joints = palette.empty() ? 0u : skin->second.joints;
    const uint32_t active_first = (uint32_t)actives.size();
    for (uint32_t k = 0; k < (uint32_t)weights.size(); k++) if (weights[k] != 0.0f) actives.push_back({k, weights[k]});
    const uint32_t active_count = (uint32_t)actives.size() - active_first;
    if (active_count) {
        const MorphRec& m = d.morphs.at(p.mesh);
        MorphJob j{};
        j.skin_first = (uint32_t)(skin != d.skins.end() ? skin->second.first : m.bind_first); j.count = (uint32_t)p.count; j.posed_first = (uint32_t)region;
        j.palette_first = palette_first; j.joint_count = joints;
        j.target_first = (uint32_t)m.first; j.padded = (uint32_t)m.padded; j.active_first = active_first; j.active_count = active_count;
        mjobs.push_back(j); mstarts.push_back(mstarts.back() + padded);
        morph_triangles += p.count;
    } else {
        if (palette.empty()) return;   // (no deformation keeps neither part)
        SkinJob j{};
        j.skin_first = (uint32_t)skin->second.first; j.count = (uint32_t)p.count; j.posed_first = (uint32_t)region; j.palette_first = palette_first; j.joint_count = joints;
        jobs.push_back(j); starts.push_back(starts.back() + padded);
    }
    if (joints) { palettes.insert(palettes.end(), palette.begin(), palette.end()); skin_triangles += p.count; }
}

// 4. The jobs of every region to compute, and what the launches will have made of each record
void DeformTick::build_jobs() {
    for (auto& kv : d.deforms) {
        DeformRec& p = kv.second;
        if (!p.reskin) continue;
        add_job(p, p.first, p.palette, p.weights);
        p.reskin = false;
        if (p.changed) { p.changed = false; p.host_current = false; }
        if (d.motion_on) { p.skinned = p.palette; p.skinned_w = p.weights; p.recorded = true; }
        if (grown && p.has_previous) add_job(p, p.other, p.previous, p.previous_w);   // the previous positions, again, into the new allocation
    }
}

// 5.
int DeformTick::upload_jobs() {
    int rc;
    StagingRing& staging = d.e.staging;
    if (!jobs.empty())
        if ((rc = d.d_skin_jobs.upload(jobs.data(), jobs.size() * sizeof(SkinJob), d.skin_stream, staging, &pageable)) ||
            (rc = d.d_skin_starts.upload(starts.data(), starts.size() * sizeof(uint32_t), d.skin_stream, staging, &pageable))) return rc;
    if (!mjobs.empty())
        if ((rc = d.d_morph_jobs.upload(mjobs.data(), mjobs.size() * sizeof(MorphJob), d.skin_stream, staging, &pageable)) ||
            (rc = d.d_morph_starts.upload(mstarts.data(), mstarts.size() * sizeof(uint32_t), d.skin_stream, staging, &pageable)) ||
            (rc = d.d_morph_active.upload(actives.data(), actives.size() * sizeof(MorphActive), d.skin_stream, staging, &pageable))) return rc;
    if (!palettes.empty())
        if ((rc = d.d_palettes.upload(palettes.data(), palettes.size() * sizeof(float), d.skin_stream, staging, &pageable))) return rc;
    return ST_OK;
}

// 6. The one writer of the regions waits for their readers, wherever they ran (the skin stream runs nothing else), and the recordings are spent;
// the two launches; the caller's stream follows them: the staging slot's event (end_uploads) comes after these copies, and so does the next frame.
int DeformTick::launch(hipStream_t stream) {
    int rc;
    if ((rc = d.posed_read.wait(d.skin_stream, Fence::AnyStream, Fence::Clear))) return rc;    // bakes of earlier ticks still reading the regions
    if ((rc = d.deform_read.wait(d.skin_stream, Fence::AnyStream, Fence::Clear))) return rc;   // frames still reading previous regions (deformation motion)
    launch_skin(d.d_skin_jobs.as<const SkinJob>(), d.d_skin_starts.as<const uint32_t>(), (uint32_t)jobs.size(), starts.back(), d.d_bind.as<const float>(),
                d.d_corners.ptr, d.d_palettes.as<const float>(), d.d_posed.as<float>(), d.skin_stream);
    launch_morph(d.d_morph_jobs.as<const MorphJob>(), d.d_morph_starts.as<const uint32_t>(), (uint32_t)mjobs.size(), mstarts.back(), d.d_bind.as<const float>(),
                 d.d_corners.ptr, d.d_palettes.as<const float>(), d.d_targets.as<const float>(), d.d_morph_active.as<const MorphActive>(), d.d_posed.as<float>(), d.skin_stream);
    ST_HIP(hipGetLastError());
    if ((rc = d.ev_skinned.record(d.skin_stream))) return rc;
    if ((rc = d.ev_skinned.wait(stream))) return rc;
    if (pageable) ST_HIP(hipStreamSynchronize(d.skin_stream));   // (staging full or disabled: the copies read the tick's vectors)
    if (skin_triangles) { d.skin_launches++; d.skinned_triangles += skin_triangles; }
    if (morph_triangles) { d.morph_ticks++; d.morphed_triangles += morph_triangles; }
    return ST_OK;
}

}  // namespace

int Deformer::tick(hipStream_t stream) {
    bool any = false;
    for (const auto& kv : deforms) any |= kv.second.reskin;
    if (!any) return ST_OK;
    if (!skin_stream) ST_HIP(hipStreamCreateWithFlags(&skin_stream.h, hipStreamNonBlocking));
    DeformTick t{*this};
    int rc;
    t.rotate_previous();
    if ((rc = t.place_regions()) || (rc = t.place_sources())) return rc;
    t.build_jobs();
    if ((rc = t.upload_jobs())) return rc;
    return t.launch(stream);
}

int Deformer::read_back() {
    std::vector<DeformRec*> todo; size_t floats = 0;
    for (auto& kv : deforms)
        if (!kv.second.host_current && kv.second.first != SIZE_MAX) { todo.push_back(&kv.second); floats += kTriangleFloats * kv.second.count; }
    if (todo.empty()) return ST_OK;
    ST_HIP(hipSetDevice(e.device));
    std::vector<float> buf(floats);
    size_t at = 0;
    for (DeformRec* p : todo) {
        ST_HIP(hipMemcpyAsync(buf.data() + at, posed_store() + kTriangleFloats * p->first, kTriangleFloats * p->count * sizeof(float), hipMemcpyDeviceToHost, skin_stream));
        at += kTriangleFloats * p->count;
    }
    ST_HIP(hipStreamSynchronize(skin_stream));
    posed_readbacks++;
    at = 0;
    for (DeformRec* p : todo) {
        const std::vector<StMeshTriangle>& bind = e.meshes.at(p->mesh);
        p->host.resize(p->count);
        for (size_t i = 0; i < p->count; i++, at += kTriangleFloats) {
            unpack_triangle(&buf[at], p->host[i]);
            memcpy(p->host[i].tangents, bind[i].tangents, sizeof(bind[i].tangents));   // tangents are not skinned (the bake's device arrays hold none)
        }
        p->host_current = true;
    }
    return ST_OK;
}

int Deformer::read_posed(uint64_t instance, float* out, size_t capacity_floats, size_t* written_floats) {
    if (!e.has_device) return fail(ST_ERR_NO_DEVICE, "host-only engine has no poses");
    auto it = deforms.find(instance);
    if (it == deforms.end()) return fail(ST_ERR_INVALID_ARGUMENT, "the instance has neither a pose nor morph weights");
    if (it->second.first == SIZE_MAX) return fail(ST_ERR_INVALID_ARGUMENT, "the deformation is not computed yet: st_tick applies it");
    const size_t n = kTriangleFloats * it->second.count;
    if (written_floats) *written_floats = n;
    if (!out) return ST_OK;
    if (capacity_floats < n) return fail(ST_ERR_INVALID_ARGUMENT, "buffer too small");
    ST_HIP(hipSetDevice(e.device));
    ST_HIP(hipMemcpyAsync(out, posed_store() + kTriangleFloats * it->second.first, n * sizeof(float), hipMemcpyDeviceToHost, skin_stream));
    ST_HIP(hipStreamSynchronize(skin_stream));
    return ST_OK;
}

}  // namespace st
