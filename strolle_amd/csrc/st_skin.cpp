// st_skin.cpp — host engine of libstrolle_hip.so: skinned meshes and morph targets (include/strolle_hip.h "skinned meshes", "morph targets";
// k_skin.hip). See st_engine.h.
//
// A tick deforms before it refreshes the scene (Engine::skin_tick): on the engine's skin stream one launch of k_skin (the instances with a
// pose and no active morph target) and one of k_morph (those with active targets, skinned behind the morph where they have a pose too) write
// the posed triangles of every instance whose pose or weights changed into its region of the posed store. A posed instance then takes the path of a moved one — its bake
// job reads the posed region instead of the mesh store (k_bvh.hip k_bvh_bake), and the tree is refitted or rebuilt as for moves. Where the
// host bakes (host refresh modes, observers of the contract stream, debug reads), the regions it lacks are read back in one batch first.
#include "st_engine.h"

#include <cmath>

namespace st {

int Engine::set_skin(uint64_t mesh, const StSkinVertex* corners, size_t corner_count, uint32_t joint_count) {
    if (!corners) return fail(ST_ERR_INVALID_ARGUMENT, "null skin corners");
    auto m = meshes.find(mesh);
    if (m == meshes.end()) return fail(ST_ERR_INVALID_ARGUMENT, "no such mesh");
    if (corner_count != 3u * m->second.size()) return fail(ST_ERR_INVALID_ARGUMENT, "corner_count is not 3 x the mesh's triangles");
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

int Engine::set_pose(uint64_t instance, const float* joint_xforms, uint32_t joint_count) {
    if (!has_device) return fail(ST_ERR_NO_DEVICE, "skinning runs on the device: a host-only engine has no poses");
    InstanceRec* inst = nullptr;
    for (auto& r : instances) if (r.id == instance) { inst = &r; break; }
    if (!inst) return fail(ST_ERR_INVALID_ARGUMENT, "no such instance");
    auto skin = skins.find(inst->mesh);
    if (skin == skins.end()) return fail(ST_ERR_INVALID_ARGUMENT, "the instance's mesh has no skin");
    if (!joint_xforms || joint_count == 0u) {   // back to the bind pose
        auto had = poses.find(instance);
        if (had != poses.end() && !had->second.palette.empty()) drop_part(instance, true, false, false);   // (morph weights stay)
        return ST_OK;
    }
    if (joint_count != skin->second.joints) return fail(ST_ERR_INVALID_ARGUMENT, "joint_count differs from the skin's");
    for (size_t i = 0; i < 12u * (size_t)joint_count; i++) if (!std::isfinite(joint_xforms[i])) return fail(ST_ERR_INVALID_ARGUMENT, "a joint matrix element is not finite");
    auto it = poses.find(instance);
    if (it == poses.end()) {
        it = poses.emplace(instance, DeformRec{}).first;
        it->second.mesh = inst->mesh; it->second.count = meshes.at(inst->mesh).size();
    }
    DeformRec& p = it->second;
    p.palette.assign(joint_xforms, joint_xforms + 12u * (size_t)joint_count);
    p.reskin = true; p.changed = true;
    inst->dirty = true; instances_dirty = true;   // xform and prev_xform stay: a pose-only change is a "move" (refresh_instances)
    return ST_OK;
}

void Engine::drop_pose(uint64_t instance, bool make_dirty) {
    auto it = poses.find(instance);
    if (it == poses.end()) return;
    if (it->second.first != SIZE_MAX) posed_free.give(it->second.first, it->second.first + it->second.count);
    if (it->second.other != SIZE_MAX) posed_free.give(it->second.other, it->second.other + it->second.count);   // (deformation motion: the previous positions go with the pose)
    poses.erase(it);
    if (make_dirty)
        for (auto& r : instances) if (r.id == instance) { r.dirty = true; instances_dirty = true; break; }
}

void Engine::drop_skin(uint64_t mesh) {
    auto it = skins.find(mesh);
    if (it == skins.end()) return;
    // its range of the skin store is reused by a later skin (whose upload is ordered behind every skin launch on the skin stream)
    if (it->second.first != SIZE_MAX) skin_free.give(it->second.first, it->second.first + it->second.corners.size() / 3u);
    skins.erase(it);
    std::vector<uint64_t> ids;   // the poses made for it, and what earlier ticks computed from such poses (morph weights stay)
    for (const auto& kv : poses) if (kv.second.mesh == mesh && (!kv.second.palette.empty() || !kv.second.skinned.empty() || !kv.second.previous.empty())) ids.push_back(kv.first);
    for (uint64_t id : ids) drop_part(id, true, false, true);
}

void Engine::drop_part(uint64_t instance, bool palette, bool weights, bool forget) {
    auto it = poses.find(instance);
    if (it == poses.end()) return;
    DeformRec& r = it->second;
    if (palette) r.palette.clear();
    if (weights) r.weights.clear();
    if (r.palette.empty() && r.weights.empty()) { drop_pose(instance, true); return; }   // back to the base mesh
    if (forget) {   // (frames still reading the second region: deform_read, as in drop_pose)
        if (r.other != SIZE_MAX) { posed_free.give(r.other, r.other + r.count); r.other = SIZE_MAX; }
        r.has_previous = false; r.recorded = false;
        r.skinned.clear(); r.previous.clear(); r.skinned_w.clear(); r.previous_w.clear();
    }
    r.reskin = true; r.changed = true;
    for (auto& i : instances) if (i.id == instance) { i.dirty = true; instances_dirty = true; break; }
}

// ---- morph targets
int Engine::set_morph_targets(uint64_t mesh, const StMorphDelta* deltas, size_t corner_count, uint32_t target_count) {
    if (!deltas) return fail(ST_ERR_INVALID_ARGUMENT, "null morph deltas");
    auto m = meshes.find(mesh);
    if (m == meshes.end()) return fail(ST_ERR_INVALID_ARGUMENT, "no such mesh");
    if (corner_count != 3u * m->second.size()) return fail(ST_ERR_INVALID_ARGUMENT, "corner_count is not 3 x the mesh's triangles");
    if (target_count < 1u || target_count > kMorphMaxTargets) return fail(ST_ERR_INVALID_ARGUMENT, "target_count is 1 ... 64");
    for (size_t i = 0; i < corner_count * target_count; i++)
        for (int c = 0; c < 3; c++)
            if (!std::isfinite(deltas[i].position[c]) || !std::isfinite(deltas[i].normal[c]))
                return fail(ST_ERR_INVALID_ARGUMENT, "target " + std::to_string(i / corner_count) + ", corner " + std::to_string(i % corner_count) + ": a delta is not finite");
    drop_morph(mesh);   // new targets replace the old ones and the weights made for them
    MorphRec& r = morphs[mesh];
    r.targets = target_count; r.count = m->second.size();
    r.padded = (r.count + kSkinBlock - 1u) / kSkinBlock * kSkinBlock;
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

int Engine::set_morph_weights(uint64_t instance, const float* weights, uint32_t target_count) {
    if (!has_device) return fail(ST_ERR_NO_DEVICE, "morphing runs on the device: a host-only engine has no morph weights");
    InstanceRec* inst = nullptr;
    for (auto& r : instances) if (r.id == instance) { inst = &r; break; }
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
    auto it = poses.find(instance);
    if (!active) {   // back to the base shape (a joint pose stays)
        if (it != poses.end() && !it->second.weights.empty()) drop_part(instance, false, true, false);
        return ST_OK;
    }
    if (it == poses.end()) {
        it = poses.emplace(instance, DeformRec{}).first;
        it->second.mesh = inst->mesh; it->second.count = meshes.at(inst->mesh).size();
    }
    DeformRec& p = it->second;
    p.weights.assign(weights, weights + target_count);
    p.reskin = true; p.changed = true;
    inst->dirty = true; instances_dirty = true;   // (as a pose: a "move")
    return ST_OK;
}

void Engine::drop_morph(uint64_t mesh) {
    auto it = morphs.find(mesh);
    if (it == morphs.end()) return;
    // its ranges are reused by later targets and skins (whose uploads are ordered behind every launch on the skin stream)
    if (it->second.first != SIZE_MAX) morph_free.give(it->second.first, it->second.first + (size_t)it->second.targets * it->second.padded);
    if (it->second.bind_first != SIZE_MAX) skin_free.give(it->second.bind_first, it->second.bind_first + it->second.count);
    morphs.erase(it);
    std::vector<uint64_t> ids;
    for (const auto& kv : poses) if (kv.second.mesh == mesh && (!kv.second.weights.empty() || !kv.second.skinned_w.empty() || !kv.second.previous_w.empty())) ids.push_back(kv.first);
    for (uint64_t id : ids) drop_part(id, false, true, true);
}

int Engine::morphing_stats(uint64_t* ticks, uint64_t* triangles, uint64_t* delta_bytes) const {
    uint64_t bytes = 0;
    for (const auto& kv : morphs) if (kv.second.first != SIZE_MAX) bytes += (uint64_t)kv.second.targets * kv.second.padded * kMorphUnitFloats * sizeof(float);
    *ticks = morph_ticks; *triangles = morphed_triangles; *delta_bytes = bytes;
    return ST_OK;
}

const std::vector<StMeshTriangle>* Engine::bake_source(const InstanceRec& inst, const std::vector<StMeshTriangle>& mesh) const {
    auto it = poses.find(inst.id);
    if (it != poses.end() && it->second.host_current && it->second.host.size() == mesh.size()) return &it->second.host;
    return &mesh;   // (a pose that no tick has skinned yet: the instance still shows the bind pose)
}

// Deformation motion: what the last tick left is forgotten before this one skins — an instance has a previous pose for the frames of the tick that
// re-skinned it, no longer. With the switch off the second regions go back to the free list (frames still reading them: deform_read).
void Engine::deform_begin_tick() {
    deform_live = 0;
    for (auto& kv : poses) {
        DeformRec& p = kv.second;
        p.has_previous = false;
        if (deform_on) continue;
        if (p.other != SIZE_MAX) { posed_free.give(p.other, p.other + p.count); p.other = SIZE_MAX; }
        std::vector<float>().swap(p.skinned); std::vector<float>().swap(p.previous); std::vector<float>().swap(p.skinned_w); std::vector<float>().swap(p.previous_w);
        p.recorded = false;
    }
}

int Engine::deformation_stats(uint64_t* instances_with_previous, uint64_t* previous_bytes) const {
    if (!has_device) return fail(ST_ERR_NO_DEVICE, "deformation motion reads the posed store: a host-only engine has none");
    uint64_t bytes = 0;
    for (const auto& kv : poses) if (kv.second.other != SIZE_MAX) bytes += (uint64_t)kv.second.count * 24u * sizeof(float);
    *instances_with_previous = deform_live; *previous_bytes = bytes;
    return ST_OK;
}

int Engine::skin_tick(hipStream_t stream) {
    bool any = false;
    for (const auto& kv : poses) any |= kv.second.reskin;
    if (!any) return ST_OK;
    if (!skin_stream) ST_HIP(hipStreamCreateWithFlags(&skin_stream.h, hipStreamNonBlocking));
    int rc;
    // deformation motion: a deformation that changed while its region holds what an earlier tick computed with the switch on (`recorded`; `skinned`
    // and `skinned_w` are that tick's palette and weights) is computed into its second region, which becomes the current one — the bake, read-backs
    // and st_debug_read_posed follow `first` — and the old one keeps the previous positions for this tick's frames. The first tick of a deformation
    // has no earlier positions and takes no second region.
    for (auto& kv : poses) {
        DeformRec& p = kv.second;
        if (!deform_on || !p.changed || p.first == SIZE_MAX || !p.recorded) continue;
        if (p.other == SIZE_MAX) {
            size_t b, e;
            if (!posed_free.take(p.count, &b, &e)) { b = posed_size; posed_size += p.count; }
            p.other = b;
        }
        std::swap(p.first, p.other);
        p.previous.swap(p.skinned); p.previous_w.swap(p.skinned_w);
        p.has_previous = true; deform_live++;
    }
    // a region of the posed store for every deformation that has none; a store that has to grow is a new allocation: everything is computed again
    for (auto& kv : poses) {
        DeformRec& p = kv.second;
        if (p.first != SIZE_MAX) continue;
        size_t b, e;
        if (!posed_free.take(p.count, &b, &e)) { b = posed_size; posed_size += p.count; }
        p.first = b;
    }
    const size_t posed_bytes = posed_size * 24u * sizeof(float);
    bool grown = false;
    if (posed_bytes > d_posed.capacity) {
        if ((rc = posed_read.host_wait())) return rc;    // (hipFree waits too; said here)
        if ((rc = deform_read.host_wait())) return rc;   // (likewise: frames reading previous regions)
        if ((rc = d_posed.reserve(posed_bytes, posed_bytes + posed_bytes / 2))) return rc;
        for (auto& kv : poses) kv.second.reskin = true;   // (the deformations themselves are unchanged: host images stay current)
        grown = true;   // ... and so is every previous region this tick's frames will read, from the palette and weights it was computed with
    }
    // what these deformations need on the device, once each: a skin's bind-pose triangles (the mesh store's layout) and corners in the skin store, a
    // target set in the target store, and for a mesh with targets and no skin its base triangles in the bind store (no corners). Each goes into a
    // range a dropped one gave back, or is appended; a store that outgrows its device allocation is sent whole into a larger one.
    std::vector<std::pair<size_t, size_t>> fresh;   // (first, triangles) of the bind ranges placed now
    std::vector<MorphRec*> fresh_targets;
    auto place_bind = [&](uint64_t mesh, const SkinRec* skin) {
        const std::vector<StMeshTriangle>& tris = meshes.at(mesh);
        size_t b, e;
        if (!skin_free.take(tris.size(), &b, &e)) {
            b = skin_bind_host.size() / 24u; e = b + tris.size();
            skin_bind_host.resize(24u * e); skin_corner_host.resize(3u * e);
        }
        for (size_t i = 0; i < tris.size(); i++) {
            const StMeshTriangle& m = tris[i];
            float* f = &skin_bind_host[24u * (b + i)];
            for (int v = 0; v < 3; v++) for (int c = 0; c < 3; c++) *f++ = m.positions[v][c];
            for (int v = 0; v < 3; v++) for (int c = 0; c < 3; c++) *f++ = m.normals[v][c];
            for (int v = 0; v < 3; v++) for (int c = 0; c < 2; c++) *f++ = m.uvs[v][c];
        }
        if (skin) std::copy(skin->corners.begin(), skin->corners.end(), skin_corner_host.begin() + 3u * b);
        fresh.push_back({b, tris.size()});
        return b;
    };
    for (auto& kv : poses) {
        DeformRec& p = kv.second;
        if (!p.reskin) continue;
        auto skin = skins.find(p.mesh);
        if (skin != skins.end() && skin->second.first == SIZE_MAX) skin->second.first = place_bind(p.mesh, &skin->second);
        auto morph = morphs.find(p.mesh);
        if (morph == morphs.end()) continue;
        MorphRec& m = morph->second;
        if (skin == skins.end() && m.bind_first == SIZE_MAX) m.bind_first = place_bind(p.mesh, nullptr);
        if (m.first == SIZE_MAX && (!p.weights.empty() || (grown && p.has_previous && !p.previous_w.empty()))) {
            size_t b, e;
            const size_t units = (size_t)m.targets * m.padded;
            if (!morph_free.take(units, &b, &e)) { b = morph_size; morph_size += units; }
            m.first = b;
            fresh_targets.push_back(&m);
        }
    }
    if (!fresh.empty() || !fresh_targets.empty()) {   // (rare: a new skin or target set) straight from the host images, then wait for the copies
        const size_t bind_bytes = skin_bind_host.size() * sizeof(float), corner_bytes = skin_corner_host.size() * sizeof(StSkinVertex);
        if (bind_bytes > d_skin_bind.capacity || corner_bytes > d_skin_corners.capacity) {
            // (the skin stream's earlier launches read the old allocations: hipFree waits for them)
            if ((rc = d_skin_bind.reserve(bind_bytes, bind_bytes + bind_bytes / 2)) || (rc = d_skin_corners.reserve(corner_bytes, corner_bytes + corner_bytes / 2))) return rc;
            fresh.assign(1, {0, skin_bind_host.size() / 24u});
        }
        for (const auto& [b, n] : fresh) {
            ST_HIP(hipMemcpyAsync(static_cast<float*>(d_skin_bind.ptr) + 24u * b, skin_bind_host.data() + 24u * b, n * 24u * sizeof(float), hipMemcpyHostToDevice, skin_stream));
            ST_HIP(hipMemcpyAsync(static_cast<StSkinVertex*>(d_skin_corners.ptr) + 3u * b, skin_corner_host.data() + 3u * b, n * 3u * sizeof(StSkinVertex), hipMemcpyHostToDevice, skin_stream));
        }
        const size_t target_bytes = morph_size * kMorphUnitFloats * sizeof(float);
        if (target_bytes > d_morph_targets.capacity) {   // (likewise) every set that has a place is sent again
            if ((rc = d_morph_targets.reserve(target_bytes, target_bytes + target_bytes / 2))) return rc;
            fresh_targets.clear();
            for (auto& kv : morphs) if (kv.second.first != SIZE_MAX) fresh_targets.push_back(&kv.second);
        }
        for (const MorphRec* m : fresh_targets)
            ST_HIP(hipMemcpyAsync(static_cast<float*>(d_morph_targets.ptr) + kMorphUnitFloats * m->first, m->planes.data(), m->planes.size() * sizeof(float), hipMemcpyHostToDevice, skin_stream));
        ST_HIP(hipStreamSynchronize(skin_stream));
    }
    // one job per region to compute, each padded to a whole workgroup: k_skin's for a palette alone, k_morph's where a weight is not zero (the host
    // compacts those into the tick's (target, weight) list)
    std::vector<SkinJob> jobs; std::vector<uint32_t> starts{0u}; std::vector<float> palettes;
    std::vector<MorphJob> mjobs; std::vector<uint32_t> mstarts{0u}; std::vector<MorphActive> actives;
    size_t skin_triangles = 0, morph_triangles = 0;
    auto add_job = [&](const DeformRec& p, size_t region, const std::vector<float>& palette, const std::vector<float>& weights) {
        const uint32_t padded = (uint32_t)((p.count + kSkinBlock - 1u) / kSkinBlock * kSkinBlock);
        const auto skin = skins.find(p.mesh);
        const uint32_t palette_first = (uint32_t)(palettes.size() / 12u), joints = palette.empty() ? 0u : skin->second.joints;
        const uint32_t active_first = (uint32_t)actives.size();
        for (uint32_t k = 0; k < (uint32_t)weights.size(); k++) if (weights[k] != 0.0f) actives.push_back({k, weights[k]});
        const uint32_t active_count = (uint32_t)actives.size() - active_first;
        if (active_count) {
            const MorphRec& m = morphs.at(p.mesh);
            MorphJob j{};
            j.skin_first = (uint32_t)(skin != skins.end() ? skin->second.first : m.bind_first); j.count = (uint32_t)p.count; j.posed_first = (uint32_t)region;
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
    };
    for (auto& kv : poses) {
        DeformRec& p = kv.second;
        if (!p.reskin) continue;
        add_job(p, p.first, p.palette, p.weights);
        p.reskin = false;
        if (p.changed) { p.changed = false; p.host_current = false; }
        if (deform_on) { p.skinned = p.palette; p.skinned_w = p.weights; p.recorded = true; }
        if (grown && p.has_previous) add_job(p, p.other, p.previous, p.previous_w);   // the previous positions, again, into the new allocation
    }
    bool pageable = false;
    if (!jobs.empty())
        if ((rc = d_skin_jobs.upload(jobs.data(), jobs.size() * sizeof(SkinJob), skin_stream, staging, &pageable)) ||
            (rc = d_skin_starts.upload(starts.data(), starts.size() * sizeof(uint32_t), skin_stream, staging, &pageable))) return rc;
    if (!mjobs.empty())
        if ((rc = d_morph_jobs.upload(mjobs.data(), mjobs.size() * sizeof(MorphJob), skin_stream, staging, &pageable)) ||
            (rc = d_morph_starts.upload(mstarts.data(), mstarts.size() * sizeof(uint32_t), skin_stream, staging, &pageable)) ||
            (rc = d_morph_active.upload(actives.data(), actives.size() * sizeof(MorphActive), skin_stream, staging, &pageable))) return rc;
    if (!palettes.empty())
        if ((rc = d_palettes.upload(palettes.data(), palettes.size() * sizeof(float), skin_stream, staging, &pageable))) return rc;
    // the one writer of the regions waits for their readers, wherever they ran (the skin stream runs nothing else), and the recordings are spent
    if ((rc = posed_read.wait(skin_stream, Fence::AnyStream, Fence::Clear))) return rc;    // bakes of earlier ticks still reading the regions
    if ((rc = deform_read.wait(skin_stream, Fence::AnyStream, Fence::Clear))) return rc;   // frames still reading previous regions (deformation motion)
    launch_skin(static_cast<const SkinJob*>(d_skin_jobs.ptr), static_cast<const uint32_t*>(d_skin_starts.ptr), (uint32_t)jobs.size(), starts.back(), static_cast<const float*>(d_skin_bind.ptr),
                d_skin_corners.ptr, static_cast<const float*>(d_palettes.ptr), static_cast<float*>(d_posed.ptr), skin_stream);
    launch_morph(static_cast<const MorphJob*>(d_morph_jobs.ptr), static_cast<const uint32_t*>(d_morph_starts.ptr), (uint32_t)mjobs.size(), mstarts.back(), static_cast<const float*>(d_skin_bind.ptr),
                 d_skin_corners.ptr, static_cast<const float*>(d_palettes.ptr), static_cast<const float*>(d_morph_targets.ptr), static_cast<const MorphActive*>(d_morph_active.ptr),
                 static_cast<float*>(d_posed.ptr), skin_stream);
    ST_HIP(hipGetLastError());
    if ((rc = ev_skinned.record(skin_stream))) return rc;
    // the caller's stream follows the launches: the staging slot's event (end_uploads) comes after these copies, and so does the next frame
    if ((rc = ev_skinned.wait(stream))) return rc;
    if (pageable) ST_HIP(hipStreamSynchronize(skin_stream));   // (staging full or disabled: the copies read the vectors above)
    if (skin_triangles) { skin_launches++; skinned_triangles += skin_triangles; }
    if (morph_triangles) { morph_ticks++; morphed_triangles += morph_triangles; }
    return ST_OK;
}

int Engine::read_back_posed() {
    std::vector<DeformRec*> todo; size_t floats = 0;
    for (auto& kv : poses)
        if (!kv.second.host_current && kv.second.first != SIZE_MAX) { todo.push_back(&kv.second); floats += 24u * kv.second.count; }
    if (todo.empty()) return ST_OK;
    ST_HIP(hipSetDevice(device));
    std::vector<float> buf(floats);
    size_t at = 0;
    for (DeformRec* p : todo) {
        ST_HIP(hipMemcpyAsync(buf.data() + at, static_cast<const float*>(d_posed.ptr) + 24u * p->first, 24u * p->count * sizeof(float), hipMemcpyDeviceToHost, skin_stream));
        at += 24u * p->count;
    }
    ST_HIP(hipStreamSynchronize(skin_stream));
    posed_readbacks++;
    at = 0;
    for (DeformRec* p : todo) {
        const std::vector<StMeshTriangle>& bind = meshes.at(p->mesh);
        p->host.resize(p->count);
        for (size_t i = 0; i < p->count; i++, at += 24u) {
            StMeshTriangle& t = p->host[i];
            memcpy(t.positions, &buf[at], 9 * sizeof(float)); memcpy(t.normals, &buf[at + 9], 9 * sizeof(float)); memcpy(t.uvs, &buf[at + 18], 6 * sizeof(float));
            memcpy(t.tangents, bind[i].tangents, sizeof(t.tangents));   // tangents are not skinned (the bake's device arrays hold none)
        }
        p->host_current = true;
    }
    return ST_OK;
}

int Engine::read_posed(uint64_t instance, float* out, size_t capacity_floats, size_t* written_floats) {
    if (!has_device) return fail(ST_ERR_NO_DEVICE, "host-only engine has no poses");
    auto it = poses.find(instance);
    if (it == poses.end()) return fail(ST_ERR_INVALID_ARGUMENT, "the instance has neither a pose nor morph weights");
    if (it->second.first == SIZE_MAX) return fail(ST_ERR_INVALID_ARGUMENT, "the deformation is not computed yet: st_tick applies it");
    const size_t n = 24u * it->second.count;
    if (written_floats) *written_floats = n;
    if (!out) return ST_OK;
    if (capacity_floats < n) return fail(ST_ERR_INVALID_ARGUMENT, "buffer too small");
    ST_HIP(hipSetDevice(device));
    ST_HIP(hipMemcpyAsync(out, static_cast<const float*>(d_posed.ptr) + 24u * it->second.first, n * sizeof(float), hipMemcpyDeviceToHost, skin_stream));
    ST_HIP(hipStreamSynchronize(skin_stream));
    return ST_OK;
}

}  // namespace st
