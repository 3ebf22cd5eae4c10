// st_skin.cpp — host engine of libstrolle_hip.so: skinned meshes (include/strolle_hip.h "skinned meshes"; k_skin.hip). See st_engine.h.
//
// A tick skins before it refreshes the scene (Engine::skin_tick): one launch of k_skin on the engine's skin stream writes the posed triangles
// of every instance whose pose changed into its region of the posed store. A posed instance then takes the path of a moved one — its bake
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
        if (poses.count(instance)) drop_pose(instance, true);
        return ST_OK;
    }
    if (joint_count != skin->second.joints) return fail(ST_ERR_INVALID_ARGUMENT, "joint_count differs from the skin's");
    for (size_t i = 0; i < 12u * (size_t)joint_count; i++) if (!std::isfinite(joint_xforms[i])) return fail(ST_ERR_INVALID_ARGUMENT, "a joint matrix element is not finite");
    auto it = poses.find(instance);
    if (it == poses.end()) {
        it = poses.emplace(instance, PoseRec{}).first;
        it->second.mesh = inst->mesh; it->second.count = meshes.at(inst->mesh).size();
    }
    PoseRec& p = it->second;
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
    std::vector<uint64_t> ids;
    for (const auto& kv : poses) if (kv.second.mesh == mesh) ids.push_back(kv.first);
    for (uint64_t id : ids) drop_pose(id, true);
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
        PoseRec& p = kv.second;
        p.has_previous = false;
        if (deform_on) continue;
        if (p.other != SIZE_MAX) { posed_free.give(p.other, p.other + p.count); p.other = SIZE_MAX; }
        std::vector<float>().swap(p.skinned); std::vector<float>().swap(p.previous);
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
    // the skins these poses need, into the skin store (once per skin: bind-pose triangles in the mesh store's layout, then the corners), each
    // into a range a dropped skin gave back or appended; a store that outgrows its device allocation is sent whole into a larger one
    std::vector<std::pair<size_t, size_t>> fresh;   // (first, triangles) of the skins placed now
    for (auto& kv : poses) {
        if (!kv.second.reskin) continue;
        SkinRec& s = skins.at(kv.second.mesh);
        if (s.first != SIZE_MAX) continue;
        const std::vector<StMeshTriangle>& tris = meshes.at(kv.second.mesh);
        size_t b, e;
        if (!skin_free.take(tris.size(), &b, &e)) {
            b = skin_bind_host.size() / 24u; e = b + tris.size();
            skin_bind_host.resize(24u * e); skin_corner_host.resize(3u * e);
        }
        s.first = b;
        for (size_t i = 0; i < tris.size(); i++) {
            const StMeshTriangle& m = tris[i];
            float* f = &skin_bind_host[24u * (b + i)];
            for (int v = 0; v < 3; v++) for (int c = 0; c < 3; c++) *f++ = m.positions[v][c];
            for (int v = 0; v < 3; v++) for (int c = 0; c < 3; c++) *f++ = m.normals[v][c];
            for (int v = 0; v < 3; v++) for (int c = 0; c < 2; c++) *f++ = m.uvs[v][c];
        }
        std::copy(s.corners.begin(), s.corners.end(), skin_corner_host.begin() + 3u * b);
        fresh.push_back({b, tris.size()});
    }
    if (!fresh.empty()) {   // (rare: a new skin) straight from the host image, then wait for the copies
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
        ST_HIP(hipStreamSynchronize(skin_stream));
    }
    // deformation motion: a pose that changed while its region holds what an earlier tick skinned (with the switch on: `skinned` is that tick's palette)
    // is skinned into its second region, which becomes the current one — the bake, read-backs and st_debug_read_posed follow `first` — and the old
    // one keeps the previous positions for this tick's frames. The first tick of a pose has no earlier positions and takes no second region.
    for (auto& kv : poses) {
        PoseRec& p = kv.second;
        if (!deform_on || !p.changed || p.first == SIZE_MAX || p.skinned.empty()) continue;
        if (p.other == SIZE_MAX) {
            size_t b, e;
            if (!posed_free.take(p.count, &b, &e)) { b = posed_size; posed_size += p.count; }
            p.other = b;
        }
        std::swap(p.first, p.other);
        p.previous.swap(p.skinned);
        p.has_previous = true; deform_live++;
    }
    // a region of the posed store for every pose that has none; a store that has to grow is a new allocation: every pose is skinned again
    for (auto& kv : poses) {
        PoseRec& p = kv.second;
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
        for (auto& kv : poses) kv.second.reskin = true;   // (the poses themselves are unchanged: host images stay current)
        grown = true;   // ... and so is every previous region this tick's frames will read, from the palette it was skinned with
    }
    // one job per pose to skin, each padded to a whole workgroup
    std::vector<SkinJob> jobs; std::vector<uint32_t> starts{0u}; std::vector<float> palettes;
    size_t triangles = 0;
    for (auto& kv : poses) {
        PoseRec& p = kv.second;
        if (!p.reskin) continue;
        const SkinRec& s = skins.at(p.mesh);
        SkinJob j{};
        j.skin_first = (uint32_t)s.first; j.count = (uint32_t)p.count; j.posed_first = (uint32_t)p.first; j.palette_first = (uint32_t)(palettes.size() / 12u); j.joint_count = s.joints;
        jobs.push_back(j);
        starts.push_back(starts.back() + (uint32_t)((p.count + kSkinBlock - 1u) / kSkinBlock * kSkinBlock));
        palettes.insert(palettes.end(), p.palette.begin(), p.palette.end());
        triangles += p.count;
        p.reskin = false;
        if (p.changed) { p.changed = false; p.host_current = false; }
        if (deform_on) p.skinned = p.palette;
        if (grown && p.has_previous) {   // the previous positions, again, into the new allocation
            SkinJob q = j;
            q.posed_first = (uint32_t)p.other; q.palette_first = (uint32_t)(palettes.size() / 12u);
            jobs.push_back(q);
            starts.push_back(starts.back() + (uint32_t)((p.count + kSkinBlock - 1u) / kSkinBlock * kSkinBlock));
            palettes.insert(palettes.end(), p.previous.begin(), p.previous.end());
            triangles += p.count;
        }
    }
    bool pageable = false;
    if ((rc = d_skin_jobs.upload(jobs.data(), jobs.size() * sizeof(SkinJob), skin_stream, staging, &pageable)) ||
        (rc = d_skin_starts.upload(starts.data(), starts.size() * sizeof(uint32_t), skin_stream, staging, &pageable)) ||
        (rc = d_palettes.upload(palettes.data(), palettes.size() * sizeof(float), skin_stream, staging, &pageable))) return rc;
    // the one writer of the regions waits for their readers, wherever they ran (the skin stream runs nothing else), and the recordings are spent
    if ((rc = posed_read.wait(skin_stream, Fence::AnyStream, Fence::Clear))) return rc;    // bakes of earlier ticks still reading the regions
    if ((rc = deform_read.wait(skin_stream, Fence::AnyStream, Fence::Clear))) return rc;   // frames still reading previous regions (deformation motion)
    launch_skin(static_cast<const SkinJob*>(d_skin_jobs.ptr), static_cast<const uint32_t*>(d_skin_starts.ptr), (uint32_t)jobs.size(), starts.back(), static_cast<const float*>(d_skin_bind.ptr),
                d_skin_corners.ptr, static_cast<const float*>(d_palettes.ptr), static_cast<float*>(d_posed.ptr), skin_stream);
    ST_HIP(hipGetLastError());
    if ((rc = ev_skinned.record(skin_stream))) return rc;
    // the caller's stream follows the skin: the staging slot's event (end_uploads) comes after these copies, and so does the next frame
    if ((rc = ev_skinned.wait(stream))) return rc;
    if (pageable) ST_HIP(hipStreamSynchronize(skin_stream));   // (staging full or disabled: the copies read the vectors above)
    skin_launches++; skinned_triangles += triangles;
    return ST_OK;
}

int Engine::read_back_posed() {
    std::vector<PoseRec*> todo; size_t floats = 0;
    for (auto& kv : poses)
        if (!kv.second.host_current && kv.second.first != SIZE_MAX) { todo.push_back(&kv.second); floats += 24u * kv.second.count; }
    if (todo.empty()) return ST_OK;
    ST_HIP(hipSetDevice(device));
    std::vector<float> buf(floats);
    size_t at = 0;
    for (PoseRec* p : todo) {
        ST_HIP(hipMemcpyAsync(buf.data() + at, static_cast<const float*>(d_posed.ptr) + 24u * p->first, 24u * p->count * sizeof(float), hipMemcpyDeviceToHost, skin_stream));
        at += 24u * p->count;
    }
    ST_HIP(hipStreamSynchronize(skin_stream));
    posed_readbacks++;
    at = 0;
    for (PoseRec* p : todo) {
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
    if (it == poses.end()) return fail(ST_ERR_INVALID_ARGUMENT, "the instance has no pose");
    if (it->second.first == SIZE_MAX) return fail(ST_ERR_INVALID_ARGUMENT, "the pose is not skinned yet: st_tick applies it");
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
