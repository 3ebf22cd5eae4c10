// st_query.cpp — host engine of libstrolle_hip.so: scene queries (include/strolle_hip.h "scene queries"; k_query.hip). Rays of the
// application walk the live scene copy the frames walk, with the same scene arguments (scene_args) and the same reader bookkeeping as
// render() (st_copies.h): a tick never refills a copy a query that is still in flight reads. See st_engine.h.
#include "st_engine.h"

namespace st {

// The handle table of the scene queries: per instance slot {StHandle lo, StHandle hi, first triangle slot, 0}. Instance slot ranges are
// contiguous (TriangleSlots::range_of), so `triangle slot - first` is the index into the mesh's own array. The fourth word belongs to deformation
// motion (st_traverse.h deform_prev_point): the first triangle of the instance's previous region of the posed store + 1, for the instances this
// tick re-skinned while the switch is on; 0 for every other one, and always while it is off.
void Engine::fill_instance_table() {
    const size_t rows = std::max<size_t>(instances.xforms.size() / 8u, 1u);
    instance_table_.assign(4 * rows, 0u);
    for (const auto& inst : instances.records) {
        size_t b, e;
        if (!slots.range_of(inst.id, &b, &e) || inst.xslot >= rows) continue;
        uint32_t* w = instance_table_.data() + 4 * (size_t)inst.xslot;
        w[0] = (uint32_t)inst.id; w[1] = (uint32_t)(inst.id >> 32); w[2] = (uint32_t)b;
        w[3] = deform.previous_word(inst.id, e - b);
    }
}

// What every query shares with render(): the frame's scene arguments and reader books. `reads`: kReadsScene while in flight after the call returns, else kReadsNothing.
int Engine::query_begin(hipStream_t stream, KArgs& a, unsigned reads) {
    if (!has_device) return fail(ST_ERR_NO_DEVICE, "scene query on a host-only engine");
    if (!copies.scene.written) return fail(ST_ERR_INVALID_ARGUMENT, "st_tick must precede a scene query");
    ST_HIP(hipSetDevice(device));
    a = KArgs{};
    if (int rc = scene_args(a, false)) return rc;
    return copies.begin(stream, reads);
}
static int launched(Engine& e, hipStream_t stream, unsigned reads) { ST_HIP(hipGetLastError()); return e.copies.end(stream, reads); }   // behind a query's launch

int Engine::trace_rays(const void* rays, uint32_t count, void* hits, uint32_t flags, hipStream_t stream, bool reader) {
    KArgs a;
    const unsigned reads = reader ? kReadsScene : kReadsNothing;
    if (int rc = query_begin(stream, a, reads)) return rc;
    // ST_RAY_COHERENT: the packet walk needs the wide stream, and is given up for good once it overflowed (st_engine.h packets_overflowed)
    const uint32_t packets = (flags & ST_RAY_COHERENT) && a.bvh_w != nullptr && !packets_overflowed ? 1u : 0u;
    const float4* nm_tri_geo = nullptr;   // ST_RAY_MAPPED_NORMAL: the flag alone decides, not the engine's switch
    if (flags & ST_RAY_MAPPED_NORMAL) if (int rc = normal_map_geo(stream, true, &nm_tri_geo)) { (void)launched(*this, stream, reads); return rc; }   // (launches already queued on the stream still end their read)
    L.launch_query_closest(a, static_cast<const float4*>(rays), count, static_cast<float4*>(hits), static_cast<const uint4*>(copies.scene.current().instance_table.ptr), packets, nm_tri_geo, stream);
    return launched(*this, stream, reads);
}

int Engine::occluded(const void* rays, uint32_t count, uint32_t* out, hipStream_t stream) {
    KArgs a;
    if (int rc = query_begin(stream, a, kReadsScene)) return rc;
    L.launch_query_occluded(a, static_cast<const float4*>(rays), count, out, stream);
    return launched(*this, stream, kReadsScene);
}

int Engine::pick(const CameraState& c, const uint32_t* pixels, uint32_t count, void* hits, hipStream_t stream) {
    KArgs a;
    if (int rc = query_begin(stream, a, kReadsScene)) return rc;
    a.cam = c.has_shown ? c.shown : serialize_camera(c.desc);
    a.width = c.has_shown ? c.shown_width : c.desc.width; a.height = c.has_shown ? c.shown_height : c.desc.height;
    const float4* nm_tri_geo = nullptr;
    if (int rc = normal_map_geo(stream, false, &nm_tri_geo)) { (void)launched(*this, stream, kReadsScene); return rc; }
    L.launch_query_pick(a, pixels, count, static_cast<float4*>(hits), static_cast<const uint4*>(copies.scene.current().instance_table.ptr), nm_tri_geo, stream);
    return launched(*this, stream, kReadsScene);
}

// Blocking: host rays -> pinned -> device, the query on the engine's own stream, device -> pinned -> host. The call has finished with the
// scene copy when it returns, so it does not count as one of its readers (no later tick can overlap it).
int Engine::trace_rays_host(const void* rays, uint32_t count, void* hits) {
    if (!has_device) return fail(ST_ERR_NO_DEVICE, "scene query on a host-only engine");
    if (!copies.scene.written) return fail(ST_ERR_INVALID_ARGUMENT, "st_tick must precede a scene query");
    ST_HIP(hipSetDevice(device));
    if (!query_stream) ST_HIP(hipStreamCreateWithFlags(&query_stream.h, hipStreamNonBlocking));
    const size_t ray_bytes = (size_t)count * sizeof(StRay), hit_bytes = (size_t)count * sizeof(StRayHit);
    if (int rc = d_query_rays.reserve(ray_bytes, ray_bytes)) return rc;
    if (int rc = d_query_hits.reserve(hit_bytes, hit_bytes)) return rc;
    if (int rc = query_pinned.reserve(hit_bytes)) return rc;   // one page-locked buffer serves both directions (the hits are the larger)
    memcpy(query_pinned.ptr, rays, ray_bytes);
    ST_HIP(hipMemcpyAsync(d_query_rays.ptr, query_pinned.ptr, ray_bytes, hipMemcpyHostToDevice, query_stream));
    if (int rc = trace_rays(d_query_rays.ptr, count, d_query_hits.ptr, 0u, query_stream, false)) { (void)hipStreamSynchronize(query_stream); return rc; }
    ST_HIP(hipMemcpyAsync(query_pinned.ptr, d_query_hits.ptr, hit_bytes, hipMemcpyDeviceToHost, query_stream));
    ST_HIP(hipStreamSynchronize(query_stream));
    memcpy(hits, query_pinned.ptr, hit_bytes);
    return ST_OK;
}

}  // namespace st
