// st_aov.cpp — host engine of libstrolle_hip.so: per-pixel AOVs (include/strolle_hip.h "per-pixel AOVs"; k_aov.hip). A reader of the live
// scene copy like the scene queries (query_begin, SceneCopies::end), through the camera of the frame on screen and its window.
#include "st_engine.h"

namespace st {

int Engine::render_aovs(const CameraState& c, const StAovTargets& t, hipStream_t stream) {
    KArgs a;
    const unsigned reads = kReadsScene | (t.planes[ST_AOV_MOTION] ? kReadsPrevious : 0u);   // (the MOTION plane reads previous regions of the posed store)
    if (int rc = query_begin(stream, a, reads)) return rc;
    // the frame on screen (render() records shown / shown_prev); before the first render, what the next render would cast through
    a.cam = c.has_shown ? c.shown : c.curr; a.prev_cam = c.has_shown ? c.shown_prev : c.prev;
    a.width = c.has_shown ? c.shown_width : c.desc.width; a.height = c.has_shown ? c.shown_height : c.desc.height;
    a.row0 = c.row0; a.row1 = c.row1; a.col0 = c.col0; a.col1 = c.col1;
    a.tile_map = tuning.tile_map;
    const float4* nm_tri_geo = nullptr;
    if (t.planes[ST_AOV_NORMAL]) if (int rc = normal_map_geo(stream, false, &nm_tri_geo)) { (void)hipGetLastError(); (void)copies.end(stream, kReadsScene); return rc; }
    L.launch_aov(a, static_cast<float*>(t.planes[ST_AOV_DEPTH]), static_cast<float4*>(t.planes[ST_AOV_NORMAL]), static_cast<float4*>(t.planes[ST_AOV_ALBEDO]),
                 static_cast<float2*>(t.planes[ST_AOV_MOTION]), static_cast<uint64_t*>(t.planes[ST_AOV_INSTANCE]), static_cast<uint32_t*>(t.planes[ST_AOV_TRIANGLE]),
                 static_cast<const uint4*>(copies.scene.current().instance_table.ptr), t.planes[ST_AOV_MOTION] ? deform.deform_posed() : nullptr, nm_tri_geo, stream);
    ST_HIP(hipGetLastError());
    return copies.end(stream, reads);
}

}  // namespace st
