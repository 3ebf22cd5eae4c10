// k_aov.hip — per-pixel AOVs (include/strolle_hip.h "per-pixel AOVs"; st_query.cpp Engine::render_aovs): depth, shading normal, base colour,
// motion vector and instance / triangle identity of the camera ray of every owned pixel, in one launch over the frame's 8x8 tiles (each wave
// holds one tile's 64 coherent primary rays, as in k_prim_visibility). The walk is k_query_pick's, the attributes are the frame's primary hit's (closest_resolve; the fast build's closest_resolve_exact off LDS); albedo
// and motion are k_prim_visibility's own formulas. The three instantiations of ST_LAUNCH_TRACE with the frame's dynamic LDS stack. A plane
// the caller did not ask for is a null pointer here: its branch is uniform over the launch and costs neither the load nor the store.
#include "k_common.h"

namespace st {
namespace ST_KNS {

// KArgs::cam / prev_cam / width / height: the camera of the frame on screen and the one before it; row0..col1: its window (st_query.cpp).
// The planes are width x height, row-major; only owned pixels are written.
template <bool LDS_SCENE, class SE>
__global__ ST_KERNEL_BOUNDS void k_aov(const KArgs a_in, float* depth, float4* normal, float4* albedo, float2* motion, uint64_t* instance,
                                       uint32_t* triangle, const uint4* table, const float* deform_posed, const float4* nm_tri_geo) {
    ST_QUERY_PROLOGUE
    ST_STACK_LDS(SE, lds);
    U2 pos;
    if (!resolve_gid(a, false, &pos) || !owns_pixel(a, pos)) return;
    const Ray ray = camera_ray(a.cam, pos);
    Candidate c; candidate_reset(&c, kF32Max);
    bool any = false; uint32_t used = 0u;   // used: the contract walk's byte count, not reported here
    // primary visibility's walk: exact leaf test, the tile's 64 rays as one packet where the frame's are; ablatable, as the pick is
    ST_CLOSEST_WALK(true, true, a, ray, lane_stack(a, lds), !LDS_SCENE && a.bvh_w != nullptr && a.primary_packets, &c, any, used);
#if ST_FAST_DEVICE
    // the frame's own primary hit: k_prim_visibility resolves it in the island's arithmetic wherever the scene does not live in LDS, so DEPTH and MOTION
    // are the G-buffer's and the velocity plane's bits in the fast build too (closest_resolve's contracted point differs from it by an ulp)
    const TriangleHit h = LDS_SCENE ? closest_resolve(a, ray, c, any) : closest_resolve_exact(a, ray, c, any);
#else
    const TriangleHit h = closest_resolve(a, ray, c, any);
#endif
    const size_t i = (size_t)pos.y * a.width + pos.x;
    if (depth) depth[i] = any ? distance(ray.origin, h.point) : kF32Max;   // the G-buffer's d0.x (k_prim_visibility g.depth)
    if (normal) {   // "the normal as the frame resolved it": mapped where the frame's is (nm_tri_geo is null while normal mapping is not active, as in k_prim_visibility)
        V3 n = h.normal;
        if (any && nm_tri_geo != nullptr) n = normal_map_apply(a, nm_tri_geo, c.tri, h.material_id, c.inv_det, h.uv, n);
        normal[i] = any ? make_float4(n.x, n.y, n.z, 0.0f) : f4z();
    }
    if (albedo) {
        float4 base = f4z();
        if (any) {
            const GpuMaterial& m = a.materials[h.material_id];
            base = sample_atlas(a, h.uv, m.base_color, m.base_color_texture);
        }
        albedo[i] = base;
    }
    if (motion) {   // prim_raster.rs:21-27 as k_prim_visibility computes the velocity plane
        float2 mv = make_float2(0.0f, 0.0f);
        if (any) {
            const float4* xf = a.instance_xforms + 8u * h.xform_slot;
            V3 prev_point = affine_point(xf + 4, affine_point(xf, h.point));
            if (deform_posed != nullptr) (void)deform_prev_point(a, table, deform_posed, h.xform_slot, c.tri, c.u, c.v, &prev_point);   // deformation motion, as in k_prim_visibility (deform_posed is null while it is off)
            const V2 velocity = clip_to_screen(a.cam, world_to_clip(a.cam, h.point)) - clip_to_screen(a.prev_cam, world_to_clip(a.prev_cam, prev_point));
            if (dot(velocity, velocity) >= 0.001f) mv = make_float2(velocity.x, velocity.y);
        }
        motion[i] = mv;
    }
    if (instance || triangle) {
        uint4 rec = make_uint4(0u, 0u, 0u, 0u);   // {handle lo, hi, first triangle slot of the instance, deformation motion's word}
        if (any) rec = table[h.xform_slot];
        if (instance) instance[i] = any ? ((uint64_t)rec.y << 32 | rec.x) : 0ull;
        if (triangle) triangle[i] = any ? c.tri - rec.z : 0xffffffffu;
    }
}

void launch_aov(const KArgs& a, float* depth, float4* normal, float4* albedo, float2* motion, uint64_t* instance, uint32_t* triangle, const uint4* table,
                const float* deform_posed, const float4* nm_tri_geo, hipStream_t s) {
    ST_LAUNCH_TRACE(k_aov, (), false, s, a, depth, normal, albedo, motion, instance, triangle, table, deform_posed, nm_tri_geo);
}

}  // namespace ST_KNS
}  // namespace st
