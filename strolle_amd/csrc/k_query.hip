// k_query.hip — scene queries (include/strolle_hip.h "scene queries"; st_query.cpp): rays of the application against the live scene copy,
// walked by the same traversal routines the frame's passes use. One ray per lane, kBlockThreads lanes per block, no tiles; the three
// instantiations of ST_LAUNCH_TRACE (the scene in LDS, 16-bit stack slots, 32-bit stack slots) with the dynamic LDS stack of the frame's
// launches (KArgs::stack_entries). Queries read no light, so their prologue stages none. They do not count rays (no KernelSlot).
#include "k_common.h"

namespace st {
namespace ST_KNS {

// StRay (2 float4: origin, t_max; direction, pad) -> Ray with len = t_max. false: a miss by contract (t_max <= 0 or NaN, an all-zero direction).
ST_D bool query_ray(const float4* rays, uint32_t i, Ray* ray) {
    const float4 r0 = rays[2 * (size_t)i], r1 = rays[2 * (size_t)i + 1];
    *ray = make_ray(v3(r0.x, r0.y, r0.z), v3(r1.x, r1.y, r1.z));   // Ray::new: the direction as given
    ray->len = r0.w;
    return r0.w > 0.0f && !(r1.x == 0.0f && r1.y == 0.0f && r1.z == 0.0f);
}
// StRayHit (4 float4) of ray i, written whole by its lane: {point, t} {normal, triangle} {uv, u, v} {instance lo, hi, hit, 0}
ST_D void store_hit(float4* hits, uint32_t i, const TriangleHit& h, const Candidate& c, bool hit, const uint4* table) {
    float4 o0 = make_float4(0.0f, 0.0f, 0.0f, kF32Max), o1 = f4z(), o2 = f4z(), o3 = f4z();
    if (hit) {
        const uint4 rec = table[h.xform_slot];   // {handle lo, hi, first triangle slot of the instance, 0}
        o0 = make_float4(h.point.x, h.point.y, h.point.z, h.distance);
        o1 = make_float4(h.normal.x, h.normal.y, h.normal.z, b2f(c.tri - rec.z));
        o2 = make_float4(h.uv.x, h.uv.y, c.u, c.v);
        o3 = make_float4(b2f(rec.x), b2f(rec.y), b2f(1u), 0.0f);
    }
    float4* o = hits + 4 * (size_t)i;
    o[0] = o0; o[1] = o1; o[2] = o2; o[3] = o3;
}

// Closest hit. Fast build: the wide stream with the contract's leaf test (t carries the contract walk's bits), else the compact stream, else the
// contract stream; `packets` (ST_RAY_COHERENT, wide stream present): the wave walks its 64 rays as one packet. Exact build: the contract walk.
// The walks are unbounded; a hit at t >= t_max is a miss, which is exactly the closest hit of the bounded ray.
template <bool LDS_SCENE, class SE>
__global__ ST_KERNEL_BOUNDS void k_query_closest(const KArgs a_in, const float4* rays, uint32_t count, float4* hits, const uint4* table, uint32_t packets, const float4* nm_tri_geo) {
    ST_QUERY_PROLOGUE
    ST_STACK_LDS(SE, lds);
    const uint32_t i = blockIdx.x * (uint32_t)kBlockThreads + threadIdx.x;
    if (i >= count) return;
    Ray ray;
    const bool valid = query_ray(rays, i, &ray);
    Candidate c; candidate_reset(&c, kF32Max);
    bool any = false; uint32_t used = 0u;   // used: the contract walk's byte count, not reported here
    if (valid) {
        // exact leaf test: t carries the contract walk's bits. Not ablatable: the ablation build is about the frame's rays. Packets: the caller's flag (ST_RAY_COHERENT), not the frame's tuning
        ST_CLOSEST_WALK(true, false, a, ray, lane_stack(a, lds), !LDS_SCENE && packets && a.bvh_w != nullptr, &c, any, used);
    }
    const bool hit = any && c.t < ray.len;
    TriangleHit h = closest_resolve(a, ray, c, hit);
    // ST_RAY_MAPPED_NORMAL (nm_tri_geo is null without the flag): StRayHit::normal bent by the material's map, every other field as without it
    if (hit && nm_tri_geo != nullptr) h.normal = normal_map_apply(a, nm_tri_geo, c.tri, h.material_id, c.inv_det, h.uv, h.normal);
    store_hit(hits, i, h, c, hit, table);
}
void launch_query_closest(const KArgs& a, const float4* rays, uint32_t count, float4* hits, const uint4* table, uint32_t packets, const float4* nm_tri_geo, hipStream_t s);

// Occlusion: the shadow rays' any-hit walk (trace_any: wide / compact / fast contract loop in the fast build, traverse<true> in exact) with len = t_max.
template <bool LDS_SCENE, class SE>
__global__ ST_KERNEL_BOUNDS void k_query_occluded(const KArgs a_in, const float4* rays, uint32_t count, uint32_t* occluded) {
    ST_QUERY_PROLOGUE
    ST_STACK_LDS(SE, lds);
    const uint32_t i = blockIdx.x * (uint32_t)kBlockThreads + threadIdx.x;
    if (i >= count) return;
    Ray ray;
    const bool valid = query_ray(rays, i, &ray);
    uint32_t used = 0u;
    const bool occ = valid && trace_any(a, ray, lane_stack(a, lds), &used);
    occluded[i] = occ ? 1u : 0u;
}

// Pixel picks: the camera ray of (x, y) walked exactly as k_ref_tracing walks depth 0 (the packet walk where the frame's primary rays take it,
// otherwise trace_closest's choice of stream), so a pick carries the bits of REF_HITS at that pixel. KArgs::cam / width / height: the camera as
// its last frame saw it (st_query.cpp).
template <bool LDS_SCENE, class SE>
__global__ ST_KERNEL_BOUNDS void k_query_pick(const KArgs a_in, const uint32_t* pixels, uint32_t count, float4* hits, const uint4* table, const float4* nm_tri_geo) {
    ST_QUERY_PROLOGUE
    ST_STACK_LDS(SE, lds);
    const uint32_t i = blockIdx.x * (uint32_t)kBlockThreads + threadIdx.x;
    if (i >= count) return;
    const uint32_t x = pixels[2 * (size_t)i], y = pixels[2 * (size_t)i + 1];
    const Ray ray = camera_ray(a.cam, u2(x, y));
    Candidate c; candidate_reset(&c, kF32Max);
    bool any = false; uint32_t used = 0u;   // used: the contract walk's byte count, not reported here
    if (x < a.width && y < a.height) {
        // k_ref_tracing's depth 0, whose bits a pick owes: trace_closest's fast leaf test and ablation switch, the packet where the frame's primary rays take it
        ST_CLOSEST_WALK(false, true, a, ray, lane_stack(a, lds), !LDS_SCENE && a.bvh_w != nullptr && a.primary_packets, &c, any, used);
    }
    TriangleHit h = closest_resolve(a, ray, c, any);
    if (any && nm_tri_geo != nullptr) h.normal = normal_map_apply(a, nm_tri_geo, c.tri, h.material_id, c.inv_det, h.uv, h.normal);   // a pick matches the frame on screen: mapped while normal mapping is active
    store_hit(hits, i, h, c, any, table);
}

// grid ceil(count / 256); the scene picks the instantiation as ST_LAUNCH_TRACE does, the stack is the frame launches' (stack_lds_bytes)
#define ST_QUERY_LAUNCH(kernel_tmpl, count, stream, ...)                                                                                                     \
    do {                                                                                                                                                    \
        if ((count) == 0u) break;                                                                                                                            \
        const dim3 grid_((uint32_t)(((uint64_t)(count) + kBlockThreads - 1u) / kBlockThreads));                                                             \
        if (scene_fits_lds(a)) ST_KLAUNCH_SMEM((kernel_tmpl<true, uint16_t>), grid_, dim3(kBlockThreads), stack_lds_bytes(a, 2), stream, __VA_ARGS__);           \
        else if (a.bvh_len < stack16_limit(a)) ST_KLAUNCH_SMEM((kernel_tmpl<false, uint16_t>), grid_, dim3(kBlockThreads), stack_lds_bytes(a, 2), stream, __VA_ARGS__); \
        else ST_KLAUNCH_SMEM((kernel_tmpl<false, uint32_t>), grid_, dim3(kBlockThreads), stack_lds_bytes(a, 4), stream, __VA_ARGS__);                            \
    } while (0)

void launch_query_closest(const KArgs& a, const float4* rays, uint32_t count, float4* hits, const uint4* table, uint32_t packets, const float4* nm_tri_geo, hipStream_t s) {
    ST_QUERY_LAUNCH(k_query_closest, count, s, a, rays, count, hits, table, packets, nm_tri_geo);
}
void launch_query_occluded(const KArgs& a, const float4* rays, uint32_t count, uint32_t* occluded, hipStream_t s) {
    ST_QUERY_LAUNCH(k_query_occluded, count, s, a, rays, count, occluded);
}
void launch_query_pick(const KArgs& a, const uint32_t* pixels, uint32_t count, float4* hits, const uint4* table, const float4* nm_tri_geo, hipStream_t s) {
    ST_QUERY_LAUNCH(k_query_pick, count, s, a, pixels, count, hits, table, nm_tri_geo);
}

}  // namespace ST_KNS
}  // namespace st
