// st_half_box.h — the f16 planes of a child box in the compact and wide streams (k_bvh.hip k_bvh_compact / k_bvh_wide, k_lbvh.hip lb_emit /
// k_lbvh_refit_nodes): rounded STRICTLY outwards. The stored lower bound lies below the f32 bound and the upper bound above it, also where f16
// holds the bound exactly, so no f16 box has zero thickness.
//
// Why strictly: the walks of these streams test a plane as fmaf(bound, inv, -origin * inv) (st_traverse.h compact_planes), whose error is the rounding
// of origin * inv: half an ulp of the ORIGIN's coordinate in position space, not of the distance to the plane. A flat floor at y = 1024 — a value f16
// holds exactly — gave a box whose two y planes were the same number; a grazing ray that starts near y = 1024 computed both, a whole unit of t off,
// outside the x and z intervals, and the floor (every triangle in it) was skipped. tests/test_gpu_geometry_extremes.py, family flat_1024, is that
// scene. One f16 step is at least 2^-11 of the bound's magnitude, 8,192 times the slab test's error for an origin as far out as the plane: a ray
// that meets the f32 box always meets the f16 one. Bounds beyond +-65504 become +-inf as before (an infinite plane never rejects).
#pragma once
#include <hip/hip_fp16.h>
#include <stdint.h>

namespace st {

__device__ inline uint32_t half_below(float x) {
    uint32_t h = __half_as_ushort(__float2half_rd(x));
    if (__half2float(__ushort_as_half((unsigned short)h)) == x)   // f16 holds x: one step further down (-inf stays)
        h = (h & 0x8000u) ? (h == 0xfc00u ? h : h + 1u) : (h == 0u ? 0x8001u : h - 1u);
    return h;
}
__device__ inline uint32_t half_above(float x) {
    uint32_t h = __half_as_ushort(__float2half_ru(x));
    if (__half2float(__ushort_as_half((unsigned short)h)) == x)   // one step further up (+inf stays)
        h = (h & 0x8000u) ? (h == 0x8000u ? 0x0001u : h - 1u) : (h == 0x7c00u ? h : h + 1u);
    return h;
}

}  // namespace st
