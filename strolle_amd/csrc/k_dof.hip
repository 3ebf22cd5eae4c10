// k_dof.hip — depth of field (include/strolle_hip.h "depth of field"; st_dof.cpp): the pack launch with its per-tile near-field maximum, the
// 3 x 3 neighbour maximum over the tile values, and the thin-lens circle-of-confusion gather (a scatter-as-gather disk filter with nearest
// texel taps). tests/dof_ref.py is the specification: everything here is float32, left to right, without FMA contraction and with
// correctly rounded division and square root in BOTH builds, like k_motion_blur.hip.
#include "k_common.h"
#include "k_output.h"

#pragma clang fp contract(off)

namespace st {
namespace ST_KNS {

constexpr uint32_t kDofW = 32u, kDofH = 8u;   // a workgroup's pixels: one quarter of a tile, inside one tile
static_assert(kDofW * kDofH == (uint32_t)kBlockThreads && kDofW == kDofTile && kDofTile % kDofH == 0u, "a workgroup lies inside one tile");

// Z: the distance along the optical axis of the point at distance d along pixel (x, y)'s ray. FLT_MAX (and +inf) stay FLT_MAX.
ST_D float dof_planar(const DofArgs& p, uint32_t x, uint32_t y, float d) {
    if (d >= kFltMax) return kFltMax;
    if (p.planar) return d;
    const float ndc_x = ((float)x + 0.5f) * 2.0f / (float)p.width - 1.0f;
    const float ndc_y = -(((float)y + 0.5f) * 2.0f / (float)p.height - 1.0f);
    const float ax = (ndc_x + p.p8) / p.p0, ay = (ndc_y + p.p9) / p.p5;
    const float c = 1.0f / sqrtf((ax * ax + ay * ay) + 1.0f);
    return d * c;
}

// ---- pack + near-field tile maximum: one workgroup per tile, thread (tx, ty) takes the pixels (tx, ty + 8 k), k = 0..3, of it. The focus
// distance, m and A depend on the launch alone (the autofocus pixel is one uniform load per workgroup), so they are wave-uniform. A near-field
// radius -coc is a non-negative float, which orders like its bits: the tile's value is one unsigned maximum, through the wave with
// cross-lane shuffles and through the four waves with one LDS step; thread 0 stores it.
template <bool FRAME>
__global__ __launch_bounds__(kBlockThreads) void k_dof_pack(const DofArgs p) {
    __shared__ uint32_t s_max[kBlockThreads / 64];
    const uint32_t tile = blockIdx.x, tile_x = tile % p.tiles_x, tile_y = tile / p.tiles_x;
    const uint32_t t = threadIdx.x, tx = t % kDofW, ty = t / kDofW;
    const uint32_t x = tile_x * kDofTile + tx;
    float s = p.focal_distance;
    if (p.autofocus) {
        const float zf = dof_planar(p, p.focus_px, p.focus_py, out_frame_depth(p.depth, (size_t)p.focus_py * p.width + p.focus_px, FRAME));
        if (zf > 0.0f && zf < kFltMax) s = zf;
    }
    const float m = out_max(s - p.focal_length, 1e-6f);
    const float A = p.k / m;
    uint32_t best = 0u;
#pragma unroll
    for (uint32_t k = 0; k < kDofTile / kDofH; k++) {
        const uint32_t y = tile_y * kDofTile + ty + kDofH * k;
        if (x >= p.width || y >= p.height) continue;
        const size_t at = (size_t)y * p.width + x;
        const float z = dof_planar(p, x, y, out_frame_depth(p.depth, at, FRAME));
        float coc = z > 0.0f ? A * (1.0f - s / z) : 0.0f;
        coc = out_min(out_max(coc, -p.max_radius), p.max_radius);
        p.packed[at] = make_float2(coc, z);
        if (coc < 0.0f) { const uint32_t b = __float_as_uint(-coc); best = b > best ? b : best; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)best, off, 64); best = o > best ? o : best; }
    if ((t & 63u) == 0u) s_max[t >> 6] = best;
    __syncthreads();
    if (t == 0u) {
        const uint32_t a = s_max[0] > s_max[1] ? s_max[0] : s_max[1], b = s_max[2] > s_max[3] ? s_max[2] : s_max[3];
        p.tile_max[tile] = __uint_as_float(a > b ? a : b);
    }
}
void launch_dof_pack(const DofArgs& p, hipStream_t s) {
    const uint32_t blocks = p.tiles_x * p.tiles_y;
    if (blocks == 0u) return;
    if (p.frame) ST_KLAUNCH(k_dof_pack<true>, dim3(blocks), dim3(kBlockThreads), s, p);
    else ST_KLAUNCH(k_dof_pack<false>, dim3(blocks), dim3(kBlockThreads), s, p);
}

// ---- neighbour maximum: one thread per tile; the largest value over the 3 x 3 tiles around it that exist (values are >= 0 and never NaN)
__global__ __launch_bounds__(kBlockThreads) void k_dof_neighbour(const DofArgs p) {
    const uint32_t tile = blockIdx.x * (uint32_t)kBlockThreads + threadIdx.x;
    if (tile >= p.tiles_x * p.tiles_y) return;
    const int tx = (int)(tile % p.tiles_x), ty = (int)(tile / p.tiles_x);
    float best = 0.0f;
    for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
            const int nx = tx + dx, ny = ty + dy;
            if (nx < 0 || ny < 0 || nx >= (int)p.tiles_x || ny >= (int)p.tiles_y) continue;
            const float v = p.tile_max[(size_t)ny * p.tiles_x + (size_t)nx];
            if (v > best) best = v;
        }
    p.tile_n[tile] = best;
}
void launch_dof_neighbour(const DofArgs& p, hipStream_t s) {
    const uint32_t tiles = p.tiles_x * p.tiles_y;
    if (tiles != 0u) ST_KLAUNCH(k_dof_neighbour, dim3((tiles + (uint32_t)kBlockThreads - 1u) / (uint32_t)kBlockThreads), dim3(kBlockThreads), s, p);
}

// ---- gather: one workgroup per 32 x 8 pixels of one tile, so the tile's n is one uniform load; the tap table arrives by value and the loop
// index is uniform, so a tap's three floats are scalar loads. A pixel whose own radius and whose neighbourhood's near field are below half a
// pixel moves its 16 B in and the output format's bytes out. Taps are read from global memory, 16 B of colour and 8 B of (coc, Z) each: the
// disk of a wave's 64 pixels (two rows of 32) overlaps almost entirely from lane to lane, so the taps of one k are two rows of consecutive
// texels shifted by one offset when r_g is uniform, and cache lines are shared among the k; a +-32-pixel apron around 32 x 8 pixels at 24 B a
// texel (96 x 72 x 24 B = 166 KB) does not fit the LDS (DESIGN.md "depth of field").
__global__ __launch_bounds__(kBlockThreads) void k_dof_gather(const DofArgs p) {
    const uint32_t groups_x = (p.width + kDofW - 1u) / kDofW;
    const uint32_t gx = blockIdx.x % groups_x, gy = blockIdx.x / groups_x;   // row-major: consecutive workgroups stream consecutive 512-B runs of the same eight rows
    const float n = p.tile_n[(size_t)(gy / (kDofTile / kDofH)) * p.tiles_x + gx];
    const uint32_t t = threadIdx.x, x = gx * kDofW + t % kDofW, y = gy * kDofH + t / kDofW;
    if (x >= p.width || y >= p.height) return;
    const size_t at = (size_t)y * p.width + x;
    const float4 cx = p.color[at];
    const float2 px = p.packed[at];
    const float r_x = fabsf(px.x), z_x = px.y;
    const float r_g = out_max(r_x, n);
    if (r_g < 0.5f) { out_store(p, at, cx); return; }
    const V3 c0 = out_colour(cx);
    float sr = c0.x, sg = c0.y, sb = c0.z, wsum = 1.0f;
    const float fx = (float)x + 0.5f, fy = (float)y + 0.5f;
    const float xmax = (float)(p.width - 1u), ymax = (float)(p.height - 1u);
    for (uint32_t k = 0; k < p.samples; k++) {
        const float tx = p.taps[3u * k], ty = p.taps[3u * k + 1u], tr = p.taps[3u * k + 2u];
        const float qx = fx + tx * r_g, qy = fy + ty * r_g;
        const uint32_t yx = (uint32_t)out_min(out_max(floorf(qx), 0.0f), xmax), yy = (uint32_t)out_min(out_max(floorf(qy), 0.0f), ymax);
        const size_t ay = (size_t)yy * p.width + yx;
        const float2 py = p.packed[ay];
        const float4 cy4 = p.color[ay];
        const float d = tr * r_g;
        float r_y = fabsf(py.x);
        if (py.y > z_x) r_y = out_min(r_y, r_x);   // a blurred background does not bleed over a sharper foreground
        const float q = out_clamp01((r_y - d) + 0.5f);
        const float w = q * q * (3.0f - 2.0f * q);
        const V3 cy = out_colour(cy4);
        sr = sr + cy.x * w; sg = sg + cy.y * w; sb = sb + cy.z * w; wsum = wsum + w;
    }
    out_store(p, at, make_float4(sr / wsum, sg / wsum, sb / wsum, 1.0f));
}
void launch_dof_gather(const DofArgs& p, hipStream_t s) {
    const uint32_t blocks = ((p.width + kDofW - 1u) / kDofW) * ((p.height + kDofH - 1u) / kDofH);
    if (blocks != 0u) ST_KLAUNCH(k_dof_gather, dim3(blocks), dim3(kBlockThreads), s, p);
}

}  // namespace ST_KNS
}  // namespace st
