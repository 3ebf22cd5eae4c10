// k_motion_blur.hip — motion blur (include/strolle_hip.h "motion blur"; st_motion_blur.cpp): the pack launch with its per-tile maximum, the
// 3 x 3 neighbour maximum over the tile vectors, and the gather along the neighbourhood's dominant velocity (McGuire et al. 2012, nearest
// texel taps). tests/motion_blur_ref.py is the specification: everything here is float32, left to right, without FMA contraction and with
// correctly rounded division and square root in BOTH builds, like k_post.hip and k_bloom.hip.
#include "k_common.h"
#include "k_output.h"

#pragma clang fp contract(off)

namespace st {
namespace ST_KNS {

constexpr uint32_t kMBlurW = 32u, kMBlurH = 8u;   // a workgroup's pixels: one quarter of a tile, inside one tile
static_assert(kMBlurW * kMBlurH == (uint32_t)kBlockThreads && kMBlurW == kMBlurTile && kMBlurTile % kMBlurH == 0u, "a workgroup lies inside one tile");

ST_D unsigned long long mb_max64(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

// ---- pack + tile maximum: one workgroup per tile, thread (tx, ty) takes the pixels (tx, ty + 8 k), k = 0..3, of it. A pixel's key is r's
// bits (r >= 0: they order like r) above the complement of its row-major index in the tile, so that one unsigned maximum finds the largest r
// and, among equal ones, the first pixel. The maximum goes through the wave with cross-lane shuffles and through the four waves with one LDS
// step; the thread that owns the winning key stores the tile's vector.
template <bool FRAME>
__global__ __launch_bounds__(kBlockThreads) void k_mblur_pack(const MBlurArgs p) {
    __shared__ unsigned long long s_key[kBlockThreads / 64];
    const uint32_t tile = blockIdx.x, tile_x = tile % p.tiles_x, tile_y = tile / p.tiles_x;
    const uint32_t t = threadIdx.x, tx = t % kMBlurW, ty = t / kMBlurW;
    const uint32_t x = tile_x * kMBlurTile + tx;
    unsigned long long best = 0ull; float best_x = 0.0f, best_y = 0.0f, best_r = 0.0f; bool have = false;
#pragma unroll
    for (uint32_t k = 0; k < kMBlurTile / kMBlurH; k++) {
        const uint32_t row = ty + kMBlurH * k, y = tile_y * kMBlurTile + row;
        if (x >= p.width || y >= p.height) continue;
        const size_t at = (size_t)y * p.width + x;
        float vx, vy, z;
        if (FRAME) {
            const float2 v = *reinterpret_cast<const float2*>(static_cast<const float4*>(p.velocity) + at);
            vx = v.x; vy = v.y;
            z = static_cast<const float4*>(p.depth)[at].x;
            if (z == 0.0f) z = kFltMax;   // sky
        } else {
            const float2 v = static_cast<const float2*>(p.velocity)[at];
            vx = v.x; vy = v.y;
            z = static_cast<const float*>(p.depth)[at];
        }
        vx = vx * p.half_shutter; vy = vy * p.half_shutter;
        float r = sqrtf(vx * vx + vy * vy);
        if (!(r >= 0.5f)) { vx = 0.0f; vy = 0.0f; r = 0.0f; }
        else if (r > p.max_radius) { const float s = p.max_radius / r; vx = vx * s; vy = vy * s; r = p.max_radius; }
        p.packed[at] = make_float2(r, z);
        const unsigned long long key = ((unsigned long long)__float_as_uint(r) << 32) | (unsigned long long)(kMBlurTile * kMBlurTile - 1u - (row * kMBlurTile + tx));
        if (!have || key > best) { best = key; best_x = vx; best_y = vy; best_r = r; have = true; }
    }
    unsigned long long m = have ? best : 0ull;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = mb_max64(m, __shfl_xor(m, off, 64));
    if ((t & 63u) == 0u) s_key[t >> 6] = m;
    __syncthreads();
    m = mb_max64(mb_max64(s_key[0], s_key[1]), mb_max64(s_key[2], s_key[3]));
    if (have && best == m) p.tile_max[tile] = make_float4(best_x, best_y, best_r, 0.0f);   // keys of pixels are distinct: one writer (pixel (0, 0) of a tile is always inside the frame)
}
void launch_mblur_pack(const MBlurArgs& p, hipStream_t s) {
    const uint32_t blocks = p.tiles_x * p.tiles_y;
    if (blocks == 0u) return;
    if (p.frame) ST_KLAUNCH(k_mblur_pack<true>, dim3(blocks), dim3(kBlockThreads), s, p);
    else ST_KLAUNCH(k_mblur_pack<false>, dim3(blocks), dim3(kBlockThreads), s, p);
}

// ---- neighbour maximum: one thread per tile; the first of the largest r in row-major order of (dy, dx) over the tiles that exist
__global__ __launch_bounds__(kBlockThreads) void k_mblur_neighbour(const MBlurArgs p) {
    const uint32_t tile = blockIdx.x * (uint32_t)kBlockThreads + threadIdx.x;
    if (tile >= p.tiles_x * p.tiles_y) return;
    const int tx = (int)(tile % p.tiles_x), ty = (int)(tile / p.tiles_x);
    float4 best = make_float4(0.0f, 0.0f, 0.0f, 0.0f); bool have = false;
    for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
            const int nx = tx + dx, ny = ty + dy;
            if (nx < 0 || ny < 0 || nx >= (int)p.tiles_x || ny >= (int)p.tiles_y) continue;
            const float4 v = p.tile_max[(size_t)ny * p.tiles_x + (size_t)nx];
            if (!have || v.z > best.z) { best = v; have = true; }
        }
    p.tile_n[tile] = best;
}
void launch_mblur_neighbour(const MBlurArgs& p, hipStream_t s) {
    const uint32_t tiles = p.tiles_x * p.tiles_y;
    if (tiles != 0u) ST_KLAUNCH(k_mblur_neighbour, dim3((tiles + (uint32_t)kBlockThreads - 1u) / (uint32_t)kBlockThreads), dim3(kBlockThreads), s, p);
}

// ---- gather: one workgroup per 32 x 8 pixels of one tile, so the tile's (n, r_n) is one uniform load and "at rest" is a uniform branch that
// moves the pixel's 16 B in and the output format's bytes out. The taps of a wave lie along one direction; they are read from global memory
// (a +-32-pixel apron around 32 x 8 pixels in LDS would be mostly texels no tap reads): 16 B of colour and 8 B of (r, Z) each.
ST_D float mb_cone(float d, float r) { return r > 0.0f ? out_clamp01(1.0f - d / r) : 0.0f; }
ST_D float mb_cyl(float d, float r) {
    if (!(r > 0.0f)) return 0.0f;
    const float q = out_clamp01((d - 0.95f * r) / (1.05f * r - 0.95f * r));
    return 1.0f - q * q * (3.0f - 2.0f * q);
}
__global__ __launch_bounds__(kBlockThreads) void k_mblur_gather(const MBlurArgs p) {
    const uint32_t groups_x = (p.width + kMBlurW - 1u) / kMBlurW;
    const uint32_t gx = blockIdx.x % groups_x, gy = blockIdx.x / groups_x;   // row-major: consecutive workgroups stream consecutive 512-B runs of the same eight rows
    const float4 n = p.tile_n[(size_t)(gy / (kMBlurTile / kMBlurH)) * p.tiles_x + gx];
    const uint32_t t = threadIdx.x, x = gx * kMBlurW + t % kMBlurW, y = gy * kMBlurH + t / kMBlurW;
    if (x >= p.width || y >= p.height) return;
    const size_t at = (size_t)y * p.width + x;
    const float4 cx = p.color[at];
    const float rn = n.z;
    if (rn < 0.5f) { out_store(p, at, cx); return; }
    const float2 px = p.packed[at];
    const float r_x = px.x, z_x = px.y;
    float j = 0.0f;
    if (p.jitter) {
        // the 4 x 4 Bayer matrix {0 8 2 10 / 12 4 14 6 / 3 11 1 9 / 15 7 13 5}: one nibble per entry, entry (x, y) at bits 16 y + 4 x
        const unsigned long long bayer = 0x5D7F91B36E4CA280ull;
        j = ((float)((uint32_t)(bayer >> (16u * (y & 3u) + 4u * (x & 3u))) & 15u) + 0.5f) / 16.0f - 0.5f;
    }
    const float w0 = 1.0f / out_max(r_x, 0.5f);
    const V3 c0 = out_colour(cx);
    float sr = c0.x * w0, sg = c0.y * w0, sb = c0.z * w0, wsum = w0;
    const float fx = (float)x + 0.5f, fy = (float)y + 0.5f, fs = (float)p.samples;
    const float xmax = (float)(p.width - 1u), ymax = (float)(p.height - 1u);
    for (uint32_t i = 0; i < p.samples; i++) {
        const float tt = (((float)i + 0.5f + j) * 2.0f) / fs - 1.0f;
        const float qx = fx + n.x * tt, qy = fy + n.y * tt;
        const uint32_t yx = (uint32_t)out_min(out_max(floorf(qx), 0.0f), xmax), yy = (uint32_t)out_min(out_max(floorf(qy), 0.0f), ymax);
        const size_t ay = (size_t)yy * p.width + yx;
        const float2 py = p.packed[ay];
        const float4 cy4 = p.color[ay];
        const float r_y = py.x, z_y = py.y;
        const float d = fabsf(tt) * rn;
        const float e = out_max(p.depth_softness * out_min(z_x, z_y), 1e-6f);
        const float f = out_clamp01(1.0f - (z_y - z_x) / e);
        const float b = out_clamp01(1.0f - (z_x - z_y) / e);
        const float w = (f * mb_cone(d, r_y) + b * mb_cone(d, r_x)) + (mb_cyl(d, r_y) * mb_cyl(d, r_x)) * 2.0f;
        const V3 cy = out_colour(cy4);
        sr = sr + cy.x * w; sg = sg + cy.y * w; sb = sb + cy.z * w; wsum = wsum + w;
    }
    out_store(p, at, make_float4(sr / wsum, sg / wsum, sb / wsum, 1.0f));
}
void launch_mblur_gather(const MBlurArgs& p, hipStream_t s) {
    const uint32_t blocks = ((p.width + kMBlurW - 1u) / kMBlurW) * ((p.height + kMBlurH - 1u) / kMBlurH);
    if (blocks != 0u) ST_KLAUNCH(k_mblur_gather, dim3(blocks), dim3(kBlockThreads), s, p);
}

}  // namespace ST_KNS
}  // namespace st
