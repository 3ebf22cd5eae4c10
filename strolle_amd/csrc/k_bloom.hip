// k_bloom.hip — bloom (include/strolle_hip.h "bloom"; st_bloom.cpp): the mip pyramid's downsamples (the first one prefilters the frame on
// the way), its upsamples blended in place, and the composite, which upsamples mip 0 onto the composed frame, runs the display transform
// and writes the output format. tests/bloom_ref.py is the specification: everything here is float32, left to right, without FMA
// contraction and with correctly rounded division in BOTH builds, like k_post.hip. Every kernel serves a 32 x 8 tile of its destination
// per workgroup, one pixel per thread, and stages the source texels the tile reads (clamped at the image's edges, so the clamping is done
// once per texel) in LDS with one 16-B load per texel.
#include "k_common.h"
#include "k_output.h"

#pragma clang fp contract(off)

namespace st {
namespace ST_KNS {

constexpr uint32_t kBloomW = 32u, kBloomH = 8u;
constexpr uint32_t kBloomDownW = 2u * kBloomW + 4u, kBloomDownH = 2u * kBloomH + 4u;   // a destination pixel reads source texels 2 x - 2 .. 2 x + 3
constexpr uint32_t kBloomUpW = kBloomW / 2u + 4u, kBloomUpH = kBloomH / 2u + 4u;       // ... and source texels floor((x + 1) / 2) - 2 .. + 1
static_assert(kBloomW * kBloomH == (uint32_t)kBlockThreads, "one destination pixel per thread");

ST_D V3 bloom_add(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
ST_D V3 bloom_mul(V3 a, float s) { return v3(a.x * s, a.y * s, a.z * s); }
ST_D V3 bloom_lerp(V3 a, V3 b, float f) { return v3(a.x + (b.x - a.x) * f, a.y + (b.y - a.y) * f, a.z + (b.z - a.z) * f); }

ST_D V3 bloom_prefilter(const BloomArgs& p, float4 t) {
    V3 c = v3(out_min(out_max(t.x, 0.0f), p.clamp), out_min(out_max(t.y, 0.0f), p.clamp), out_min(out_max(t.z, 0.0f), p.clamp));
    if (p.threshold_on) {
        const float m = out_max(out_max(c.x, c.y), c.z);
        float s = out_min(out_max(m - p.knee_lo, 0.0f), p.knee2);
        s = (s * s) / p.knee_div;
        const float w = out_max(m - p.threshold, s) / out_max(m, 1e-4f);
        c = bloom_mul(c, w);
    }
    return c;
}

// The 13-tap downsample of one destination pixel. t(i, j) is the source texel (2 x - 2 + i, 2 y - 2 + j), i, j in 0..5, already clamped to its
// image (and prefiltered where the header says P(t)). Every kernel of this file computes a downsample through this one function, so the tile
// kernels and the fused tail round alike.
template <class T>
ST_D V3 bloom_down13(T&& t, bool firefly) {
    auto S = [&](int dx, int dy) {
        const int i = dx + 2, j = dy + 2;
        return bloom_mul(bloom_add(bloom_add(t(i, j), t(i + 1, j)), bloom_add(t(i, j + 1), t(i + 1, j + 1))), 0.25f);
    };
    auto G = [&](V3 q0, V3 q1, V3 q2, V3 q3) { return bloom_mul(bloom_add(bloom_add(bloom_add(q0, q1), q2), q3), 0.25f); };
    const V3 a = S(-2, -2), b = S(0, -2), c = S(2, -2), d = S(-2, 0), e = S(0, 0), f = S(2, 0), g = S(-2, 2), h = S(0, 2), i = S(2, 2);
    const V3 j = S(-1, -1), k = S(1, -1), l = S(-1, 1), m = S(1, 1);
    const V3 g0 = G(a, b, d, e), g1 = G(b, c, e, f), g2 = G(d, e, g, h), g3 = G(e, f, h, i), g4 = G(j, k, l, m);
    float w0 = 0.125f, w1 = 0.125f, w2 = 0.125f, w3 = 0.125f, w4 = 0.5f;
    if (firefly) {
        w0 = w0 * (1.0f / (1.0f + display_luma(g0.x, g0.y, g0.z))); w1 = w1 * (1.0f / (1.0f + display_luma(g1.x, g1.y, g1.z)));
        w2 = w2 * (1.0f / (1.0f + display_luma(g2.x, g2.y, g2.z))); w3 = w3 * (1.0f / (1.0f + display_luma(g3.x, g3.y, g3.z)));
        w4 = w4 * (1.0f / (1.0f + display_luma(g4.x, g4.y, g4.z)));
    }
    V3 r = bloom_add(bloom_add(bloom_add(bloom_add(bloom_mul(g0, w0), bloom_mul(g1, w1)), bloom_mul(g2, w2)), bloom_mul(g3, w3)), bloom_mul(g4, w4));
    if (firefly) { const float ws = (((w0 + w1) + w2) + w3) + w4; r = v3(r.x / ws, r.y / ws, r.z / ws); }
    return r;
}
// The 3 x 3 tent upsample at one destination pixel. t(i, j) is the source texel (i0 - 1 + i, j0 - 1 + j), i, j in 0..3, clamped; fx, fy are
// 0.75 for an even destination coordinate, 0.25 for an odd one. The four horizontal blends of a row are shared by the look-ups above and below.
template <class T>
ST_D V3 bloom_up9(T&& t, float fx, float fy) {
    V3 hz[4][3];
#pragma unroll
    for (int r4 = 0; r4 < 4; r4++) {
        const V3 t0 = t(0, r4), t1 = t(1, r4), t2 = t(2, r4), t3 = t(3, r4);
        hz[r4][0] = bloom_lerp(t0, t1, fx); hz[r4][1] = bloom_lerp(t1, t2, fx); hz[r4][2] = bloom_lerp(t2, t3, fx);
    }
    const float wgt[3][3] = {{0.0625f, 0.125f, 0.0625f}, {0.125f, 0.25f, 0.125f}, {0.0625f, 0.125f, 0.0625f}};
    V3 u = bloom_mul(bloom_lerp(hz[0][0], hz[1][0], fy), wgt[0][0]);
#pragma unroll
    for (int oy = 0; oy < 3; oy++)
#pragma unroll
        for (int ox = 0; ox < 3; ox++)
            if (oy != 0 || ox != 0) u = bloom_add(u, bloom_mul(bloom_lerp(hz[oy][ox], hz[oy + 1][ox], fy), wgt[oy][ox]));
    return u;
}
ST_D V3 bloom_blend(V3 r, V3 u, float factor, bool additive) {
    const V3 ub = bloom_mul(u, factor);
    return additive ? bloom_add(r, ub) : bloom_add(bloom_mul(r, 1.0f - factor), ub);
}

// ---- one level down. LDS: (2 * 32 + 4) x (2 * 8 + 4) texels (21.25 KiB); texel (lx, ly) of it is source texel (2 tile_x - 2 + lx, 2 tile_y - 2 + ly)
template <bool FIRST>
__global__ __launch_bounds__(kBlockThreads) void k_bloom_down(const BloomArgs p) {
    __shared__ float4 s_t[kBloomDownH][kBloomDownW];
    const uint32_t tiles_x = (p.dw + kBloomW - 1u) / kBloomW;
    const int tile_x = (int)((blockIdx.x % tiles_x) * kBloomW), tile_y = (int)((blockIdx.x / tiles_x) * kBloomH);
    const uint32_t t = threadIdx.x, tx = t % kBloomW, ty = t / kBloomW;
    for (uint32_t i = t; i < kBloomDownW * kBloomDownH; i += (uint32_t)kBlockThreads) {
        const uint32_t lx = i % kBloomDownW, ly = i / kBloomDownW;
        const int sx = out_clampi(2 * tile_x - 2 + (int)lx, (int)p.sw), sy = out_clampi(2 * tile_y - 2 + (int)ly, (int)p.sh);
        const float4 v = p.src[(size_t)sy * p.sw + (size_t)sx];
        if (FIRST) { const V3 c = bloom_prefilter(p, v); s_t[ly][lx] = make_float4(c.x, c.y, c.z, 1.0f); }
        else s_t[ly][lx] = v;
    }
    __syncthreads();
    const int x = tile_x + (int)tx, y = tile_y + (int)ty;
    if (x >= (int)p.dw || y >= (int)p.dh) return;
    // source texel (2 x - 2 + i, 2 y - 2 + j) = LDS (2 tx + i, 2 ty + j)
    const V3 r = bloom_down13([&](int i, int j) { return xyz(s_t[2u * ty + (uint32_t)j][2u * tx + (uint32_t)i]); }, FIRST && p.firefly != 0u);
    static_cast<float4*>(p.dst)[(size_t)y * p.dw + (size_t)x] = make_float4(r.x, r.y, r.z, 1.0f);
}
void launch_bloom_down(const BloomArgs& p, bool first, hipStream_t s) {
    const uint32_t blocks = ((p.dw + kBloomW - 1u) / kBloomW) * ((p.dh + kBloomH - 1u) / kBloomH);
    if (blocks == 0u) return;
    if (first) ST_KLAUNCH(k_bloom_down<true>, dim3(blocks), dim3(kBlockThreads), s, p);
    else ST_KLAUNCH(k_bloom_down<false>, dim3(blocks), dim3(kBlockThreads), s, p);
}

// ---- one level up, blended into the destination. LDS: (32 / 2 + 4) x (8 / 2 + 4) texels; texel (lx, ly) of it is source texel
// (tile_x / 2 - 2 + lx, tile_y / 2 - 2 + ly) (tile origins are even). COMPOSITE: the destination is the composed frame (`base`); the result
// goes through the display transform into `dst` in `format`; sw == 0 (no level fits the frame): the frame itself goes there.
template <bool COMPOSITE>
__global__ __launch_bounds__(kBlockThreads) void k_bloom_up(const BloomArgs p) {
    __shared__ float4 s_t[kBloomUpH][kBloomUpW];
    const uint32_t tiles_x = (p.dw + kBloomW - 1u) / kBloomW;
    const int tile_x = (int)((blockIdx.x % tiles_x) * kBloomW), tile_y = (int)((blockIdx.x / tiles_x) * kBloomH);
    const uint32_t t = threadIdx.x, tx = t % kBloomW, ty = t / kBloomW;
    const bool any = !COMPOSITE || p.sw != 0u;
    if (any && t < kBloomUpW * kBloomUpH) {
        const uint32_t lx = t % kBloomUpW, ly = t / kBloomUpW;
        const int sx = out_clampi(tile_x / 2 - 2 + (int)lx, (int)p.sw), sy = out_clampi(tile_y / 2 - 2 + (int)ly, (int)p.sh);
        s_t[ly][lx] = p.src[(size_t)sy * p.sw + (size_t)sx];
    }
    __syncthreads();
    const int x = tile_x + (int)tx, y = tile_y + (int)ty;
    if (x >= (int)p.dw || y >= (int)p.dh) return;
    const size_t at = (size_t)y * p.dw + (size_t)x;
    const float4 c4 = COMPOSITE ? p.base[at] : static_cast<const float4*>(p.dst)[at];
    V3 r = xyz(c4);
    if (any) {
        // texels i0 - 1 .. i0 + 2 with i0 = floor((x + 1) / 2) - 1: LDS columns ((tx + 1) >> 1) .. + 3
        const uint32_t bx = (tx + 1u) >> 1, by = (ty + 1u) >> 1;
        const V3 u = bloom_up9([&](int i, int j) { return xyz(s_t[by + (uint32_t)j][bx + (uint32_t)i]); }, (tx & 1u) ? 0.25f : 0.75f, (ty & 1u) ? 0.25f : 0.75f);
        r = bloom_blend(r, u, p.factor, p.additive != 0u);
    }
    if (COMPOSITE) store_output(p.dst, (uint32_t)at, display_transform(make_float4(r.x, r.y, r.z, 1.0f), p.display.tonemap, display_scale(p.display)), p.format);
    else static_cast<float4*>(p.dst)[at] = make_float4(r.x, r.y, r.z, 1.0f);
}
void launch_bloom_up(const BloomArgs& p, hipStream_t s) {
    const uint32_t blocks = ((p.dw + kBloomW - 1u) / kBloomW) * ((p.dh + kBloomH - 1u) / kBloomH);
    if (blocks != 0u) ST_KLAUNCH(k_bloom_up<false>, dim3(blocks), dim3(kBlockThreads), s, p);
}
void launch_bloom_composite(const BloomArgs& p, hipStream_t s) {
    const uint32_t blocks = ((p.dw + kBloomW - 1u) / kBloomW) * ((p.dh + kBloomH - 1u) / kBloomH);
    if (blocks != 0u) ST_KLAUNCH(k_bloom_up<true>, dim3(blocks), dim3(kBlockThreads), s, p);
}

// ---- the fused tail: ONE workgroup takes the pyramid from mip t - 1 (`base`, in device memory) down through its last levels and back up
// into mip t - 1, the levels t .. L - 1 living in LDS as three floats per texel, with a barrier between levels. It replaces 2 (L - t) launches
// of at most a few dozen workgroups each, whose cost is launch latency. Every pixel goes through bloom_down13 / bloom_up9 / bloom_blend like the
// tile kernels': the same bits.
constexpr uint32_t kBloomTailThreads = 1024u;   // the one workgroup is all the parallelism this launch has (its 244 B of scratch per lane is the argument struct, indexed by level)
struct BloomTailFetch {   // texel (x, y) of an LDS level, clamped
    const float* s; int w, h;
    ST_D V3 operator()(int x, int y) const { const float* q = s + 3 * (out_clampi(y, h) * w + out_clampi(x, w)); return v3(q[0], q[1], q[2]); }
};
__global__ __launch_bounds__(kBloomTailThreads) void k_bloom_tail(const BloomTailArgs p) {
    extern __shared__ __align__(16) float s_tail[];
    const uint32_t t = threadIdx.x;
    {   // mip t - 1 (device memory) -> level 0 of the tail
        const int w = (int)p.w[0], h = (int)p.h[0];
        for (int at = (int)t; at < w * h; at += (int)kBloomTailThreads) {
            const int x = at % w, y = at / w;
            const V3 r = bloom_down13([&](int i, int j) {
                return xyz(p.base[(size_t)out_clampi(2 * y - 2 + j, (int)p.bh) * p.bw + (size_t)out_clampi(2 * x - 2 + i, (int)p.bw)]); }, false);
            float* q = s_tail + p.off[0] + 3 * at;
            q[0] = r.x; q[1] = r.y; q[2] = r.z;
        }
    }
    __syncthreads();
    for (uint32_t k = 1; k < p.n; k++) {   // down inside LDS
        const BloomTailFetch src{s_tail + p.off[k - 1u], (int)p.w[k - 1u], (int)p.h[k - 1u]};
        const int w = (int)p.w[k], h = (int)p.h[k];
        for (int at = (int)t; at < w * h; at += (int)kBloomTailThreads) {
            const int x = at % w, y = at / w;
            const V3 r = bloom_down13([&](int i, int j) { return src(2 * x - 2 + i, 2 * y - 2 + j); }, false);
            float* q = s_tail + p.off[k] + 3 * at;
            q[0] = r.x; q[1] = r.y; q[2] = r.z;
        }
        __syncthreads();
    }
    for (uint32_t k = p.n; k-- > 1u;) {   // back up inside LDS: level k into level k - 1, every thread its own pixels
        const BloomTailFetch src{s_tail + p.off[k], (int)p.w[k], (int)p.h[k]};
        const int w = (int)p.w[k - 1u], h = (int)p.h[k - 1u];
        for (int at = (int)t; at < w * h; at += (int)kBloomTailThreads) {
            const int x = at % w, y = at / w, bx = ((x + 1) >> 1) - 2, by = ((y + 1) >> 1) - 2;
            const V3 u = bloom_up9([&](int i, int j) { return src(bx + i, by + j); }, (x & 1) ? 0.25f : 0.75f, (y & 1) ? 0.25f : 0.75f);
            float* q = s_tail + p.off[k - 1u] + 3 * at;
            const V3 r = bloom_blend(v3(q[0], q[1], q[2]), u, p.factor[k], p.additive != 0u);
            q[0] = r.x; q[1] = r.y; q[2] = r.z;
        }
        __syncthreads();
    }
    {   // level 0 of the tail into mip t - 1
        const BloomTailFetch src{s_tail + p.off[0], (int)p.w[0], (int)p.h[0]};
        const int w = (int)p.bw, h = (int)p.bh;
        for (int at = (int)t; at < w * h; at += (int)kBloomTailThreads) {
            const int x = at % w, y = at / w, bx = ((x + 1) >> 1) - 2, by = ((y + 1) >> 1) - 2;
            const V3 u = bloom_up9([&](int i, int j) { return src(bx + i, by + j); }, (x & 1) ? 0.25f : 0.75f, (y & 1) ? 0.25f : 0.75f);
            const V3 r = bloom_blend(xyz(p.base[at]), u, p.factor[0], p.additive != 0u);
            p.base[at] = make_float4(r.x, r.y, r.z, 1.0f);
        }
    }
}
// the LDS one workgroup of the tail may use on this device: what the runtime grants above the 64 KiB every kernel may have, up to a CU's 160 KiB
void launch_bloom_tail_limit(uint32_t* bytes) {
    static uint32_t limit = 0u;
    if (limit == 0u) {
        limit = 64u << 10;
        for (uint32_t want : {160u << 10, 128u << 10, 96u << 10}) {
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_bloom_tail), hipFuncAttributeMaxDynamicSharedMemorySize, (int)want) == hipSuccess) { limit = want; break; }
            (void)hipGetLastError();
        }
    }
    *bytes = limit;
}
void launch_bloom_tail(const BloomTailArgs& p, hipStream_t s) {
    if (p.n != 0u) ST_KLAUNCH_SMEM(k_bloom_tail, dim3(1), dim3(kBloomTailThreads), p.lds_bytes, s, p);
}

}  // namespace ST_KNS
}  // namespace st
