// k_upscale.hip — the upscale stage (include/strolle_hip.h "upscaling"; st_upscale.cpp): the edge-adaptive upscaler and the contrast-adaptive
// sharpening step behind FXAA. tests/upscale_ref.py is the specification: everything here is float32, left to right, without FMA contraction
// and with correctly rounded division and square root in BOTH builds (plain `/` and sqrtf, like k_post.hip), so that the branches (the
// direction's threshold, the guards of the sharpening step) cannot flip on an ulp between the builds or against numpy. The two kernels that
// frames launch serve one output pixel per thread, a workgroup a 64 x 4 tile of the output, and write the output format through store_output;
// the fused form at the end is kept for measurement (DESIGN.md "The upscale stage": it loses to the two launches).
#include "k_common.h"
#include "k_output.h"

#pragma clang fp contract(off)

namespace st {
namespace ST_KNS {

struct Up3 { float r, g, b; };
ST_D Up3 up_texel(const UpscaleArgs& p, int x, int y) {   // a display-referred texel: clamped index, clamped colour
    const float4 c = p.src[(size_t)out_clampi(y, (int)p.height) * p.width + (size_t)out_clampi(x, (int)p.width)];
    return {post_unit(c.x), post_unit(c.y), post_unit(c.z)};
}
ST_D float up_luma(const Up3& c) { return 0.5f * c.b + (0.5f * c.r + c.g); }

// ---- the upscaler
// one arm pair of a stencil along one axis: p, q, r the lumas before, at and behind the centre
ST_D void up_arm(float p, float q, float r, float w, float& dir, float& len) {
    dir = dir + (r - p) * w;
    const float m = out_max(fabsf(r - q), fabsf(q - p));
    const float t = m > 0.0f ? out_min(fabsf(r - p) / m, 1.0f) : 0.0f;
    len = len + (t * t) * w;
}
struct UpKernel { float fx, fy, dx, dy, l2x, l2y, lob, clp; };
ST_D void up_tap(const UpKernel& k, const Up3& c, float tx, float ty, Up3& sum, float& wsum) {
    const float ox = tx - k.fx, oy = ty - k.fy;
    const float vx = (ox * k.dx + oy * k.dy) * k.l2x, vy = (-ox * k.dy + oy * k.dx) * k.l2y;
    const float d2 = out_min(vx * vx + vy * vy, k.clp);
    const float tb = 0.4f * d2 - 1.0f, wb = 1.5625f * (tb * tb) - 0.5625f, ta = k.lob * d2 - 1.0f;
    const float w = wb * (ta * ta);
    sum.r = sum.r + c.r * w; sum.g = sum.g + c.g * w; sum.b = sum.b + c.b * w;
    wsum = wsum + w;
}
ST_D Up3 up_pixel(const UpscaleArgs& p, uint32_t ox, uint32_t oy) {
    int x0, y0; UpKernel k;
    post_resample_axis(ox, p.width, p.out_width, &x0, &k.fx);
    post_resample_axis(oy, p.height, p.out_height, &y0, &k.fy);
    const Up3 b = up_texel(p, x0, y0 - 1), c = up_texel(p, x0 + 1, y0 - 1);
    const Up3 e = up_texel(p, x0 - 1, y0), f = up_texel(p, x0, y0), g = up_texel(p, x0 + 1, y0), h = up_texel(p, x0 + 2, y0);
    const Up3 i = up_texel(p, x0 - 1, y0 + 1), j = up_texel(p, x0, y0 + 1), kk = up_texel(p, x0 + 1, y0 + 1), l = up_texel(p, x0 + 2, y0 + 1);
    const Up3 n = up_texel(p, x0, y0 + 2), o = up_texel(p, x0 + 1, y0 + 2);
    const float bL = up_luma(b), cL = up_luma(c), eL = up_luma(e), fL = up_luma(f), gL = up_luma(g), hL = up_luma(h);
    const float iL = up_luma(i), jL = up_luma(j), kL = up_luma(kk), lL = up_luma(l), nL = up_luma(n), oL = up_luma(o);
    float dirx = 0.0f, diry = 0.0f, len = 0.0f;
    const float wf = (1.0f - k.fx) * (1.0f - k.fy), wg = k.fx * (1.0f - k.fy), wj = (1.0f - k.fx) * k.fy, wk = k.fx * k.fy;
    up_arm(eL, fL, gL, wf, dirx, len); up_arm(bL, fL, jL, wf, diry, len);
    up_arm(fL, gL, hL, wg, dirx, len); up_arm(cL, gL, kL, wg, diry, len);
    up_arm(iL, jL, kL, wj, dirx, len); up_arm(fL, jL, nL, wj, diry, len);
    up_arm(jL, kL, lL, wk, dirx, len); up_arm(gL, kL, oL, wk, diry, len);
    const float r2 = dirx * dirx + diry * diry;
    if (r2 < 1.0f / 32768.0f) { k.dx = 1.0f; k.dy = 0.0f; }
    else { const float s = sqrtf(r2); k.dx = dirx / s; k.dy = diry / s; }
    len = 0.5f * len;
    len = len * len;
    const float stretch = (k.dx * k.dx + k.dy * k.dy) / out_max(fabsf(k.dx), fabsf(k.dy));
    k.l2x = 1.0f + (stretch - 1.0f) * len;
    k.l2y = 1.0f - 0.5f * len;
    k.lob = 0.5f + ((0.25f - 0.04f) - 0.5f) * len;
    k.clp = 1.0f / k.lob;
    Up3 sum = {0.0f, 0.0f, 0.0f}; float wsum = 0.0f;
    up_tap(k, b, 0.0f, -1.0f, sum, wsum); up_tap(k, c, 1.0f, -1.0f, sum, wsum);
    up_tap(k, e, -1.0f, 0.0f, sum, wsum); up_tap(k, f, 0.0f, 0.0f, sum, wsum); up_tap(k, g, 1.0f, 0.0f, sum, wsum); up_tap(k, h, 2.0f, 0.0f, sum, wsum);
    up_tap(k, i, -1.0f, 1.0f, sum, wsum); up_tap(k, j, 0.0f, 1.0f, sum, wsum); up_tap(k, kk, 1.0f, 1.0f, sum, wsum); up_tap(k, l, 2.0f, 1.0f, sum, wsum);
    up_tap(k, n, 0.0f, 2.0f, sum, wsum); up_tap(k, o, 1.0f, 2.0f, sum, wsum);
    const bool ok = wsum > 0.0f;
    Up3 v;
    v.r = post_box(ok ? sum.r / wsum : f.r, f.r, g.r, j.r, kk.r);
    v.g = post_box(ok ? sum.g / wsum : f.g, f.g, g.g, j.g, kk.g);
    v.b = post_box(ok ? sum.b / wsum : f.b, f.b, g.b, j.b, kk.b);
    return v;
}

__global__ __launch_bounds__(kBlockThreads) void k_upscale(const UpscaleArgs p) {
    const uint32_t tiles_x = (p.out_width + 63u) / 64u;
    const uint32_t ox = (blockIdx.x % tiles_x) * 64u + (threadIdx.x & 63u), oy = (blockIdx.x / tiles_x) * 4u + (threadIdx.x >> 6);
    if (ox >= p.out_width || oy >= p.out_height) return;
    const Up3 v = up_pixel(p, ox, oy);
    store_output(p.dst, oy * p.out_width + ox, make_float4(v.r, v.g, v.b, 1.0f), p.format);
}
void launch_upscale(const UpscaleArgs& p, hipStream_t s) {
    const uint32_t blocks = ((p.out_width + 63u) / 64u) * ((p.out_height + 3u) / 4u);
    if (blocks == 0u) return;
    ST_KLAUNCH(k_upscale, dim3(blocks), dim3(kBlockThreads), s, p);
}

// ---- the sharpening step: e the pixel, b d f h its N W E S neighbours
ST_D float sharpen_lobe1(float b, float d, float e, float f, float h) {
    const float mn4 = out_min(out_min(out_min(b, d), f), h), mx4 = out_max(out_max(out_max(b, d), f), h);
    const float hit_min = mx4 == 0.0f ? 0.0f : out_min(mn4, e) / (4.0f * mx4);
    const float den = 4.0f * mn4 - 4.0f;
    const float hit_max = den == 0.0f ? 0.0f : (1.0f - out_max(mx4, e)) / den;
    return out_max(-hit_min, hit_max);
}
ST_D float sharpen1(float lobe, float b, float d, float e, float f, float h) { return ((((lobe * b + lobe * d) + lobe * h) + lobe * f) + e) / (4.0f * lobe + 1.0f); }
ST_D Up3 sharpen_pixel(const Up3& b, const Up3& d, const Up3& e, const Up3& f, const Up3& h, float sharpness, bool denoise) {
    const float lr = sharpen_lobe1(b.r, d.r, e.r, f.r, h.r), lg = sharpen_lobe1(b.g, d.g, e.g, f.g, h.g), lb = sharpen_lobe1(b.b, d.b, e.b, f.b, h.b);
    float lobe = out_max(-0.1875f, out_min(out_max(out_max(lr, lg), lb), 0.0f)) * sharpness;
    if (denoise) {
        const float bL = up_luma(b), dL = up_luma(d), fL = up_luma(f), hL = up_luma(h), eL = up_luma(e);
        const float range = out_max(out_max(out_max(out_max(bL, dL), fL), hL), eL) - out_min(out_min(out_min(out_min(bL, dL), fL), hL), eL);
        const float nz = range == 0.0f ? 0.0f : out_min(fabsf((((0.25f * bL + 0.25f * dL) + 0.25f * fL) + 0.25f * hL) - eL) / range, 1.0f);
        lobe = lobe * (1.0f - 0.5f * nz);
    }
    return {sharpen1(lobe, b.r, d.r, e.r, f.r, h.r), sharpen1(lobe, b.g, d.g, e.g, f.g, h.g), sharpen1(lobe, b.b, d.b, e.b, f.b, h.b)};
}

__global__ __launch_bounds__(kBlockThreads) void k_sharpen(const UpscaleArgs p) {
    const uint32_t tiles_x = (p.width + 63u) / 64u;
    const uint32_t x = (blockIdx.x % tiles_x) * 64u + (threadIdx.x & 63u), y = (blockIdx.x / tiles_x) * 4u + (threadIdx.x >> 6);
    if (x >= p.width || y >= p.height) return;
    const int ix = (int)x, iy = (int)y;
    const Up3 v = sharpen_pixel(up_texel(p, ix, iy - 1), up_texel(p, ix - 1, iy), up_texel(p, ix, iy), up_texel(p, ix + 1, iy), up_texel(p, ix, iy + 1),
                                p.sharpness, p.denoise != 0u);
    store_output(p.dst, y * p.width + x, make_float4(v.r, v.g, v.b, 1.0f), p.format);
}
void launch_sharpen(const UpscaleArgs& p, hipStream_t s) {
    const uint32_t blocks = ((p.width + 63u) / 64u) * ((p.height + 3u) / 4u);
    if (blocks == 0u) return;
    ST_KLAUNCH(k_sharpen, dim3(blocks), dim3(kBlockThreads), s, p);
}

// ---- both steps in one launch: a workgroup upscales its TW x TH output tile plus a one-pixel ring into LDS (three planes of floats) and
// sharpens from there — the output-size RGBA32F plane between the two launches is neither written nor read, the ring's pixels are computed
// again by the neighbouring workgroups. The per-pixel arithmetic is up_pixel and sharpen_pixel, as in the two launches: the same bits.
// A ring pixel outside the image is the upscaled pixel at the clamped position, which is what the sharpening launch reads there.
template <uint32_t TW, uint32_t TH>
__global__ __launch_bounds__(kBlockThreads) void k_upscale_sharpen(const UpscaleArgs p) {
    constexpr uint32_t LW = TW + 2u, LH = TH + 2u, N = LW * LH;
    __shared__ float s_r[N], s_g[N], s_b[N];
    const uint32_t tiles_x = (p.out_width + TW - 1u) / TW;
    const int tile_x = (int)((blockIdx.x % tiles_x) * TW), tile_y = (int)((blockIdx.x / tiles_x) * TH);
    for (uint32_t i = threadIdx.x; i < N; i += (uint32_t)kBlockThreads) {
        const int ox = out_clampi(tile_x + (int)(i % LW) - 1, (int)p.out_width), oy = out_clampi(tile_y + (int)(i / LW) - 1, (int)p.out_height);
        const Up3 v = up_pixel(p, (uint32_t)ox, (uint32_t)oy);
        s_r[i] = post_unit(v.r); s_g[i] = post_unit(v.g); s_b[i] = post_unit(v.b);   // (the identity on an upscaled colour: what the sharpening launch's look-up does)
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < TW * TH; i += (uint32_t)kBlockThreads) {
        const uint32_t x = (uint32_t)tile_x + i % TW, y = (uint32_t)tile_y + i / TW;
        if (x >= p.out_width || y >= p.out_height) continue;
        const uint32_t c = (i / TW + 1u) * LW + i % TW + 1u;
        auto at = [&](uint32_t k) { return Up3{s_r[k], s_g[k], s_b[k]}; };
        const Up3 v = sharpen_pixel(at(c - LW), at(c - 1u), at(c), at(c + 1u), at(c + LW), p.sharpness, p.denoise != 0u);
        store_output(p.dst, y * p.out_width + x, make_float4(v.r, v.g, v.b, 1.0f), p.format);
    }
}
template <uint32_t TW, uint32_t TH> static void launch_upscale_sharpen_tile(const UpscaleArgs& p, hipStream_t s) {
    const uint32_t blocks = ((p.out_width + TW - 1u) / TW) * ((p.out_height + TH - 1u) / TH);
    if (blocks == 0u) return;
    ST_KLAUNCH((k_upscale_sharpen<TW, TH>), dim3(blocks), dim3(kBlockThreads), s, p);
}
void launch_upscale_sharpen(const UpscaleArgs& p, uint32_t tile, hipStream_t s) {
    if (tile == 2u) launch_upscale_sharpen_tile<32u, 32u>(p, s);
    else if (tile == 3u) launch_upscale_sharpen_tile<64u, 16u>(p, s);
    else launch_upscale_sharpen_tile<64u, 8u>(p, s);
}

}  // namespace ST_KNS
}  // namespace st
