// k_post.hip — output post-processing (include/strolle_hip.h "post-processing"; st_post.cpp): FXAA over the display-referred colour and the
// resampler that writes the camera's output format. Both run behind the composing launch on the caller's stream, or on their own from
// st_post_process. tests/post_ref.py is the specification: everything here is float32, left to right, without FMA contraction and with
// correctly rounded division and square root in BOTH builds (plain `/` and sqrtf, like the display transform and the ray chain's exact
// islands), so that a branchy algorithm (edge or no edge, horizontal or vertical) cannot flip on an ulp between the builds or against numpy.
#include "k_common.h"
#include "k_output.h"

#pragma clang fp contract(off)

namespace st {
namespace ST_KNS {

ST_D float4 post_texel(const PostArgs& p, int x, int y) { return p.src[(size_t)out_clampi(y, (int)p.height) * p.width + (size_t)out_clampi(x, (int)p.width)]; }
ST_D float post_luma(float4 c) { return sqrtf(display_luma(post_unit(c.x), post_unit(c.y), post_unit(c.z))); }
ST_D float post_blend(float a, float b, float f) { return f == 0.0f ? a : a + (b - a) * f; }
ST_D float4 post_blend4(float4 a, float4 b, float f) { return make_float4(post_blend(a.x, b.x, f), post_blend(a.y, b.y, f), post_blend(a.z, b.z, f), 1.0f); }
// the texels i0, i0 + 1 and the fraction of a continuous position along one axis
ST_D void post_axis(float p, int* i0, float* f) { const float q = p - 0.5f, fl = floorf(q); *i0 = (int)fl; *f = q - fl; }

// bilinear look-ups at a continuous position: x first, then y; an axis with f == 0 takes the texel itself (and reads nothing else)
ST_D float4 post_bilinear(const PostArgs& p, int x0, float fx, int y0, float fy) {
    float4 top = post_texel(p, x0, y0);
    if (fx != 0.0f) top = post_blend4(top, post_texel(p, x0 + 1, y0), fx);
    if (fy == 0.0f) return top;
    float4 bot = post_texel(p, x0, y0 + 1);
    if (fx != 0.0f) bot = post_blend4(bot, post_texel(p, x0 + 1, y0 + 1), fx);
    return post_blend4(top, bot, fy);
}
ST_D float post_bilinear_luma(const PostArgs& p, float px, float py) {
    int x0, y0; float fx, fy;
    post_axis(px, &x0, &fx); post_axis(py, &y0, &fy);
    float top = post_luma(post_texel(p, x0, y0));
    if (fx != 0.0f) top = post_blend(top, post_luma(post_texel(p, x0 + 1, y0)), fx);
    if (fy == 0.0f) return top;
    float bot = post_luma(post_texel(p, x0, y0 + 1));
    if (fx != 0.0f) bot = post_blend(bot, post_luma(post_texel(p, x0 + 1, y0 + 1)), fx);
    return post_blend(top, bot, fy);
}

// ---- FXAA. A workgroup serves a 64 x 8 tile: a wave reads one row of 64 texels (1 KiB, one 16-B load per lane), every thread two pixels.
// The tile's luma with a one-texel halo sits in LDS. Pixels that fail the contrast test are stored at once from the registers that hold
// their colour: one colour read, five LDS reads, one write. The others are queued in LDS and served afterwards by dense lanes, so the
// divergent edge walk (look-ups up to 26.5 pixels along the edge, from global memory) stays out of the common path and of its registers.
constexpr uint32_t kFxaaW = 64u, kFxaaH = 8u, kFxaaLdsW = kFxaaW + 2u, kFxaaLdsH = kFxaaH + 2u, kFxaaHalo = 2u * kFxaaLdsW + 2u * kFxaaH;
__constant__ const float kFxaaWalk[12] = {1.0f, 2.0f, 3.0f, 4.0f, 5.0f, 6.5f, 8.5f, 10.5f, 12.5f, 14.5f, 18.5f, 26.5f};

ST_D void fxaa_edge_pixel(const PostArgs& p, const float (*s_l)[kFxaaLdsW], uint32_t lx, uint32_t ly, int x, int y) {
    const float M = s_l[ly][lx], N = s_l[ly - 1u][lx], S = s_l[ly + 1u][lx], E = s_l[ly][lx + 1u], W = s_l[ly][lx - 1u];
    const float NW = s_l[ly - 1u][lx - 1u], NE = s_l[ly - 1u][lx + 1u], SW = s_l[ly + 1u][lx - 1u], SE = s_l[ly + 1u][lx + 1u];
    const float mx = fmaxf(fmaxf(fmaxf(N, W), fmaxf(S, M)), E), mn = fminf(fminf(fminf(N, W), fminf(S, M)), E);
    const float range = mx - mn;
    const float eh = fabsf((NW + SW) - 2.0f * W) + 2.0f * fabsf((N + S) - 2.0f * M) + fabsf((NE + SE) - 2.0f * E);
    const float ev = fabsf((NW + NE) - 2.0f * N) + 2.0f * fabsf((W + E) - 2.0f * M) + fabsf((SW + SE) - 2.0f * S);
    const bool horz = eh >= ev;
    const float neg = horz ? N : W, pos = horz ? S : E;
    const float gn = fabsf(neg - M), gp = fabsf(pos - M);
    const bool pick_n = gn >= gp;
    const float gs = 0.25f * (pick_n ? gn : gp);
    const float A = 0.5f * ((pick_n ? neg : pos) + M);
    const float cx = (float)x + 0.5f, cy = (float)y + 0.5f;
    const float half = pick_n ? -0.5f : 0.5f;
    const float px = horz ? cx : cx + half, py = horz ? cy + half : cy;
    float dist_n = 26.5f, dist_p = 26.5f, delta_n = 0.0f, delta_p = 0.0f;
    bool done_n = false, done_p = false;
    for (int i = 0; i < 12 && !(done_n && done_p); i++) {
        const float d = kFxaaWalk[i];
        if (!done_n) {
            delta_n = post_bilinear_luma(p, horz ? px + -1.0f * d : px, horz ? py : py + -1.0f * d) - A;
            dist_n = d; done_n = fabsf(delta_n) >= gs;
        }
        if (!done_p) {
            delta_p = post_bilinear_luma(p, horz ? px + d : px, horz ? py : py + d) - A;
            dist_p = d; done_p = fabsf(delta_p) >= gs;
        }
    }
    const bool near_n = dist_n < dist_p;
    float off_edge = 0.5f - (near_n ? dist_n : dist_p) / (dist_n + dist_p);
    const bool good = ((near_n ? delta_n : delta_p) < 0.0f) != ((M - A) < 0.0f);
    if (!good) off_edge = 0.0f;
    float a = fabsf((((N + S) + (E + W)) * 2.0f + ((NW + NE) + (SW + SE))) / 12.0f - M) / range;
    a = a < 1.0f ? a : 1.0f;
    const float s = ((-2.0f * a + 3.0f) * a) * a;
    const float off_sub = (s * s) * p.subpixel;
    const float off = off_edge > off_sub ? off_edge : off_sub;
    const float sgn = pick_n ? -off : off;
    int x0, y0; float fx, fy;
    post_axis(horz ? cx : cx + sgn, &x0, &fx); post_axis(horz ? cy + sgn : cy, &y0, &fy);
    const float4 c = post_bilinear(p, x0, fx, y0, fy);
    store_output(p.dst, (uint32_t)y * p.width + (uint32_t)x, make_float4(c.x, c.y, c.z, 1.0f), p.format);
}

__global__ __launch_bounds__(kBlockThreads) void k_post_fxaa(const PostArgs p) {
    __shared__ float s_l[kFxaaLdsH][kFxaaLdsW];
    __shared__ uint16_t s_list[kFxaaW * kFxaaH];
    __shared__ uint32_t s_n;
    const uint32_t tiles_x = (p.width + kFxaaW - 1u) / kFxaaW;
    const int tile_x = (int)((blockIdx.x % tiles_x) * kFxaaW), tile_y = (int)((blockIdx.x / tiles_x) * kFxaaH);
    const uint32_t t = threadIdx.x, tx = t & 63u, ty = t >> 6;
    float4 c[2];
    for (uint32_t k = 0; k < 2u; k++) {   // out-of-image pixels of a partial tile read the clamped texel: what their in-image neighbours see there
        c[k] = post_texel(p, tile_x + (int)tx, tile_y + (int)(ty + 4u * k));
        s_l[ty + 4u * k + 1u][tx + 1u] = post_luma(c[k]);
    }
    if (t < kFxaaHalo) {   // the ring: the rows above and below (66 each), then the columns left and right (8 each)
        uint32_t lx, ly;
        if (t < 2u * kFxaaLdsW) { ly = t < kFxaaLdsW ? 0u : kFxaaLdsH - 1u; lx = t < kFxaaLdsW ? t : t - kFxaaLdsW; }
        else { const uint32_t r = t - 2u * kFxaaLdsW; lx = r < kFxaaH ? 0u : kFxaaLdsW - 1u; ly = 1u + (r < kFxaaH ? r : r - kFxaaH); }
        s_l[ly][lx] = post_luma(post_texel(p, tile_x + (int)lx - 1, tile_y + (int)ly - 1));
    }
    if (t == 0u) s_n = 0u;
    __syncthreads();
    for (uint32_t k = 0; k < 2u; k++) {
        const uint32_t lx = tx + 1u, ly = ty + 4u * k + 1u;
        const int x = tile_x + (int)tx, y = tile_y + (int)(ty + 4u * k);
        if (x >= (int)p.width || y >= (int)p.height) continue;
        const float M = s_l[ly][lx], N = s_l[ly - 1u][lx], S = s_l[ly + 1u][lx], E = s_l[ly][lx + 1u], W = s_l[ly][lx - 1u];
        const float mx = fmaxf(fmaxf(fmaxf(N, W), fmaxf(S, M)), E), mn = fminf(fminf(fminf(N, W), fminf(S, M)), E);
        if (mx - mn < fmaxf(p.edge_threshold_min, mx * p.edge_threshold)) store_output(p.dst, (uint32_t)y * p.width + (uint32_t)x, make_float4(c[k].x, c[k].y, c[k].z, 1.0f), p.format);
        else s_list[atomicAdd(&s_n, 1u)] = (uint16_t)((ty + 4u * k) * kFxaaW + tx);
    }
    __syncthreads();
    const uint32_t n = s_n;
    for (uint32_t i = t; i < n; i += (uint32_t)kBlockThreads) {
        const uint32_t e = s_list[i], ex = e % kFxaaW, ey = e / kFxaaW;
        fxaa_edge_pixel(p, s_l, ex + 1u, ey + 1u, tile_x + (int)ex, tile_y + (int)ey);
    }
}
void launch_post_fxaa(const PostArgs& p, hipStream_t s) {
    const uint32_t blocks = ((p.width + kFxaaW - 1u) / kFxaaW) * ((p.height + kFxaaH - 1u) / kFxaaH);
    if (blocks == 0u) return;
    ST_KLAUNCH(k_post_fxaa, dim3(blocks), dim3(kBlockThreads), s, p);
}

// ---- the resampler: one output pixel per thread, a workgroup a 64 x 4 tile of the output; writes the output format through store_output
// (st_passes.h: the composing kernels' own conversion). Positions are evaluated in integers (post_ref.axis_resample; k_output.h post_resample_axis).
struct CrWeights { float w0, w1, w2, w3; };
ST_D CrWeights post_cr_weights(float f) {
    CrWeights w;
    w.w0 = ((-0.5f * f + 1.0f) * f - 0.5f) * f;
    w.w1 = ((1.5f * f - 2.5f) * f) * f + 1.0f;
    w.w2 = ((-1.5f * f + 2.0f) * f + 0.5f) * f;
    w.w3 = ((0.5f * f - 0.5f) * f) * f;
    return w;
}
ST_D float post_cr1(float t0, float t1, float t2, float t3, const CrWeights& w, float f) { return f == 0.0f ? t1 : ((t0 * w.w0 + t1 * w.w1) + t2 * w.w2) + t3 * w.w3; }
ST_D float4 post_cr4(float4 t0, float4 t1, float4 t2, float4 t3, const CrWeights& w, float f) {
    return make_float4(post_cr1(t0.x, t1.x, t2.x, t3.x, w, f), post_cr1(t0.y, t1.y, t2.y, t3.y, w, f), post_cr1(t0.z, t1.z, t2.z, t3.z, w, f), 1.0f);
}

template <int FILTER>
__global__ __launch_bounds__(kBlockThreads) void k_post_resample(const PostArgs p) {
    const uint32_t tiles_x = (p.out_width + 63u) / 64u;
    const uint32_t ox = (blockIdx.x % tiles_x) * 64u + (threadIdx.x & 63u), oy = (blockIdx.x / tiles_x) * 4u + (threadIdx.x >> 6);
    if (ox >= p.out_width || oy >= p.out_height) return;
    float4 c;
    if (FILTER == 0) {
        c = post_texel(p, (int)(((2u * ox + 1u) * p.width) / (2u * p.out_width)), (int)(((2u * oy + 1u) * p.height) / (2u * p.out_height)));
    } else {
        int x0, y0; float fx, fy;
        post_resample_axis(ox, p.width, p.out_width, &x0, &fx);
        post_resample_axis(oy, p.height, p.out_height, &y0, &fy);
        if (FILTER == 1) c = post_bilinear(p, x0, fx, y0, fy);
        else if (fx == 0.0f && fy == 0.0f) c = post_texel(p, x0, y0);
        else {
            const CrWeights wx = post_cr_weights(fx), wy = post_cr_weights(fy);
            float4 row[4];
            for (int k = 0; k < 4; k++)
                row[k] = post_cr4(post_texel(p, x0 - 1, y0 - 1 + k), post_texel(p, x0, y0 - 1 + k), post_texel(p, x0 + 1, y0 - 1 + k), post_texel(p, x0 + 2, y0 - 1 + k), wx, fx);
            const float4 v = post_cr4(row[0], row[1], row[2], row[3], wy, fy);
            const float4 a = post_texel(p, x0, y0), b = post_texel(p, x0 + 1, y0), e = post_texel(p, x0, y0 + 1), g = post_texel(p, x0 + 1, y0 + 1);
            c = make_float4(post_box(v.x, a.x, b.x, e.x, g.x), post_box(v.y, a.y, b.y, e.y, g.y), post_box(v.z, a.z, b.z, e.z, g.z), 1.0f);
        }
    }
    store_output(p.dst, oy * p.out_width + ox, make_float4(c.x, c.y, c.z, 1.0f), p.format);
}
void launch_post_resample(const PostArgs& p, hipStream_t s) {
    const uint32_t blocks = ((p.out_width + 63u) / 64u) * ((p.out_height + 3u) / 4u);
    if (blocks == 0u) return;
    if (p.filter == 0u) ST_KLAUNCH(k_post_resample<0>, dim3(blocks), dim3(kBlockThreads), s, p);
    else if (p.filter == 1u) ST_KLAUNCH(k_post_resample<1>, dim3(blocks), dim3(kBlockThreads), s, p);
    else ST_KLAUNCH(k_post_resample<2>, dim3(blocks), dim3(kBlockThreads), s, p);
}

}  // namespace ST_KNS
}  // namespace st
