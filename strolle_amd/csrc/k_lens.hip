// k_lens.hip — lens effects (include/strolle_hip.h "lens effects"; st_lens.cpp): radial distortion, chromatic fringing, vignette and film
// grain in one launch between bloom and colour grading. With the distortion or the fringe step the pixel is a free-form gather: up to 16
// bilinear look-ups at source positions on the pixel's own radius; without them it is a pointwise pass. tests/lens_ref.py is the
// specification: everything here is float32, left to right, without FMA contraction and with correctly rounded division in BOTH builds,
// like k_fog.hip; there is no transcendental and the grain's hash is integer-only, so the two builds and numpy agree bit for bit.
#include "k_common.h"
#include "k_output.h"

#pragma clang fp contract(off)

namespace st {
namespace ST_KNS {

// A workgroup's pixels, as k_fog's: a wave is 32 x 2 pixels. A tap maps the wave's footprint to a scaled copy of itself, so at the scales
// a lens uses (0.7 .. 1.4) its bilinear look-ups touch three to four rows of about 33 texels: 15 to 20 128-B lines for 256 16-B loads,
// the same count a 16 x 4 footprint gives and fewer than 8 x 8's 18 — and the pointwise instantiation keeps fog's two 512-B runs.
constexpr uint32_t kLensW = 32u, kLensH = 8u;
static_assert(kLensW * kLensH == (uint32_t)kBlockThreads, "one pixel per thread");

// one PCG round (the header writes it out; st_engine.h seed_hash on the host)
ST_D uint32_t lens_hash(uint32_t v) {
    v = v * 747796405u + 2891336453u;
    const uint32_t w = ((v >> ((v >> 28) + 4u)) ^ v) * 277803737u;
    return (w >> 22) ^ w;
}

// The post-processing section's BILINEAR look-up of out_colour(texel) at the continuous position (px, py), indices clamped to the image.
// All four texels are read whatever the fractions: a clamped colour is finite and not negative, so a + (b - a) * 0 is a itself, which is
// the section's "an axis with f == 0 takes texel a" without a divergent branch around two loads. Positions are bounded by the
// descriptor's checks (|u| <= 8192, g <= 1.95 * 4 * fit, tap_scale <= 1.1), far inside int's range; the clamp keeps every index in the
// plane whatever the position is.
ST_D V3 lens_bilinear(const LensArgs& p, float px, float py) {
    const float qx = px - 0.5f, qy = py - 0.5f;
    const float bx = floorf(qx), by = floorf(qy);
    const float fx = qx - bx, fy = qy - by;
    const int ix = (int)bx, iy = (int)by, w = (int)p.width, h = (int)p.height;
    const size_t r0 = (size_t)out_clampi(iy, h) * p.width, r1 = (size_t)out_clampi(iy + 1, h) * p.width;
    const uint32_t x0 = (uint32_t)out_clampi(ix, w), x1 = (uint32_t)out_clampi(ix + 1, w);
    const V3 a = out_colour(p.color[r0 + x0]), b = out_colour(p.color[r0 + x1]), c = out_colour(p.color[r1 + x0]), d = out_colour(p.color[r1 + x1]);
    const float tx = a.x + (b.x - a.x) * fx, ty = a.y + (b.y - a.y) * fx, tz = a.z + (b.z - a.z) * fx;
    const float ux = c.x + (d.x - c.x) * fx, uy = c.y + (d.y - c.y) * fx, uz = c.z + (d.z - c.z) * fx;
    return v3(tx + (ux - tx) * fy, ty + (uy - ty) * fy, tz + (uz - tz) * fy);
}

// One workgroup per 32 x 8 pixels of the frame, row-major, one pixel per lane. GATHER: per tap four 16-B texel loads and twelve blends;
// the tap table arrives by value with the rest of the arguments and is read with scalar loads at the loop's uniform index. Without GATHER
// the kernel is fog's shape: one 16-B load, one store, no loop. The step branches are wave-uniform. No LDS, no atomics, no scratch.
template <bool GATHER>
__global__ __launch_bounds__(kBlockThreads) void k_lens(const LensArgs p) {
    const uint32_t groups_x = (p.width + kLensW - 1u) / kLensW;
    const uint32_t gx = blockIdx.x % groups_x, gy = blockIdx.x / groups_x;
    const uint32_t t = threadIdx.x, x = gx * kLensW + t % kLensW, y = gy * kLensH + t / kLensW;
    if (x >= p.width || y >= p.height) return;
    const size_t at = (size_t)y * p.width + x;
    const float u = ((float)x + 0.5f) - p.cx, v = ((float)y + 0.5f) - p.cy;
    const float r2 = (u * u + v * v) * p.inv_hd2;
    float o[3];
    if (GATHER) {
        float g = 1.0f;
        if (p.steps & kLensDistortion) g = ((p.k2 * r2 + p.k1) * r2 + 1.0f) * p.scale_eff;
        o[0] = o[1] = o[2] = 0.0f;
        for (uint32_t i = 0; i < p.taps; i++) {
            const float w0 = p.tap_weight[i][0], w1 = p.tap_weight[i][1], w2 = p.tap_weight[i][2];
            if (w0 == 0.0f && w1 == 0.0f && w2 == 0.0f) continue;
            const float s = g * p.tap_scale[i];
            const V3 c = lens_bilinear(p, u * s + p.cx, v * s + p.cy);
            o[0] = o[0] + c.x * w0; o[1] = o[1] + c.y * w1; o[2] = o[2] + c.z * w2;
        }
    } else {
        const float4 c = p.color[at];
        if (!(p.steps & (kLensVignette | kLensGrain))) { out_store(p, at, c); return; }   // every step neutral: the pixel's own four words
        const V3 cc = out_colour(c);
        o[0] = cc.x; o[1] = cc.y; o[2] = cc.z;
    }
    if (p.steps & kLensVignette) {
        float m = r2;
        if (!p.round) { const float a = u / p.cx, b = v / p.cy; m = (a * a + b * b) * 0.5f; }
        const float q = 1.0f + m * p.vignette_falloff;
        const float fall = 1.0f / (q * q);
        const float k = (1.0f - p.vignette_intensity) + p.vignette_intensity * fall;
#pragma unroll
        for (int i = 0; i < 3; i++) o[i] = o[i] * k;
    }
    if (p.steps & kLensGrain) {
        const uint32_t h = lens_hash(x / p.grain_size + lens_hash(y / p.grain_size + p.seed));
        const float eta = (((float)(h & 0xffffu) + (float)(h >> 16)) - 65535.0f) / 65536.0f;
        const float k = 1.0f + p.grain_intensity * eta;
#pragma unroll
        for (int i = 0; i < 3; i++) o[i] = o[i] * k;
    }
    out_store(p, at, make_float4(out_min(o[0], kColourMax), out_min(o[1], kColourMax), out_min(o[2], kColourMax), 1.0f));
}
void launch_lens(const LensArgs& p, hipStream_t s) {
    if (p.width == 0u || p.height == 0u) return;
    const uint32_t blocks = ((p.width + kLensW - 1u) / kLensW) * ((p.height + kLensH - 1u) / kLensH);
    if ((p.steps & (kLensDistortion | kLensFringe)) || p.force_gather) ST_KLAUNCH(k_lens<true>, dim3(blocks), dim3(kBlockThreads), s, p);
    else ST_KLAUNCH(k_lens<false>, dim3(blocks), dim3(kBlockThreads), s, p);
}

}  // namespace ST_KNS
}  // namespace st
