// k_grade.hip — colour grading (include/strolle_hip.h "colour grading"; st_grade.cpp): one pointwise launch, the last HDR node. It grades
// the scene-referred colour (white balance, contrast, saturation), applies the camera's display transform, grades the display-referred
// result (ASC CDL, a 3-D look-up table read tetrahedrally, deband dither) and stores the target's format. tests/grade_ref.py is the
// specification: everything here is float32, left to right, without FMA contraction and with correctly rounded division in BOTH builds,
// like k_fog.hip; the only transcendentals are st_math.h's exp2_poly_ and log2_poly_ (never the hardware's v_exp_f32 / v_log_f32), so the
// two builds and numpy agree bit for bit.
#include "k_common.h"
#include "k_output.h"

#pragma clang fp contract(off)

namespace st {
namespace ST_KNS {

constexpr uint32_t kGradeW = 32u, kGradeH = 8u;   // a workgroup's pixels, as k_fog's: each wave reads two 512-B runs of colour
static_assert(kGradeW * kGradeH == (uint32_t)kBlockThreads, "one pixel per thread");

ST_D float grade_pow(float x, float p) { return x == 0.0f ? 0.0f : exp2_poly_(p * log2_poly_(x)); }
ST_D float grade_saturate(float v, float y, float s) { return out_max(y + (v - y) * s, 0.0f); }

// the LUT coordinate of one channel: u in [0, 1] -> (cell index, fraction)
ST_D void grade_cell(float u, uint32_t n, int& i, float& f) {
    const float p = u * (float)(n - 1u);
    i = (int)floorf(p);
    i = i > (int)n - 2 ? (int)n - 2 : (i < 0 ? 0 : i);
    f = p - (float)i;
}

// One workgroup per 32 x 8 pixels of the window, row-major. Per pixel one 16-B colour load and one store; with a LUT four 16-B corner loads
// from a table that stays in L2 (33^3 float4 = 575 KB). Everything else arrives by value and is wave-uniform, so the step branches do not
// diverge; LUT picks the instantiation, so a frame without a table carries no corner loads and none of their registers. No LDS, no
// atomics, no scratch.
template <bool LUT>
__global__ __launch_bounds__(kBlockThreads) void k_grade(const GradeArgs p) {
    const uint32_t groups_x = (p.col1 - p.col0 + kGradeW - 1u) / kGradeW;
    const uint32_t gx = blockIdx.x % groups_x, gy = blockIdx.x / groups_x;
    const uint32_t t = threadIdx.x, x = p.col0 + gx * kGradeW + t % kGradeW, y = p.row0 + gy * kGradeH + t / kGradeW;
    if (x >= p.col1 || y >= p.row1) return;
    const size_t at = (size_t)y * p.width + x;
    float4 c = p.color[at];
    // A. scene-referred
    if (p.steps & kGradeStageA) {
        const V3 v0 = out_colour(c);
        float v[3] = {v0.x, v0.y, v0.z};
        if (p.steps & kGradeWhiteBalance) {
            const float r = v[0], g = v[1], b = v[2];
#pragma unroll
            for (int k = 0; k < 3; k++) v[k] = out_max((p.M[3 * k] * r + p.M[3 * k + 1] * g) + p.M[3 * k + 2] * b, 0.0f);
        }
        if (p.steps & kGradeContrast) {
#pragma unroll
            for (int k = 0; k < 3; k++) v[k] = 0.18f * grade_pow(v[k] / 0.18f, p.contrast);
        }
        if (p.steps & kGradeSaturation) {
            const float l = display_luma(v[0], v[1], v[2]);
#pragma unroll
            for (int k = 0; k < 3; k++) v[k] = grade_saturate(v[k], l, p.saturation);
        }
        c = make_float4(out_min(v[0], kColourMax), out_min(v[1], kColourMax), out_min(v[2], kColourMax), 1.0f);
    }
    // B. the display transform, as out_store applies it
    if (p.display.on) c = display_transform(c, p.display.tonemap, display_scale(p.display));
    // C. display-referred
    if (p.steps & (kGradeCdl | kGradeLut | kGradeDither)) {
        float v[3] = {c.x, c.y, c.z};
        if (p.steps & kGradeCdl) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                v[k] = out_max(v[k] * p.slope[k] + p.offset[k], 0.0f);
                if (p.cdl_pow & (1u << k)) v[k] = grade_pow(v[k], p.power[k]);
            }
            if (p.cdl_sat_on) {
                const float l = display_luma(v[0], v[1], v[2]);
#pragma unroll
                for (int k = 0; k < 3; k++) v[k] = grade_saturate(v[k], l, p.cdl_saturation);
            }
        }
        if (LUT) {
            const uint32_t n = p.lut_n;
            int i[3]; float f[3];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                float u;
                if (p.lut_log2) u = v[k] > 0.0f ? out_clamp01((log2_poly_(v[k]) - p.ev_min) * p.inv_range) : 0.0f;
                else u = out_clamp01(v[k]);
                grade_cell(u, n, i[k], f[k]);
            }
            // the axes by descending fraction, ties in the order r, g, b: a, b, c
            int a, b, cc;
            if (f[0] >= f[1]) {
                if (f[1] >= f[2]) { a = 0; b = 1; cc = 2; } else if (f[0] >= f[2]) { a = 0; b = 2; cc = 1; } else { a = 2; b = 0; cc = 1; }
            } else {
                if (f[0] >= f[2]) { a = 1; b = 0; cc = 2; } else if (f[1] >= f[2]) { a = 1; b = 2; cc = 0; } else { a = 2; b = 1; cc = 0; }
            }
            const uint32_t stride[3] = {1u, n, n * n};
            const uint32_t i0 = ((uint32_t)i[2] * n + (uint32_t)i[1]) * n + (uint32_t)i[0];
            const uint32_t sa = a == 0 ? stride[0] : (a == 1 ? stride[1] : stride[2]), sb = b == 0 ? stride[0] : (b == 1 ? stride[1] : stride[2]);
            const float fa = a == 0 ? f[0] : (a == 1 ? f[1] : f[2]), fb = b == 0 ? f[0] : (b == 1 ? f[1] : f[2]), fc = cc == 0 ? f[0] : (cc == 1 ? f[1] : f[2]);
            const float4 t0 = p.lut[i0], t1 = p.lut[i0 + sa], t2 = p.lut[i0 + sa + sb], t3 = p.lut[i0 + stride[0] + stride[1] + stride[2]];
            const float w0 = 1.0f - fa, w1 = fa - fb, w2 = fb - fc;
            const float L[3] = {((t0.x * w0 + t1.x * w1) + t2.x * w2) + t3.x * fc, ((t0.y * w0 + t1.y * w1) + t2.y * w2) + t3.y * fc,
                                ((t0.z * w0 + t1.z * w1) + t2.z * w2) + t3.z * fc};
#pragma unroll
            for (int k = 0; k < 3; k++) v[k] = p.lut_blend ? v[k] + (L[k] - v[k]) * p.lut_strength : L[k];
        }
        if (p.steps & kGradeDither) {
            const float d = (float)(int)(171u * x + 231u * y);
            const float q[3] = {103.0f, 71.0f, 97.0f};
#pragma unroll
            for (int k = 0; k < 3; k++) {
                float tt = d / q[k];
                tt = tt - floorf(tt);
                const float delta = (tt - 0.5f) / 255.0f;
                v[k] = grade_pow(out_max(grade_pow(out_max(v[k], 0.0f), 0.45454545454545453f) + delta, 0.0f), 2.2f);
            }
        }
        c = make_float4(v[0], v[1], v[2], 1.0f);
    }
    if (p.raw) static_cast<float4*>(p.dst)[at] = c;
    else store_output(p.dst, (uint32_t)at, c, p.format);
}
void launch_grade(const GradeArgs& p, hipStream_t s) {
    if (p.col1 <= p.col0 || p.row1 <= p.row0) return;
    const uint32_t blocks = ((p.col1 - p.col0 + kGradeW - 1u) / kGradeW) * ((p.row1 - p.row0 + kGradeH - 1u) / kGradeH);
    if ((p.steps & kGradeLut) && p.lut && p.lut_n >= 2u) ST_KLAUNCH(k_grade<true>, dim3(blocks), dim3(kBlockThreads), s, p);
    else ST_KLAUNCH(k_grade<false>, dim3(blocks), dim3(kBlockThreads), s, p);
}

}  // namespace ST_KNS
}  // namespace st
