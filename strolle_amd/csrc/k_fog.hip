// k_fog.hip — distance and height fog (include/strolle_hip.h "fog"; st_fog.cpp): one pointwise launch in front of depth of field. It turns the
// composed HDR colour and the distance along the pixel's ray into the colour behind a homogeneous or height-stratified medium, with an
// optional glow towards a directional light. tests/fog_ref.py is the specification: everything here is float32, left to right, without FMA
// contraction and with correctly rounded division and square root in BOTH builds, like k_dof.hip; the only transcendentals are st_math.h's
// exp2_poly_ and log2_poly_ (never the hardware's v_exp_f32 / v_log_f32), so the two builds and numpy agree bit for bit.
#include "k_common.h"
#include "k_output.h"

#pragma clang fp contract(off)

namespace st {
namespace ST_KNS {

constexpr uint32_t kFogW = 32u, kFogH = 8u;   // a workgroup's pixels: each wave reads two 512-B runs of colour, consecutive workgroups consecutive runs
static_assert(kFogW * kFogH == (uint32_t)kBlockThreads, "one pixel per thread");

ST_D float fog_pow(float s, float p) { return s == 0.0f ? 0.0f : exp2_poly_(p * log2_poly_(s)); }

// One workgroup per 32 x 8 pixels of the window, row-major: consecutive workgroups stream consecutive 512-B runs of the same eight rows.
// Per pixel one 16-B colour load, one 4-B depth read and one store; everything else arrives by value and is wave-uniform, so the falloff,
// height, lobe and sky branches do not diverge. No LDS, no atomics, no scratch.
template <bool FRAME>
__global__ __launch_bounds__(kBlockThreads) void k_fog(const FogArgs p) {
    const uint32_t groups_x = (p.col1 - p.col0 + kFogW - 1u) / kFogW;
    const uint32_t gx = blockIdx.x % groups_x, gy = blockIdx.x / groups_x;
    const uint32_t t = threadIdx.x, x = p.col0 + gx * kFogW + t % kFogW, y = p.row0 + gy * kFogH + t / kFogW;
    if (x >= p.col1 || y >= p.row1) return;
    const size_t at = (size_t)y * p.width + x;
    const float4 cx = p.color[at];
    const float D = out_frame_depth(p.depth, at, FRAME);
    // 2. distance
    if (!(D > 0.0f)) { out_store(p, at, cx); return; }
    float d = D;
    if (D >= kFltMax) {
        if (!p.sky) { out_store(p, at, cx); return; }
        d = p.sky_distance;
    }
    // 1. ray
    float wx = 0.0f, wy = 0.0f, wz = 0.0f;
    if (p.height_on || p.lobe_on) {
        const float ndc_x = ((float)x + 0.5f) * 2.0f / (float)p.width - 1.0f;
        const float ndc_y = -(((float)y + 0.5f) * 2.0f / (float)p.height - 1.0f);
        const float ax = (ndc_x + p.p8) / p.p0, ay = (ndc_y + p.p9) / p.p5;
        const float c = 1.0f / sqrtf((ax * ax + ay * ay) + 1.0f);
        const float vx = ax * c, vy = ay * c, vz = -c;
        wx = p.m0[0] * vx + p.m1[0] * vy + p.m2[0] * vz;
        wy = p.m0[1] * vx + p.m1[1] * vy + p.m2[1] * vz;
        wz = p.m0[2] * vx + p.m1[2] * vy + p.m2[2] * vz;
    }
    // 3. height
    float de = d;
    if (p.height_on) {
        const float k = out_min(out_max((p.b * wy) * d, -80.0f), 80.0f);
        const float G = fabsf(k) < 0.03125f ? 1.0f - k * (0.5f - k * 0.16666667f) : (1.0f - out_exp(-k)) / k;
        de = out_min(d * (p.E0 * G), kFltMax);
    }
    // 4. factors
    float ge[3], gi[3];
    if (p.falloff == 3u) {
#pragma unroll
        for (int i = 0; i < 3; i++) {
            ge[i] = (1.0f - out_exp(-(p.extinction[i] * de))) * p.a;
            gi[i] = (1.0f - out_exp(-(p.inscattering[i] * de))) * p.a;
        }
    } else {
        float g;
        if (p.falloff == 0u) g = out_min(out_max((de - p.start) / (p.end - p.start), 0.0f), 1.0f);
        else if (p.falloff == 1u) g = 1.0f - out_exp(-(p.density * de));
        else { const float u = p.density * de; g = 1.0f - out_exp(-(u * u)); }
        ge[0] = ge[1] = ge[2] = gi[0] = gi[1] = gi[2] = g * p.a;
    }
    if (ge[0] == 0.0f && ge[1] == 0.0f && ge[2] == 0.0f && gi[0] == 0.0f && gi[1] == 0.0f && gi[2] == 0.0f) { out_store(p, at, cx); return; }
    // 5. colour
    float F[3] = {p.rgb[0], p.rgb[1], p.rgb[2]};
    if (p.lobe_on) {
        const float s = out_min(out_max((wx * p.L[0] + wy * p.L[1]) + wz * p.L[2], 0.0f), 1.0f);
        const float lobe = fog_pow(s, p.light_exponent);
#pragma unroll
        for (int i = 0; i < 3; i++) F[i] = out_min(p.rgb[i] + p.light_color[i] * lobe, kFltMax);
    }
    const float c3[3] = {cx.x, cx.y, cx.z};
    float o[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const float cc = out_min(out_max(c3[i], 0.0f), kColourMax);
        o[i] = cc * (1.0f - ge[i]) + F[i] * gi[i];
    }
    out_store(p, at, make_float4(o[0], o[1], o[2], 1.0f));
}
void launch_fog(const FogArgs& p, hipStream_t s) {
    if (p.col1 <= p.col0 || p.row1 <= p.row0) return;
    const uint32_t blocks = ((p.col1 - p.col0 + kFogW - 1u) / kFogW) * ((p.row1 - p.row0 + kFogH - 1u) / kFogH);
    if (p.frame) ST_KLAUNCH(k_fog<true>, dim3(blocks), dim3(kBlockThreads), s, p);
    else ST_KLAUNCH(k_fog<false>, dim3(blocks), dim3(kBlockThreads), s, p);
}

}  // namespace ST_KNS
}  // namespace st
