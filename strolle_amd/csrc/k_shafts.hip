// k_shafts.hip — light shafts (include/strolle_hip.h "light shafts"; st_shafts.cpp): shadowed single scattering along the primary ray, between
// fog and depth of field. Two launches. k_shafts_march is a tracing kernel: one lane per cell of divisor x divisor pixels, one 8 x 8-cell
// tile per wave, `steps` strata along the cell's ray, one any-hit walk (trace_any, the scene queries' and the renderer's shadow walk) per
// stratum and light whose radiance times phase is not all zero; it writes (S.rgb, d_c) per cell. k_shafts_apply is pointwise like k_fog:
// it brings S to the pixel (depth-aware bilinear at divisor 2) and adds it to the composed colour. tests/shafts_ref.py is the
// specification of this file's OWN arithmetic: float32, left to right, no FMA contraction, correctly rounded division and square root in
// BOTH builds, exp2_poly_ the only transcendental and the cone's arccosine polynomial restated here (st_math.h's goes to the hardware's
// square root in the fast build). The pragma stands behind the includes on purpose: the walk inlined from st_traverse.h stays compiled as
// k_query.hip compiles it, so a shadow ray's answer here is st_scene_occluded's for the same ray.
#include "k_common.h"
#include "k_output.h"

#pragma clang fp contract(off)

namespace st {
namespace ST_KNS {

constexpr uint32_t kShaftsW = 32u, kShaftsH = 8u;   // the apply launch's workgroup, as k_fog's
static_assert(kShaftsW * kShaftsH == (uint32_t)kBlockThreads, "one pixel per thread");
static_assert(sizeof(KArgs) + sizeof(ShaftsArgs) <= 4096u, "both structs travel as kernel arguments");

// glam's acos_approx (st_math.h glam_acos_approx), with the correctly rounded square root in both builds
ST_D float sh_acos(float v) {
    const float x = fabsf(v);
    float omx = 1.0f - x;
    if (omx < 0.0f) omx = 0.0f;
    const float root = sqrtf(omx);
    float r = ((((((-0.0012624911f * x + 0.0066700901f) * x - 0.0170881256f) * x + 0.0308918810f) * x - 0.0501743046f) * x + 0.0889789874f) * x - 0.2145988016f) * x + 1.5707963050f;
    r = r * root;
    return v >= 0.0f ? r : 3.14159265358979323846f - r;
}
// the ray through (fx, fy) in pixels: fog's step 1
ST_D void sh_ray(const ShaftsArgs& p, float fx, float fy, float* wx, float* wy, float* wz) {
    const float ndc_x = fx * 2.0f / (float)p.width - 1.0f;
    const float ndc_y = -(fy * 2.0f / (float)p.height - 1.0f);
    const float ax = (ndc_x + p.p8) / p.p0, ay = (ndc_y + p.p9) / p.p5;
    const float c = 1.0f / sqrtf((ax * ax + ay * ay) + 1.0f);
    const float vx = ax * c, vy = ay * c, vz = -c;
    *wx = p.m0[0] * vx + p.m1[0] * vy + p.m2[0] * vz;
    *wy = p.m0[1] * vx + p.m1[1] * vy + p.m2[1] * vz;
    *wz = p.m0[2] * vx + p.m1[2] * vy + p.m2[2] * vz;
}
ST_D float sh_phase(const ShaftsArgs& p, float c) {
    const float q = p.k2 - p.k3 * c;
    return p.k1 / (q * sqrtf(q));
}
// V of the StRay {o, t_max; d}: st_scene_occluded's answer (k_query.hip query_ray + trace_any)
template <class SE>
ST_D bool sh_occluded(const KArgs& a, float ox, float oy, float oz, float dx, float dy, float dz, float t_max, SE* stack) {
    if (!(t_max > 0.0f) || (dx == 0.0f && dy == 0.0f && dz == 0.0f)) return false;
    Ray ray = make_ray(v3(ox, oy, oz), v3(dx, dy, dz));
    ray.len = t_max;
    uint32_t used = 0u;
    return trace_any(a, ray, stack, &used);
}

// One lane per cell; KArgs::width x height is the CELL grid here (st_shafts.cpp), so resolve_gid deals 8 x 8-cell tiles to waves as it deals
// pixel tiles to them in every other tracing launch. `steps` is wave-uniform: every lane runs the same trip count. No scratch.
template <bool LDS_SCENE, class SE>
__global__ ST_KERNEL_BOUNDS void k_shafts_march(const KArgs a_in, const ShaftsArgs p) {
    ST_SCENE_PROLOGUE
    ST_STACK_LDS(SE, lds);
    U2 cell;
    if (!resolve_gid(a, false, &cell)) return;
    if (cell.x >= p.cells_w || cell.y >= p.cells_h) return;
    const uint32_t cx = cell.x, cy = cell.y, div = p.divisor;
    // the cell's depth
    float d_c = 0.0f; bool any = false;
    const bool take_max = ((cx + cy) & 1u) != 0u;
    for (uint32_t by = 0u; by < div; by++) for (uint32_t bx = 0u; bx < div; bx++) {
        const uint32_t x = cx * div + bx, y = cy * div + by;
        if (x >= p.width || y >= p.height) continue;
        const float D = out_frame_depth(p.depth, (size_t)y * p.width + x, p.frame);
        if (!(D > 0.0f)) continue;
        if (!any) d_c = D; else if (take_max ? D > d_c : D < d_c) d_c = D;
        any = true;
    }
    float4* out = p.cells + (size_t)cy * p.cells_w + cx;
    if (!any) { *out = make_float4(0.0f, 0.0f, 0.0f, 0.0f); return; }
    out->w = d_c;   // now: d_c is not carried through the walks
    float wx, wy, wz;
    sh_ray(p, (float)(cx * div) + 0.5f * (float)div, (float)(cy * div) + 0.5f * (float)div, &wx, &wy, &wz);
    const float d_end = out_min(d_c, p.max_distance);
    const float delta = d_end / (float)p.steps;
    const unsigned long long bayer = 0x5D7F91B36E4CA280ull;   // the 4 x 4 Bayer matrix {0 8 2 10 / 12 4 14 6 / 3 11 1 9 / 15 7 13 5}, as in k_motion_blur.hip
    const float j = ((float)((uint32_t)(bayer >> (16u * (cy & 3u) + 4u * (cx & 3u))) & 15u) + 0.5f) / 16.0f;
    // the sun's term does not depend on the sample: its phase is the one value carried (sun_color is wave-uniform)
    float sun_ph = 0.0f; bool sun_on = false;
    if (p.sun_on) {
        const float c = out_min(out_max((wx * p.L[0] + wy * p.L[1]) + wz * p.L[2], -1.0f), 1.0f);
        sun_ph = sh_phase(p, c);
        sun_on = !(p.sun_color[0] * sun_ph == 0.0f && p.sun_color[1] * sun_ph == 0.0f && p.sun_color[2] * sun_ph == 0.0f);
    }
    SE* const stack = lane_stack(a, lds);
    float S[3] = {0.0f, 0.0f, 0.0f};
    uint32_t rays = 0u;
    for (uint32_t k = 0u; k < p.steps; k++) {
        const float t = ((float)k + j) * delta;
        const float px = p.origin[0] + wx * t, py = p.origin[1] + wy * t, pz = p.origin[2] + wz * t;
        float A[3] = {0.0f, 0.0f, 0.0f};
        if (sun_on) {
            rays++;
            if (!sh_occluded(a, px, py, pz, p.L[0], p.L[1], p.L[2], kFltMax, stack)) { A[0] = A[0] + p.sun_color[0] * sun_ph; A[1] = A[1] + p.sun_color[1] * sun_ph; A[2] = A[2] + p.sun_color[2] * sun_ph; }
        }
        for (uint32_t li = 0u; li < p.light_count; li++) {
            const GpuLight l = light_get(a, p.lights[li]);
            const uint32_t kind = f2b(l.d2.x);
            if (kind == 0u) continue;
            const float vx = l.d0.x - px, vy = l.d0.y - py, vz = l.d0.z - pz;
            const float l2 = (vx * vx + vy * vy) + vz * vz;
            const float len = sqrtf(l2);
            if (!(len > l.d0.w)) continue;
            const float dx = vx / len, dy = vy / len, dz = vz / len;
            float f_angle = 1.0f;
            if (kind != 1u) {
                // Normal::decode without its final normalisation, which the angle's own division takes out again
                const float ex = l.d2.y * 2.0f - 1.0f, ey = l.d2.z * 2.0f - 1.0f;
                float nx = ex, ny = ey;
                const float nz = (1.0f - fabsf(ex)) - fabsf(ey);
                const float tt = out_max(-nz, 0.0f);
                nx = nx - copysignf(tt, nx); ny = ny - copysignf(tt, ny);
                const float ux = -vx, uy = -vy, uz = -vz;
                const float n2 = (nx * nx + ny * ny) + nz * nz;
                const float angle = sh_acos(((nx * ux + ny * uy) + nz * uz) / sqrtf(n2 * l2));
                const float r = angle / l.d2.w;
                f_angle = out_clamp01(1.0f - (r * r) * r);
            }
            float f_dist = 1.0f;
            if (l.d1.w != INFINITY) {
                const float inv_r2 = 1.0f / (l.d1.w * l.d1.w);
                const float factor = l2 * inv_r2;
                const float sm = out_clamp01(1.0f - factor * factor);
                f_dist = (sm * sm) / out_max(l2, 0.0001f);
            }
            float fe = f_angle * f_dist;
            if (p.light_extinction) fe = fe * out_exp(-(p.density * len));
            const float c = out_min(out_max((wx * dx + wy * dy) + wz * dz, -1.0f), 1.0f);
            const float ph = sh_phase(p, c);
            const float e0 = (l.d1.x * fe) * ph, e1 = (l.d1.y * fe) * ph, e2 = (l.d1.z * fe) * ph;
            if (e0 == 0.0f && e1 == 0.0f && e2 == 0.0f) continue;   // no ray: out of range, outside the cone, a black light
            rays++;
            if (!sh_occluded(a, px, py, pz, dx, dy, dz, len - l.d0.w, stack)) { A[0] = A[0] + e0; A[1] = A[1] + e1; A[2] = A[2] + e2; }
        }
        const float m = (out_exp(-(p.density * t)) * delta) * p.density;
#pragma unroll
        for (int i = 0; i < 3; i++) S[i] = S[i] + (m * p.scatter[i]) * A[i];
    }
    // held in [0, FLT_MAX]: the apply launch multiplies S by weights that may be 0
    out->x = out_min(out_max(S[0], 0.0f), kFltMax); out->y = out_min(out_max(S[1], 0.0f), kFltMax); out->z = out_min(out_max(S[2], 0.0f), kFltMax);
    if (p.count && rays) count_rays_many(a, rays, 0ull);
}
void launch_shafts_march(const KArgs& a, const ShaftsArgs& p, hipStream_t s) {
    if (p.cells_w == 0u || p.cells_h == 0u) return;
    ST_LAUNCH_TRACE(k_shafts_march, (), false, s, a, p);
}

// One workgroup per 32 x 8 pixels, row-major. Per pixel one 16-B colour load, one depth read, one (divisor 1) or four (divisor 2) 16-B cell
// reads that neighbours share, one store. No LDS, no atomics, no scratch.
__global__ __launch_bounds__(kBlockThreads) void k_shafts_apply(const ShaftsArgs p) {
    const uint32_t groups_x = (p.width + kShaftsW - 1u) / kShaftsW;
    const uint32_t gx = blockIdx.x % groups_x, gy = blockIdx.x / groups_x;
    const uint32_t t = threadIdx.x, x = gx * kShaftsW + t % kShaftsW, y = gy * kShaftsH + t / kShaftsW;
    if (x >= p.width || y >= p.height) return;
    const size_t at = (size_t)y * p.width + x;
    const float4 cx = p.color[at];
    const float D = out_frame_depth(p.depth, at, p.frame);
    if (!(D > 0.0f)) { out_store(p, at, cx); return; }
    float S[3] = {0.0f, 0.0f, 0.0f};
    if (p.divisor == 1u) {
        const float4 c = p.cells[at];
        S[0] = c.x; S[1] = c.y; S[2] = c.z;
    } else {
        const float d_p = out_min(D, p.max_distance);
        const float ux = ((float)x + 0.5f) * 0.5f - 0.5f, uy = ((float)y + 0.5f) * 0.5f - 0.5f;
        const float flx = floorf(ux), fly = floorf(uy);
        const float fx = ux - flx, fy = uy - fly;
        const int ix = (int)flx, iy = (int)fly;
        float total = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int qx = ix + (k & 1), qy = iy + (k >> 1);
            const uint32_t ccx = (uint32_t)(qx < 0 ? 0 : (qx >= (int)p.cells_w ? (int)p.cells_w - 1 : qx));
            const uint32_t ccy = (uint32_t)(qy < 0 ? 0 : (qy >= (int)p.cells_h ? (int)p.cells_h - 1 : qy));
            const float4 c = p.cells[(size_t)ccy * p.cells_w + ccx];
            if (!(c.w > 0.0f)) continue;   // an empty cell
            const float b = ((k & 1) ? fx : 1.0f - fx) * ((k >> 1) ? fy : 1.0f - fy);
            const float wgt = b * (1.0f / (0.001f + fabsf(out_min(c.w, p.max_distance) - d_p) / d_p));
            S[0] = S[0] + wgt * c.x; S[1] = S[1] + wgt * c.y; S[2] = S[2] + wgt * c.z;
            total = total + wgt;
        }
        if (total > 0.0f) { S[0] = S[0] / total; S[1] = S[1] / total; S[2] = S[2] / total; }
        else { S[0] = 0.0f; S[1] = 0.0f; S[2] = 0.0f; }
    }
    const float a0 = p.intensity * S[0], a1 = p.intensity * S[1], a2 = p.intensity * S[2];
    if (a0 == 0.0f && a1 == 0.0f && a2 == 0.0f) { out_store(p, at, cx); return; }
    out_store(p, at, make_float4(out_min(out_min(out_max(cx.x, 0.0f), kColourMax) + a0, kFltMax), out_min(out_min(out_max(cx.y, 0.0f), kColourMax) + a1, kFltMax),
                                out_min(out_min(out_max(cx.z, 0.0f), kColourMax) + a2, kFltMax), cx.w));
}
void launch_shafts_apply(const ShaftsArgs& p, hipStream_t s) {
    if (p.width == 0u || p.height == 0u) return;
    const uint32_t blocks = ((p.width + kShaftsW - 1u) / kShaftsW) * ((p.height + kShaftsH - 1u) / kShaftsH);
    ST_KLAUNCH(k_shafts_apply, dim3(blocks), dim3(kBlockThreads), s, p);
}

}  // namespace ST_KNS
}  // namespace st
