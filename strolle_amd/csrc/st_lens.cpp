// st_lens.cpp — lens effects (include/strolle_hip.h "lens effects"): the setter's checks, the host constants (st_lens_plan: the frame's
// centre, the tap table of the fringe, the fit that keeps every tap inside the frame, which steps run) and the one launch (k_lens.hip)
// that st_render_camera and st_lens_process share. The camera's HDR plane: st_engine.h CameraState::lens. The node needs no scratch: the
// stateless call allocates nothing. The plan is pure host arithmetic in double over this file alone.
#include <cmath>

#include "st_engine.h"

namespace st {

static_assert(KS_COUNT <= ST_PROFILE_MAX_KERNELS, "st_profile_read's callers size their arrays with ST_PROFILE_MAX_KERNELS");
static_assert(sizeof(StLensDesc) == 48, "StLensDesc is 48 B");
static_assert(offsetof(StLensDesc, k1) == 8 && offsetof(StLensDesc, scale) == 16 && offsetof(StLensDesc, fringe) == 20 && offsetof(StLensDesc, fringe_taps) == 24 &&
              offsetof(StLensDesc, vignette_intensity) == 28 && offsetof(StLensDesc, grain_intensity) == 36 && offsetof(StLensDesc, grain_size) == 40 &&
              offsetof(StLensDesc, grain_seed) == 44, "StLensDesc's fields are twelve 4-B words: no implicit padding");
static_assert(sizeof(StLensPlan) == 284 && offsetof(StLensPlan, cx) == 8 && offsetof(StLensPlan, fit) == 20 && offsetof(StLensPlan, tap_scale) == 28 &&
              offsetof(StLensPlan, tap_weight) == 92, "StLensPlan is 71 4-B words");
static_assert(kLensDistortion == ST_LENS_STEP_DISTORTION && kLensFringe == ST_LENS_STEP_FRINGE && kLensVignette == ST_LENS_STEP_VIGNETTE && kLensGrain == ST_LENS_STEP_GRAIN &&
              kLensMaxTaps == ST_LENS_MAX_TAPS, "st_types.h restates ST_LENS_STEP_* and ST_LENS_MAX_TAPS");

static bool within(float x, float lo, float hi) { return x >= lo && x <= hi; }   // (NaN: false)

static int check_lens(const StLensDesc& d) {
    if (d.struct_size != sizeof(StLensDesc)) return fail(ST_ERR_INVALID_ARGUMENT, "StLensDesc.struct_size is not sizeof(StLensDesc)");
    if ((d.flags & ~(uint32_t)(ST_LENS_FIT | ST_LENS_VIGNETTE_ROUND | ST_LENS_GRAIN_ANIMATE)) != 0u) return fail(ST_ERR_INVALID_ARGUMENT, "unknown lens flag bits");
    if (!finite(d.k1) || !finite(d.k2) || !(3.0 * std::fabs((double)d.k1) + 5.0 * std::fabs((double)d.k2) <= 0.95))
        return fail(ST_ERR_INVALID_ARGUMENT, "k1 and k2 must be finite with 3 |k1| + 5 |k2| <= 0.95 (the radial map must not fold over)");
    if (!within(d.scale, 0.25f, 4.0f)) return fail(ST_ERR_INVALID_ARGUMENT, "scale must be in [0.25, 4]");
    if (!within(d.fringe, 0.0f, 0.1f)) return fail(ST_ERR_INVALID_ARGUMENT, "fringe must be in [0, 0.1]");
    if (d.fringe != 0.0f && (d.fringe_taps < 3u || d.fringe_taps > (uint32_t)ST_LENS_MAX_TAPS)) return fail(ST_ERR_INVALID_ARGUMENT, "fringe_taps must be in 3..16 when fringe is not 0");
    if (!within(d.vignette_intensity, 0.0f, 1.0f)) return fail(ST_ERR_INVALID_ARGUMENT, "vignette_intensity must be in [0, 1]");
    if (d.vignette_intensity != 0.0f && !positive_finite(d.vignette_falloff)) return fail(ST_ERR_INVALID_ARGUMENT, "vignette_falloff must be finite and above 0 when the intensity is not 0");
    if (!(d.grain_intensity >= 0.0f && d.grain_intensity < 1.0f)) return fail(ST_ERR_INVALID_ARGUMENT, "grain_intensity must be in [0, 1)");
    if (d.grain_intensity != 0.0f && (d.grain_size < 1u || d.grain_size > 8u)) return fail(ST_ERR_INVALID_ARGUMENT, "grain_size must be in 1..8 when the intensity is not 0");
    return ST_OK;
}

// a double rounded to float towards zero (the fit must not leave the frame by its own rounding)
static float round_towards_zero(double x) {
    float f = (float)x;
    if ((double)f > x) f = std::nextafter(f, 0.0f);
    return f;
}

// The host constants, in double, each rounded to float once (the header's "host constants")
int Engine::lens_plan(const StLensDesc& d, uint32_t w, uint32_t h, StLensPlan& out) {
    if (int rc = check_lens(d)) return rc;
    if (w == 0u || h == 0u || w > kMaxImageSide || h > kMaxImageSide) return fail(ST_ERR_INVALID_ARGUMENT, "the image's sides must be in 1..16384");
    out = StLensPlan{};
    const double cx = 0.5 * (double)w, cy = 0.5 * (double)h, inv_hd2 = 1.0 / (cx * cx + cy * cy);
    out.cx = (float)cx; out.cy = (float)cy; out.inv_hd2 = (float)inv_hd2;
    // the tap table: one centre tap, or fringe_taps taps spread over [1 - fringe, 1 + fringe] under three spectral tents, each tent normalised
    double t_max = 1.0;
    if (d.fringe != 0.0f) {
        const uint32_t n = d.fringe_taps;
        double tent[ST_LENS_MAX_TAPS][3], sum[3] = {0.0, 0.0, 0.0};
        for (uint32_t i = 0; i < n; i++) {
            const double t = (double)i / (double)(n - 1u);
            out.tap_scale[i] = (float)(1.0 + (double)d.fringe * (2.0 * t - 1.0));
            tent[i][0] = std::max(1.0 - 2.0 * t, 0.0); tent[i][1] = 1.0 - std::fabs(2.0 * t - 1.0); tent[i][2] = std::max(2.0 * t - 1.0, 0.0);
            for (int k = 0; k < 3; k++) sum[k] += tent[i][k];
            t_max = std::max(t_max, (double)out.tap_scale[i]);
        }
        for (uint32_t i = 0; i < n; i++) for (int k = 0; k < 3; k++) out.tap_weight[i][k] = (float)(tent[i][k] / sum[k]);
        out.taps = n; out.steps |= kLensFringe;
    } else {
        out.taps = 1u; out.tap_scale[0] = 1.0f;
        out.tap_weight[0][0] = out.tap_weight[0][1] = out.tap_weight[0][2] = 1.0f;
    }
    // the fit: the largest factor on `scale` at which the outermost tap of every border pixel still lands in [0, W] x [0, H]. The bound on
    // k1, k2 makes u f(r2) grow with |u| along a row (and v f likewise along a column), so the border pixels bind
    out.fit = 1.0f;
    if (d.flags & ST_LENS_FIT) {
        double fit = HUGE_VAL;
        auto pixel = [&](uint32_t x, uint32_t y) {
            const double u = ((double)x + 0.5) - cx, v = ((double)y + 0.5) - cy;
            const double r2 = (u * u + v * v) * inv_hd2, g = (((double)d.k2 * r2 + (double)d.k1) * r2 + 1.0) * (double)d.scale * t_max;
            if (u != 0.0) fit = std::min(fit, cx / (std::fabs(u) * g));
            if (v != 0.0) fit = std::min(fit, cy / (std::fabs(v) * g));
        };
        for (uint32_t x = 0; x < w; x++) { pixel(x, 0u); pixel(x, h - 1u); }
        for (uint32_t y = 0; y < h; y++) { pixel(0u, y); pixel(w - 1u, y); }
        if (fit != HUGE_VAL) out.fit = round_towards_zero(fit);   // (a 1 x 1 frame constrains nothing)
    }
    out.scale_eff = (float)((double)d.scale * (double)out.fit);
    if (d.k1 != 0.0f || d.k2 != 0.0f || out.scale_eff != 1.0f) out.steps |= kLensDistortion;
    if (d.vignette_intensity != 0.0f) out.steps |= kLensVignette;
    if (d.grain_intensity != 0.0f) out.steps |= kLensGrain;
    return ST_OK;
}

int Engine::set_lens(CameraState& c, const StLensDesc* desc) { return set_node(c.windowed(), c.lens, desc, check_lens); }

// The launch's arguments over the whole frame. Compulsory bytes per pixel: 16 B of colour in — every texel is needed once, however many
// taps read it — and the format's bytes out.
void Engine::lens_step(const StLensDesc& d, const StLensPlan& plan, const NodeSource& src, uint32_t frame, bool force_gather, const NodeTarget& target, LensStep& out) {
    LensArgs& a = out.args;
    a = LensArgs{};
    a.color = static_cast<const float4*>(src.color);
    a.width = src.w; a.height = src.h;
    apply_target(target, a);
    a.steps = plan.steps; a.taps = plan.taps <= kLensMaxTaps ? plan.taps : kLensMaxTaps; a.force_gather = force_gather ? 1u : 0u;
    a.round = (d.flags & ST_LENS_VIGNETTE_ROUND) ? 1u : 0u;
    a.grain_size = d.grain_size ? d.grain_size : 1u;
    a.seed = d.grain_seed + ((d.flags & ST_LENS_GRAIN_ANIMATE) ? frame : 0u);
    a.cx = plan.cx; a.cy = plan.cy; a.inv_hd2 = plan.inv_hd2; a.k1 = d.k1; a.k2 = d.k2; a.scale_eff = plan.scale_eff;
    a.vignette_intensity = d.vignette_intensity; a.vignette_falloff = d.vignette_falloff; a.grain_intensity = d.grain_intensity;
    for (uint32_t i = 0; i < kLensMaxTaps; i++) { a.tap_scale[i] = plan.tap_scale[i]; for (int k = 0; k < 3; k++) a.tap_weight[i][k] = plan.tap_weight[i][k]; }
    out.step = {KS_LENS, (double)src.w * (double)src.h * (16.0 + format_bytes(a.format))};
}

int Engine::lens_process(const StLensDesc* desc, const StDisplayDesc* display, const void* src, uint32_t w, uint32_t h, void* dst, int format, hipStream_t stream) {
    if (!desc || !src || !dst) return fail(ST_ERR_INVALID_ARGUMENT, "null argument");
    StLensPlan plan;
    if (int rc = lens_plan(*desc, w, h, plan)) return rc;
    if (desc->flags & ST_LENS_GRAIN_ANIMATE) return fail(ST_ERR_INVALID_ARGUMENT, "st_lens_process does not take ST_LENS_GRAIN_ANIMATE: the frame counter is a camera's state");
    NodeTarget target;
    if (int rc = process_target("st_lens_process", display, dst, format, target)) return rc;
    if (!has_device) return fail(ST_ERR_NO_DEVICE, "st_lens_process on a host-only engine");
    ST_HIP(hipSetDevice(device));
    LensStep step;
    lens_step(*desc, plan, {src, nullptr, nullptr, false, w, h}, 0u, lens_force_gather, target, step);
    L.launch_lens(step.args, stream);
    ST_HIP(hipGetLastError());
    return ST_OK;
}

}  // namespace st
