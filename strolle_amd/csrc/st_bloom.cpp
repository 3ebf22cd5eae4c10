// st_bloom.cpp — bloom (include/strolle_hip.h "bloom"): the setter's checks, the plan (level count, mip sizes, blend factors: host arithmetic
// that st_bloom_plan reports) and the chain of launches (k_bloom.hip) that st_render_camera and st_bloom_process share. The HDR plane and
// the pyramids: st_engine.h CameraState::bloom, Engine::bloom_scratch.
#include <cmath>

#include "st_engine.h"

namespace st {

static_assert(KS_COUNT <= ST_PROFILE_MAX_KERNELS, "st_profile_read's callers size their arrays with ST_PROFILE_MAX_KERNELS");
static_assert(sizeof(StBloomDesc) == 40, "StBloomDesc is 40 B");
static constexpr uint32_t kBloomMaxLevels = 8u, kBloomDefaultLevels = 6u;
static constexpr float kBloomDefaultClamp = 65504.0f;

static int check_bloom(const StBloomDesc& d) {
    if (d.struct_size != sizeof(StBloomDesc)) return fail(ST_ERR_INVALID_ARGUMENT, "StBloomDesc.struct_size is not sizeof(StBloomDesc)");
    if ((d.flags & ~(uint32_t)(ST_BLOOM_ADDITIVE | ST_BLOOM_FIREFLY_SUPPRESS)) != 0u) return fail(ST_ERR_INVALID_ARGUMENT, "unknown bloom flag bits");
    if (d.levels > kBloomMaxLevels) return fail(ST_ERR_INVALID_ARGUMENT, "bloom levels above 8");
    if (!std::isfinite(d.intensity) || d.intensity < 0.0f) return fail(ST_ERR_INVALID_ARGUMENT, "bloom intensity is negative or not finite");
    if (!(d.flags & ST_BLOOM_ADDITIVE) && d.intensity > 1.0f) return fail(ST_ERR_INVALID_ARGUMENT, "bloom intensity above 1 without ST_BLOOM_ADDITIVE");
    if (!(d.low_frequency_boost >= 0.0f && d.low_frequency_boost <= 1.0f)) return fail(ST_ERR_INVALID_ARGUMENT, "low_frequency_boost is outside [0, 1]");
    if (!(d.low_frequency_boost_curvature >= 0.0f && d.low_frequency_boost_curvature < 1.0f)) return fail(ST_ERR_INVALID_ARGUMENT, "low_frequency_boost_curvature is outside [0, 1)");
    if (!(d.high_pass_frequency > 0.0f && d.high_pass_frequency <= 1.0f)) return fail(ST_ERR_INVALID_ARGUMENT, "high_pass_frequency is outside (0, 1]");
    if (!std::isfinite(d.threshold) || d.threshold < 0.0f) return fail(ST_ERR_INVALID_ARGUMENT, "bloom threshold is negative or not finite");
    if (!(d.threshold_softness >= 0.0f && d.threshold_softness <= 1.0f)) return fail(ST_ERR_INVALID_ARGUMENT, "threshold_softness is outside [0, 1]");
    if (!std::isfinite(d.clamp) || d.clamp < 0.0f) return fail(ST_ERR_INVALID_ARGUMENT, "bloom clamp is negative or not finite");
    return ST_OK;
}

int Engine::bloom_plan(const StBloomDesc& d, uint32_t w, uint32_t h, BloomPlan& plan) {
    plan = BloomPlan();
    if (int rc = check_bloom(d)) return rc;
    if (w > kMaxImageSide || h > kMaxImageSide) return fail(ST_ERR_INVALID_ARGUMENT, "a frame side above 16384");
    const uint32_t wanted = d.levels ? d.levels : kBloomDefaultLevels;
    uint32_t mw = w, mh = h;
    while (plan.levels < wanted) {
        mw = (mw + 1u) / 2u; mh = (mh + 1u) / 2u;
        if (mw < 2u || mh < 2u) break;
        plan.w[plan.levels] = mw; plan.h[plan.levels] = mh;
        plan.offset[plan.levels] = plan.texels; plan.texels += (size_t)mw * mh;
        plan.levels++;
    }
    const double intensity = d.intensity, f = d.high_pass_frequency;
    for (uint32_t k = 0; k < plan.levels; k++) {
        const double x = (double)k / (double)std::max(plan.levels - 1u, 1u);
        double lf = (1.0 - std::pow(1.0 - x, 1.0 / (1.0 - (double)d.low_frequency_boost_curvature))) * (double)d.low_frequency_boost;
        if (!(d.flags & ST_BLOOM_ADDITIVE)) lf *= 1.0 - intensity;
        const double hp = 1.0 - std::min(std::max((x - f) / f, 0.0), 1.0);
        plan.factor[k] = (float)((intensity + lf) * hp);
    }
    return ST_OK;
}

int Engine::set_bloom(CameraState& c, const StBloomDesc* desc) {
    return set_node(c.windowed(), c.bloom, desc, check_bloom);
}

// The fused tail takes the levels t .. L - 1 whose mips, three floats per texel, fit `tail_lds_bytes` together; t >= 1 (mip t - 1 is its input and
// output in device memory; the frame and its prefilter stay with the first downsample).
uint32_t Engine::bloom_tail_first(const BloomPlan& plan, uint32_t tail_lds_bytes) {
    uint32_t t = plan.levels;
    size_t bytes = 0;
    while (t > 1u) {
        const size_t more = (size_t)plan.w[t - 1u] * plan.h[t - 1u] * 3u * sizeof(float);
        if (bytes + more > tail_lds_bytes) break;
        bytes += more; t--;
    }
    return t;
}
uint32_t Engine::bloom_tail_bytes() {
    if (bloom_tail_wanted == 0 || !has_device) return 0u;
    uint32_t limit = 0u;
    L.launch_bloom_tail_limit(&limit);
    return bloom_tail_wanted < 0 ? limit : std::min(limit, (uint32_t)bloom_tail_wanted);
}

// The straightforward chain: L downsamples (frame -> mip 0 -> .. -> mip L - 1), L - 1 upsamples (mip k into mip k - 1, k = L - 1 .. 1) and the
// composite. With a tail from level t: t downsamples, the tail (levels t .. L - 1 down and back up into mip t - 1), t - 1 upsamples, the composite.
// Compulsory bytes: every source texel read once, every destination pixel read (where it is blended) and written once.
Engine::BloomSteps Engine::bloom_steps(const StBloomDesc& d, const BloomPlan& plan, const void* src, uint32_t w, uint32_t h, float4* pyramid, const NodeTarget& target, uint32_t tail_lds_bytes) {
    BloomSteps s;
    BloomArgs base{};
    base.additive = (d.flags & ST_BLOOM_ADDITIVE) ? 1u : 0u;
    base.firefly = (d.flags & ST_BLOOM_FIREFLY_SUPPRESS) ? 1u : 0u;
    base.clamp = d.clamp != 0.0f ? d.clamp : kBloomDefaultClamp;
    base.threshold_on = d.threshold > 0.0f ? 1u : 0u;
    const float knee = d.threshold * d.threshold_softness;
    base.threshold = d.threshold; base.knee_lo = d.threshold - knee; base.knee2 = 2.0f * knee; base.knee_div = 4.0f * knee + 1e-4f;
    // a raw target (colour grading behind bloom reads the plane): the colour untransformed, which is this composite's store at NONE and scale 1 —
    // st_bloom_process without a display — into RGBA32F; the grade applies the display transform
    const uint32_t format = target.raw ? (uint32_t)ST_FORMAT_RGBA32F : target.format;
    base.display = target.display;
    if (target.raw) { base.display = DisplayArgs{}; base.display.scale = 1.0f; }
    const uint32_t L = plan.levels, T = bloom_tail_first(plan, tail_lds_bytes);
    for (uint32_t k = 0; k < T; k++) {
        BloomArgs a = base;
        a.src = k == 0u ? static_cast<const float4*>(src) : pyramid + plan.offset[k - 1u];
        a.sw = k == 0u ? w : plan.w[k - 1u]; a.sh = k == 0u ? h : plan.h[k - 1u];
        a.dst = pyramid + plan.offset[k]; a.dw = plan.w[k]; a.dh = plan.h[k];
        s.step[s.count++] = {{KS_BLOOM_DOWN, ((double)a.sw * a.sh + (double)a.dw * a.dh) * 16.0}, k == 0u, a, BloomTailArgs{}};
    }
    if (T < L) {
        BloomTailArgs t{};
        t.base = pyramid + plan.offset[T - 1u]; t.bw = plan.w[T - 1u]; t.bh = plan.h[T - 1u];
        t.n = L - T; t.additive = base.additive;
        uint32_t floats = 0u;
        for (uint32_t i = 0; i < t.n; i++) {
            t.w[i] = plan.w[T + i]; t.h[i] = plan.h[T + i]; t.factor[i] = plan.factor[T + i];
            t.off[i] = floats; floats += t.w[i] * t.h[i] * 3u;
        }
        t.lds_bytes = floats * (uint32_t)sizeof(float);
        s.step[s.count++] = {{KS_BLOOM_TAIL, (double)t.bw * t.bh * 48.0}, false, BloomArgs{}, t};   // mip t - 1 read by the downsample, then read and written by the blend
    }
    for (uint32_t k = T; k-- > 1u;) {
        BloomArgs a = base;
        a.src = pyramid + plan.offset[k]; a.sw = plan.w[k]; a.sh = plan.h[k];
        a.dst = pyramid + plan.offset[k - 1u]; a.dw = plan.w[k - 1u]; a.dh = plan.h[k - 1u];
        a.factor = plan.factor[k];
        s.step[s.count++] = {{KS_BLOOM_UP, (double)a.sw * a.sh * 16.0 + (double)a.dw * a.dh * 32.0}, false, a, BloomTailArgs{}};
    }
    BloomArgs a = base;
    a.src = L ? pyramid + plan.offset[0] : nullptr; a.sw = L ? plan.w[0] : 0u; a.sh = L ? plan.h[0] : 0u;
    a.base = static_cast<const float4*>(src); a.dst = target.dst; a.dw = w; a.dh = h; a.format = format;
    a.factor = L ? plan.factor[0] : 0.0f;
    s.step[s.count++] = {{KS_BLOOM_COMPOSITE, (double)a.sw * a.sh * 16.0 + (double)w * h * (16.0 + format_bytes(format))}, false, a, BloomTailArgs{}};
    return s;
}

void Engine::launch_bloom_step(const BloomStep& s, hipStream_t stream) {
    if (s.step.slot == KS_BLOOM_DOWN) L.launch_bloom_down(s.args, s.first, stream);
    else if (s.step.slot == KS_BLOOM_UP) L.launch_bloom_up(s.args, stream);
    else if (s.step.slot == KS_BLOOM_TAIL) L.launch_bloom_tail(s.tail, stream);
    else L.launch_bloom_composite(s.args, stream);
}

int Engine::bloom_process(const StBloomDesc* desc, const StDisplayDesc* display, const void* src, uint32_t w, uint32_t h, void* dst, int format, hipStream_t stream) {
    if (!desc || !src || !dst) return fail(ST_ERR_INVALID_ARGUMENT, "null argument");
    if (w == 0u || h == 0u || w > kMaxImageSide || h > kMaxImageSide) return fail(ST_ERR_INVALID_ARGUMENT, "the image's sides must be in 1..16384");
    BloomPlan plan;
    if (int rc = bloom_plan(*desc, w, h, plan)) return rc;
    NodeTarget target;
    if (int rc = process_target("st_bloom_process", display, dst, format, target)) return rc;
    if (!has_device) return fail(ST_ERR_NO_DEVICE, "st_bloom_process on a host-only engine");
    ST_HIP(hipSetDevice(device));
    const size_t bytes = plan.texels * sizeof(float4);   // the engine's pyramid (0: the image holds no level)
    if (bytes) if (int rc = bloom_scratch.acquire({bytes}, bloom_scratch.Grow, stream)) return rc;
    const BloomSteps steps = bloom_steps(*desc, plan, src, w, h, bloom_scratch.plane[0].as<float4>(), target, bloom_tail_bytes());
    for (uint32_t i = 0; i < steps.count; i++) launch_bloom_step(steps.step[i], stream);
    if (bytes) if (int rc = bloom_scratch.done(stream)) return rc;
    ST_HIP(hipGetLastError());
    return ST_OK;
}

}  // namespace st
