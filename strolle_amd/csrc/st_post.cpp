// st_post.cpp — output post-processing (include/strolle_hip.h "post-processing"): the setter's checks, the plan of at most two launches
// (k_post.hip: FXAA, then the resampler, which also writes the output format) that st_render_camera and st_post_process share. The planes
// between them: st_engine.h CameraState::post, Engine::post_scratch.
#include <cmath>

#include "st_engine.h"

namespace st {

static_assert(KS_COUNT <= ST_PROFILE_MAX_KERNELS, "st_profile_read's callers size their arrays with ST_PROFILE_MAX_KERNELS");
static constexpr float kFxaaEdgeThreshold = 0.166f, kFxaaEdgeThresholdMin = 0.0833f;

static int check_post(const StPostDesc& d) {
    if (d.struct_size != sizeof(StPostDesc)) return fail(ST_ERR_INVALID_ARGUMENT, "StPostDesc.struct_size is not sizeof(StPostDesc)");
    if ((d.flags & ~(uint32_t)ST_POST_FXAA) != 0u) return fail(ST_ERR_INVALID_ARGUMENT, "unknown post-processing flag bits");
    if (d.filter > ST_RESAMPLE_CATMULL_ROM) return fail(ST_ERR_INVALID_ARGUMENT, "unknown resampling filter");
    if ((d.output_width == 0u) != (d.output_height == 0u)) return fail(ST_ERR_INVALID_ARGUMENT, "output_width and output_height are both 0 (the render size) or both set");
    if (d.output_width > kMaxImageSide || d.output_height > kMaxImageSide) return fail(ST_ERR_INVALID_ARGUMENT, "an output side above 16384");
    for (float v : {d.fxaa_edge_threshold, d.fxaa_edge_threshold_min})
        if (!std::isfinite(v) || v < 0.0f) return fail(ST_ERR_INVALID_ARGUMENT, "an FXAA threshold is negative or not finite");
    if (!(d.fxaa_subpixel >= 0.0f && d.fxaa_subpixel <= 1.0f)) return fail(ST_ERR_INVALID_ARGUMENT, "fxaa_subpixel is outside [0, 1]");
    return ST_OK;
}

int Engine::set_post(CameraState& c, const StPostDesc* desc) {
    return set_node(c.windowed(), c.post, desc, [&](const StPostDesc& d) {
        if (int rc = check_post(d)) return rc;
        // the upscale stage takes the resampler's place (st_upscale.cpp): FXAA alone is fine
        if (c.upscale.on && d.output_width != 0u && (d.output_width != c.desc.width || d.output_height != c.desc.height)) return fail(ST_ERR_INVALID_ARGUMENT, resize_refused_by_upscale());
        return (int)ST_OK;
    });
}

// FXAA (when `fxaa`) over src, then the resampler when the sizes differ — or when nothing else would write dst. FXAA alone writes dst in
// `format` itself; followed by the resampler it writes `mid` (w x h RGBA32F).
Engine::PostPlan Engine::post_plan(const StPostDesc& d, bool fxaa, const void* src, uint32_t w, uint32_t h, void* mid, void* dst, uint32_t format) {
    PostPlan p;
    const uint32_t ow = d.output_width ? d.output_width : w, oh = d.output_width ? d.output_height : h;
    p.fxaa = fxaa;
    p.resample = ow != w || oh != h || !fxaa;
    PostArgs a{};
    a.width = w; a.height = h; a.out_width = ow; a.out_height = oh; a.filter = d.filter;
    a.edge_threshold = d.fxaa_edge_threshold != 0.0f ? d.fxaa_edge_threshold : kFxaaEdgeThreshold;
    a.edge_threshold_min = d.fxaa_edge_threshold_min != 0.0f ? d.fxaa_edge_threshold_min : kFxaaEdgeThresholdMin;
    a.subpixel = d.fxaa_subpixel;
    p.fx = a; p.fx.src = static_cast<const float4*>(src); p.fx.dst = p.resample ? mid : dst; p.fx.format = p.resample ? (uint32_t)ST_FORMAT_RGBA32F : format;
    p.fx.out_width = w; p.fx.out_height = h;
    p.rs = a; p.rs.src = static_cast<const float4*>(p.fxaa ? mid : src); p.rs.dst = dst; p.rs.format = format;
    // compulsory bytes: every source texel read once, every output pixel written once (neighbour taps assumed cache-served, like st_kernels.h)
    p.fxaa_bytes = (double)w * h * (16.0 + format_bytes(p.fx.format));
    p.resample_bytes = (double)w * h * 16.0 + (double)ow * oh * format_bytes(format);
    return p;
}

int Engine::post_process(const StPostDesc* desc, const void* src, uint32_t w, uint32_t h, void* dst, int format, hipStream_t stream) {
    if (!desc || !src || !dst) return fail(ST_ERR_INVALID_ARGUMENT, "null argument");
    if (int rc = check_post(*desc)) return rc;
    if (w == 0u || h == 0u || w > kMaxImageSide || h > kMaxImageSide) return fail(ST_ERR_INVALID_ARGUMENT, "the image's sides must be in 1..16384");
    if (format < ST_FORMAT_RGBA32F || format > ST_FORMAT_BGRA8_UNORM_SRGB) return fail(ST_ERR_INVALID_ARGUMENT, "unknown output format");
    if (!has_device) return fail(ST_ERR_NO_DEVICE, "st_post_process on a host-only engine");
    ST_HIP(hipSetDevice(device));
    const bool fxaa = (desc->flags & ST_POST_FXAA) != 0u;
    const bool resizes = desc->output_width != 0u && (desc->output_width != w || desc->output_height != h);
    void* mid = nullptr;
    if (fxaa && resizes) {   // the engine's intermediate plane
        if (int rc = post_scratch.acquire({(size_t)w * h * sizeof(float4)}, post_scratch.Grow, stream)) return rc;
        mid = post_scratch.plane[0].ptr;
    }
    const PostPlan plan = post_plan(*desc, fxaa, src, w, h, mid, dst, (uint32_t)format);
    if (plan.fxaa) L.launch_post_fxaa(plan.fx, stream);
    if (plan.resample) L.launch_post_resample(plan.rs, stream);
    if (mid) if (int rc = post_scratch.done(stream)) return rc;
    ST_HIP(hipGetLastError());
    return ST_OK;
}

}  // namespace st
