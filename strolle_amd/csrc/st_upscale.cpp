// st_upscale.cpp — the upscale stage (include/strolle_hip.h "upscaling"): the setter's checks, the plan of at most two launches (k_upscale.hip:
// the upscaler, then the sharpening step — or both in one —; the last one writes the output format) that st_render_camera and st_upscale_process share. The
// planes: st_engine.h CameraState::upscale (and post.planes, which the stage reads), Engine::upscale_scratch.
#include <cmath>

#include "st_engine.h"

namespace st {

static_assert(KS_COUNT <= ST_PROFILE_MAX_KERNELS, "st_profile_read's callers size their arrays with ST_PROFILE_MAX_KERNELS");

// w x h: the size of the image the stage reads (a camera's render size)
static int check_upscale(const StUpscaleDesc& d, uint32_t w, uint32_t h) {
    if (d.struct_size != sizeof(StUpscaleDesc)) return fail(ST_ERR_INVALID_ARGUMENT, "StUpscaleDesc.struct_size is not sizeof(StUpscaleDesc)");
    if ((d.flags & ~(uint32_t)ST_UPSCALE_DENOISE) != 0u) return fail(ST_ERR_INVALID_ARGUMENT, "unknown upscaling flag bits");
    if (d._pad[0] != 0u || d._pad[1] != 0u || d._pad[2] != 0u) return fail(ST_ERR_INVALID_ARGUMENT, "StUpscaleDesc._pad is not zero");
    if ((d.output_width == 0u) != (d.output_height == 0u)) return fail(ST_ERR_INVALID_ARGUMENT, "output_width and output_height are both 0 (the render size) or both set");
    if (d.output_width > kMaxImageSide || d.output_height > kMaxImageSide) return fail(ST_ERR_INVALID_ARGUMENT, "an output side above 16384");
    if (d.output_width != 0u && (d.output_width < w || d.output_height < h)) return fail(ST_ERR_INVALID_ARGUMENT, "an output side smaller than the render side: this is an upscaler");
    if (!(d.sharpness >= 0.0f && d.sharpness <= 1.0f)) return fail(ST_ERR_INVALID_ARGUMENT, "sharpness is outside [0, 1]");
    return ST_OK;
}

int Engine::set_upscale(CameraState& c, const StUpscaleDesc* desc) {
    return set_node(c.windowed(), c.upscale, desc, [&](const StUpscaleDesc& d) {
        if (int rc = check_upscale(d, c.desc.width, c.desc.height)) return rc;
        if (c.post_resizes()) return fail(ST_ERR_INVALID_ARGUMENT, upscale_refuses_resize());
        return (int)ST_OK;
    });
}

int Engine::upscale_camera_update(const CameraState& c, uint32_t nw, uint32_t nh) {
    if (!c.upscale.on) return ST_OK;
    const StUpscaleDesc& d = c.upscale.desc;
    if (d.output_width != 0u && (nw > d.output_width || nh > d.output_height))
        return fail(ST_ERR_INVALID_ARGUMENT, "a render size larger than the output size of the camera's upscaling: this is an upscaler");
    if (c.post.on && c.post.desc.output_width != 0u && (c.post.desc.output_width != nw || c.post.desc.output_height != nh))
        return fail(ST_ERR_INVALID_ARGUMENT, resize_refused_by_upscale());
    return ST_OK;
}

// The upscaler when the sizes differ, the sharpening step when sharpness > 0; followed by the sharpening step the upscaler writes `mid`
// (output size, RGBA32F), else `dst` in `format` itself.
Engine::UpscalePlan Engine::upscale_plan(const StUpscaleDesc& d, const void* src, uint32_t w, uint32_t h, void* mid, void* dst, uint32_t format, uint32_t fused) {
    UpscalePlan p;
    const uint32_t ow = d.output_width ? d.output_width : w, oh = d.output_width ? d.output_height : h;
    p.upscale = ow != w || oh != h;
    p.sharpen = d.sharpness > 0.0f;
    p.fused = p.upscale && p.sharpen ? fused : 0u;
    p.mid_bytes = p.upscale && p.sharpen && !p.fused ? (size_t)ow * oh * sizeof(float4) : 0;
    UpscaleArgs a{};
    a.sharpness = d.sharpness; a.denoise = (d.flags & ST_UPSCALE_DENOISE) != 0u ? 1u : 0u;
    p.up = a; p.up.src = static_cast<const float4*>(src); p.up.dst = p.sharpen ? mid : dst; p.up.format = p.sharpen ? (uint32_t)ST_FORMAT_RGBA32F : format;
    p.up.width = w; p.up.height = h; p.up.out_width = ow; p.up.out_height = oh;
    p.sh = a; p.sh.src = static_cast<const float4*>(p.upscale ? mid : src); p.sh.dst = dst; p.sh.format = format;
    p.sh.width = ow; p.sh.height = oh; p.sh.out_width = ow; p.sh.out_height = oh;
    p.fu = p.up; p.fu.dst = dst; p.fu.format = format;
    p.fused_bytes = (double)w * h * 16.0 + (double)ow * oh * format_bytes(format);
    // compulsory bytes: every source texel read once, every output pixel written once (neighbour taps assumed cache-served, like st_post.cpp)
    p.upscale_bytes = (double)w * h * 16.0 + (double)ow * oh * format_bytes(p.up.format);
    p.sharpen_bytes = (double)ow * oh * (16.0 + format_bytes(format));
    return p;
}

int Engine::upscale_process(const StUpscaleDesc* desc, const void* src, uint32_t w, uint32_t h, void* dst, int format, hipStream_t stream) {
    if (!desc || !src || !dst) return fail(ST_ERR_INVALID_ARGUMENT, "null argument");
    if (w == 0u || h == 0u || w > kMaxImageSide || h > kMaxImageSide) return fail(ST_ERR_INVALID_ARGUMENT, "the image's sides must be in 1..16384");
    if (int rc = check_upscale(*desc, w, h)) return rc;
    if (format < ST_FORMAT_RGBA32F || format > ST_FORMAT_BGRA8_UNORM_SRGB) return fail(ST_ERR_INVALID_ARGUMENT, "unknown output format");
    const uint32_t ow = desc->output_width ? desc->output_width : w, oh = desc->output_width ? desc->output_height : h;
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(src), s1 = s0 + (uintptr_t)w * h * sizeof(float4);
    const uintptr_t d0 = reinterpret_cast<uintptr_t>(dst), d1 = d0 + (uintptr_t)((double)ow * oh * format_bytes((uint32_t)format));
    if (s0 < d1 && d0 < s1) return fail(ST_ERR_INVALID_ARGUMENT, "src and dst overlap");
    if (!has_device) return fail(ST_ERR_NO_DEVICE, "st_upscale_process on a host-only engine");
    ST_HIP(hipSetDevice(device));
    UpscalePlan plan = upscale_plan(*desc, src, w, h, nullptr, dst, (uint32_t)format, upscale_fused);
    if (!plan.upscale && !plan.sharpen) {   // neither step: the resampler's format-converting copy
        StPostDesc copy{}; copy.struct_size = sizeof(StPostDesc);
        L.launch_post_resample(post_plan(copy, false, src, w, h, nullptr, dst, (uint32_t)format).rs, stream);
        ST_HIP(hipGetLastError());
        return ST_OK;
    }
    if (plan.mid_bytes) {   // the engine's plane between the two steps
        if (int rc = upscale_scratch.acquire({plan.mid_bytes}, upscale_scratch.Grow, stream)) return rc;
        plan = upscale_plan(*desc, src, w, h, upscale_scratch.plane[0].ptr, dst, (uint32_t)format, upscale_fused);
    }
    if (plan.fused) L.launch_upscale_sharpen(plan.fu, plan.fused, stream);
    else {
        if (plan.upscale) L.launch_upscale(plan.up, stream);
        if (plan.sharpen) L.launch_sharpen(plan.sh, stream);
    }
    if (plan.mid_bytes) if (int rc = upscale_scratch.done(stream)) return rc;
    ST_HIP(hipGetLastError());
    return ST_OK;
}

}  // namespace st
