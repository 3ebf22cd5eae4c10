// st_motion_blur.cpp — motion blur (include/strolle_hip.h "motion blur"): the setter's checks, the plan (tile counts, plane sizes) and the
// three launches (k_motion_blur.hip) that st_render_camera and st_motion_blur_process share. The HDR plane, the packed plane and the tile
// vectors: st_engine.h CameraState::mblur, Engine::mblur_scratch.
#include <cmath>

#include "st_engine.h"

namespace st {

static_assert(KS_COUNT <= ST_PROFILE_MAX_KERNELS, "st_profile_read's callers size their arrays with ST_PROFILE_MAX_KERNELS");
static_assert(sizeof(StMotionBlurDesc) == 24, "StMotionBlurDesc is 24 B");
static_assert(offsetof(StMotionBlurDesc, samples) == 8 && offsetof(StMotionBlurDesc, shutter) == 12 && offsetof(StMotionBlurDesc, depth_softness) == 20, "StMotionBlurDesc's fields are six 4-B words");
static constexpr uint32_t kMBlurDefaultSamples = 8u, kMBlurMaxSamples = 32u;
static constexpr float kMBlurMaxRadius = 32.0f, kMBlurDefaultSoftness = 0.05f;
static_assert(kMBlurMaxRadius <= (float)kMBlurTile, "a streak reaches no further than the 3 x 3 tiles the neighbour maximum covers");

static int check_motion_blur(const StMotionBlurDesc& d) {
    if (d.struct_size != sizeof(StMotionBlurDesc)) return fail(ST_ERR_INVALID_ARGUMENT, "StMotionBlurDesc.struct_size is not sizeof(StMotionBlurDesc)");
    if ((d.flags & ~(uint32_t)ST_MOTION_BLUR_NO_JITTER) != 0u) return fail(ST_ERR_INVALID_ARGUMENT, "unknown motion blur flag bits");
    if (d.samples != 0u && ((d.samples & 1u) != 0u || d.samples < 2u || d.samples > kMBlurMaxSamples)) return fail(ST_ERR_INVALID_ARGUMENT, "motion blur samples must be even and in 2..32 (0 = default)");
    if (!(d.shutter >= 0.0f && d.shutter <= 4.0f)) return fail(ST_ERR_INVALID_ARGUMENT, "shutter is outside [0, 4]");
    if (!(d.max_radius >= 0.0f && d.max_radius <= kMBlurMaxRadius)) return fail(ST_ERR_INVALID_ARGUMENT, "max_radius is outside (0, 32] (0 = default)");
    if (!(d.depth_softness >= 0.0f && d.depth_softness <= 1.0f)) return fail(ST_ERR_INVALID_ARGUMENT, "depth_softness is outside (0, 1] (0 = default)");
    return ST_OK;
}

int Engine::mblur_plan(const StMotionBlurDesc& d, uint32_t w, uint32_t h, MBlurPlan& plan) {
    plan = MBlurPlan();
    if (int rc = check_motion_blur(d)) return rc;
    if (w > kMaxImageSide || h > kMaxImageSide) return fail(ST_ERR_INVALID_ARGUMENT, "a frame side above 16384");
    plan.tiles_x = (w + kMBlurTile - 1u) / kMBlurTile; plan.tiles_y = (h + kMBlurTile - 1u) / kMBlurTile;
    plan.packed_bytes = (size_t)w * h * sizeof(float2);
    plan.tile_bytes = (size_t)plan.tiles_x * plan.tiles_y * sizeof(float4);
    return ST_OK;
}

int Engine::set_motion_blur(CameraState& c, const StMotionBlurDesc* desc) {
    return set_node(c.windowed(), c.mblur, desc, check_motion_blur);
}

// Pack (+ tile maximum), neighbour maximum, gather. Compulsory bytes: pack reads both planes
// (whole 16-B texels in a frame) and writes 8 B a pixel and 16 B a tile; the neighbour launch reads and writes each tile vector once; the gather
// is credited what it moves at rest, a pixel's 16 B in and the format's bytes out (the taps of moving tiles are cache-served neighbours).
void Engine::mblur_steps(const StMotionBlurDesc& d, const MBlurPlan& plan, const NodeSource& src, float2* packed, float4* tile_max, float4* tile_n, const NodeTarget& target, MBlurSteps& out) {
    MBlurArgs& a = out.args;
    a = MBlurArgs{};
    a.velocity = src.velocity; a.depth = src.depth; a.color = static_cast<const float4*>(src.color);
    a.packed = packed; a.tile_max = tile_max; a.tile_n = tile_n;
    a.width = src.w; a.height = src.h; a.tiles_x = plan.tiles_x; a.tiles_y = plan.tiles_y; a.frame = src.frame ? 1u : 0u;
    a.samples = d.samples ? d.samples : kMBlurDefaultSamples; a.jitter = (d.flags & ST_MOTION_BLUR_NO_JITTER) ? 0u : 1u;
    apply_target(target, a);
    a.half_shutter = 0.5f * d.shutter;
    a.max_radius = d.max_radius != 0.0f ? d.max_radius : kMBlurMaxRadius;
    a.depth_softness = d.depth_softness != 0.0f ? d.depth_softness : kMBlurDefaultSoftness;
    const double n = (double)src.w * src.h, tiles = (double)plan.tiles_x * plan.tiles_y;
    out.step[0] = {KS_MBLUR_PACK, n * (src.frame ? 40.0 : 20.0) + tiles * 16.0};
    out.step[1] = {KS_MBLUR_NEIGHBOUR, tiles * 32.0};
    out.step[2] = {KS_MBLUR_GATHER, n * (16.0 + format_bytes(a.format)) + tiles * 16.0};
}

void Engine::launch_mblur_step(const MBlurSteps& s, uint32_t i, hipStream_t stream) {
    if (s.step[i].slot == KS_MBLUR_PACK) L.launch_mblur_pack(s.args, stream);
    else if (s.step[i].slot == KS_MBLUR_NEIGHBOUR) L.launch_mblur_neighbour(s.args, stream);
    else L.launch_mblur_gather(s.args, stream);
}

int Engine::motion_blur_process(const StMotionBlurDesc* desc, const StDisplayDesc* display, const void* color, const void* velocity, const void* depth, uint32_t w, uint32_t h, void* dst, int format, hipStream_t stream) {
    if (!desc || !color || !velocity || !depth || !dst) return fail(ST_ERR_INVALID_ARGUMENT, "null argument");
    if (w == 0u || h == 0u || w > kMaxImageSide || h > kMaxImageSide) return fail(ST_ERR_INVALID_ARGUMENT, "the image's sides must be in 1..16384");
    MBlurPlan plan;
    if (int rc = mblur_plan(*desc, w, h, plan)) return rc;
    NodeTarget target;
    if (int rc = process_target("st_motion_blur_process", display, dst, format, target)) return rc;
    if (!has_device) return fail(ST_ERR_NO_DEVICE, "st_motion_blur_process on a host-only engine");
    ST_HIP(hipSetDevice(device));
    if (int rc = mblur_scratch.acquire({plan.packed_bytes, plan.tile_bytes, plan.tile_bytes}, mblur_scratch.Grow, stream)) return rc;
    MBlurSteps steps;
    mblur_steps(*desc, plan, {color, depth, velocity, false, w, h}, mblur_scratch.plane[0].as<float2>(), mblur_scratch.plane[1].as<float4>(), mblur_scratch.plane[2].as<float4>(), target, steps);
    for (uint32_t i = 0; i < 3u; i++) launch_mblur_step(steps, i, stream);
    if (int rc = mblur_scratch.done(stream)) return rc;
    ST_HIP(hipGetLastError());
    return ST_OK;
}

}  // namespace st
