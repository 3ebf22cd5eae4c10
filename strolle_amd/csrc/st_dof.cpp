// st_dof.cpp — depth of field (include/strolle_hip.h "depth of field"): the setter's checks, the plan (sample count, tile counts, plane sizes,
// the tap table), the host constants and the three launches (k_dof.hip) that st_render_camera and st_dof_process share. The HDR plane, the
// packed plane and the tile values: st_engine.h CameraState::dof, Engine::dof_scratch.
#include <cmath>

#include "st_engine.h"

namespace st {

static_assert(KS_COUNT <= ST_PROFILE_MAX_KERNELS, "st_profile_read's callers size their arrays with ST_PROFILE_MAX_KERNELS");
static_assert(sizeof(StDofDesc) == 40, "StDofDesc is 40 B");
static_assert(offsetof(StDofDesc, samples) == 8 && offsetof(StDofDesc, focal_distance) == 12 && offsetof(StDofDesc, max_radius) == 24 && offsetof(StDofDesc, focus_y) == 32,
              "StDofDesc's fields are ten 4-B words");
static constexpr uint32_t kDofDefaultSamples = 32u, kDofMinSamples = 4u;
static constexpr float kDofMaxRadius = 32.0f, kDofDefaultStops = 1.0f, kDofDefaultSensor = 0.01866f;
static_assert(kDofMaxRadius <= (float)kDofTile, "a near-field disk reaches no further than the 3 x 3 tiles the neighbour maximum covers");
static constexpr double kGoldenAngle = 2.399963229728653;


static int check_dof(const StDofDesc& d) {
    if (d.struct_size != sizeof(StDofDesc)) return fail(ST_ERR_INVALID_ARGUMENT, "StDofDesc.struct_size is not sizeof(StDofDesc)");
    if ((d.flags & ~(uint32_t)(ST_DOF_AUTOFOCUS | ST_DOF_PLANAR_DEPTH)) != 0u) return fail(ST_ERR_INVALID_ARGUMENT, "unknown depth-of-field flag bits");
    if (d.samples != 0u && (d.samples < kDofMinSamples || d.samples > kDofMaxSamples)) return fail(ST_ERR_INVALID_ARGUMENT, "depth-of-field samples must be in 4..64 (0 = default)");
    if (!positive_finite(d.focal_distance)) return fail(ST_ERR_INVALID_ARGUMENT, "focal_distance must be finite and above 0");
    if (!finite_not_negative(d.aperture_f_stops)) return fail(ST_ERR_INVALID_ARGUMENT, "aperture_f_stops must be finite and above 0 (0 = default)");
    if (!finite_not_negative(d.sensor_height)) return fail(ST_ERR_INVALID_ARGUMENT, "sensor_height must be finite and above 0 (0 = default)");
    if (!(d.max_radius >= 0.0f && d.max_radius <= kDofMaxRadius)) return fail(ST_ERR_INVALID_ARGUMENT, "max_radius is outside (0, 32] (0 = default)");
    if ((d.flags & ST_DOF_AUTOFOCUS) && !(d.focus_x >= 0.0f && d.focus_x <= 1.0f && d.focus_y >= 0.0f && d.focus_y <= 1.0f))
        return fail(ST_ERR_INVALID_ARGUMENT, "the autofocus point is outside [0, 1]^2");
    return ST_OK;
}

int Engine::dof_plan(const StDofDesc& d, uint32_t w, uint32_t h, DofPlan& plan) {
    plan = DofPlan();
    if (int rc = check_dof(d)) return rc;
    if (w > kMaxImageSide || h > kMaxImageSide) return fail(ST_ERR_INVALID_ARGUMENT, "a frame side above 16384");
    plan.samples = d.samples ? d.samples : kDofDefaultSamples;
    plan.max_radius = d.max_radius != 0.0f ? d.max_radius : kDofMaxRadius;
    plan.tiles_x = (w + kDofTile - 1u) / kDofTile; plan.tiles_y = (h + kDofTile - 1u) / kDofTile;
    plan.packed_bytes = (size_t)w * h * sizeof(float2);
    plan.tile_bytes = (size_t)plan.tiles_x * plan.tiles_y * sizeof(float);
    // the golden-angle spiral over the unit disk, in double, rounded once: equal-area rings, so the taps cover the disk uniformly
    for (uint32_t k = 0; k < plan.samples; k++) {
        const double rho = std::sqrt(((double)k + 0.5) / (double)plan.samples), th = (double)k * kGoldenAngle;
        plan.taps[3u * k] = (float)(rho * std::cos(th)); plan.taps[3u * k + 1u] = (float)(rho * std::sin(th)); plan.taps[3u * k + 2u] = (float)rho;
    }
    return ST_OK;
}

int Engine::set_dof(CameraState& c, const StDofDesc* desc) {
    if (int rc = set_node(c.windowed(), c.dof, desc, check_dof)) return rc;
    c.dof.desc._pad = 0u;
    return ST_OK;
}

// Pack (+ tile maximum), neighbour maximum, gather. A frame's depth does not honour ST_DOF_PLANAR_DEPTH. Compulsory bytes: pack reads a
// pixel's depth (the 4 B it needs; a frame's texel is 16 B wide, so the lines it touches hold four times that) and writes 8 B a pixel and 4 B
// a tile; the neighbour launch reads and writes each tile value once; the gather is credited what it moves for an in-focus pixel, 16 B of
// colour and 8 B of (coc, Z) in and the format's bytes out (the taps of blurred pixels are cache-served neighbours).
void Engine::dof_steps(const StDofDesc& d, const DofPlan& plan, const float projection[16], const NodeSource& src, float2* packed, float* tile_max, float* tile_n, const NodeTarget& target, DofSteps& out) {
    const uint32_t w = src.w, h = src.h;
    DofArgs& a = out.args;
    a = DofArgs{};
    a.depth = src.depth; a.color = static_cast<const float4*>(src.color);
    a.packed = packed; a.tile_max = tile_max; a.tile_n = tile_n;
    a.width = w; a.height = h; a.tiles_x = plan.tiles_x; a.tiles_y = plan.tiles_y; a.frame = src.frame ? 1u : 0u;
    a.samples = plan.samples;
    apply_target(target, a);
    a.planar = (!src.frame && (d.flags & ST_DOF_PLANAR_DEPTH)) ? 1u : 0u;
    a.autofocus = (d.flags & ST_DOF_AUTOFOCUS) ? 1u : 0u;
    if (a.autofocus) {   // floor(focus W) in float, as the header states it
        a.focus_px = std::min((uint32_t)std::floor(d.focus_x * (float)w), w - 1u);
        a.focus_py = std::min((uint32_t)std::floor(d.focus_y * (float)h), h - 1u);
    }
    apply_projection(projection, a);
    // the host constants, in double, rounded once
    const double sensor = (double)(d.sensor_height != 0.0f ? d.sensor_height : kDofDefaultSensor), stops = (double)(d.aperture_f_stops != 0.0f ? d.aperture_f_stops : kDofDefaultStops);
    const double f = 0.5 * sensor * (double)projection[5];
    const double k = 0.5 * f * f / (stops * sensor) * (double)h;
    a.focal_length = (float)f; a.k = (float)k;
    a.focal_distance = d.focal_distance; a.max_radius = plan.max_radius;
    for (uint32_t i = 0; i < kDofMaxSamples * 3u; i++) a.taps[i] = plan.taps[i];
    const double n = (double)w * h, tiles = (double)plan.tiles_x * plan.tiles_y;
    out.step[0] = {KS_DOF_PACK, n * 12.0 + tiles * 4.0};
    out.step[1] = {KS_DOF_NEIGHBOUR, tiles * 8.0};
    out.step[2] = {KS_DOF_GATHER, n * (24.0 + format_bytes(a.format)) + tiles * 4.0};
}

void Engine::launch_dof_step(const DofSteps& s, uint32_t i, hipStream_t stream) {
    if (s.step[i].slot == KS_DOF_PACK) L.launch_dof_pack(s.args, stream);
    else if (s.step[i].slot == KS_DOF_NEIGHBOUR) L.launch_dof_neighbour(s.args, stream);
    else L.launch_dof_gather(s.args, stream);
}

int Engine::dof_process(const StDofDesc* desc, const StDisplayDesc* display, const float* projection, const void* color, const void* depth, uint32_t w, uint32_t h, void* dst, int format, hipStream_t stream) {
    if (!desc || !projection || !color || !depth || !dst) return fail(ST_ERR_INVALID_ARGUMENT, "null argument");
    if (w == 0u || h == 0u || w > kMaxImageSide || h > kMaxImageSide) return fail(ST_ERR_INVALID_ARGUMENT, "the image's sides must be in 1..16384");
    DofPlan plan;
    if (int rc = dof_plan(*desc, w, h, plan)) return rc;
    if (!dof_perspective(projection))
        return fail(ST_ERR_INVALID_ARGUMENT, "st_dof_process takes a perspective projection: the focal length is derived from it");
    NodeTarget target;
    if (int rc = process_target("st_dof_process", display, dst, format, target)) return rc;
    if (!has_device) return fail(ST_ERR_NO_DEVICE, "st_dof_process on a host-only engine");
    ST_HIP(hipSetDevice(device));
    if (int rc = dof_scratch.acquire({plan.packed_bytes, plan.tile_bytes, plan.tile_bytes}, dof_scratch.Grow, stream)) return rc;
    DofSteps steps;
    dof_steps(*desc, plan, projection, {color, depth, nullptr, false, w, h}, dof_scratch.plane[0].as<float2>(), dof_scratch.plane[1].as<float>(), dof_scratch.plane[2].as<float>(), target, steps);
    for (uint32_t i = 0; i < 3u; i++) launch_dof_step(steps, i, stream);
    if (int rc = dof_scratch.done(stream)) return rc;
    ST_HIP(hipGetLastError());
    return ST_OK;
}

}  // namespace st
