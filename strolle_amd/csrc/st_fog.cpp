// st_fog.cpp — distance and height fog (include/strolle_hip.h "fog"): the setter's checks, the host constants (step 0) and the one launch
// (k_fog.hip) that st_render_camera and st_fog_process share. The camera's HDR plane: st_engine.h CameraState::fog. The node needs
// no scratch: the stateless call allocates nothing.
#include <cmath>

#include "st_engine.h"

namespace st {

static_assert(KS_COUNT <= ST_PROFILE_MAX_KERNELS, "st_profile_read's callers size their arrays with ST_PROFILE_MAX_KERNELS");
static_assert(sizeof(StFogDesc) == 112, "StFogDesc is 112 B");
static_assert(offsetof(StFogDesc, color) == 16 && offsetof(StFogDesc, start) == 32 && offsetof(StFogDesc, sky_distance) == 52 && offsetof(StFogDesc, extinction) == 56 &&
              offsetof(StFogDesc, light_color) == 80 && offsetof(StFogDesc, light_exponent) == 92 && offsetof(StFogDesc, light_direction) == 96,
              "StFogDesc's fields are twenty-eight 4-B words");

static bool fog_lobe(const StFogDesc& d) { return d.light_color[0] != 0.0f || d.light_color[1] != 0.0f || d.light_color[2] != 0.0f; }

static int check_fog(const StFogDesc& d) {
    if (d.struct_size != sizeof(StFogDesc)) return fail(ST_ERR_INVALID_ARGUMENT, "StFogDesc.struct_size is not sizeof(StFogDesc)");
    if (d.falloff > (uint32_t)ST_FOG_ATMOSPHERIC) return fail(ST_ERR_INVALID_ARGUMENT, "unknown fog falloff");
    if ((d.flags & ~(uint32_t)(ST_FOG_SKY | ST_FOG_FOLLOW_SUN)) != 0u) return fail(ST_ERR_INVALID_ARGUMENT, "unknown fog flag bits");
    for (int i = 0; i < 3; i++) if (!finite_not_negative(d.color[i])) return fail(ST_ERR_INVALID_ARGUMENT, "the fog colour must be finite and not negative");
    if (!(d.color[3] >= 0.0f && d.color[3] <= 1.0f)) return fail(ST_ERR_INVALID_ARGUMENT, "the fog colour's alpha is outside [0, 1]");
    if (d.falloff == ST_FOG_LINEAR && !(finite(d.start) && finite(d.end) && d.start < d.end)) return fail(ST_ERR_INVALID_ARGUMENT, "linear fog needs finite start < end");
    if ((d.falloff == ST_FOG_EXPONENTIAL || d.falloff == ST_FOG_EXPONENTIAL_SQUARED) && !finite_not_negative(d.density))
        return fail(ST_ERR_INVALID_ARGUMENT, "the fog density must be finite and not negative");
    if (d.falloff == ST_FOG_ATMOSPHERIC)
        for (int i = 0; i < 3; i++) if (!finite_not_negative(d.extinction[i]) || !finite_not_negative(d.inscattering[i]))
            return fail(ST_ERR_INVALID_ARGUMENT, "extinction and inscattering must be finite and not negative");
    if (!finite_not_negative(d.height_falloff)) return fail(ST_ERR_INVALID_ARGUMENT, "height_falloff must be finite and not negative");
    if (!finite(d.height_reference)) return fail(ST_ERR_INVALID_ARGUMENT, "height_reference must be finite");
    if ((d.flags & ST_FOG_SKY) && !positive_finite(d.sky_distance)) return fail(ST_ERR_INVALID_ARGUMENT, "sky_distance must be finite and above 0 with ST_FOG_SKY");
    for (int i = 0; i < 3; i++) if (!finite_not_negative(d.light_color[i])) return fail(ST_ERR_INVALID_ARGUMENT, "light_color must be finite and not negative");
    if (fog_lobe(d)) {
        if (!positive_finite(d.light_exponent)) return fail(ST_ERR_INVALID_ARGUMENT, "light_exponent must be finite and above 0 when light_color is not all 0");
        if (!(d.flags & ST_FOG_FOLLOW_SUN) && !finite_direction(d.light_direction)) return fail(ST_ERR_INVALID_ARGUMENT, "light_direction must be finite and not of length 0");
    }
    return ST_OK;
}

int Engine::set_fog(CameraState& c, const StFogDesc* desc) {
    if (int rc = set_node(c.windowed(), c.fog, desc, check_fog)) return rc;
    c.fog.desc._pad = 0u; c.fog.desc._pad2 = 0.0f;
    return ST_OK;
}

// The launch's arguments over the window [row0, row1) x [col0, col1). view.sun: the direction ST_FOG_FOLLOW_SUN takes. Compulsory bytes per
// pixel of the window: 16 B of colour and the 4 B of depth it needs in (a frame's texel is 16 B wide, so the lines it touches hold four
// times that), the format's bytes out.
void Engine::fog_step(const StFogDesc& d, const NodeView& view, const NodeSource& src, uint32_t row0, uint32_t row1, uint32_t col0, uint32_t col1, const NodeTarget& target, FogStep& out) {
    FogArgs& a = out.args;
    a = FogArgs{};
    a.color = static_cast<const float4*>(src.color); a.depth = src.depth;
    a.width = src.w; a.height = src.h; a.row0 = row0; a.row1 = row1; a.col0 = col0; a.col1 = col1; a.frame = src.frame ? 1u : 0u;
    apply_target(target, a);
    a.falloff = d.falloff; a.sky = (d.flags & ST_FOG_SKY) ? 1u : 0u; a.height_on = d.height_falloff != 0.0f ? 1u : 0u; a.lobe_on = fog_lobe(d) ? 1u : 0u;
    apply_projection(view.projection, a); apply_axes(view.transform, a);
    // the host constants, in double, rounded once
    if (a.lobe_on) (void)unit_direction((d.flags & ST_FOG_FOLLOW_SUN) ? view.sun : d.light_direction, a.L);
    const double arg = -(double)d.height_falloff * ((double)view.transform[13] - (double)d.height_reference);
    a.E0 = (float)std::exp(std::min(std::max(arg, -80.0), 80.0));
    a.b = d.height_falloff; a.a = d.color[3];
    for (int i = 0; i < 3; i++) { a.rgb[i] = d.color[i]; a.light_color[i] = d.light_color[i]; a.extinction[i] = d.extinction[i]; a.inscattering[i] = d.inscattering[i]; }
    a.light_exponent = d.light_exponent;
    a.start = d.start; a.end = d.end; a.density = d.density; a.sky_distance = d.sky_distance;
    out.step = {KS_FOG, (double)(row1 - row0) * (double)(col1 - col0) * (20.0 + format_bytes(a.format))};
}

int Engine::fog_process(const StFogDesc* desc, const StDisplayDesc* display, const float* transform, const float* projection, const void* color, const void* depth,
                        uint32_t w, uint32_t h, void* dst, int format, hipStream_t stream) {
    if (!desc || !transform || !projection || !color || !depth || !dst) return fail(ST_ERR_INVALID_ARGUMENT, "null argument");
    if (w == 0u || h == 0u || w > kMaxImageSide || h > kMaxImageSide) return fail(ST_ERR_INVALID_ARGUMENT, "the image's sides must be in 1..16384");
    if (int rc = check_fog(*desc)) return rc;
    if (desc->flags & ST_FOG_FOLLOW_SUN) return fail(ST_ERR_INVALID_ARGUMENT, "st_fog_process does not take ST_FOG_FOLLOW_SUN: the sun is an engine's state");
    if (!dof_perspective(projection)) return fail(ST_ERR_INVALID_ARGUMENT, "st_fog_process takes a perspective projection: the pixel's ray is derived from it");
    NodeTarget target;
    if (int rc = process_target("st_fog_process", display, dst, format, target)) return rc;
    if (!has_device) return fail(ST_ERR_NO_DEVICE, "st_fog_process on a host-only engine");
    ST_HIP(hipSetDevice(device));
    const float no_sun[3] = {0.0f, 0.0f, 0.0f};
    FogStep step;
    fog_step(*desc, {transform, projection, no_sun}, {color, depth, nullptr, false, w, h}, 0u, h, 0u, w, target, step);
    L.launch_fog(step.args, stream);
    ST_HIP(hipGetLastError());
    return ST_OK;
}

}  // namespace st
