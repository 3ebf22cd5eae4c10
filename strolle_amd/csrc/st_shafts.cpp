// st_shafts.cpp — light shafts (include/strolle_hip.h "light shafts"): the setter's checks, the plan (cell grid, jitter table), the host
// constants (step 0) and the two launches (k_shafts.hip) that st_render_camera and st_light_shafts_process share. The camera's HDR and
// cell planes: st_engine.h CameraState::shafts; the stateless call's cell plane: Engine::shafts_scratch.
#include <cmath>

#include "st_engine.h"

namespace st {

static_assert(KS_COUNT <= ST_PROFILE_MAX_KERNELS, "st_profile_read's callers size their arrays with ST_PROFILE_MAX_KERNELS");
static_assert(sizeof(StLightShaftsDesc) == 144, "StLightShaftsDesc is 144 B");
static_assert(offsetof(StLightShaftsDesc, density) == 16 && offsetof(StLightShaftsDesc, scatter) == 32 && offsetof(StLightShaftsDesc, sun_color) == 48 &&
              offsetof(StLightShaftsDesc, sun_direction) == 64 && offsetof(StLightShaftsDesc, light_count) == 76 && offsetof(StLightShaftsDesc, lights) == 80,
              "StLightShaftsDesc: twenty 4-B words, then eight handles");
static_assert(ST_SHAFTS_MAX_LIGHTS == kShaftsMaxLights, "the desc's handle list is the launch's slot list");

static bool shafts_sun(const StLightShaftsDesc& d) { return d.sun_color[0] != 0.0f || d.sun_color[1] != 0.0f || d.sun_color[2] != 0.0f; }

static int check_shafts(const StLightShaftsDesc& d) {
    if (d.struct_size != sizeof(StLightShaftsDesc)) return fail(ST_ERR_INVALID_ARGUMENT, "StLightShaftsDesc.struct_size is not sizeof(StLightShaftsDesc)");
    if ((d.flags & ~(uint32_t)(ST_SHAFTS_FOLLOW_SUN | ST_SHAFTS_LIGHT_EXTINCTION)) != 0u) return fail(ST_ERR_INVALID_ARGUMENT, "unknown light-shafts flag bits");
    if (d.steps < 1u || d.steps > 64u) return fail(ST_ERR_INVALID_ARGUMENT, "steps must be in 1..64");
    if (d.divisor != 1u && d.divisor != 2u) return fail(ST_ERR_INVALID_ARGUMENT, "divisor must be 1 or 2");
    if (!finite_not_negative(d.density)) return fail(ST_ERR_INVALID_ARGUMENT, "density must be finite and not negative");
    if (!(d.anisotropy >= -0.95f && d.anisotropy <= 0.95f)) return fail(ST_ERR_INVALID_ARGUMENT, "anisotropy is outside [-0.95, 0.95]");
    if (!positive_finite(d.max_distance)) return fail(ST_ERR_INVALID_ARGUMENT, "max_distance must be finite and above 0");
    if (!finite_not_negative(d.intensity)) return fail(ST_ERR_INVALID_ARGUMENT, "intensity must be finite and not negative");
    for (int i = 0; i < 3; i++) if (!(d.scatter[i] >= 0.0f && d.scatter[i] <= 1.0f)) return fail(ST_ERR_INVALID_ARGUMENT, "scatter is outside [0, 1]");
    for (int i = 0; i < 3; i++) if (!finite_not_negative(d.sun_color[i])) return fail(ST_ERR_INVALID_ARGUMENT, "sun_color must be finite and not negative");
    if (shafts_sun(d) && !(d.flags & ST_SHAFTS_FOLLOW_SUN) && !finite_direction(d.sun_direction)) return fail(ST_ERR_INVALID_ARGUMENT, "sun_direction must be finite and not of length 0");
    if (d.light_count > (uint32_t)ST_SHAFTS_MAX_LIGHTS) return fail(ST_ERR_INVALID_ARGUMENT, "light_count is above 8");
    return ST_OK;
}

int Engine::shafts_plan(const StLightShaftsDesc& d, uint32_t w, uint32_t h, ShaftsPlan& out) {
    if (int rc = check_shafts(d)) return rc;
    if (w == 0u || h == 0u || w > kMaxImageSide || h > kMaxImageSide) return fail(ST_ERR_INVALID_ARGUMENT, "the image's sides must be in 1..16384");
    out.cells_w = (w + d.divisor - 1u) / d.divisor; out.cells_h = (h + d.divisor - 1u) / d.divisor;
    out.cell_bytes = (size_t)out.cells_w * out.cells_h * sizeof(float4);
    static const uint32_t bayer[16] = {0, 8, 2, 10, 12, 4, 14, 6, 3, 11, 1, 9, 15, 7, 13, 5};   // row cy & 3, column cx & 3
    for (int i = 0; i < 16; i++) out.jitter[i] = ((float)bayer[i] + 0.5f) / 16.0f;
    return ST_OK;
}

int Engine::set_shafts(CameraState& c, const StLightShaftsDesc* desc) {
    if (int rc = set_node(c.windowed(), c.shafts, desc, check_shafts)) return rc;
    c.shafts.desc._pad = 0.0f; c.shafts.desc._pad2 = 0.0f;
    for (uint32_t i = c.shafts.desc.light_count; i < (uint32_t)ST_SHAFTS_MAX_LIGHTS; i++) c.shafts.desc.lights[i] = 0u;
    return ST_OK;
}

// Both launches' arguments. view.sun: the direction ST_SHAFTS_FOLLOW_SUN takes. The handles become slots of
// the light table of the last st_tick (LightStore::uploaded_slot); a handle without a light there is skipped. Bytes: the march reads a pixel's
// depth and writes 16 B a cell (its time is the walks'); the apply launch reads 16 B of colour, the depth and a cell's 16 B that
// divisor^2 pixels share, and writes the format's bytes.
void Engine::shafts_steps(const StLightShaftsDesc& d, const ShaftsPlan& plan, const NodeView& view, const NodeSource& src, float4* cells, const NodeTarget& target, bool count, ShaftsSteps& out) const {
    ShaftsArgs& a = out.args;
    a = ShaftsArgs{};
    a.color = static_cast<const float4*>(src.color); a.depth = src.depth; a.cells = cells;
    a.width = src.w; a.height = src.h; a.cells_w = plan.cells_w; a.cells_h = plan.cells_h; a.divisor = d.divisor; a.steps = d.steps; a.frame = src.frame ? 1u : 0u;
    apply_target(target, a); a.count = count ? 1u : 0u;
    a.light_extinction = (d.flags & ST_SHAFTS_LIGHT_EXTINCTION) ? 1u : 0u;
    apply_projection(view.projection, a); apply_axes(view.transform, a);
    for (int i = 0; i < 3; i++) a.origin[i] = view.transform[12 + i];
    // the host constants, in double, rounded once
    if (shafts_sun(d) && unit_direction((d.flags & ST_SHAFTS_FOLLOW_SUN) ? view.sun : d.sun_direction, a.L)) a.sun_on = 1u;
    const double g = (double)d.anisotropy;
    a.k1 = (float)((1.0 - g * g) / (4.0 * 3.14159265358979323846)); a.k2 = (float)(1.0 + g * g); a.k3 = (float)(2.0 * g);
    a.density = d.density; a.max_distance = d.max_distance; a.intensity = d.intensity;
    for (int i = 0; i < 3; i++) { a.scatter[i] = d.scatter[i]; a.sun_color[i] = d.sun_color[i]; }
    for (uint32_t i = 0; i < d.light_count; i++) {
        uint32_t slot;
        if (lights.uploaded_slot(d.lights[i], &slot)) a.lights[a.light_count++] = slot;
    }
    const double n = (double)src.w * src.h, cells_n = (double)plan.cells_w * plan.cells_h;
    out.step[0] = {KS_SHAFTS_MARCH, n * 4.0 + cells_n * 16.0};
    out.step[1] = {KS_SHAFTS_APPLY, n * (20.0 + format_bytes(a.format)) + cells_n * 16.0};
}

// The march is a tracing launch over the CELL grid: the frame's (or the query's) scene and light arguments with the grid as its viewport.
void Engine::launch_shafts_step(const KArgs& scene, const ShaftsSteps& s, uint32_t i, hipStream_t stream) {
    if (i == 0u) {
        KArgs a = scene;
        a.width = s.args.cells_w; a.height = s.args.cells_h; a.row0 = 0u; a.row1 = a.height; a.col0 = 0u; a.col1 = a.width;
        L.launch_shafts_march(a, s.args, stream);
    } else L.launch_shafts_apply(s.args, stream);
}

int Engine::shafts_process(const StLightShaftsDesc* desc, const StDisplayDesc* display, const float* transform, const float* projection, const void* color, const void* depth,
                           uint32_t w, uint32_t h, void* dst, int format, hipStream_t stream) {
    if (!desc || !transform || !projection || !color || !depth || !dst) return fail(ST_ERR_INVALID_ARGUMENT, "null argument");
    ShaftsPlan plan;
    if (int rc = shafts_plan(*desc, w, h, plan)) return rc;
    if (!dof_perspective(projection)) return fail(ST_ERR_INVALID_ARGUMENT, "st_light_shafts_process takes a perspective projection: the cell's ray is derived from it");
    NodeTarget target;
    if (int rc = process_target("st_light_shafts_process", display, dst, format, target)) return rc;
    // the live scene copy and light table, with the scene queries' reader bookkeeping (st_query.cpp)
    KArgs scene;
    if (int rc = query_begin(stream, scene, kReadsScene | kReadsShading)) return rc;
    light_args(scene);
    scene.tile_map = 0u;
    if (int rc = shafts_scratch.acquire({plan.cell_bytes}, shafts_scratch.Grow, stream)) return rc;
    const float sun[3] = {sun_dir_.x, sun_dir_.y, sun_dir_.z};
    ShaftsSteps steps;
    shafts_steps(*desc, plan, {transform, projection, sun}, {color, depth, nullptr, false, w, h}, shafts_scratch.plane[0].as<float4>(), target, false, steps);
    for (uint32_t i = 0; i < 2u; i++) launch_shafts_step(scene, steps, i, stream);
    if (int rc = shafts_scratch.done(stream)) return rc;
    ST_HIP(hipGetLastError());
    return copies.end(stream, kReadsScene | kReadsShading);
}

}  // namespace st
