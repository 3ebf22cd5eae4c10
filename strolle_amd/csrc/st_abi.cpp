// st_abi.cpp — the C ABI of libstrolle_hip.so (include/strolle_hip.h): one entry point per strolle::Engine method
// (strolle/src/lib.rs:132-301) plus the seams this library adds. See st_engine.h.
#include "st_engine.h"

using namespace st;
static Engine* E(StEngine* e) { return reinterpret_cast<Engine*>(e); }
#define ST_REQUIRE(cond, msg) do { if (!(cond)) return fail(ST_ERR_INVALID_ARGUMENT, msg); } while (0)
// `CameraState& c`: camera `h` of engine `e`, or the function returns ST_ERR_UNKNOWN_CAMERA
#define ST_CAMERA(c, e, h)                                                                                        \
    const auto c##_it = E(e)->cameras.find(h);                                                                    \
    if (c##_it == E(e)->cameras.end()) return fail(ST_ERR_UNKNOWN_CAMERA, "camera does not exist");               \
    CameraState& c = *c##_it->second

// st_camera_set_<stage>: the stage's setter (its checks are there) on camera `h`
template <class Desc> static int camera_set(StEngine* e, StHandle h, int (Engine::*set)(CameraState&, const Desc*), const Desc* desc) {
    ST_REQUIRE(e, "null engine");
    ST_CAMERA(cam, e, h);
    return (E(e)->*set)(cam, desc);
}
// st_camera_get_<stage>: the last descriptor set and whether the stage is on, for every stage a CameraState holds as a NodeSetting
template <class Desc, int N> static int camera_get(StEngine* e, StHandle h, NodeSetting<Desc, N> CameraState::*setting, Desc* out, int* enabled) {
    ST_REQUIRE(e, "null engine");
    ST_CAMERA(cam, e, h);
    const NodeSetting<Desc, N>& s = cam.*setting;
    if (out) { *out = s.desc; out->struct_size = sizeof(Desc); }
    if (enabled) *enabled = s.on ? 1 : 0;
    return ST_OK;
}

extern "C" {

const char* st_last_error(void) { return g_last_error.c_str(); }
// the commit this library was built from (csrc/Makefile writes st_build_commit.inc; "+dirty": the kernel / host sources differed from that commit)
#if __has_include("st_build_commit.inc")
#include "st_build_commit.inc"
#endif
#ifndef ST_BUILD_COMMIT
#define ST_BUILD_COMMIT "unknown"
#endif
const char* st_build_commit(void) { return ST_BUILD_COMMIT; }
// st_gltf.cpp reports through the same thread-local message
extern "C" int st_internal_fail(int status, const char* message) { return fail(status, message ? message : ""); }

int st_engine_create(int device_ordinal, StEngine** out) {
    ST_REQUIRE(out, "out is NULL");
    std::unique_ptr<Engine> e(new Engine());
    if (device_ordinal >= 0) {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= device_ordinal)
            return fail(ST_ERR_NO_DEVICE, "no HIP device with that ordinal (this library has no CPU rendering path)");
        ST_HIP(hipSetDevice(device_ordinal));
        e->device = device_ordinal; e->has_device = true;
        // LUT storage (zero until the first non-heatmap render generates them)
        const size_t lut_bytes[3] = {sizeof(float4) * 256 * 64, sizeof(float4) * 32 * 32, sizeof(float4) * 256 * 256};
        DeviceArray* luts[3] = {&e->d_transmittance, &e->d_scattering, &e->d_sky};
        for (int i = 0; i < 3; i++) { if (int rc = luts[i]->reserve(lut_bytes[i], lut_bytes[i])) return rc; ST_HIP(hipMemset(luts[i]->ptr, 0, lut_bytes[i])); }
        if (int rc = e->d_byte_luts.reserve(sizeof(float) * 1024, sizeof(float) * 1024)) return rc;
        {   // the wide walks' overflow words (st_engine.h walk_flags_host): page-locked, mapped, written by a kernel only when a push is dropped
            void* dev = nullptr;
            if (int rc = e->walk_flags_mem.reserve(64, hipHostMallocMapped)) return rc;
            memset(e->walk_flags_mem.ptr, 0, 64);
            ST_HIP(hipHostGetDevicePointer(&dev, e->walk_flags_mem.ptr, 0));
            e->walk_flags_host = static_cast<volatile uint32_t*>(e->walk_flags_mem.ptr); e->walk_flags_dev = static_cast<uint32_t*>(dev);
        }
        e->L.launch_build_byte_luts(static_cast<float*>(e->d_byte_luts.ptr), nullptr);
        ST_HIP(hipDeviceSynchronize());
    }
    *out = reinterpret_cast<StEngine*>(e.release());
    return ST_OK;
}
void st_engine_destroy(StEngine* e) { delete E(e); }

// ---- the scene stores (st_stores.h; st_scene.cpp)
int st_mesh_insert(StEngine* e, StHandle id, const StMeshTriangle* t, size_t count) {
    ST_REQUIRE(e && (t || count == 0), "null argument");
    if (count == 0) return fail(ST_ERR_EMPTY_MESH, "mesh contains no triangles");
    E(e)->insert_mesh(id, t, count);
    return ST_OK;
}
int st_mesh_remove(StEngine* e, StHandle id) { ST_REQUIRE(e, "null engine"); E(e)->remove_mesh(id); return ST_OK; }

int st_material_insert(StEngine* e, StHandle id, const StMaterial* m) { ST_REQUIRE(e && m, "null argument"); E(e)->materials.insert(id, *m); return ST_OK; }
int st_material_has(StEngine* e, StHandle id) { return e && E(e)->materials.has(id) ? 1 : 0; }
int st_material_remove(StEngine* e, StHandle id) { ST_REQUIRE(e, "null engine"); E(e)->materials.remove(id); return ST_OK; }

int st_image_insert_rgba8(StEngine* e, StHandle id, uint32_t w, uint32_t h, const uint8_t* rgba, int /*srgb*/) {
    ST_REQUIRE(e && rgba && w && h && id, "bad image");
    return E(e)->images.insert_rgba8(id, w, h, rgba);
}
int st_image_insert_device_rgba8(StEngine* e, StHandle id, uint32_t w, uint32_t h, const void* device_rgba, size_t row_pitch_bytes, int is_dynamic) {
    ST_REQUIRE(e && device_rgba && w && h && id, "bad image");
    ST_REQUIRE(row_pitch_bytes >= (size_t)w * 4, "row pitch smaller than a row");
    if (!E(e)->has_device) return fail(ST_ERR_NO_DEVICE, "device images need a device engine");
    return E(e)->images.insert_device(id, w, h, device_rgba, row_pitch_bytes, is_dynamic != 0);
}
int st_image_remove(StEngine* e, StHandle id) { ST_REQUIRE(e, "null engine"); E(e)->images.remove(id); return ST_OK; }
int st_debug_image_rect(StEngine* e, StHandle id, uint32_t out_xywh[4]) {
    ST_REQUIRE(e && out_xywh, "null argument");
    const ImageAtlas::Rect* r = E(e)->images.rect_texels(id);
    if (!r) return fail(ST_ERR_INVALID_ARGUMENT, "no such image");
    out_xywh[0] = r->x; out_xywh[1] = r->y; out_xywh[2] = r->w; out_xywh[3] = r->h;
    return ST_OK;
}

int st_instance_insert(StEngine* e, StHandle id, StHandle mesh, StHandle material, const float xform[12]) {
    ST_REQUIRE(e && xform, "null argument");
    E(e)->insert_instance(id, mesh, material, affine_from12(xform));
    return ST_OK;
}
int st_instance_remove(StEngine* e, StHandle id) { ST_REQUIRE(e, "null engine"); E(e)->remove_instance(id); return ST_OK; }

// ---- skinned meshes (st_deform.cpp)
int st_mesh_set_skin(StEngine* e, StHandle mesh, const StSkinVertex* corners, size_t corner_count, uint32_t joint_count) {
    ST_REQUIRE(e, "null engine");
    return E(e)->deform.set_skin(mesh, corners, corner_count, joint_count);
}
int st_instance_set_pose(StEngine* e, StHandle instance, const float* joint_xforms, uint32_t joint_count) {
    ST_REQUIRE(e, "null engine");
    return E(e)->deform.set_pose(instance, joint_xforms, joint_count);
}
int st_debug_skinning(StEngine* e, uint64_t* launches, uint64_t* triangles, uint64_t* host_readbacks) {
    ST_REQUIRE(e && launches && triangles && host_readbacks, "null argument");
    E(e)->deform.skinning_stats(launches, triangles, host_readbacks);
    return ST_OK;
}
int st_debug_read_posed(StEngine* e, StHandle instance, float* out, size_t capacity_floats, size_t* written_floats) {
    ST_REQUIRE(e, "null engine");
    return E(e)->deform.read_posed(instance, out, capacity_floats, written_floats);
}
// ---- morph targets (st_deform.cpp)
int st_mesh_set_morph_targets(StEngine* e, StHandle mesh, const StMorphDelta* deltas, size_t corner_count, uint32_t target_count) {
    ST_REQUIRE(e, "null engine");
    return E(e)->deform.set_morph_targets(mesh, deltas, corner_count, target_count);
}
int st_instance_set_morph_weights(StEngine* e, StHandle instance, const float* weights, uint32_t target_count) {
    ST_REQUIRE(e, "null engine");
    return E(e)->deform.set_morph_weights(instance, weights, target_count);
}
int st_debug_morphing(StEngine* e, uint64_t* ticks, uint64_t* triangles, uint64_t* delta_bytes) {
    ST_REQUIRE(e && ticks && triangles && delta_bytes, "null argument");
    return E(e)->deform.morphing_stats(ticks, triangles, delta_bytes);
}
int st_engine_set_deformation_motion(StEngine* e, int enabled) { ST_REQUIRE(e, "null engine"); E(e)->deform.motion_on = enabled != 0; return ST_OK; }
int st_engine_get_deformation_motion(StEngine* e, int* enabled) { ST_REQUIRE(e && enabled, "null argument"); *enabled = E(e)->deform.motion_on ? 1 : 0; return ST_OK; }
// normal mapping (st_engine.h normal_map_geo): only a flag, so a host-only engine takes it too
int st_engine_set_normal_mapping(StEngine* e, int enabled) { ST_REQUIRE(e, "null engine"); E(e)->normal_mapping = enabled != 0; return ST_OK; }
int st_engine_get_normal_mapping(StEngine* e, int* enabled) { ST_REQUIRE(e && enabled, "null argument"); *enabled = E(e)->normal_mapping ? 1 : 0; return ST_OK; }
int st_debug_deformation(StEngine* e, uint64_t* instances_with_previous, uint64_t* previous_bytes) {
    ST_REQUIRE(e && instances_with_previous && previous_bytes, "null argument");
    return E(e)->deform.deformation_stats(instances_with_previous, previous_bytes);
}
int st_light_insert(StEngine* e, StHandle id, const StLight* l) { ST_REQUIRE(e && l, "null argument"); E(e)->lights.insert(id, *l); return ST_OK; }
int st_light_remove(StEngine* e, StHandle id) { ST_REQUIRE(e, "null engine"); E(e)->lights.remove(id); return ST_OK; }
int st_sun_update(StEngine* e, float azimuth, float altitude) { ST_REQUIRE(e, "null engine"); E(e)->sun_azimuth = azimuth; E(e)->sun_altitude = altitude; E(e)->sun_dirty = true; return ST_OK; }

int st_camera_create(StEngine* e, const StCamera* c, StHandle* out) {
    ST_REQUIRE(e && c && out && c->width && c->height, "bad camera");
    Engine* en = E(e);
    std::unique_ptr<CameraState> s(new CameraState());
    s->desc = *c;
    s->curr = Engine::serialize_camera(*c); s->prev = s->curr;
    const int rc = en->allocate_camera(*s);
    if (rc) return rc;
    *out = en->next_camera++;
    s->handle = *out;
    en->cameras[*out] = std::move(s);
    return ST_OK;
}
int st_camera_update(StEngine* e, StHandle h, const StCamera* c) {
    ST_REQUIRE(e && c && c->width && c->height, "bad camera");
    Engine* en = E(e);
    ST_CAMERA(s, e, h);
    if (int rc = Engine::upscale_camera_update(s, c->width, c->height)) return rc;   // refused: the camera stays as it was
    const bool invalidated = s.desc.mode != c->mode || s.desc.denoise != c->denoise || s.desc.depth != c->depth || s.desc.width != c->width || s.desc.height != c->height;
    s.desc = *c;
    s.prev = s.curr;
    s.curr = Engine::serialize_camera(*c);
    if (invalidated) { if (en->has_device) { ST_HIP(hipSetDevice(en->device)); ST_HIP(hipDeviceSynchronize()); } return en->allocate_camera(s); }  // camera.rs:17-48: buffers are rebuilt
    return ST_OK;
}
int st_camera_delete(StEngine* e, StHandle h) {
    ST_REQUIRE(e, "null engine");
    Engine* en = E(e);
    auto it = en->cameras.find(h);
    if (it == en->cameras.end()) return ST_OK;
    if (en->has_device) { ST_HIP(hipSetDevice(en->device)); ST_HIP(hipDeviceSynchronize()); }
    en->dist_forget_camera(h);
    en->cameras.erase(it);   // with the device current and idle: what the camera owns goes with it
    return ST_OK;
}
int st_camera_set_window(StEngine* e, StHandle h, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1) {
    ST_REQUIRE(e, "null engine");
    ST_CAMERA(s, e, h);
    if (x0 == 0 && x1 == 0) x1 = s.desc.width;
    if (y0 == 0 && y1 == 0) y1 = s.desc.height;
    ST_REQUIRE(y0 < y1 && y1 <= s.desc.height, "bad row window");
    ST_REQUIRE(x0 < x1 && x1 <= s.desc.width, "bad column window");
    // half-resolution passes work on 2x1 cells in tiles of 8 cells: a window starts and ends on a multiple of 16 pixels (or at the frame's edge)
    ST_REQUIRE(x0 % 16u == 0u && (x1 % 16u == 0u || x1 == s.desc.width), "window columns must be multiples of 16 (or the frame's right edge)");
    const bool full = x0 == 0u && y0 == 0u && x1 == s.desc.width && y1 == s.desc.height;
    ST_REQUIRE(full || !s.display_auto(), "a window on a camera with auto-exposure would meter the tile alone (include/strolle_hip.h \"display transforms\")");
    // each stage's own rule (st_output_chain.h), as its setter states it; fog and colour grading carry none
    const std::initializer_list<std::pair<bool, const WindowRule*>> stages = {{s.post.on, s.post.window}, {s.bloom.on, s.bloom.window}, {s.mblur.on, s.mblur.window},
                                                                              {s.dof.on, s.dof.window}, {s.fog.on, s.fog.window}, {s.shafts.on, s.shafts.window}, {s.grade.on, s.grade.window}, {s.lens.on, s.lens.window},
                                                                              {s.upscale.on, s.upscale.window}};
    for (const auto& st : stages) if (!full && st.first && st.second) return fail(ST_ERR_INVALID_ARGUMENT, window_refused_by(*st.second));
    s.row0 = y0; s.row1 = y1; s.col0 = x0; s.col1 = x1;
    return ST_OK;
}
int st_camera_set_rows(StEngine* e, StHandle h, uint32_t y0, uint32_t y1) { return st_camera_set_window(e, h, 0u, y0, 0u, y1); }

int st_camera_set_output_format(StEngine* e, StHandle h, int format) {
    ST_REQUIRE(e, "null engine");
    ST_CAMERA(cam, e, h);
    ST_REQUIRE(format >= ST_FORMAT_RGBA32F && format <= ST_FORMAT_BGRA8_UNORM_SRGB, "unknown output format");
    cam.out_format = (uint32_t)format;
    return ST_OK;
}

// ---- display transforms (st_display.cpp)
int st_camera_set_display(StEngine* e, StHandle h, const StDisplayDesc* desc) { return camera_set(e, h, &Engine::set_display, desc); }
int st_camera_get_display(StEngine* e, StHandle h, StDisplayDesc* out, int* enabled) {
    ST_REQUIRE(e, "null engine");
    ST_CAMERA(s, e, h);
    if (out) { *out = s.display; out->struct_size = sizeof(StDisplayDesc); }
    if (enabled) *enabled = s.display_on ? 1 : 0;
    return ST_OK;
}
int st_camera_exposure(StEngine* e, StHandle h, float* scale, float* metered_ev, float* adapted_ev) {
    ST_REQUIRE(e, "null engine");
    ST_CAMERA(cam, e, h);
    return E(e)->display_exposure(cam, scale, metered_ev, adapted_ev);
}
int st_debug_camera_histogram(StEngine* e, StHandle h, uint32_t bins[64]) {
    ST_REQUIRE(e && bins, "null argument");
    ST_CAMERA(cam, e, h);
    return E(e)->display_histogram(cam, bins);
}

// ---- output post-processing (st_post.cpp)
int st_camera_set_post(StEngine* e, StHandle h, const StPostDesc* desc) { return camera_set(e, h, &Engine::set_post, desc); }
int st_camera_get_post(StEngine* e, StHandle h, StPostDesc* out, int* enabled) { return camera_get(e, h, &CameraState::post, out, enabled); }
int st_camera_output_size(StEngine* e, StHandle h, uint32_t* width, uint32_t* height) {
    ST_REQUIRE(e, "null engine");
    ST_CAMERA(cam, e, h);
    if (width) *width = cam.out_width();
    if (height) *height = cam.out_height();
    return ST_OK;
}
int st_post_process(StEngine* e, const StPostDesc* desc, const void* src, uint32_t width, uint32_t height, void* dst, int dst_format, void* stream) {
    ST_REQUIRE(e, "null engine");
    return E(e)->post_process(desc, src, width, height, dst, dst_format, static_cast<hipStream_t>(stream));
}

// ---- the upscale stage (st_upscale.cpp)
int st_camera_set_upscale(StEngine* e, StHandle h, const StUpscaleDesc* desc) { return camera_set(e, h, &Engine::set_upscale, desc); }
int st_camera_get_upscale(StEngine* e, StHandle h, StUpscaleDesc* out, int* enabled) { return camera_get(e, h, &CameraState::upscale, out, enabled); }
int st_upscale_process(StEngine* e, const StUpscaleDesc* desc, const void* src, uint32_t width, uint32_t height, void* dst, int dst_format, void* stream) {
    ST_REQUIRE(e, "null engine");
    return E(e)->upscale_process(desc, src, width, height, dst, dst_format, static_cast<hipStream_t>(stream));
}

int st_debug_set_upscale_fused(StEngine* e, int tile) {
    ST_REQUIRE(e, "null engine");
    ST_REQUIRE(tile >= 0 && tile <= 3, "tile is 0 (two launches), 1 (64 x 8), 2 (32 x 32) or 3 (64 x 16)");
    E(e)->upscale_fused = (uint32_t)tile;
    return ST_OK;
}

// ---- lens effects (st_lens.cpp)
int st_camera_set_lens(StEngine* e, StHandle h, const StLensDesc* desc) { return camera_set(e, h, &Engine::set_lens, desc); }
int st_camera_get_lens(StEngine* e, StHandle h, StLensDesc* out, int* enabled) { return camera_get(e, h, &CameraState::lens, out, enabled); }
int st_lens_plan(const StLensDesc* desc, uint32_t width, uint32_t height, StLensPlan* out) {
    ST_REQUIRE(desc, "null desc");
    StLensPlan plan;
    if (int rc = Engine::lens_plan(*desc, width, height, plan)) return rc;
    if (out) *out = plan;
    return ST_OK;
}
int st_lens_process(StEngine* e, const StLensDesc* desc, const StDisplayDesc* display, const void* src, uint32_t width, uint32_t height, void* dst, int dst_format, void* stream) {
    ST_REQUIRE(e, "null engine");
    return E(e)->lens_process(desc, display, src, width, height, dst, dst_format, static_cast<hipStream_t>(stream));
}
int st_debug_set_lens_gather(StEngine* e, int force) {
    ST_REQUIRE(e, "null engine");
    E(e)->lens_force_gather = force != 0;
    return ST_OK;
}

// ---- bloom (st_bloom.cpp)
int st_camera_set_bloom(StEngine* e, StHandle h, const StBloomDesc* desc) { return camera_set(e, h, &Engine::set_bloom, desc); }
int st_camera_get_bloom(StEngine* e, StHandle h, StBloomDesc* out, int* enabled) { return camera_get(e, h, &CameraState::bloom, out, enabled); }
int st_bloom_plan(const StBloomDesc* desc, uint32_t width, uint32_t height, uint32_t* levels, uint32_t sizes_wh[16], float factors[8]) {
    ST_REQUIRE(desc, "null desc");
    Engine::BloomPlan plan;
    if (int rc = Engine::bloom_plan(*desc, width, height, plan)) return rc;
    if (levels) *levels = plan.levels;
    for (uint32_t k = 0; k < 8u; k++) {
        if (sizes_wh) { sizes_wh[2u * k] = plan.w[k]; sizes_wh[2u * k + 1u] = plan.h[k]; }
        if (factors) factors[k] = plan.factor[k];
    }
    return ST_OK;
}
int st_bloom_process(StEngine* e, const StBloomDesc* desc, const StDisplayDesc* display, const void* src, uint32_t width, uint32_t height, void* dst, int dst_format, void* stream) {
    ST_REQUIRE(e, "null engine");
    return E(e)->bloom_process(desc, display, src, width, height, dst, dst_format, static_cast<hipStream_t>(stream));
}

// ---- motion blur (st_motion_blur.cpp)
int st_camera_set_motion_blur(StEngine* e, StHandle h, const StMotionBlurDesc* desc) { return camera_set(e, h, &Engine::set_motion_blur, desc); }
int st_camera_get_motion_blur(StEngine* e, StHandle h, StMotionBlurDesc* out, int* enabled) { return camera_get(e, h, &CameraState::mblur, out, enabled); }
int st_motion_blur_process(StEngine* e, const StMotionBlurDesc* desc, const StDisplayDesc* display, const void* color, const void* velocity, const void* depth,
                           uint32_t width, uint32_t height, void* dst, int dst_format, void* stream) {
    ST_REQUIRE(e, "null engine");
    return E(e)->motion_blur_process(desc, display, color, velocity, depth, width, height, dst, dst_format, static_cast<hipStream_t>(stream));
}

// ---- depth of field (st_dof.cpp)
int st_camera_set_dof(StEngine* e, StHandle h, const StDofDesc* desc) { return camera_set(e, h, &Engine::set_dof, desc); }
int st_camera_get_dof(StEngine* e, StHandle h, StDofDesc* out, int* enabled) { return camera_get(e, h, &CameraState::dof, out, enabled); }
int st_dof_plan(const StDofDesc* desc, uint32_t width, uint32_t height, uint32_t* samples, uint32_t tiles_xy[2], float taps_xyr[64 * 3]) {
    ST_REQUIRE(desc, "null desc");
    Engine::DofPlan plan;
    if (int rc = Engine::dof_plan(*desc, width, height, plan)) return rc;
    if (samples) *samples = plan.samples;
    if (tiles_xy) { tiles_xy[0] = plan.tiles_x; tiles_xy[1] = plan.tiles_y; }
    if (taps_xyr) for (uint32_t i = 0; i < kDofMaxSamples * 3u; i++) taps_xyr[i] = plan.taps[i];
    return ST_OK;
}
int st_dof_process(StEngine* e, const StDofDesc* desc, const StDisplayDesc* display, const float projection[16], const void* color, const void* depth,
                   uint32_t width, uint32_t height, void* dst, int dst_format, void* stream) {
    ST_REQUIRE(e, "null engine");
    return E(e)->dof_process(desc, display, projection, color, depth, width, height, dst, dst_format, static_cast<hipStream_t>(stream));
}

// ---- fog (st_fog.cpp)
int st_camera_set_fog(StEngine* e, StHandle h, const StFogDesc* desc) { return camera_set(e, h, &Engine::set_fog, desc); }
int st_camera_get_fog(StEngine* e, StHandle h, StFogDesc* out, int* enabled) { return camera_get(e, h, &CameraState::fog, out, enabled); }
int st_fog_process(StEngine* e, const StFogDesc* desc, const StDisplayDesc* display, const float transform[16], const float projection[16], const void* color, const void* depth,
                   uint32_t width, uint32_t height, void* dst, int dst_format, void* stream) {
    ST_REQUIRE(e, "null engine");
    return E(e)->fog_process(desc, display, transform, projection, color, depth, width, height, dst, dst_format, static_cast<hipStream_t>(stream));
}

// ---- colour grading (st_grade.cpp)
int st_camera_set_color_grading(StEngine* e, StHandle h, const StColorGradingDesc* desc) { return camera_set(e, h, &Engine::set_grade, desc); }
int st_camera_get_color_grading(StEngine* e, StHandle h, StColorGradingDesc* out, int* enabled) { return camera_get(e, h, &CameraState::grade, out, enabled); }
int st_color_grading_plan(const StColorGradingDesc* desc, StColorGradingPlan* out) {
    ST_REQUIRE(desc, "null desc");
    Engine::GradePlan plan;
    if (int rc = Engine::grade_plan(*desc, plan)) return rc;
    if (out) {
        out->steps = plan.steps; out->lut_inv_range = plan.inv_range; out->_pad = 0u;
        for (int i = 0; i < 9; i++) out->white_balance[i] = plan.M[i];
    }
    return ST_OK;
}
int st_color_grading_process(StEngine* e, const StColorGradingDesc* desc, const StDisplayDesc* display, const void* lut, uint32_t lut_size, const void* src, uint32_t width,
                             uint32_t height, void* dst, int dst_format, void* stream) {
    ST_REQUIRE(e, "null engine");
    return E(e)->grade_process(desc, display, lut, lut_size, src, width, height, dst, dst_format, static_cast<hipStream_t>(stream));
}
int st_lut_insert(StEngine* e, StHandle id, uint32_t size, const float* rgb) {
    ST_REQUIRE(e, "null engine");
    return E(e)->lut_insert(id, size, rgb);
}
int st_lut_remove(StEngine* e, StHandle id) {
    ST_REQUIRE(e, "null engine");
    return E(e)->lut_remove(id);
}

// ---- light shafts (st_shafts.cpp)
int st_camera_set_light_shafts(StEngine* e, StHandle h, const StLightShaftsDesc* desc) { return camera_set(e, h, &Engine::set_shafts, desc); }
int st_camera_get_light_shafts(StEngine* e, StHandle h, StLightShaftsDesc* out, int* enabled) { return camera_get(e, h, &CameraState::shafts, out, enabled); }
int st_light_shafts_plan(const StLightShaftsDesc* desc, uint32_t width, uint32_t height, uint32_t cells_wh[2], float jitter[16]) {
    ST_REQUIRE(desc, "null desc");
    Engine::ShaftsPlan plan;
    if (int rc = Engine::shafts_plan(*desc, width, height, plan)) return rc;
    if (cells_wh) { cells_wh[0] = plan.cells_w; cells_wh[1] = plan.cells_h; }
    if (jitter) for (int i = 0; i < 16; i++) jitter[i] = plan.jitter[i];
    return ST_OK;
}
int st_light_shafts_process(StEngine* e, const StLightShaftsDesc* desc, const StDisplayDesc* display, const float transform[16], const float projection[16], const void* color,
                            const void* depth, uint32_t width, uint32_t height, void* dst, int dst_format, void* stream) {
    ST_REQUIRE(e, "null engine");
    return E(e)->shafts_process(desc, display, transform, projection, color, depth, width, height, dst, dst_format, static_cast<hipStream_t>(stream));
}

int st_debug_set_bloom_tail(StEngine* e, int lds_bytes, uint32_t* in_force) {
    ST_REQUIRE(e, "null engine");
    ST_REQUIRE(lds_bytes >= -1, "lds_bytes is -1 (what the device grants), 0 (no fused tail) or a byte count");
    E(e)->bloom_tail_wanted = lds_bytes;
    if (in_force) *in_force = E(e)->bloom_tail_bytes();
    return ST_OK;
}

int st_tick(StEngine* e, void* stream) { ST_REQUIRE(e, "null engine"); return E(e)->tick(static_cast<hipStream_t>(stream)); }
int st_render_camera(StEngine* e, StHandle h, void* out, void* stream) {
    ST_REQUIRE(e, "null engine");
    ST_CAMERA(cam, e, h);
    return E(e)->render(cam, out, static_cast<hipStream_t>(stream));
}

// ---- scene queries (st_query.cpp): argument checks first, so that a host-only engine answers them too
int st_scene_trace_rays(StEngine* e, const StRay* rays, uint32_t count, StRayHit* hits, uint32_t flags, void* stream) {
    ST_REQUIRE(e, "null engine");
    // ST_RAY_MAPPED_NORMAL is a bit only an engine with a device knows: a host-only engine has no records to map with and keeps answering it as it did before the flag existed
    const uint32_t known = ST_RAY_COHERENT | (E(e)->has_device ? (uint32_t)ST_RAY_MAPPED_NORMAL : 0u);
    ST_REQUIRE((flags & ~known) == 0u, "unknown flag bits");
    if (count == 0u) return ST_OK;
    ST_REQUIRE(rays && hits, "null argument");
    return E(e)->trace_rays(rays, count, hits, flags, static_cast<hipStream_t>(stream));
}
int st_scene_occluded(StEngine* e, const StRay* rays, uint32_t count, uint32_t* occluded, void* stream) {
    ST_REQUIRE(e, "null engine");
    if (count == 0u) return ST_OK;
    ST_REQUIRE(rays && occluded, "null argument");
    return E(e)->occluded(rays, count, occluded, static_cast<hipStream_t>(stream));
}
int st_camera_pick(StEngine* e, StHandle h, const uint32_t* pixels_xy, uint32_t count, StRayHit* hits, void* stream) {
    ST_REQUIRE(e, "null engine");
    if (count == 0u) return ST_OK;
    ST_REQUIRE(pixels_xy && hits, "null argument");
    ST_CAMERA(cam, e, h);
    return E(e)->pick(cam, pixels_xy, count, hits, static_cast<hipStream_t>(stream));
}
int st_scene_trace_rays_host(StEngine* e, const StRay* rays, uint32_t count, StRayHit* hits) {
    ST_REQUIRE(e, "null engine");
    if (count == 0u) return ST_OK;
    ST_REQUIRE(rays && hits, "null argument");
    return E(e)->trace_rays_host(rays, count, hits);
}
// per-pixel AOVs (st_aov.cpp): the argument checks come first here too
int st_camera_render_aovs(StEngine* e, StHandle h, const StAovTargets* targets, void* stream) {
    ST_REQUIRE(e, "null engine");
    ST_REQUIRE(targets, "null targets");
    ST_REQUIRE(targets->struct_size == sizeof(StAovTargets), "StAovTargets.struct_size is not sizeof(StAovTargets)");
    bool any = false;
    for (int k = 0; k < ST_AOV_COUNT; k++) any |= targets->planes[k] != nullptr;
    ST_REQUIRE(any, "no AOV plane requested");
    ST_CAMERA(cam, e, h);
    return E(e)->render_aovs(cam, *targets, static_cast<hipStream_t>(stream));
}

int st_debug_keep_all_planes(StEngine* e, int keep) { ST_REQUIRE(e, "null engine"); E(e)->tuning.lean_frame = keep == 0 ? 1u : 0u; return ST_OK; }
int st_camera_present_copy(StEngine* e, StHandle h, const void* src_device, void* dst_host, size_t bytes, void* stream) {
    ST_REQUIRE(e && src_device && dst_host && bytes, "null argument");
    ST_CAMERA(cam, e, h);
    return E(e)->present_copy(cam, src_device, dst_host, bytes, static_cast<hipStream_t>(stream));
}
int st_camera_present_ready(StEngine* e, StHandle h, const void* dst_host, int wait, int* ready) {
    ST_REQUIRE(e && ready, "null argument");
    ST_CAMERA(cam, e, h);
    return E(e)->present_ready(cam, dst_host, wait, ready);
}

int st_set_seed(StEngine* e, uint64_t seed) { ST_REQUIRE(e, "null engine"); E(e)->base_seed = seed; return ST_OK; }
int st_set_blue_noise(StEngine* e, const uint8_t* rgba, size_t bytes) {
    ST_REQUIRE(e && rgba && bytes == 256 * 256 * 4, "blue noise must be 256x256 RGBA8");
    E(e)->blue_noise.assign(rgba, rgba + bytes); E(e)->blue_noise_dirty = true;
    return ST_OK;
}
int st_debug_read_lut(StEngine* e, int what, float* out, size_t capacity_floats, size_t* written_floats) {
    ST_REQUIRE(e && what >= 0 && what < 3, "bad lut id");
    Engine* en = E(e);
    if (!en->has_device) return fail(ST_ERR_NO_DEVICE, "host-only engine has no LUTs");
    const size_t n[3] = {256 * 64 * 4, 32 * 32 * 4, 256 * 256 * 4};
    const DeviceArray* src[3] = {&en->d_transmittance, &en->d_scattering, &en->d_sky};
    if (written_floats) *written_floats = n[what];
    if (!out) return ST_OK;
    ST_REQUIRE(capacity_floats >= n[what], "buffer too small");
    ST_HIP(hipSetDevice(en->device));
    ST_HIP(hipDeviceSynchronize());
    ST_HIP(hipMemcpy(out, src[what]->ptr, n[what] * sizeof(float), hipMemcpyDeviceToHost));
    return ST_OK;
}

int st_camera_read_buffer(StEngine* e, StHandle h, int id, void* out, size_t capacity, size_t* written) {
    ST_REQUIRE(e && id >= 0 && id < ST_BUF_COUNT, "bad buffer id");
    Engine* en = E(e);
    ST_CAMERA(c, e, h);
    if (!en->has_device) return fail(ST_ERR_NO_DEVICE, "host-only engine has no camera buffers");
    if (written) *written = c.plane_bytes[id];
    if (!out) return ST_OK;
    ST_REQUIRE(capacity >= c.plane_bytes[id], "buffer too small");
    ST_HIP(hipSetDevice(en->device));
    ST_HIP(hipDeviceSynchronize());
    const float4* src = (id == ST_BUF_GI_RESERVOIRS_1 && c.gi_aliased) ? c.plane[ST_BUF_GI_RESERVOIRS_0] : c.plane[id];
    ST_HIP(hipMemcpy(out, src, c.plane_bytes[id], hipMemcpyDeviceToHost));
    return ST_OK;
}
// Did the camera's last frame leave this plane unwritten (the lean frame, st_debug_keep_all_planes)? A read-back then returns what an
// earlier launch or frame stored there.
int st_camera_buffer_stale(StEngine* e, StHandle h, int id, int* stale) {
    ST_REQUIRE(e && stale && id >= 0 && id < ST_BUF_COUNT, "bad argument");
    ST_CAMERA(c, e, h);
    const uint32_t lean = c.last_lean;
    bool s = false;
    if (lean & kLeanPrim) s |= (id == ST_BUF_VELOCITY_MAP && !(lean & kLeanKeepVelocity)) || id == ST_BUF_PRIM_SURFACE_MAP_A || id == ST_BUF_PRIM_SURFACE_MAP_B;   // (a frame that blurs keeps the velocity map)
    if (lean & kLeanSamples) s |= id == ST_BUF_DI_DIFF_SAMPLES || id == ST_BUF_GI_DIFF_SAMPLES;
    if (lean & kLeanGiRes2) s |= id == ST_BUF_GI_RESERVOIRS_2;
    if (lean & kLeanGiMid) s |= id == ST_BUF_GI_RESERVOIRS_3;
    if (c.last_lean_composed) s |= id == ST_BUF_DI_DIFF_CURR_COLORS || id == ST_BUF_GI_DIFF_CURR_COLORS;
    *stale = s ? 1 : 0;
    return ST_OK;
}
int st_camera_write_buffer(StEngine* e, StHandle h, int id, const void* data, size_t bytes) {
    ST_REQUIRE(e && data && id >= 0 && id < ST_BUF_COUNT, "bad buffer id");
    Engine* en = E(e);
    ST_CAMERA(c, e, h);
    if (!en->has_device) return fail(ST_ERR_NO_DEVICE, "host-only engine has no camera buffers");
    ST_REQUIRE(bytes == c.plane_bytes[id], "size does not match the buffer");
    ST_HIP(hipSetDevice(en->device));
    ST_HIP(hipDeviceSynchronize());
    { const int rc = materialize_gi_history(c); if (rc) return rc; }
    ST_HIP(hipMemcpy(c.plane[id], data, bytes, hipMemcpyHostToDevice));
    if (id == ST_BUF_PRIM_SURFACE_MAP_A) c.surface_map_replaced[0] = true;
    if (id == ST_BUF_PRIM_SURFACE_MAP_B) c.surface_map_replaced[1] = true;
    return ST_OK;
}
int st_debug_variance_flags(StEngine* e, StHandle h, uint64_t* tile_mask_out, size_t capacity_tiles, size_t* tiles) {
    ST_REQUIRE(e && tiles, "null argument");
    Engine* en = E(e);
    ST_CAMERA(c, e, h);
    if (!en->has_device) return fail(ST_ERR_NO_DEVICE, "host-only engine");
    *tiles = c.tile_mask_tiles();
    if (!tile_mask_out) return ST_OK;
    ST_REQUIRE(capacity_tiles >= c.tile_mask_tiles(), "buffer too small");
    ST_HIP(hipSetDevice(en->device)); ST_HIP(hipDeviceSynchronize());
    ST_HIP(hipMemcpy(tile_mask_out, c.tile_mask.ptr, c.tile_mask_tiles() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return ST_OK;
}
int st_debug_set_pass_mask(StEngine* e, uint64_t mask) {
    ST_REQUIRE(e, "null engine");
    Engine* en = E(e);
    if (en->has_device) { ST_HIP(hipSetDevice(en->device)); for (auto& kv : en->cameras) { const int rc = materialize_gi_history(*kv.second); if (rc) return rc; } }
    en->pass_mask = mask;
    return ST_OK;
}
int st_debug_set_launch_filter(StEngine* e, uint64_t filter) {
    ST_REQUIRE(e, "null engine");
    E(e)->launch_filter = filter;
    return ST_OK;
}
int st_debug_last_launches(StEngine* e, uint64_t* out_bits, size_t capacity, size_t* count) {
    ST_REQUIRE(e && count, "null argument");
    const std::vector<uint64_t>& v = E(e)->last_launches;
    *count = v.size();
    for (size_t i = 0; i < v.size() && i < capacity && out_bits; i++) out_bits[i] = v[i];
    return ST_OK;
}
int st_engine_set_arithmetic(StEngine* e, int arithmetic) {
    ST_REQUIRE(e, "null engine");
    ST_REQUIRE(arithmetic == ST_ARITH_FAST || arithmetic == ST_ARITH_EXACT, "unknown arithmetic");
    Engine* en = E(e);
    if (en->arithmetic == arithmetic) return ST_OK;
    en->arithmetic = arithmetic;
    en->L = arithmetic == ST_ARITH_EXACT ? launchers_exact() : launchers_fast();
    if (en->has_device) {  // frames in flight finish with the tables they were launched with; the byte tables follow the build
        ST_HIP(hipSetDevice(en->device));
        ST_HIP(hipDeviceSynchronize());
        en->L.launch_build_byte_luts(static_cast<float*>(en->d_byte_luts.ptr), nullptr);
        ST_HIP(hipDeviceSynchronize());
        // the atmosphere LUTs are regenerated by the next render with the new build's routines
        en->atmosphere_initialized = false; en->sky_known = false;
    }
    return ST_OK;
}
int st_engine_get_tuning(StEngine* e, StTuning* out) { ST_REQUIRE(e && out, "null argument"); *out = E(e)->tuning; return ST_OK; }
int st_engine_set_tuning(StEngine* e, const StTuning* t) { ST_REQUIRE(e && t, "null argument"); return E(e)->set_tuning(*t); }
int st_engine_get_arithmetic(StEngine* e, int* out) { ST_REQUIRE(e && out, "null argument"); *out = E(e)->arithmetic; return ST_OK; }
int st_camera_ray_count(StEngine* e, StHandle h, uint64_t* out, int reset) {
    ST_REQUIRE(e && out, "null argument");
    Engine* en = E(e);
    ST_CAMERA(cam, e, h);
    if (!en->has_device) return fail(ST_ERR_NO_DEVICE, "host-only engine");
    unsigned long long host[2 * KS_COUNT];
    ST_HIP(hipSetDevice(en->device));
    ST_HIP(hipDeviceSynchronize());
    { const int rc2 = read_counters(cam, host); if (rc2) return rc2; }
    uint64_t total = 0;
    for (int i = 0; i < KS_COUNT; i++) total += host[2 * i];
    *out = total;
    if (reset) { ST_HIP(hipMemset(cam.counters.ptr, 0, kCounterBytes)); memset(cam.profiled_traversal_bytes, 0, sizeof(cam.profiled_traversal_bytes)); ST_HIP(hipDeviceSynchronize()); }
    return ST_OK;
}
int st_debug_read_scene(StEngine* e, int what, void* out, size_t capacity, size_t* written) {
    ST_REQUIRE(e, "null engine");
    Engine* en = E(e);
    const void* p; size_t bytes;
    if (SceneTree::debug_reads(what)) {   // the tree's buffers (0, 4, 6 - 17): it brings them up to date itself
        if (int rc = en->tree.debug_read(what, &p, &bytes)) return rc;
    } else {
        if (what == 1 && en->instances.any_host_stale()) en->bake_stale_on_host();   // instances the device moved: the host arrays catch up
        if (int rc = en->take_deferred_status()) return rc;   // (their posed triangles could not be read back)
        switch (what) {
            case 1: p = en->slots.triangles().data(); bytes = en->slots.size() * sizeof(HostTriangle); break;
            case 2: p = en->lights.table().data(); bytes = en->lights.table().size() * sizeof(GpuLight); break;
            case 3: p = en->materials.gpu().data(); bytes = en->materials.gpu().size() * sizeof(GpuMaterial); break;
            default: return fail(ST_ERR_INVALID_ARGUMENT, "unknown scene buffer");
        }
    }
    if (written) *written = bytes;
    if (!out) return ST_OK;
    ST_REQUIRE(capacity >= bytes, "buffer too small");
    if (bytes) memcpy(out, p, bytes);
    return ST_OK;
}
int st_debug_world(StEngine* e, uint32_t* light_count, uint32_t* next_frame) {
    ST_REQUIRE(e && light_count && next_frame, "null argument");
    *light_count = E(e)->lights.count(); *next_frame = E(e)->frame;
    return ST_OK;
}

int st_set_bvh_refresh(StEngine* e, int mode) {
    ST_REQUIRE(e, "null engine");
    ST_REQUIRE(mode == ST_BVH_REBUILD || mode == ST_BVH_REFIT || mode == ST_BVH_REFIT_DEVICE || mode == ST_BVH_BUILD_DEVICE || mode == ST_BVH_AUTO, "unknown refresh mode");
    E(e)->tree.set_refresh_mode(mode);
    return ST_OK;
}
int st_debug_device_builds(StEngine* e, uint64_t* ticks) { ST_REQUIRE(e && ticks, "null argument"); *ticks = E(e)->tree.device_build_ticks(); return ST_OK; }
int st_debug_device_tree_refits(StEngine* e, uint64_t* ticks) { ST_REQUIRE(e && ticks, "null argument"); *ticks = E(e)->tree.device_tree_refit_ticks(); return ST_OK; }
int st_debug_bvh_depth(StEngine* e, uint32_t* deepest_internal_chain, uint32_t* stack_entries) {
    ST_REQUIRE(e && deepest_internal_chain && stack_entries, "null argument");
    E(e)->tree.depth(deepest_internal_chain, stack_entries);
    return ST_OK;
}
int st_debug_walk_overflow(StEngine* e, uint64_t* overflows, uint32_t* wide_stack_entries, uint32_t* packets_off) {
    ST_REQUIRE(e && overflows && wide_stack_entries && packets_off, "null argument");
    if (E(e)->has_device && E(e)->walk_flags_host) {   // frames still in flight count too: wait for them, then look (the next st_tick reports what is found here)
        ST_HIP(hipSetDevice(E(e)->device)); ST_HIP(hipDeviceSynchronize());
        if ((E(e)->walk_flags_host[0] | E(e)->walk_flags_host[1]) != 0u) E(e)->note_walk_overflow();
    }
    *overflows = E(e)->walk_overflows; *wide_stack_entries = E(e)->wide_stack_entries_now(); *packets_off = E(e)->packets_overflowed ? 1u : 0u;
    return ST_OK;
}
int st_debug_auto_tree(StEngine* e, float* leaf_run_weight, uint32_t* first_tree_on_device) {
    ST_REQUIRE(e && leaf_run_weight && first_tree_on_device, "null argument");
    E(e)->tree.auto_tree(leaf_run_weight, first_tree_on_device);
    return ST_OK;
}
int st_debug_bvh_refits(StEngine* e, uint64_t* rebuilds, uint64_t* refits) {
    ST_REQUIRE(e && rebuilds && refits, "null argument");
    E(e)->tree.refit_stats(rebuilds, refits);
    return ST_OK;
}
int st_debug_bvh_device_refits(StEngine* e, uint64_t* device_refits) {
    ST_REQUIRE(e && device_refits, "null argument");
    *device_refits = E(e)->tree.device_refit_ticks();
    return ST_OK;
}
int st_debug_device_bakes(StEngine* e, uint64_t* ticks, uint64_t* triangles) {
    ST_REQUIRE(e && ticks && triangles, "null argument");
    *ticks = E(e)->device_bakes; *triangles = E(e)->device_baked_triangles;
    return ST_OK;
}
int st_debug_bvh_refresh(StEngine* e, uint64_t* primitives, uint64_t* reused) {
    ST_REQUIRE(e && primitives && reused, "null argument");
    E(e)->tree.refresh_stats(primitives, reused);
    return ST_OK;
}

// Streaming ceiling of this device by this library's own kernel: `iters` grid-stride float4 copies of `bytes` (src -> dst, both
// allocated here), best of them, as (bytes read + bytes written) / time in GB/s.
int st_debug_copy_bandwidth(StEngine* e, size_t bytes, int iters, double* out_gbps) {
    ST_REQUIRE(e && out_gbps && bytes >= 16 && iters > 0, "bad argument");
    Engine* en = E(e);
    if (!en->has_device) return fail(ST_ERR_NO_DEVICE, "host-only engine");
    ST_HIP(hipSetDevice(en->device));
    const size_t n = bytes / 16;
    void *src = nullptr, *dst = nullptr;
    ST_HIP(hipMalloc(&src, n * 16));
    if (hipMalloc(&dst, n * 16) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(src); return fail(ST_ERR_HIP, "hipMalloc(copy destination) failed"); }
    hipEvent_t t0 = nullptr, t1 = nullptr;
    int rc = ST_OK; double best = 0.0;
    if (hipMemset(src, 0x3c, n * 16) != hipSuccess || hipEventCreate(&t0) != hipSuccess || hipEventCreate(&t1) != hipSuccess) rc = fail(ST_ERR_HIP, "copy bandwidth set-up failed");
    for (int i = 0; rc == ST_OK && i < iters + 1; i++) {   // the first pass is a warm-up
        (void)hipEventRecord(t0, nullptr);
        en->L.launch_copy_float4(static_cast<float4*>(dst), static_cast<const float4*>(src), n, 256u * 16u, nullptr);
        (void)hipEventRecord(t1, nullptr);
        if (hipEventSynchronize(t1) != hipSuccess) { rc = fail(ST_ERR_HIP, "copy kernel failed"); break; }
        float ms = 0.0f; (void)hipEventElapsedTime(&ms, t0, t1);
        if (i > 0 && ms > 0.0f) best = std::max(best, 2.0 * (double)(n * 16) / (ms * 1e-3) / 1e9);
    }
    if (t0) (void)hipEventDestroy(t0);
    if (t1) (void)hipEventDestroy(t1);
    (void)hipFree(src); (void)hipFree(dst);
    *out_gbps = best;
    return rc;
}

int st_profile_enable(StEngine* e, int enabled) { ST_REQUIRE(e, "null engine"); E(e)->profiling = (enabled & 1) != 0; E(e)->count_bytes = (enabled & 2) != 0; E(e)->profile_group_atrous = (enabled & 4) != 0; E(e)->profile_kernel_events = (enabled & 8) != 0; return ST_OK; }
int st_profile_read(StEngine* e, StKernelProfile* out, size_t capacity, size_t* count, int reset) {
    ST_REQUIRE(e && out && count, "null argument");
    Engine* en = E(e);
    if (!en->has_device) return fail(ST_ERR_NO_DEVICE, "host-only engine");
    ST_HIP(hipSetDevice(en->device));
    const int rc = en->drain_profile();
    if (rc) return rc;
    // traversal bytes (the reference's used_memory, summed on the device) join the screen-space bytes per kernel
    ST_HIP(hipDeviceSynchronize());
    for (auto& kv : en->cameras) {
        CameraState& c = *kv.second;
        unsigned long long host[2 * KS_COUNT];
        { const int rc2 = read_counters(c, host); if (rc2) return rc2; }
        for (int i = 0; i < KS_COUNT; i++) {
            const unsigned long long total = host[2 * i + 1];
            if (total >= c.profiled_traversal_bytes[i]) {
                en->profile_totals[i].algorithmic_bytes += (double)(total - c.profiled_traversal_bytes[i]);
                en->profile_totals[i].traversal_bytes += (double)(total - c.profiled_traversal_bytes[i]);
            }
            c.profiled_traversal_bytes[i] = total;
        }
    }
    size_t n = 0;
    for (int i = 0; i < KS_COUNT && n < capacity; i++) {
        if (en->profile_totals[i].launches == 0 && en->profile_totals[i].traversal_bytes == 0.0) continue;  // bytes-only mode records no launches
        out[n] = en->profile_totals[i];
        n++;
    }
    *count = n;
    if (reset) en->reset_profile_totals();
    return ST_OK;
}

}  // extern "C"
