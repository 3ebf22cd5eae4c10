//! Raw bindings of include/strolle_hip.h (the C ABI of libstrolle_hip.so) and of the HIP runtime calls the present
//! step needs (allocation only: the copy itself is the library's, `st_camera_present_copy`). One `extern "C"` item per entry point; the comment names the `strolle::Engine` method it stands behind
//! (reference: strolle/src/lib.rs:132-395).
#![allow(non_camel_case_types, dead_code)]
use std::ffi::c_void;
use std::os::raw::c_char;

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct StMeshTriangle {
    pub positions: [[f32; 3]; 3],
    pub normals: [[f32; 3]; 3],
    pub uvs: [[f32; 2]; 3],
    pub tangents: [[f32; 4]; 3],
}

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct StMaterial {
    pub base_color: [f32; 4],
    pub emissive: [f32; 4],
    pub perceptual_roughness: f32,
    pub metallic: f32,
    pub reflectance: f32,
    pub ior: f32,
    pub base_color_texture: u64, // 0 = None
    pub emissive_texture: u64,
    pub metallic_roughness_texture: u64,
    pub normal_map_texture: u64,
    pub alpha_mode: u32, // 0 Opaque, 1 Blend
    pub _pad: u32,
}

pub const ST_LIGHT_POINT: u32 = 0;
pub const ST_LIGHT_SPOT: u32 = 1;

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct StLight {
    pub kind: u32,
    pub position: [f32; 3],
    pub radius: f32,
    pub color: [f32; 3],
    pub range: f32,
    pub direction: [f32; 3],
    pub angle: f32,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct StCamera {
    pub mode: u32,
    pub denoise: u32,
    pub depth: u32,
    pub width: u32,
    pub height: u32,
    pub pos_x: u32,
    pub pos_y: u32,
    pub _pad: u32,
    pub transform: [f32; 16],  // glam Mat4::to_cols_array
    pub projection: [f32; 16],
}

pub const ST_OK: i32 = 0;
pub const ST_FORMAT_RGBA32F: i32 = 0;
pub const ST_FORMAT_RGBA16F: i32 = 1;
pub const ST_FORMAT_RGBA8_UNORM_SRGB: i32 = 2;
pub const ST_FORMAT_BGRA8_UNORM_SRGB: i32 = 3;

pub const ST_ERR_BVH_TOO_DEEP: i32 = 10; // st_tick: the tree is deeper than the kernels' traversal stack (uploaded all the same)
pub const ST_ERR_DIST: i32 = 11;

/// include/strolle_hip.h StTuning: scheduling / tuning switches of one engine (get, change, set).
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct StTuning {
    pub struct_size: u32,
    pub overlap: u32,
    pub fuse: u32,
    pub fuse_di_head: u32,
    pub fuse_spatial: u32,
    pub fuse_gi_sampling: u32,
    pub fuse_gi_validation: u32,
    pub fuse_gi_reprojection: u32,
    pub fuse_wavelet: u32,
    pub fuse_compose: u32,
    pub preview_both: u32,
    pub variance_in_reproject: u32,
    pub lean_frame: u32,
    pub skip_scratch_stores: u32,
    pub di_head_on_main: u32,
    pub alias_gi_history: u32,
    pub tile_map: u32,
    pub tile_map_denoise: u32,
    pub side_priority: i32,
    pub staging: u32,
    pub double_buffer: u32,
    pub packed_base: u32,
    pub tick_timing: u32,
    pub anyhit_fast: u32,
    pub compact_bvh: u32,
    pub allow_deep_bvh: u32,
    pub device_bake: u32,
    pub wide_bvh: u32,
    pub wide_stack_entries: u32,
    pub primary_packets: u32,
    pub side_start: u32,
}

/// [x0, x1) x [y0, y1) in pixels (st_dist_partition / st_dist_window)
/// A (cost-weighted) tile grid every rank holds identically (st_dist_grid / st_dist_grid_rebalance / st_dist_set_grid)
#[repr(C)]
#[derive(Clone, Copy, PartialEq, Eq, Debug)]
pub struct StDistGrid {
    pub cols: u32,
    pub rows: u32,
    pub row_edge: [u32; 17],
    pub col_edge: [[u32; 17]; 16],
}

#[repr(C)]
#[derive(Clone, Copy, Default, PartialEq, Eq, Debug)]
pub struct StDistRect {
    pub x0: u32,
    pub y0: u32,
    pub x1: u32,
    pub y1: u32,
}

/// ncclUniqueId: rank 0 makes one (st_dist_unique_id) and hands it to the other processes by the host's own means
#[repr(C)]
#[derive(Clone, Copy)]
pub struct StDistUniqueId {
    pub internal: [c_char; 128],
}

pub enum StEngine {}

// st_scene_trace_rays flags
pub const ST_RAY_COHERENT: u32 = 1;
pub const ST_RAY_MAPPED_NORMAL: u32 = 2; // StRayHit.normal bent by the material's normal map

extern "C" {
    pub fn st_engine_create(device_ordinal: i32, out: *mut *mut StEngine) -> i32; // Engine::new
    pub fn st_engine_destroy(e: *mut StEngine); // Drop
    pub fn st_last_error() -> *const c_char;
    pub fn st_build_commit() -> *const c_char;
    pub fn st_mesh_insert(e: *mut StEngine, id: u64, triangles: *const StMeshTriangle, count: usize) -> i32; // insert_mesh
    pub fn st_mesh_remove(e: *mut StEngine, id: u64) -> i32; // remove_mesh
    pub fn st_material_insert(e: *mut StEngine, id: u64, material: *const StMaterial) -> i32; // insert_material
    pub fn st_material_has(e: *mut StEngine, id: u64) -> i32; // has_material
    pub fn st_material_remove(e: *mut StEngine, id: u64) -> i32; // remove_material
    pub fn st_image_insert_rgba8(e: *mut StEngine, id: u64, w: u32, h: u32, rgba: *const u8, srgb: i32) -> i32; // insert_image
    pub fn st_image_insert_device_rgba8(e: *mut StEngine, id: u64, w: u32, h: u32, device_rgba: *const c_void, row_pitch: usize, is_dynamic: i32) -> i32;
    pub fn st_image_remove(e: *mut StEngine, id: u64) -> i32; // remove_image
    pub fn st_instance_insert(e: *mut StEngine, id: u64, mesh: u64, material: u64, xform12: *const f32) -> i32; // insert_instance
    pub fn st_instance_remove(e: *mut StEngine, id: u64) -> i32; // remove_instance
    pub fn st_light_insert(e: *mut StEngine, id: u64, light: *const StLight) -> i32; // insert_light
    pub fn st_light_remove(e: *mut StEngine, id: u64) -> i32; // remove_light
    pub fn st_sun_update(e: *mut StEngine, azimuth: f32, altitude: f32) -> i32; // update_sun
    pub fn st_camera_create(e: *mut StEngine, camera: *const StCamera, out: *mut u64) -> i32; // create_camera
    pub fn st_camera_update(e: *mut StEngine, camera: u64, desc: *const StCamera) -> i32; // update_camera
    pub fn st_camera_delete(e: *mut StEngine, camera: u64) -> i32; // delete_camera
    pub fn st_camera_set_output_format(e: *mut StEngine, camera: u64, format: i32) -> i32; // Camera::viewport.format
    pub fn st_tick(e: *mut StEngine, hip_stream: *mut c_void) -> i32; // tick
    pub fn st_render_camera(e: *mut StEngine, camera: u64, out_device: *mut c_void, hip_stream: *mut c_void) -> i32; // render_camera
    // the present hand-over (present.rs): frame N leaves for host memory behind its composition while frame N+1 renders
    pub fn st_camera_present_copy(e: *mut StEngine, camera: u64, src_device: *const c_void, dst_host: *mut c_void, bytes: usize, hip_stream: *mut c_void) -> i32;
    pub fn st_camera_present_ready(e: *mut StEngine, camera: u64, dst_host: *const c_void, wait: i32, ready: *mut i32) -> i32;
    pub fn st_set_seed(e: *mut StEngine, seed: u64) -> i32;
    pub fn st_set_blue_noise(e: *mut StEngine, rgba: *const u8, bytes: usize) -> i32; // Noise::new (noise.rs:40-50)
    pub fn st_engine_set_arithmetic(e: *mut StEngine, arithmetic: i32) -> i32;
    pub fn st_set_bvh_refresh(e: *mut StEngine, mode: i32) -> i32; // 0 rebuild, 1 refit, 2 refit on the device, 3 build on the device (ST_BVH_BUILD_DEVICE), 4 the default (ST_BVH_AUTO: first tree on the host unless its leaf runs are long, changes on the device)
    pub fn st_debug_walk_overflow(e: *mut StEngine, overflows: *mut u64, wide_stack_entries: *mut u32, packets_off: *mut u32) -> i32;
    pub fn st_debug_auto_tree(e: *mut StEngine, leaf_run_weight: *mut f32, first_tree_on_device: *mut u32) -> i32;
    pub fn st_debug_device_builds(e: *mut StEngine, ticks: *mut u64) -> i32;
    pub fn st_debug_device_tree_refits(e: *mut StEngine, ticks: *mut u64) -> i32;
    pub fn st_engine_get_tuning(e: *mut StEngine, out: *mut StTuning) -> i32;
    pub fn st_engine_set_tuning(e: *mut StEngine, tuning: *const StTuning) -> i32;
    // multi-GPU behind the boundary: one process per GPU, tiles + ONE gather to rank 0 over RCCL (dist.rs)
    pub fn st_camera_set_window(e: *mut StEngine, camera: u64, x0: u32, y0: u32, x1: u32, y1: u32) -> i32;
    pub fn st_dist_partition(width: u32, height: u32, world: u32, cols: u32, rank: u32, owned: *mut StDistRect) -> i32;
    pub fn st_dist_window(width: u32, height: u32, owned: *const StDistRect, apron: u32, window: *mut StDistRect) -> i32;
    pub fn st_dist_unique_id(out: *mut StDistUniqueId) -> i32;
    pub fn st_dist_init(e: *mut StEngine, rank: i32, world: i32, id: *const StDistUniqueId) -> i32;
    pub fn st_dist_shutdown(e: *mut StEngine) -> i32;
    pub fn st_dist_set_partition(e: *mut StEngine, camera: u64, cols: u32, apron: u32, owned: *mut StDistRect, window: *mut StDistRect) -> i32;
    pub fn st_dist_grid(width: u32, height: u32, world: u32, cols: u32, out: *mut StDistGrid) -> i32;
    pub fn st_dist_grid_tile(grid: *const StDistGrid, rank: u32, owned: *mut StDistRect) -> i32;
    pub fn st_dist_grid_rebalance(width: u32, height: u32, current: *const StDistGrid, tile_cost: *const f32, max_step: u32, out: *mut StDistGrid) -> i32;
    pub fn st_dist_set_grid(e: *mut StEngine, camera: u64, grid: *const StDistGrid, apron: u32, owned: *mut StDistRect, window: *mut StDistRect) -> i32;
    pub fn st_dist_gather(e: *mut StEngine, camera: u64, frame: *const c_void, full_on_root: *mut c_void, hip_stream: *mut c_void) -> i32;
    pub fn st_dist_wait(e: *mut StEngine, camera: u64, frame: *const c_void, hip_stream: *mut c_void, host_wait: i32) -> i32;
}

// ---- environment lighting: an equirectangular HDR map in place of the atmosphere (include/strolle_hip.h "environment lighting")
pub const ST_ENV_KEEP_SUN: u32 = 1;
pub const ST_ENV_UNIFORM_SAMPLING: u32 = 2;
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct StEnvironmentDesc {
    pub struct_size: u32,
    pub flags: u32,
    pub intensity: f32,
    pub yaw: f32,
}
extern "C" {
    pub fn st_environment_set(e: *mut StEngine, texels: *const f32, width: u32, height: u32, channels: u32, desc: *const StEnvironmentDesc) -> i32;
    pub fn st_environment_set_device(e: *mut StEngine, texels_device: *const c_void, width: u32, height: u32, channels: u32, row_pitch_bytes: usize, desc: *const StEnvironmentDesc) -> i32;
    pub fn st_environment_update(e: *mut StEngine, desc: *const StEnvironmentDesc) -> i32;
    pub fn st_environment_clear(e: *mut StEngine) -> i32;
    pub fn st_decode_hdr(bytes: *const c_void, size: usize, out_rgb: *mut f32, capacity_floats: usize, width: *mut u32, height: *mut u32) -> i32;
    pub fn st_debug_environment_eval(e: *mut StEngine, dirs_device: *const f32, n: u32, rgb_device: *mut f32, hip_stream: *mut c_void) -> i32;
    pub fn st_debug_environment_sample(e: *mut StEngine, u_device: *const f32 /* triples */, n: u32, dir_pdf_device: *mut f32, hip_stream: *mut c_void) -> i32;
    pub fn st_debug_environment_pdf(e: *mut StEngine, dirs_device: *const f32, n: u32, pdf_device: *mut f32, hip_stream: *mut c_void) -> i32;
    pub fn st_debug_environment_sanitized(e: *mut StEngine, texels: *mut u64) -> i32;
    pub fn st_debug_environment_table(e: *mut StEngine, table: *mut c_void, capacity_bytes: usize, cells_x: *mut u32, cells_y: *mut u32) -> i32;
}

// display transforms (include/strolle_hip.h "display transforms"): exposure, tone mapping and auto-exposure of a camera's output
pub const ST_TONEMAP_NONE: u32 = 0;
pub const ST_TONEMAP_REINHARD: u32 = 1;
pub const ST_TONEMAP_REINHARD_LUMINANCE: u32 = 2;
pub const ST_TONEMAP_ACES_FITTED: u32 = 3;
pub const ST_TONEMAP_PBR_NEUTRAL: u32 = 4;
pub const ST_DISPLAY_AUTO_EXPOSURE: u32 = 1;
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct StDisplayDesc {
    pub struct_size: u32,
    pub tonemap: u32,
    pub flags: u32,
    pub exposure_ev: f32,
    pub ev_min: f32,
    pub ev_max: f32,
    pub low_fraction: f32,
    pub high_fraction: f32,
    pub max_ev_step_up: f32,
    pub max_ev_step_down: f32,
}
extern "C" {
    pub fn st_camera_set_display(e: *mut StEngine, camera: u64, desc: *const StDisplayDesc) -> i32; // null = off
    pub fn st_camera_get_display(e: *mut StEngine, camera: u64, out: *mut StDisplayDesc, enabled: *mut i32) -> i32;
    pub fn st_camera_exposure(e: *mut StEngine, camera: u64, scale: *mut f32, metered_ev: *mut f32, adapted_ev: *mut f32) -> i32;
    pub fn st_debug_camera_histogram(e: *mut StEngine, camera: u64, bins: *mut u32) -> i32;
}

// ---- deformation motion (include/strolle_hip.h "skinned meshes"): off by default
extern "C" {
    pub fn st_engine_set_deformation_motion(e: *mut StEngine, enabled: i32) -> i32;
    pub fn st_engine_get_deformation_motion(e: *mut StEngine, enabled: *mut i32) -> i32;
    pub fn st_engine_set_normal_mapping(e: *mut StEngine, enabled: i32) -> i32;
    pub fn st_engine_get_normal_mapping(e: *mut StEngine, enabled: *mut i32) -> i32;
    pub fn st_debug_deformation(e: *mut StEngine, instances_with_previous: *mut u64, previous_bytes: *mut u64) -> i32;
}

// ---- morph targets (include/strolle_hip.h "morph targets"): targets per mesh, weights per instance, applied on the device at the next tick
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct StMorphDelta {
    pub position: [f32; 3],
    pub normal: [f32; 3],
}
extern "C" {
    pub fn st_mesh_set_morph_targets(e: *mut StEngine, mesh: u64, deltas: *const StMorphDelta, corner_count: usize, target_count: u32) -> i32;
    pub fn st_instance_set_morph_weights(e: *mut StEngine, instance: u64, weights: *const f32, target_count: u32) -> i32; // null / 0 = the base shape
    pub fn st_debug_morphing(e: *mut StEngine, ticks: *mut u64, triangles: *mut u64, delta_bytes: *mut u64) -> i32;
}

// output post-processing (include/strolle_hip.h "post-processing"): FXAA and resampling of a camera's output
pub const ST_RESAMPLE_NEAREST: u32 = 0;
pub const ST_RESAMPLE_BILINEAR: u32 = 1;
pub const ST_RESAMPLE_CATMULL_ROM: u32 = 2;
pub const ST_POST_FXAA: u32 = 1;
pub const ST_PASS_POST: u64 = 1 << 30;
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct StPostDesc {
    pub struct_size: u32,
    pub flags: u32,
    pub output_width: u32,
    pub output_height: u32,
    pub filter: u32,
    pub fxaa_edge_threshold: f32,
    pub fxaa_edge_threshold_min: f32,
    pub fxaa_subpixel: f32,
}
extern "C" {
    pub fn st_camera_set_post(e: *mut StEngine, camera: u64, desc: *const StPostDesc) -> i32; // null = off
    pub fn st_camera_get_post(e: *mut StEngine, camera: u64, out: *mut StPostDesc, enabled: *mut i32) -> i32;
    pub fn st_camera_output_size(e: *mut StEngine, camera: u64, width: *mut u32, height: *mut u32) -> i32;
    pub fn st_post_process(e: *mut StEngine, desc: *const StPostDesc, src_rgba32f_device: *const c_void, width: u32, height: u32, dst_device: *mut c_void, dst_format: i32, hip_stream: *mut c_void) -> i32;
}

// the upscale stage (include/strolle_hip.h "upscaling"): the edge-adaptive upscaler and contrast-adaptive sharpening behind FXAA
pub const ST_UPSCALE_DENOISE: u32 = 1;
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct StUpscaleDesc {
    pub struct_size: u32,
    pub flags: u32,
    pub output_width: u32,
    pub output_height: u32,
    pub sharpness: f32,
    pub _pad: [u32; 3],
}
extern "C" {
    pub fn st_camera_set_upscale(e: *mut StEngine, camera: u64, desc: *const StUpscaleDesc) -> i32; // null = off
    pub fn st_camera_get_upscale(e: *mut StEngine, camera: u64, out: *mut StUpscaleDesc, enabled: *mut i32) -> i32;
    pub fn st_upscale_process(e: *mut StEngine, desc: *const StUpscaleDesc, src_rgba32f_device: *const c_void, width: u32, height: u32, dst_device: *mut c_void, dst_format: i32, hip_stream: *mut c_void) -> i32;
    pub fn st_debug_set_upscale_fused(e: *mut StEngine, tile: i32) -> i32; // 0 = two launches, 1 / 2 / 3 = one launch over 64 x 8 / 32 x 32 / 64 x 16 tiles
}

// bloom (include/strolle_hip.h "bloom"): an HDR mip-pyramid glow in front of the display transform
pub const ST_BLOOM_ADDITIVE: u32 = 1;
pub const ST_BLOOM_FIREFLY_SUPPRESS: u32 = 2;
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct StBloomDesc {
    pub struct_size: u32,
    pub flags: u32,
    pub levels: u32,
    pub intensity: f32,
    pub low_frequency_boost: f32,
    pub low_frequency_boost_curvature: f32,
    pub high_pass_frequency: f32,
    pub threshold: f32,
    pub threshold_softness: f32,
    pub clamp: f32,
}
extern "C" {
    pub fn st_camera_set_bloom(e: *mut StEngine, camera: u64, desc: *const StBloomDesc) -> i32; // null = off
    pub fn st_camera_get_bloom(e: *mut StEngine, camera: u64, out: *mut StBloomDesc, enabled: *mut i32) -> i32;
    pub fn st_bloom_plan(desc: *const StBloomDesc, width: u32, height: u32, levels: *mut u32, sizes_wh: *mut u32, factors: *mut f32) -> i32;
    pub fn st_debug_set_bloom_tail(e: *mut StEngine, lds_bytes: i32, in_force: *mut u32) -> i32;
    pub fn st_bloom_process(e: *mut StEngine, desc: *const StBloomDesc, display: *const StDisplayDesc, src_rgba32f_device: *const c_void, width: u32, height: u32, dst_device: *mut c_void, dst_format: i32, hip_stream: *mut c_void) -> i32;
}

// motion blur (include/strolle_hip.h "motion blur"): a velocity-driven gather in front of bloom
pub const ST_MOTION_BLUR_NO_JITTER: u32 = 1;
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct StMotionBlurDesc {
    pub struct_size: u32,
    pub flags: u32,
    pub samples: u32,
    pub shutter: f32,
    pub max_radius: f32,
    pub depth_softness: f32,
}
extern "C" {
    pub fn st_camera_set_motion_blur(e: *mut StEngine, camera: u64, desc: *const StMotionBlurDesc) -> i32; // null = off
    pub fn st_camera_get_motion_blur(e: *mut StEngine, camera: u64, out: *mut StMotionBlurDesc, enabled: *mut i32) -> i32;
    pub fn st_motion_blur_process(e: *mut StEngine, desc: *const StMotionBlurDesc, display: *const StDisplayDesc, color_device: *const c_void, velocity_device: *const c_void, depth_device: *const c_void, width: u32, height: u32, dst_device: *mut c_void, dst_format: i32, hip_stream: *mut c_void) -> i32;
}

// depth of field (include/strolle_hip.h "depth of field"): a thin-lens circle-of-confusion gather in front of motion blur
pub const ST_DOF_AUTOFOCUS: u32 = 1;
pub const ST_DOF_PLANAR_DEPTH: u32 = 2;
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct StDofDesc {
    pub struct_size: u32,
    pub flags: u32,
    pub samples: u32,
    pub focal_distance: f32,
    pub aperture_f_stops: f32,
    pub sensor_height: f32,
    pub max_radius: f32,
    pub focus_x: f32,
    pub focus_y: f32,
    pub _pad: u32,
}
extern "C" {
    pub fn st_camera_set_dof(e: *mut StEngine, camera: u64, desc: *const StDofDesc) -> i32; // null = off
    pub fn st_camera_get_dof(e: *mut StEngine, camera: u64, out: *mut StDofDesc, enabled: *mut i32) -> i32;
    pub fn st_dof_plan(desc: *const StDofDesc, width: u32, height: u32, samples: *mut u32, tiles_xy: *mut u32, taps_xyr: *mut f32) -> i32; // pure host
    pub fn st_dof_process(e: *mut StEngine, desc: *const StDofDesc, display: *const StDisplayDesc, projection: *const f32, color_device: *const c_void, depth_device: *const c_void, width: u32, height: u32, dst_device: *mut c_void, dst_format: i32, hip_stream: *mut c_void) -> i32;
}

// fog (include/strolle_hip.h "fog"): distance and height fog in front of depth of field
pub const ST_FOG_LINEAR: u32 = 0;
pub const ST_FOG_EXPONENTIAL: u32 = 1;
pub const ST_FOG_EXPONENTIAL_SQUARED: u32 = 2;
pub const ST_FOG_ATMOSPHERIC: u32 = 3;
pub const ST_FOG_SKY: u32 = 1;
pub const ST_FOG_FOLLOW_SUN: u32 = 2;
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct StFogDesc {
    pub struct_size: u32,
    pub falloff: u32,
    pub flags: u32,
    pub _pad: u32,
    pub color: [f32; 4],
    pub start: f32,
    pub end: f32,
    pub density: f32,
    pub height_falloff: f32,
    pub height_reference: f32,
    pub sky_distance: f32,
    pub extinction: [f32; 3],
    pub inscattering: [f32; 3],
    pub light_color: [f32; 3],
    pub light_exponent: f32,
    pub light_direction: [f32; 3],
    pub _pad2: f32,
}
extern "C" {
    pub fn st_camera_set_fog(e: *mut StEngine, camera: u64, desc: *const StFogDesc) -> i32; // null = off
    pub fn st_camera_get_fog(e: *mut StEngine, camera: u64, out: *mut StFogDesc, enabled: *mut i32) -> i32;
    pub fn st_fog_process(e: *mut StEngine, desc: *const StFogDesc, display: *const StDisplayDesc, transform: *const f32, projection: *const f32, color_device: *const c_void, depth_device: *const c_void, width: u32, height: u32, dst_device: *mut c_void, dst_format: i32, hip_stream: *mut c_void) -> i32;
}

// light shafts (include/strolle_hip.h "light shafts"): shadowed in-scattering between fog and depth of field
pub const ST_SHAFTS_FOLLOW_SUN: u32 = 1;
pub const ST_SHAFTS_LIGHT_EXTINCTION: u32 = 2;
pub const ST_SHAFTS_MAX_LIGHTS: usize = 8;
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct StLightShaftsDesc {
    pub struct_size: u32,
    pub flags: u32,
    pub steps: u32,
    pub divisor: u32,
    pub density: f32,
    pub anisotropy: f32,
    pub max_distance: f32,
    pub intensity: f32,
    pub scatter: [f32; 3],
    pub _pad: f32,
    pub sun_color: [f32; 3],
    pub _pad2: f32,
    pub sun_direction: [f32; 3],
    pub light_count: u32,
    pub lights: [u64; 8],
}
extern "C" {
    pub fn st_camera_set_light_shafts(e: *mut StEngine, camera: u64, desc: *const StLightShaftsDesc) -> i32; // null = off
    pub fn st_camera_get_light_shafts(e: *mut StEngine, camera: u64, out: *mut StLightShaftsDesc, enabled: *mut i32) -> i32;
    pub fn st_light_shafts_plan(desc: *const StLightShaftsDesc, width: u32, height: u32, cells_wh: *mut u32, jitter: *mut f32) -> i32; // pure host
    pub fn st_light_shafts_process(e: *mut StEngine, desc: *const StLightShaftsDesc, display: *const StDisplayDesc, transform: *const f32, projection: *const f32, color_device: *const c_void, depth_device: *const c_void, width: u32, height: u32, dst_device: *mut c_void, dst_format: i32, hip_stream: *mut c_void) -> i32;
}

// colour grading (include/strolle_hip.h "colour grading"): white balance, contrast, CDL, a 3-D LUT and dither around the display transform
pub const ST_GRADE_DITHER: u32 = 1;
pub const ST_LUT_DOMAIN_UNIT: u32 = 0;
pub const ST_LUT_DOMAIN_LOG2: u32 = 1;
pub const ST_GRADE_STEP_WHITE_BALANCE: u32 = 1;
pub const ST_GRADE_STEP_CONTRAST: u32 = 2;
pub const ST_GRADE_STEP_SATURATION: u32 = 4;
pub const ST_GRADE_STEP_CDL: u32 = 8;
pub const ST_GRADE_STEP_LUT: u32 = 16;
pub const ST_GRADE_STEP_DITHER: u32 = 32;
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct StColorGradingDesc {
    pub struct_size: u32,
    pub flags: u32,
    pub temperature: f32,
    pub tint: f32,
    pub contrast: f32,
    pub saturation: f32,
    pub slope: [f32; 3],
    pub offset: [f32; 3],
    pub power: [f32; 3],
    pub cdl_saturation: f32,
    pub lut: u64,
    pub lut_domain: u32,
    pub lut_ev_min: f32,
    pub lut_ev_max: f32,
    pub lut_strength: f32,
    pub _pad: [u32; 2],
}
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct StColorGradingPlan {
    pub steps: u32,
    pub white_balance: [f32; 9],
    pub lut_inv_range: f32,
    pub _pad: u32,
}
extern "C" {
    pub fn st_camera_set_color_grading(e: *mut StEngine, camera: u64, desc: *const StColorGradingDesc) -> i32; // null = off
    pub fn st_camera_get_color_grading(e: *mut StEngine, camera: u64, out: *mut StColorGradingDesc, enabled: *mut i32) -> i32;
    pub fn st_lut_insert(e: *mut StEngine, id: u64, size: u32, rgb: *const f32) -> i32;
    pub fn st_lut_remove(e: *mut StEngine, id: u64) -> i32;
    pub fn st_color_grading_plan(desc: *const StColorGradingDesc, out: *mut StColorGradingPlan) -> i32; // pure host
    pub fn st_color_grading_process(e: *mut StEngine, desc: *const StColorGradingDesc, display: *const StDisplayDesc, lut_rgba_device: *const c_void, lut_size: u32, src_rgba32f_device: *const c_void, width: u32, height: u32, dst_device: *mut c_void, dst_format: i32, hip_stream: *mut c_void) -> i32;
    pub fn st_decode_cube(bytes: *const c_void, size: usize, out_rgb: *mut f32, capacity_floats: usize, lut_size: *mut u32) -> i32;
}

// lens effects (include/strolle_hip.h "lens effects"): distortion, fringing, vignette and film grain between bloom and colour grading
pub const ST_LENS_FIT: u32 = 1;
pub const ST_LENS_VIGNETTE_ROUND: u32 = 2;
pub const ST_LENS_GRAIN_ANIMATE: u32 = 4;
pub const ST_LENS_STEP_DISTORTION: u32 = 1;
pub const ST_LENS_STEP_FRINGE: u32 = 2;
pub const ST_LENS_STEP_VIGNETTE: u32 = 4;
pub const ST_LENS_STEP_GRAIN: u32 = 8;
pub const ST_LENS_MAX_TAPS: u32 = 16;
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct StLensDesc {
    pub struct_size: u32,
    pub flags: u32,
    pub k1: f32,
    pub k2: f32,
    pub scale: f32,
    pub fringe: f32,
    pub fringe_taps: u32,
    pub vignette_intensity: f32,
    pub vignette_falloff: f32,
    pub grain_intensity: f32,
    pub grain_size: u32,
    pub grain_seed: u32,
}
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct StLensPlan {
    pub steps: u32,
    pub taps: u32,
    pub cx: f32,
    pub cy: f32,
    pub inv_hd2: f32,
    pub fit: f32,
    pub scale_eff: f32,
    pub tap_scale: [f32; 16],
    pub tap_weight: [[f32; 3]; 16],
}
extern "C" {
    pub fn st_camera_set_lens(e: *mut StEngine, camera: u64, desc: *const StLensDesc) -> i32; // null = off
    pub fn st_camera_get_lens(e: *mut StEngine, camera: u64, out: *mut StLensDesc, enabled: *mut i32) -> i32;
    pub fn st_lens_plan(desc: *const StLensDesc, width: u32, height: u32, out: *mut StLensPlan) -> i32; // pure host
    pub fn st_lens_process(e: *mut StEngine, desc: *const StLensDesc, display: *const StDisplayDesc, src_rgba32f_device: *const c_void, width: u32, height: u32, dst_device: *mut c_void, dst_format: i32, hip_stream: *mut c_void) -> i32;
    pub fn st_debug_set_lens_gather(e: *mut StEngine, force: i32) -> i32;
}

// ---- the HIP runtime, as far as the staging-copy present needs it (libamdhip64)
pub type hipStream_t = *mut c_void;
extern "C" {
    pub fn hipMalloc(ptr: *mut *mut c_void, bytes: usize) -> i32;
    pub fn hipFree(ptr: *mut c_void) -> i32;
    pub fn hipHostMalloc(ptr: *mut *mut c_void, bytes: usize, flags: u32) -> i32;
    pub fn hipHostFree(ptr: *mut c_void) -> i32;
    pub fn hipStreamCreate(stream: *mut hipStream_t) -> i32;
    pub fn hipStreamDestroy(stream: hipStream_t) -> i32;
}
