// st_types.h — PODs shared by the host engine and the kernels (device buffer layouts).
#pragma once
#include "st_math.h"

namespace st {

// strolle-gpu/src/camera.rs:9-17 (160 B uniform)
struct GpuCamera {
    M4 projection_view;
    M4 ndc_to_world;
    float4 origin;
    float4 screen;
};
static_assert(sizeof(GpuCamera) == 160, "Camera uniform is 160 B");

// strolle-gpu/src/material.rs:8-23 (112 B)
struct GpuMaterial {
    float4 base_color, base_color_texture, emissive, emissive_texture;
    float roughness, metallic, reflectance, ior;
    float4 metallic_roughness_texture, normal_map_texture;
};
static_assert(sizeof(GpuMaterial) == 112, "Material is 112 B");

// strolle-gpu/src/light.rs:12-43 (112 B)
struct GpuLight { float4 d0, d1, d2, d3, prev_d0, prev_d1, prev_d2; };
static_assert(sizeof(GpuLight) == 112, "Light is 112 B");

// The reference's 144-B AoS triangle (strolle-gpu/src/triangle.rs:9-21), kept on the HOST only (debug
// read-back + BVH build). The device gets:
//   tri_attr[4 float4 / triangle]: (n0, uv0.x) (n1, uv0.y) (n2, uv1.x) (uv1.y, uv2.x, uv2.y, instance slot)
//     fetched once per ray, for the winning triangle only;
//   the hit-test record (v0.xyz, 0) (v1-v0, 0) (v2-v0, 0) — all a hit test reads (48 B) — inline in the BVH stream:
// device BVH stream: the serializer's stream (bvh/serializer.rs:20-110, what st_debug_bvh_stream returns and the
//   stream-contract test compares) re-laid so that EVERY entry is four float4 and entry k starts at texel 4 k:
//     internal node  (min0.xyz, 0) (max0.xyz, far child's byte offset) (min1.xyz, -) (max1.xyz, -)   the near child is the next entry
//     leaf entry     (flags, triangle, material, marker != 0) (v0.xyz, 0) (v1-v0, 0) (v2-v0, 0)   flags & 1: another
//                    entry of the same leaf follows
//   One 64-B fetch per traversal step, whichever kind the entry is; traversal pointers are byte offsets into this form
//   (the per-lane stack keeps entry numbers). Visiting order and the `used_memory` count are those of the serializer's stream.
struct HostTriangle { float4 d0, d1, d2, d3, d4, d5, d6, d7, d8; };
static_assert(sizeof(HostTriangle) == 144, "Triangle is 144 B");

// KArgs::lean bits
constexpr uint32_t kRefitBatch = 512;  // leaves one workgroup of k_bvh_refit takes (st_engine.cpp index_device_tree): 26 KB of LDS
constexpr uint32_t kLeanPrim = 1u;     // primary visibility + frame reprojection in one launch: the velocity map (consumed in registers) and the
                                       // encoded surface map (every kernel reads its decoded twin, KArgs::sn) stay unwritten
constexpr uint32_t kLeanSamples = 2u;  // di / gi diffuse sample planes: the fused denoise-reproject stages consume them in registers
constexpr uint32_t kLeanGiRes2 = 4u;   // tracing frames: the reprojected GI reservoirs the fused temporal pass consumes in registers (on odd
                                       // tracing frames the spatial pass rewrites the whole plane anyway — given an even tile count AND an even width)
constexpr uint32_t kLeanGiMid = 8u;    // both GI preview passes in one launch: a first-pass result that is a plain normalisation of its input (the pixel drew
                                       // no neighbour: every pixel once the reservoirs have history) is not stored to GI_RESERVOIRS_3; the few pixels
                                       // whose second pass does resample rebuild such a neighbour's record from the pass's input (KArgs::gi_mid_src)
constexpr uint32_t kLeanKeepVelocity = 16u;   // with kLeanPrim, while the camera blurs (st_motion_blur.cpp): primary visibility stores the velocity map after all; the
                                       // pack launch of the motion blur reads it. Nothing else about the lean frame changes
constexpr int kBvhStackSize = 24;  // strolle-gpu/src/lib.rs:76
constexpr int kBvhStackSizeDeep = 32;  // trees whose deepest chain of internal nodes exceeds kBvhStackSize (st_bvh_refresh.cpp measure_stack_need)
constexpr uint32_t kLightIdSky = 0xffffffffu;
constexpr uint32_t kLdsSceneTexels = 448;  // device streams up to this many float4 are copied into LDS by the tracing kernels (7 KiB per block: 112 entries, e.g. 56 one-triangle leaves + 55 internal nodes)
constexpr uint32_t kLdsLights = 16;  // lights the tracing kernels keep in LDS (k_common.h ST_SCENE_PROLOGUE)
constexpr uint32_t kCounterLines = 256;  // ray/byte counters are spread over this many 64-B lines per kernel slot

// One cell of the environment map's importance table (Vose alias table, built on the host from the device's luminance grid): with
// probability q the cell itself, else `alias`; p = the cell's own probability (the solid-angle pdf is p * cells / (2 pi^2 sin theta)).
struct EnvCell { float q; uint32_t alias; float p; };
static_assert(sizeof(EnvCell) == 12, "an importance cell is 12 B");

// Camera display transform (include/strolle_hip.h "display transforms"; st_display.cpp, k_display.hip). `on` == 0: the composing kernels
// are the parent's instantiations, which never read the rest. With `meter` set the kernels take the scale from the camera's device state
// (DisplayState::scale, written by the previous frame's finalize) and add their pixels to `hist`.
constexpr uint32_t kDisplayBins = 64;
constexpr uint32_t kDisplayRaw = 0xffffffffu;   // DisplayArgs::tonemap of a frame that blooms: meter, store the composed colour as it is (k_bloom.hip transforms it later)
struct DisplayArgs {
    uint32_t on, tonemap, meter;
    float scale;               // manual: 2^exposure_ev (rounded from double on the host)
    const float* state;        // meter: the DisplayState below
    uint32_t* hist;            // meter: kDisplayReplicas x kDisplayBins counters, cleared by the finalize kernel
    float ev_min, bins_per_ev; // meter: bin = floor((log2 Y - ev_min) * bins_per_ev), clamped to [0, 63]
};
// One camera's device exposure state (one allocation: hist[kDisplayReplicas][64], last[64], then this). `scale` is what the next frame
// multiplies by. Workgroup b adds to replica b % kDisplayReplicas: every workgroup of a frame adding to the same 256 B serialises in the L2
// (measured: 8,100 adds at 1080p doubled the composing launch), 64 replicas spread them over 64 rows; the finalize sums the replicas.
constexpr uint32_t kDisplayReplicas = 64;
struct DisplayState { float scale, metered_ev, adapted_ev; uint32_t primed, frames, pad[3]; };
static_assert(sizeof(DisplayState) == 32, "the display state is 32 B");
constexpr size_t kDisplayLastOffset = (size_t)kDisplayReplicas * kDisplayBins * sizeof(uint32_t);
constexpr size_t kDisplayStateOffset = kDisplayLastOffset + kDisplayBins * sizeof(uint32_t);
constexpr size_t kDisplayBytes = kDisplayStateOffset + sizeof(DisplayState);

// Output post-processing (include/strolle_hip.h "post-processing"; st_post.cpp, k_post.hip): one launch's arguments. FXAA reads `src`
// (width x height RGBA32F) and writes `dst` at the same size; the resampler writes out_width x out_height. Both store `format`.
struct PostArgs {
    const float4* src; void* dst;
    uint32_t width, height, out_width, out_height, format, filter;
    float edge_threshold, edge_threshold_min, subpixel;   // FXAA, defaults resolved by the host
};

// The upscale stage (include/strolle_hip.h "upscaling"; st_upscale.cpp, k_upscale.hip): one launch's arguments. The upscaler reads `src`
// (width x height RGBA32F) and writes out_width x out_height; the sharpening step reads and writes width x height. Both store `format`.
struct UpscaleArgs {
    const float4* src; void* dst;
    uint32_t width, height, out_width, out_height, format, denoise;
    float sharpness;
};

// Bloom (include/strolle_hip.h "bloom"; st_bloom.cpp, k_bloom.hip): one launch's arguments. A downsample reads `src` (sw x sh) and writes
// `dst` (dw x dh float4, ceil(sw / 2) x ceil(sh / 2)); an upsample reads `src` (sw x sh) and blends it into `dst` (dw x dh float4) in place
// with `factor`; the composite upsamples `src` (mip 0; sw == 0: no level, nothing is added) onto `base` (the dw x dh composed frame), runs
// the display transform and stores `format` into `dst`. The prefilter's constants are resolved by the host.
struct BloomArgs {
    const float4* src; void* dst; const float4* base;
    uint32_t sw, sh, dw, dh, format, additive, firefly, threshold_on;
    float factor, clamp, threshold, knee_lo /* threshold - knee */, knee2 /* 2 knee */, knee_div /* 4 knee + 1e-4 */;
    DisplayArgs display;
};

// The fused tail of the bloom chain (k_bloom.hip k_bloom_tail): `base` is mip t - 1 (bw x bh, read and blended in place), the n levels below it
// live in LDS at float offsets `off` (three floats per texel), `factor[i]` blends tail level i into the level above it.
struct BloomTailArgs {
    float4* base; uint32_t bw, bh, n, additive, lds_bytes;
    uint32_t w[8], h[8], off[8];
    float factor[8];
};

// Motion blur (include/strolle_hip.h "motion blur"; st_motion_blur.cpp, k_motion_blur.hip): the arguments of its three launches. Tiles are
// kMBlurTile pixels square, tiles_x x tiles_y of them. Pack reads the velocity and the depth — in a frame the velocity map's xy (16 B a
// pixel) and PRIM_GBUFFER_D0.x with 0 read as FLT_MAX (`frame` != 0), in st_motion_blur_process a float2 and a float plane as they are —
// and writes `packed` (r, Z) and `tile_max` (v.x, v.y, r, 0 per tile); the neighbour launch writes `tile_n`; the gather reads `color`,
// `packed` and `tile_n` and stores `dst` in `format` (`raw` != 0: RGBA32F with no display transform, the plane bloom reads).
constexpr uint32_t kMBlurTile = 32u;
struct MBlurArgs {
    const void* velocity; const void* depth; const float4* color;
    float2* packed; float4* tile_max; float4* tile_n; void* dst;
    uint32_t width, height, tiles_x, tiles_y, frame, samples, jitter, format, raw;
    float half_shutter, max_radius, depth_softness;
    DisplayArgs display;
};

// Depth of field (include/strolle_hip.h "depth of field"; st_dof.cpp, k_dof.hip): the arguments of its three launches. Tiles are kDofTile
// pixels square, tiles_x x tiles_y of them. Pack reads the depth — in a frame PRIM_GBUFFER_D0.x with 0 read as FLT_MAX (`frame` != 0), in
// st_dof_process a float plane as it is — and writes `packed` (coc, Z) and `tile_max` (the largest near-field radius of each tile, a
// non-negative float); the neighbour launch writes `tile_n`; the gather reads `color`, `packed` and `tile_n` and stores `dst` in `format`
// (`raw` != 0: RGBA32F with no display transform, the plane the next HDR node reads). p0, p5, p8, p9: the projection's entries [0], [5],
// [8], [9]. `taps` holds (rho cos th, rho sin th, rho) of each of the `samples` taps: by value, so no frame waits for an upload.
constexpr uint32_t kDofTile = 32u, kDofMaxSamples = 64u;
struct DofArgs {
    const void* depth; const float4* color;
    float2* packed; float* tile_max; float* tile_n; void* dst;
    uint32_t width, height, tiles_x, tiles_y, frame, samples, format, raw, planar, autofocus, focus_px, focus_py;
    float p0, p5, p8, p9, focal_length /* f */, k /* K */, focal_distance, max_radius;
    DisplayArgs display;
    float taps[kDofMaxSamples * 3u];
};

// Fog (include/strolle_hip.h "fog"; st_fog.cpp, k_fog.hip): the arguments of its one launch. It reads `color` and the depth — in a frame
// PRIM_GBUFFER_D0.x with 0 read as FLT_MAX (`frame` != 0), in st_fog_process a float plane as it is — of the pixels of the window
// [row0, row1) x [col0, col1), at their absolute coordinates in the width x height frame, and stores `dst` in `format` (`raw` != 0: RGBA32F
// with no display transform, the plane the next HDR node reads). p0, p5, p8, p9: the projection's entries [0], [5], [8], [9]; m0, m1, m2:
// the first three columns of the camera transform. L, E0 and the desc's fields are the host's (step 0): all of it is wave-uniform.
struct FogArgs {
    const float4* color; const void* depth; void* dst;
    uint32_t width, height, row0, row1, col0, col1, frame, format, raw;
    uint32_t falloff, sky, height_on /* b != 0 */, lobe_on /* light_color is not all 0 */;
    float p0, p5, p8, p9, m0[3], m1[3], m2[3];
    float L[3], E0, b, a /* color[3] */, rgb[3], light_color[3], light_exponent;
    float start, end, density, sky_distance, extinction[3], inscattering[3];
    DisplayArgs display;
};

// Light shafts (include/strolle_hip.h "light shafts"; st_shafts.cpp, k_shafts.hip): the arguments of its two launches. The march reads the
// depth (as FogArgs states it) and writes `cells`, cells_w x cells_h float4 (S.rgb, d_c); the apply launch reads `color`, the depth and
// `cells` and stores `dst` as fog's launch does. origin: M[12..14]; k1, k2, k3: the phase function's constants; L: the sun's direction;
// lights: slots of the light table the frame's KArgs carries. count: the march adds its rays to KArgs::ray_counter. All wave-uniform.
constexpr uint32_t kShaftsMaxLights = 8;
struct ShaftsArgs {
    const float4* color; const void* depth; float4* cells; void* dst;
    uint32_t width, height, cells_w, cells_h, divisor, steps, frame, format, raw, count;
    uint32_t sun_on, light_extinction, light_count, lights[kShaftsMaxLights];
    float p0, p5, p8, p9, m0[3], m1[3], m2[3], origin[3];
    float L[3], k1, k2, k3, density, max_distance, intensity, scatter[3], sun_color[3];
    DisplayArgs display;
};

// Colour grading (include/strolle_hip.h "colour grading"; st_grade.cpp, k_grade.hip): the arguments of its one launch. It reads `color`
// over the window [row0, row1) x [col0, col1) at absolute coordinates in the width x height frame and stores `dst` in `format` behind the
// display transform (it is the last node: `raw` is never set by a frame). `steps`: ST_GRADE_STEP_* of the steps that run; cdl_pow: bit k
// set when channel k's power is not 1. lut: lut_n^3 float4, red fastest (lut_n == 0: no table). M: white balance, row major; inv_range:
// the LOG2 domain's 1 / (ev_max - ev_min). All wave-uniform.
constexpr uint32_t kGradeWhiteBalance = 1u, kGradeContrast = 2u, kGradeSaturation = 4u, kGradeCdl = 8u, kGradeLut = 16u, kGradeDither = 32u;   // ST_GRADE_STEP_*
constexpr uint32_t kGradeStageA = kGradeWhiteBalance | kGradeContrast | kGradeSaturation;
struct GradeArgs {
    const float4* color; const float4* lut; void* dst;
    uint32_t width, height, row0, row1, col0, col1, format, raw;
    uint32_t steps, cdl_pow, cdl_sat_on, lut_n, lut_log2, lut_blend;
    float M[9], contrast, saturation, slope[3], offset[3], power[3], cdl_saturation, ev_min, inv_range, lut_strength;
    DisplayArgs display;
};

// Lens effects (include/strolle_hip.h "lens effects"; st_lens.cpp, k_lens.hip): the arguments of its one launch over the whole width x
// height frame (the node excludes windows). It reads `color` — with the distortion or the fringe step at up to `taps` bilinear look-ups per
// pixel anywhere in the plane, indices clamped — and stores `dst` as fog's launch does. `steps`: ST_LENS_STEP_* of the steps that run;
// force_gather: the debug seam that sends a descriptor without taps through the gather instantiation. cx, cy, inv_hd2, scale_eff,
// tap_scale and tap_weight are st_lens_plan's; seed: grain_seed plus the camera's frame counter under ST_LENS_GRAIN_ANIMATE. All wave-uniform.
constexpr uint32_t kLensDistortion = 1u, kLensFringe = 2u, kLensVignette = 4u, kLensGrain = 8u;   // ST_LENS_STEP_*
constexpr uint32_t kLensMaxTaps = 16u;
struct LensArgs {
    const float4* color; void* dst;
    uint32_t width, height, format, raw;
    uint32_t steps, taps, round, grain_size, seed, force_gather;
    float cx, cy, inv_hd2, k1, k2, scale_eff, vignette_intensity, vignette_falloff, grain_intensity;
    float tap_scale[kLensMaxTaps], tap_weight[kLensMaxTaps][3];
    DisplayArgs display;
};

// Everything a per-pixel kernel can touch, passed by value as the kernel argument (scalar loads).
struct KArgs {
    GpuCamera cam, prev_cam;
    // engine-level bindings
    const float4* bvh; const float4* tri_attr;
    const float4* instance_xforms;  // 8 float4 per instance slot: curr_xform_inv (3 axes + translation), prev_xform; slot = tri_attr[4 t + 3].w
    const GpuMaterial* materials; const GpuLight* lights;
    const GpuLight* lights_lds;   // set by the tracing kernels' prologue: the first kLdsLights lights in LDS (nullptr from the host)
    const uint32_t* material_base_packed;  // per material: gbuffer_pack_base_color(base_color), valid where it has no base-colour texture
    const uchar4* atlas; const uchar4* blue_noise;
    const float* byte_luts;  // 256 sRGB->linear + 256 unorm8 values (st_device.h kLut*), generated on the device at engine creation
    const float4* transmittance_lut; const float4* sky_lut;
    uint32_t bvh_len, n_lights_buf, light_count, atlas_w, atlas_h;
    uint32_t stack_entries;    // pending entries per lane of the traversal stack: kBvhStackSize, or kBvhStackSizeDeep for deeper trees (dynamic LDS, sized at the launch)
    // k_denoise.hip "variance in the reproject stage": the fused reproject stages store each pixel's long-history variance in
    // curr_colors.w and the DI one flags short-history pixels per 8x8 tile (bit = lane) for the variance kernel
    unsigned long long* tile_mask; uint32_t variance_in_reproject;
    // k_gi.hip k_gi_preview_both: pixels whose second preview pass resamples, per 8x8 tile (bit = lane); gi_preview_late: the
    // second-pass launch serves flagged pixels only
    unsigned long long* gi_late_mask; uint32_t gi_preview_late;
    uint32_t skip_dead_scratch;  // the fused DI spatial launch keeps its pick / trace records in registers only: resolving, denoise-reproject and the a-trous chain rewrite the three scratch planes later in this frame
    uint32_t gi_skip_history_copy;  // gi_resolving leaves GI_RESERVOIRS_0 alone: the engine swaps plane pointers instead (st_engine.cpp gi_aliased)
    // The lean frame (fast build, whole pass graph, Image{denoise}; st_engine.cpp `lean_frame`): stores that nothing reads —
    // not a later pass of this frame, not the next frame — are not made. Bits: kLean*. st_debug_keep_all_planes(1) /
    // ST_KEEP_ALL_PLANES=1 keeps every plane as the reference leaves it.
    uint32_t lean;
    const float4* gi_mid_src;  // kLeanGiMid, second-pass launch only: the first preview pass's input plane (nullptr: GI_RESERVOIRS_3 holds every first-pass result)
    const float4* bvh_c;       // fast build: the compact stream the shadow rays walk (k_bvh.hip k_bvh_compact; nullptr: they walk `bvh`)
    uint32_t bvh_c_root;       // ... its entry 0 with the kind bit (entry << 1 | is a leaf entry)
    const float4* bvh_w;       // fast build: the WIDE stream's nodes (k_bvh.hip k_bvh_wide: four f16 child boxes + four links per 64-B line; nullptr: none)
    uint32_t bvh_w_leaf_off;   // ... byte offset of its leaf records (48 B each) in the same allocation
    uint32_t bvh_w_root;       // ... the root's link (index << 1 | is a leaf record)
    uint32_t primary_packets;  // ... 1: primary visibility walks it as ONE packet per wave (st_traverse.h closest_hit_packet; StTuning::primary_packets)
    uint32_t bvh_w_link_mask;  // ... 32-bit form: (1 << bits) - 1, bits = what the largest link needs (the sort key keeps the link there)
    uint32_t bvh_w_links16;    // ... 1: links are 16-bit (fewer than 32768 nodes and leaf records): kernels run with 16-bit stack slots
    uint32_t* walk_flags;      // ... two sticky words in page-locked host memory: [0] a per-lane wide walk, [1] the packet walk found its stack full and DROPPED a push (st_traverse.h wide_walk_overflowed; st_tick.cpp reads them)
    uint32_t exp_flags;        // A/B switches of experiments in flight (ST_EXP in the environment; 0 in the shipped configuration)
    uint32_t anyhit_contract;  // fast build: shadow rays walk the contract loop (set while the reference's used_memory bytes are counted, or by StTuning::anyhit_fast = 0)
    uint32_t count_bytes;  // st_profile_enable bit 1: kernels also sum the reference's used_memory over their rays
    uint32_t tri_slots;  // triangle records in tri_attr (upper bound of every triangle id in the BVH stream)
    float sun_altitude;
    float sun_dir[3];
    // per-camera planes (A/B resolved for this frame)
    float4 *g0, *g1, *sm;                // prim_gbuffer_d0/d1, prim_surface_map (curr)
    const float4 *pg0, *pg1, *psm;       // previous frame's
    // Decoded twin of the surface map: (normal.xyz, depth) per pixel, written by primary visibility. Neighbour-tap loops
    // (à-trous, variance, preview resampling, reprojection validity) read it instead of re-running the octahedral decode
    // (a sqrt and a division per tap); the bytes per tap are the same 16. Not part of the reference's buffer set.
    float4* sn; const float4* psn;
    float4 *reprojection, *velocity;
    float4* di_res[3];
    float4 *di_diff_samples, *di_diff_prev_colors, *di_diff_curr_colors, *di_diff_moments, *di_diff_stash, *di_spec_samples;
    const float4* di_diff_prev_moments;
    float4 *gi_d0, *gi_d1, *gi_d2;
    float4* gi_res[4];
    float4 *gi_diff_samples, *gi_diff_prev_colors, *gi_diff_curr_colors, *gi_diff_moments, *gi_diff_stash, *gi_spec_samples;
    const float4* gi_diff_prev_moments;
    float4 *ref_hits, *ref_rays, *ref_colors;
    uint32_t* dbg_used_memory;
    unsigned long long* ray_counter;
    uint32_t width, height, row0, row1;  // [row0,row1) x [col0,col1): the window of the viewport this launch covers (multi-GPU row bands / 2-D tiles;
    uint32_t col0, col1;                 // st_camera_set_rows / st_camera_set_window); pixels keep their absolute coordinates
    uint32_t frame;
    uint32_t tile_map;  // blockIdx -> tile mapping (st_device.h tile_for_thread)
    // environment lighting (include/strolle_hip.h "environment lighting"; st_env.cpp): nullptr = no map, the sky is the atmosphere
    const float4* env_map;      // env_w x env_h texels (rgb, 0), row 0 the zenith, sanitised on upload
    const EnvCell* env_table;   // env_gw x env_gh alias-table cells over the downsampled luminance grid
    uint32_t env_w, env_h, env_gw, env_gh;
    float env_intensity, env_cos_yaw, env_sin_yaw;
    uint32_t env_uniform;       // ST_ENV_UNIFORM_SAMPLING: GI samples the sky as it does for the atmosphere
};

}  // namespace st
