// st_launchers.inc — X-macro list of the kernel launchers (one entry per launch_* function of the k_*.hip files).
// Included by st_kernels.h with ST_LAUNCHER defined as a declaration, a function-pointer member or a table initialiser.
// Each launcher enqueues exactly one kernel on its stream; `KArgs` travels by value in the kernarg segment.
// atmosphere LUTs (passes/atmosphere.rs: transmittance + scattering once, sky on sun-altitude change)
ST_LAUNCHER(launch_atmosphere_static, (float4* transmittance_lut, float4* scattering_lut, hipStream_t s))
ST_LAUNCHER(launch_atmosphere_sky, (const float4* transmittance_lut, const float4* scattering_lut, float sun_altitude, float4* sky_lut, hipStream_t s))
// ray-tracing passes
ST_LAUNCHER(launch_bvh_heatmap, (const KArgs& a, hipStream_t s))
ST_LAUNCHER(launch_ref_tracing, (const KArgs& a, uint32_t depth, hipStream_t s))
ST_LAUNCHER(launch_ref_shading, (const KArgs& a, uint32_t seed, uint32_t depth, hipStream_t s))
ST_LAUNCHER(launch_prim_visibility, (const KArgs& a, bool fuse_frame_reprojection, const uint4* deform_table, const float* deform_posed, const float4* nm_tri_geo, hipStream_t s))
ST_LAUNCHER(launch_build_byte_luts, (float* out /* kByteLutFloats */, hipStream_t s))  // st_device.h byte decode tables
ST_LAUNCHER(launch_frame_reprojection, (const KArgs& a, hipStream_t s))
// ReSTIR DI
ST_LAUNCHER(launch_di_sampling, (const KArgs& a, uint32_t seed, hipStream_t s))
ST_LAUNCHER(launch_di_temporal, (const KArgs& a, uint32_t seed, hipStream_t s))
ST_LAUNCHER(launch_di_sampling_temporal, (const KArgs& a, uint32_t seed_sampling, uint32_t seed_temporal, hipStream_t s))  // both passes, one launch
ST_LAUNCHER(launch_di_spatial_pick, (const KArgs& a, uint32_t seed, hipStream_t s))
ST_LAUNCHER(launch_spatial_trace, (const KArgs& a, const float4* buf_d0, const float4* buf_d1, float4* buf_d2, hipStream_t s))
ST_LAUNCHER(launch_di_spatial_sample, (const KArgs& a, uint32_t seed, hipStream_t s))
ST_LAUNCHER(launch_di_spatial_fused, (const KArgs& a, uint32_t seed_pick, uint32_t seed_sample, hipStream_t s))  // pick + trace + sample per cell
ST_LAUNCHER(launch_di_resolving, (const KArgs& a, bool fuse_denoise_reproject, hipStream_t s))
// ReSTIR GI
ST_LAUNCHER(launch_gi_reprojection, (const KArgs& a, hipStream_t s))
ST_LAUNCHER(launch_gi_sampling_a, (const KArgs& a, uint32_t seed, hipStream_t s))
ST_LAUNCHER(launch_gi_sampling_b, (const KArgs& a, uint32_t seed, hipStream_t s))
ST_LAUNCHER(launch_gi_sampling_ab, (const KArgs& a, uint32_t seed_a, uint32_t seed_b, bool reproject, hipStream_t s))
// fuse_reprojection: gi_reprojection.rs runs inside this launch (legal on tracing frames, where nothing else reads gi_res[2] before)
ST_LAUNCHER(launch_gi_temporal, (const KArgs& a, uint32_t seed, bool fuse_reprojection, hipStream_t s))
ST_LAUNCHER(launch_gi_spatial_pick, (const KArgs& a, uint32_t seed, hipStream_t s))
ST_LAUNCHER(launch_gi_spatial_sample, (const KArgs& a, uint32_t seed, hipStream_t s))
ST_LAUNCHER(launch_gi_spatial_fused, (const KArgs& a, uint32_t seed_pick, uint32_t seed_sample, hipStream_t s))  // pick + trace + sample per cell
ST_LAUNCHER(launch_gi_preview, (const KArgs& a, uint32_t seed, uint32_t nth, const float4* in, float4* out, hipStream_t s))
ST_LAUNCHER(launch_gi_resolving, (const KArgs& a, uint32_t source, hipStream_t s))
// second preview pass + gi_resolving (+ the GI half of denoise reproject) in one launch
ST_LAUNCHER(launch_gi_preview_resolve, (const KArgs& a, uint32_t seed, uint32_t nth, const float4* in, uint32_t source, bool fuse_denoise_reproject, hipStream_t s))
ST_LAUNCHER(launch_gi_preview_both, (const KArgs& a, uint32_t seed, const float4* in, float4* mid, uint32_t source, bool fuse_denoise_reproject, hipStream_t s))
// SVGF + composition
ST_LAUNCHER(launch_denoise_reproject, (const KArgs& a, const float4* prev_colors, const float4* prev_moments, const float4* samples, float4* colors, float4* moments, hipStream_t s))
// di_out / gi_out: the stash planes (reference), or the internal pair when the strides-1+2 launch follows
ST_LAUNCHER(launch_denoise_variance, (const KArgs& a, float4* di_out, float4* gi_out, hipStream_t s))
// one à-trous pass (strides 1, 2, 4 staged through LDS, 8 and 16 gathered); input and output planes must differ
ST_LAUNCHER(launch_denoise_wavelet, (const KArgs& a, uint32_t stride, float strength, const float4* di_in, float4* di_out, const float4* gi_in, float4* gi_out, hipStream_t s))
// the last pass of the chain (a gather pass: stride 8 or 16) with frame_composition.rs appended for the same pixel; keep_colours == false:
// the pass's own output planes stay unwritten (nothing but composition reads them)
ST_LAUNCHER(launch_denoise_wavelet_compose, (const KArgs& a, uint32_t stride, float strength, const float4* di_in, float4* di_out, const float4* gi_in, float4* gi_out, uint32_t camera_mode, void* out, uint32_t format, bool keep_colours, const DisplayArgs& d, hipStream_t s))
// strides 1 and 2 in one launch: *_mid receive the stride-1 output, *_out the stride-2 output; *_in must not alias either
ST_LAUNCHER(launch_denoise_wavelet_12, (const KArgs& a, float strength0, float strength1, const float4* di_in, float4* di_mid, float4* di_out, const float4* gi_in, float4* gi_mid, float4* gi_out, hipStream_t s))
// d.on: the camera's display transform (st_passes.h store_display; include/strolle_hip.h "display transforms") in both composing launches
ST_LAUNCHER(launch_composition, (const KArgs& a, uint32_t camera_mode, const float4* di_diff, const float4* gi_diff, void* out, uint32_t format, const DisplayArgs& d, hipStream_t s))
// debug seam (st_camera_write_buffer): regenerates the planes this library derives from the reference's — the decoded surface
// twins (KArgs::sn / psn) from both surface maps
ST_LAUNCHER(launch_refresh_internal_planes, (const KArgs& a, uint32_t which /* bit 0: sn from sm, bit 1: psn from psm */, hipStream_t s))
// BVH refit on the device (k_bvh.hip; st_set_bvh_refresh(ST_BVH_REFIT_DEVICE))
ST_LAUNCHER(launch_bvh_patch_leaves, (float4* bvh, const float4* tri_geo, const uint32_t* entry_of_tri, uint32_t lo, uint32_t hi, hipStream_t s))
ST_LAUNCHER(launch_bvh_refit, (float4* bvh, const float4* tri_bounds, const uint32_t* parent, const uint32_t* local, const uint32_t* items, const uint32_t* batch_off, uint32_t first_batch, uint32_t batches, hipStream_t s))
// measurement helper (k_util.hip): grid-stride float4 copy, the device's own streaming ceiling
ST_LAUNCHER(launch_copy_float4, (float4* dst, const float4* src, size_t n, uint32_t blocks, hipStream_t s))
// pitched rectangle copy (tile pack / unpack of the multi-GPU gather, st_dist.cpp); row_bytes a multiple of 4
ST_LAUNCHER(launch_rect_copy, (void* dst, size_t dst_pitch, const void* src, size_t src_pitch, size_t row_bytes, uint32_t rows, hipStream_t s))
// world-space baking of moved instances on the device (k_bvh.hip; StTuning::device_bake): jobs = 128-B records (xform, inverse rows, mesh / slot ranges);
// a job whose x.w is nonzero reads its object-space triangles from `posed` (the posed store of skinned instances, k_skin.hip) instead of `mesh`
ST_LAUNCHER(launch_bvh_bake, (const void* jobs, const uint32_t* job_start, uint32_t n_jobs, uint32_t total, const float* mesh, const float* posed, float4* tri_geo, float4* tri_bounds, float4* tri_attr, float4* bvh, const uint32_t* entry_of_tri, hipStream_t s))
// the compact stream (48-B entries, f16 conservative boxes) of the fast build's shadow rays, regenerated from the contract stream (k_bvh.hip)
ST_LAUNCHER(launch_bvh_compact, (const float4* bvh, uint32_t n_entries, float4* out, hipStream_t s))
ST_LAUNCHER(launch_bvh_wide, (const float4* bvh, const uint32_t* topo, uint32_t n_nodes, const uint32_t* leaf_entry, uint32_t n_leaves, uint32_t links16, float4* nodes, float4* leaves, hipStream_t s))
// scene queries (k_query.hip; st_query.cpp): one ray per lane, 256 per block. rays: 2 float4 per StRay; hits: 4 float4 per StRayHit;
// table: per instance slot {StHandle lo, hi, first triangle slot, 0}; pixels: (x, y) pairs
ST_LAUNCHER(launch_query_closest, (const KArgs& a, const float4* rays, uint32_t count, float4* hits, const uint4* table, uint32_t packets, const float4* nm_tri_geo, hipStream_t s))
ST_LAUNCHER(launch_query_occluded, (const KArgs& a, const float4* rays, uint32_t count, uint32_t* occluded, hipStream_t s))
ST_LAUNCHER(launch_query_pick, (const KArgs& a, const uint32_t* pixels, uint32_t count, float4* hits, const uint4* table, const float4* nm_tri_geo, hipStream_t s))
// per-pixel AOVs (k_aov.hip; st_aov.cpp): over the window's 8x8 tiles like the frame's passes; each plane width x height, nullptr = not requested
ST_LAUNCHER(launch_aov, (const KArgs& a, float* depth, float4* normal, float4* albedo, float2* motion, uint64_t* instance, uint32_t* triangle, const uint4* table, const float* deform_posed, const float4* nm_tri_geo, hipStream_t s))
// environment lighting (k_env.hip; st_env.cpp): a map's upload from device memory (pitched rows of 3 or 4 floats -> sanitised float4 texels,
// `bad` counts texels that had a NaN, infinite or negative channel), the luminance grid of its importance table, the debug seams
ST_LAUNCHER(launch_env_upload, (const void* src, size_t pitch, uint32_t w, uint32_t h, uint32_t channels, float4* texels, uint32_t* bad, hipStream_t s))
ST_LAUNCHER(launch_env_grid, (const float4* texels, uint32_t w, uint32_t h, uint32_t gw, uint32_t gh, float* weights, hipStream_t s))
ST_LAUNCHER(launch_env_debug, (const KArgs& a, uint32_t what /* 0 eval, 1 sample, 2 pdf */, const float* in, uint32_t n, float* out, hipStream_t s))
// display transforms (k_display.hip; st_display.cpp): the camera's device exposure state reset to its first-frame values, and the
// one-workgroup finalize behind a metered frame (histogram -> metered / adapted EV and the next frame's scale; the histogram cleared)
ST_LAUNCHER(launch_display_reset, (void* state /* kDisplayBytes */, float scale, float adapted_ev, hipStream_t s))
ST_LAUNCHER(launch_display_finalize, (void* state, float ev_min, float ev_max, float low_fraction, float high_fraction, float step_up, float step_down, float compensation_ev, hipStream_t s))
// output post-processing (k_post.hip; st_post.cpp): FXAA over a display-referred RGBA32F image (dst: the same size, any output format) and the
// resampler (nearest / bilinear / Catmull-Rom to out_width x out_height, any output format); equal sizes make it a format-converting copy
ST_LAUNCHER(launch_post_fxaa, (const PostArgs& p, hipStream_t s))
ST_LAUNCHER(launch_post_resample, (const PostArgs& p, hipStream_t s))
// bloom (k_bloom.hip; st_bloom.cpp): one level down (first: the prefilter, and firefly suppression when asked, on the way), one level up blended in
// place, and the composite (the last upsample + the blend with the composed frame + the display transform + the output format)
ST_LAUNCHER(launch_bloom_down, (const BloomArgs& p, bool first, hipStream_t s))
ST_LAUNCHER(launch_bloom_up, (const BloomArgs& p, hipStream_t s))
ST_LAUNCHER(launch_bloom_composite, (const BloomArgs& p, hipStream_t s))
// ... and the fused tail: the last levels down and back up in one single-workgroup launch, in LDS (`limit`: the bytes that launch may use here)
ST_LAUNCHER(launch_bloom_tail_limit, (uint32_t* bytes))
ST_LAUNCHER(launch_bloom_tail, (const BloomTailArgs& p, hipStream_t s))
// motion blur (k_motion_blur.hip; st_motion_blur.cpp): pack + per-tile maximum (one workgroup per 32 x 32 tile), the 3 x 3 neighbour maximum over
// the tile vectors, and the gather (one workgroup per 32 x 8 pixels: the tile's vector is uniform in it; tiles at rest are a copy)
ST_LAUNCHER(launch_mblur_pack, (const MBlurArgs& p, hipStream_t s))
ST_LAUNCHER(launch_mblur_neighbour, (const MBlurArgs& p, hipStream_t s))
ST_LAUNCHER(launch_mblur_gather, (const MBlurArgs& p, hipStream_t s))
// depth of field (k_dof.hip; st_dof.cpp): pack + the per-tile near-field maximum (one workgroup per 32 x 32 tile), the 3 x 3 neighbour maximum
// over the tile values, and the gather (one workgroup per 32 x 8 pixels: the tile's value is uniform in it; in-focus pixels are a copy)
ST_LAUNCHER(launch_dof_pack, (const DofArgs& p, hipStream_t s))
ST_LAUNCHER(launch_dof_neighbour, (const DofArgs& p, hipStream_t s))
ST_LAUNCHER(launch_dof_gather, (const DofArgs& p, hipStream_t s))
// fog (k_fog.hip; st_fog.cpp): one pointwise launch over the window, one workgroup per 32 x 8 pixels
ST_LAUNCHER(launch_fog, (const FogArgs& p, hipStream_t s))
// light shafts (k_shafts.hip; st_shafts.cpp): the march over the cell grid (a tracing launch: KArgs::width x height is the cell grid), then one pointwise launch
ST_LAUNCHER(launch_shafts_march, (const KArgs& a, const ShaftsArgs& p, hipStream_t s))
ST_LAUNCHER(launch_shafts_apply, (const ShaftsArgs& p, hipStream_t s))
// colour grading (k_grade.hip; st_grade.cpp): one pointwise launch over the window, one workgroup per 32 x 8 pixels; the last HDR node
ST_LAUNCHER(launch_grade, (const GradeArgs& p, hipStream_t s))
// the upscale stage (k_upscale.hip; st_upscale.cpp): the edge-adaptive upscaler over a display-referred RGBA32F image (dst: out_width x out_height,
// any output format) and the sharpening step at one size (src: RGBA32F; dst: any output format)
ST_LAUNCHER(launch_upscale, (const UpscaleArgs& p, hipStream_t s))
ST_LAUNCHER(launch_sharpen, (const UpscaleArgs& p, hipStream_t s))
// ... and both steps in one launch, the upscaled tile and its one-pixel ring in LDS (`tile`: 1 = 64 x 8 output pixels per workgroup, 2 = 32 x 32, 3 = 64 x 16)
ST_LAUNCHER(launch_upscale_sharpen, (const UpscaleArgs& p, uint32_t tile, hipStream_t s))
// lens effects (k_lens.hip; st_lens.cpp): one launch over the whole frame, one workgroup per 32 x 8 pixels; a gather with the distortion or the fringe step, else pointwise
ST_LAUNCHER(launch_lens, (const LensArgs& p, hipStream_t s))
