/* strolle_hip.h — C ABI of libstrolle_hip.so, the MI355X-native replacement for the
 * per-pixel hot path of Patryk27/strolle.
 *
 * Every entry point below replaces one method of the reference's `strolle::Engine<P>`
 * (reference paths relative to /root/reference). u64 handles stand in for the
 * `Params` associated handle types (strolle/src/lib.rs:402-409); POD structs stand in
 * for the Rust value types; `int` status codes stand in for the reference's
 * panics/asserts. See INTEGRATION.md for the Rust-side FFI stub a maintainer adds.
 *
 * Threading: like the reference (`&mut self` everywhere, lib.rs:105-395) an engine is
 * single-owner; calls on one engine must not overlap. Stream contract: everything
 * st_render_camera enqueues is complete once the `hipStream_t` it was given (0 = the null
 * stream) has drained — the engine may run part of a frame on an internal side stream, but
 * joins it into the caller's stream before the frame's last kernel. Frames may be enqueued
 * back to back without host synchronisation. st_tick queues its uploads on the stream it was given (from
 * page-locked copies, so the scene may be edited again as soon as it returns); st_render_camera orders itself behind them.
 * Scheduling and tuning switches: StTuning below (st_engine_get_tuning / st_engine_set_tuning; environment variables of the
 * same meaning override the defaults when an engine is created).
 */
#ifndef STROLLE_HIP_H
#define STROLLE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct StEngine StEngine;
typedef uint64_t StHandle;

enum StStatus {
    ST_OK = 0,
    ST_ERR_INVALID_ARGUMENT = 1,
    ST_ERR_NO_DEVICE = 2,        /* engine was created host-only, or HIP is unavailable */
    ST_ERR_UNKNOWN_CAMERA = 3,   /* reference: panic "camera does not exist" (camera_controllers.rs:21-34) */
    ST_ERR_EMPTY_MESH = 4,       /* reference: assert "contains no triangles" (triangles.rs:50-53) */
    ST_ERR_HIP = 5,              /* a HIP runtime call failed; see st_last_error() */
    ST_ERR_ATLAS_FULL = 6,       /* reference: warn + drop (images.rs:71-79) */
    ST_ERR_IO = 7,               /* scene ingest: a file could not be read */
    ST_ERR_PARSE = 8,            /* scene ingest: malformed glTF / GLB / PNG; st_last_error() says where */
    ST_ERR_UNSUPPORTED = 9,      /* scene ingest: valid file using something this loader does not read (JPEG, Draco, ...) */
    ST_ERR_BVH_TOO_DEEP = 10,    /* st_tick: the tree's deepest chain of internal nodes exceeds the deepest traversal stack the kernels take
                                  * (24 entries as strolle-gpu/src/lib.rs:76 — the reference indexes past its stack array beyond that —, grown
                                  * to the chain's own length for deeper trees, up to 32). The scene IS uploaded and
                                  * renders — pushes beyond the stack are dropped, so geometry behind them can be missed — but the tick
                                  * says so instead of returning ST_OK; StTuning::allow_deep_bvh = 1 turns the status back into a warning */
    ST_ERR_DIST = 11             /* st_dist_*: the collective transport failed (RCCL status in st_last_error()) */
};

/* strolle/src/mesh_triangle.rs:6-33 — object-space triangle */
typedef struct StMeshTriangle {
    float positions[3][3];
    float normals[3][3];
    float uvs[3][2];
    float tangents[3][4];
} StMeshTriangle;

/* strolle/src/material.rs:8-23; texture handles: 0 = None */
typedef struct StMaterial {
    float base_color[4];
    float emissive[4];
    float perceptual_roughness;
    float metallic;
    float reflectance;
    float ior;
    StHandle base_color_texture;
    StHandle emissive_texture;
    StHandle metallic_roughness_texture;
    StHandle normal_map_texture;
    uint32_t alpha_mode; /* 0 = Opaque, 1 = Blend (material.rs:72-91) */
    uint32_t _pad;
} StMaterial;

/* strolle/src/light.rs:6-22 */
enum StLightKind { ST_LIGHT_POINT = 0, ST_LIGHT_SPOT = 1 };
typedef struct StLight {
    uint32_t kind;
    float position[3];
    float radius;
    float color[3];
    float range;
    float direction[3]; /* spot only */
    float angle;        /* spot only */
} StLight;

/* strolle/src/camera.rs:8-14,83-105,170-175. Matrices are column-major (glam Mat4::to_cols_array). */
enum StCameraMode {
    ST_MODE_IMAGE = 0, ST_MODE_DI_DIFFUSE = 1, ST_MODE_DI_SPECULAR = 2, ST_MODE_GI_DIFFUSE = 3,
    ST_MODE_GI_SPECULAR = 4, ST_MODE_BVH_HEATMAP = 5, ST_MODE_REFERENCE = 6
};
typedef struct StCamera {
    uint32_t mode;     /* StCameraMode */
    uint32_t denoise;  /* CameraMode::{Image,Di*,Gi*}{denoise} */
    uint32_t depth;    /* CameraMode::Reference{depth} */
    uint32_t width, height;   /* viewport.size */
    uint32_t pos_x, pos_y;    /* viewport.position (kept for API parity; the output buffer is viewport-sized) */
    uint32_t _pad;
    float transform[16];
    float projection[16];
} StCamera;

/* ---- lifecycle: Engine::new (lib.rs:132-158).
 * device_ordinal >= 0: HIP device; -1: host-only engine (scene stores + BVH build work,
 * every call that needs the GPU returns ST_ERR_NO_DEVICE — never a CPU fallback). */
int st_engine_create(int device_ordinal, StEngine** out);
void st_engine_destroy(StEngine* e);
const char* st_last_error(void);
/* The commit libstrolle_hip.so was built from ("<hash>" or "<hash>+dirty"; "unknown" for a build outside a git tree): a property of the binary. */
const char* st_build_commit(void);

/* ---- scene: insert_xxx / remove_xxx (lib.rs:161-246) */
int st_mesh_insert(StEngine* e, StHandle id, const StMeshTriangle* triangles, size_t count);   /* lib.rs:161 */
int st_mesh_remove(StEngine* e, StHandle id);                                                    /* lib.rs:169 */
int st_material_insert(StEngine* e, StHandle id, const StMaterial* material);                   /* lib.rs:174 */
int st_material_has(StEngine* e, StHandle id);                                                   /* lib.rs:184; returns 0/1 */
int st_material_remove(StEngine* e, StHandle id);                                                /* lib.rs:192 */
int st_image_insert_rgba8(StEngine* e, StHandle id, uint32_t width, uint32_t height, const uint8_t* rgba, int srgb); /* lib.rs:198 */
int st_image_remove(StEngine* e, StHandle id);                                                   /* lib.rs:211 */
/* lib.rs:198 with ImageData::Texture{texture, is_dynamic} (image.rs:46-59): the pixels are RGBA8 in device memory,
 * rows `row_pitch_bytes` apart. Static images are copied into the atlas once, by the next st_tick; dynamic ones by every
 * st_tick (images.rs:187-213) on the stream st_tick is given — the caller keeps the buffer alive and orders its writes
 * before that tick. Needs a device engine. */
int st_image_insert_device_rgba8(StEngine* e, StHandle id, uint32_t width, uint32_t height, const void* device_rgba,
                                 size_t row_pitch_bytes, int is_dynamic);
/* xform: glam Affine3A as 12 floats, column-major (x_axis, y_axis, z_axis, translation) */
int st_instance_insert(StEngine* e, StHandle id, StHandle mesh, StHandle material, const float xform[12]); /* lib.rs:217 */
int st_instance_remove(StEngine* e, StHandle id);                                                /* lib.rs:226 */
int st_light_insert(StEngine* e, StHandle id, const StLight* light);                            /* lib.rs:232 */
int st_light_remove(StEngine* e, StHandle id);                                                   /* lib.rs:237 */
int st_sun_update(StEngine* e, float azimuth, float altitude);                                   /* lib.rs:242 */

/* ---- cameras (lib.rs:252-297) */
int st_camera_create(StEngine* e, const StCamera* camera, StHandle* out_handle);                /* lib.rs:252 */
int st_camera_update(StEngine* e, StHandle camera, const StCamera* desc);                       /* lib.rs:262 */
int st_camera_delete(StEngine* e, StHandle camera);                                              /* lib.rs:292 */

/* ---- per frame */
int st_tick(StEngine* e, void* hip_stream);                                                      /* lib.rs:301 */
/* Records and launches every pass of CameraController::render (camera_controller.rs:87-174) on
 * `hip_stream` and writes the composed HDR frame (RGBA32F, width*height*16 B, row-major) to the
 * DEVICE pointer `out_device` (width x height pixels of the camera's output format, RGBA32F unless
 * st_camera_set_output_format said otherwise; may be NULL to skip composition). Asynchronous. */
int st_render_camera(StEngine* e, StHandle camera, void* out_device, void* hip_stream); /* lib.rs:279 */

/* ---- present hand-over. Engine::render_camera (lib.rs:279-286) records the frame into the caller's wgpu encoder and
 * texture view; a facade over this library (rust/strolle-hip) owns no resource the other API can sample, so the composed
 * frame has to reach it through host memory. These two calls do that WITHOUT stalling the pipeline:
 *   st_camera_present_copy  enqueues `bytes` of `src_device` (the buffer st_render_camera just composed into on
 *                           `hip_stream`) -> `dst_host` on a copy stream the camera owns, ordered behind that frame only;
 *                           returns at once. The next frames' kernels overlap the copy (8 MB per 1080p RGBA8 frame).
 *   st_camera_present_ready *ready = 1 once the copy into `dst_host` has landed (wait != 0: block until then).
 * Use page-locked host memory (hipHostMalloc) — a pageable destination makes the copy synchronous — and alternate two
 * (src_device, dst_host) pairs: frame N-1 is presented while frame N renders (one frame of latency). Rendering into a
 * `src_device` whose copy is still in flight is safe: the engine orders that frame's composition behind the copy. */
int st_camera_present_copy(StEngine* e, StHandle camera, const void* src_device, void* dst_host, size_t bytes, void* hip_stream);
int st_camera_present_ready(StEngine* e, StHandle camera, const void* dst_host, int wait, int* ready);

/* ---- NEW seams (no counterpart in the reference) */
/* BVH refresh policy for scenes that change every frame (examples/stress-bvh.rs).
 * ST_BVH_REBUILD is the reference's behaviour: every change rebuilds the tree — with unchanged subtrees
 * reused, builder.rs:183-301 — and the result is the tree a from-scratch build gives. ST_BVH_REFIT keeps the tree
 * while instances only move (same triangles, same materials, same Blend flags) and recomputes its boxes bottom-up,
 * which costs a fraction of a rebuild; traversal stays correct, `used_memory` and the tree's quality follow the old
 * topology until something other than a transform changes (or the mode is set again), which rebuilds. */
enum StBvhRefresh { ST_BVH_REBUILD = 0, ST_BVH_REFIT = 1,
                    ST_BVH_REFIT_DEVICE = 2 /* as ST_BVH_REFIT, but the boxes are recomputed ON THE DEVICE: st_tick sends the moved triangles'
                                               hit-test records and bounds (80 B each) instead of refitting the stream on the host and
                                               re-sending all of it; k_bvh.hip patches the leaf entries and refits the boxes bottom-up (one launch per
                                               level of 512-leaf subtrees: two at 208 k triangles). Same bits as ST_BVH_REFIT. */,
                    ST_BVH_BUILD_DEVICE = 3 /* (round 5) after a scene change the tree is BUILT ON THE DEVICE, straight into the wide stream the fast
                                               build's rays walk (k_lbvh.hip: Morton codes, radix sort, the binary radix tree of Karras 2012, boxes by
                                               range queries, collapsed into 4-wide nodes): spawning or removing an instance costs a few hundred
                                               microseconds of device time instead of the host rebuild (26-28 ms at 208 k triangles). It is ANOTHER tree
                                               than the reference's binned SAH — the hits are the same, traversal costs about a fifth more for
                                               incoherent rays —, so it is used only while nothing observes the contract stream (a tick in which
                                               instances only MOVED refits that tree: st_debug_device_tree_refits): fast arithmetic, no
                                               BvhHeatmap camera, no byte counting. A tick that finds such an observer builds on the host as
                                               ST_BVH_REBUILD does; a heatmap camera created later renders after the next st_tick. */,
                    ST_BVH_AUTO = 4         /* (round 6) THE DEFAULT. The first tree of a scene is built on the host as ST_BVH_REBUILD builds it — the
                                               reference's binned SAH, paid once while the scene loads; every later change (spawn, despawn, move) is
                                               answered as ST_BVH_BUILD_DEVICE answers it, under the same conditions, so that a default engine no longer
                                               stalls for tens of milliseconds per spawn. The host's first tree is MEASURED (st_debug_auto_tree: the
                                               surface-area-weighted mean length of its leaf runs): above 3.4 — long runs of coplanar triangles on large
                                               faces, a step of the wide walk each — the device builder's tree is used from that very tick on: 5-17 %
                                               faster there; over 17 measured scene x mode rows of 13 k - 537 k triangles the default picks the faster
                                               tree, or one within 1 % of it, in 16 (profiles/r06_tree_choice_auto.txt).
                                               Scenes whose stream fits the kernels' LDS copy (at most 112
                                               entries: the Cornell box), host-only engines, the exact build and observed contract streams behave as
                                               under ST_BVH_REBUILD. */ };
/* Ticks whose tree was built on the device so far (ST_BVH_BUILD_DEVICE). */
int st_debug_device_builds(StEngine* e, uint64_t* ticks);
/* Ticks of that mode in which instances only moved and the device-built tree was REFITTED instead (same shape, every box recomputed: 5 launches
   against 22; at most 15 in a row, then the next change rebuilds; ST_NO_DEVICE_TREE_REFIT=1 in the environment rebuilds always). */
int st_debug_device_tree_refits(StEngine* e, uint64_t* ticks);
int st_set_bvh_refresh(StEngine* e, int mode);
int st_debug_bvh_refits(StEngine* e, uint64_t* rebuilds, uint64_t* refits);
int st_debug_bvh_device_refits(StEngine* e, uint64_t* device_refits);
/* Launches of the device bake so far and the triangles they baked (StTuning::device_bake: under ST_BVH_REFIT_DEVICE instances that only moved are
 * baked into world space on the device from object-space meshes uploaded once; a tick then sends 132 B per moved instance). */
int st_debug_device_bakes(StEngine* e, uint64_t* ticks, uint64_t* triangles);   /* ticks whose boxes were recomputed by k_bvh.hip (ST_BVH_REFIT_DEVICE) */
/* Depth check of the last BVH build: the longest chain of internal nodes (= the most far-child pointers one traversal can
 * have pending) against the per-ray stack the launches that walk this tree take: 24 entries (strolle-gpu/src/lib.rs:76) while that is
 * enough, the chain's own length for a deeper tree, up to 32 (dynamic LDS). The reference writes past its stack array when a tree is
 * deeper than 24; this library drops a push only beyond 32 and says so — a scene for which *deepest_internal_chain > *stack_entries can
 * miss geometry behind the dropped subtrees. */
int st_debug_bvh_depth(StEngine* e, uint32_t* deepest_internal_chain, uint32_t* stack_entries);
/* The WIDE stream (StTuning::wide_bvh) is another tree than the contract stream and its walks keep StTuning::wide_stack_entries (0 = 24) pending
 * entries per ray — every scene measured needs 11-14. A walk that does find its stack full drops the push (geometry behind it can be missed) and
 * sets a sticky word the engine owns; the next st_tick that sees it re-arms every later launch with a deeper stack (24 -> 32 -> 48 -> 56 entries;
 * the primary rays' packet walk, 64 entries in one register, is replaced by the per-lane walk) and returns ST_ERR_BVH_TOO_DEEP once
 * (StTuning::allow_deep_bvh = 1: a warning on stderr instead). *overflows: ticks that found a word set; *wide_stack_entries: what the wide walks
 * hold now; *packets_off: 1 once the packet walk overflowed. */
int st_debug_walk_overflow(StEngine* e, uint64_t* overflows, uint32_t* wide_stack_entries, uint32_t* packets_off);
/* What ST_BVH_AUTO's choice of a scene's first tree rests on. *leaf_run_weight: the surface-area-weighted mean length of the leaf runs of the host's
 * last binned-SAH build (1 = every leaf holds one triangle); *first_tree_on_device: 1 when that weight exceeded 3.4 at the scene's first tick and the
 * device builder's tree was used from that tick on (measured: profiles/r06_tree_choice*.txt). */
int st_debug_auto_tree(StEngine* e, float* leaf_run_weight, uint32_t* first_tree_on_device);

/* Deterministic seeds: every pass draws seed = pass_seed(base, frame, pass_id) instead of
 * rand::thread_rng() (camera_controller.rs:189-194; passes/ref_*.rs:49-59). */
int st_set_seed(StEngine* e, uint64_t base_seed);
/* Blue-noise texture (256x256 RGBA8), decoded by the caller from strolle/assets/blue-noise.png
 * (strolle/src/noise.rs:40-50 embeds the PNG; this library carries no image decoder). */
int st_set_blue_noise(StEngine* e, const uint8_t* rgba_256x256x4, size_t bytes);
/* Multi-GPU tiling: restrict every per-pixel launch of this camera to the window [x0, x1) x [y0, y1) of the full viewport
 * (x0 = x1 = 0: all columns; y0 = y1 = 0: all rows). Pixels keep their absolute coordinates — RNG, reprojection and every
 * neighbour tap are those of the full frame, so Reference / heatmap tiles reproduce the single-GPU image bit for bit; Image
 * mode reads neighbours, which is what the apron of st_dist_set_partition is for. x0 and x1 must be multiples of 16 (the
 * half-resolution passes work on 2x1 cells in tiles of 8) or the frame's right edge. st_camera_set_rows = all columns. */
int st_camera_set_window(StEngine* e, StHandle camera, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1);
int st_camera_set_rows(StEngine* e, StHandle camera, uint32_t y0, uint32_t y1);

/* ---- scene queries (NEW seam): rays cast by the application against the scene the renderer draws (k_query.hip).
 * Scene. A query sees the scene of the last st_tick: edits made since then are not visible. It is enqueued on `hip_stream`
 *   after that tick's uploads (it waits on them as st_render_camera does) and returns at once, like st_render_camera.
 * Hits. Both faces of a triangle are hit, as in the reference. Blend materials are honoured as the renderer's rays honour
 *   them: base-colour alpha < 1 at the hit's uv is not a hit. `t` is in units of |direction| (the direction is used as given,
 *   not normalised: Ray::new, strolle-gpu/src/ray.rs); a closest hit counts for 0 < t < t_max.
 * Occlusion. st_scene_occluded writes 1 per ray that has any hit with 0 < t < t_max, else 0 (the shadow rays' walk: ray.rs:84-112).
 * Picks. st_camera_pick casts the camera ray (Camera::ray) of pixel (x, y) of the camera as its last st_render_camera saw it,
 *   so that the pick matches the frame on screen; a camera that has not rendered yet uses its current description. Pixels
 *   outside that viewport are misses.
 * Misses. A ray with t_max <= 0 or NaN, or with an all-zero direction, is a miss. A miss writes hit = 0, t = FLT_MAX and 0
 *   everywhere else.
 * Errors. A host-only engine returns ST_ERR_NO_DEVICE (there is no CPU fallback). count == 0 is a no-op returning ST_OK. Null
 *   pointers with count > 0, unknown flag bits and a query before the first st_tick are ST_ERR_INVALID_ARGUMENT; an unknown
 *   camera is ST_ERR_UNKNOWN_CAMERA. In the exact build (ST_ARITH_EXACT) a live scene copy whose tree was built on the device
 *   has no contract stream: ST_ERR_INVALID_ARGUMENT, as st_render_camera reports it.
 * Stack overflow. A walk whose stack overflows sets the engine's sticky walk word: the next st_tick reports it and re-arms
 *   the walks as it does for frames (st_debug_walk_overflow).
 * Buffers. `rays_device`, `hits_device`, `occluded_device` and `pixels_xy_device` are device memory of the engine's device. */
typedef struct StRay {            /* 32 B */
    float origin[3]; float t_max; /* hits count for 0 < t < t_max; FLT_MAX or +inf = unbounded */
    float direction[3];           /* used as given, not normalised */
    uint32_t _pad;
} StRay;
typedef struct StRayHit {         /* 64 B */
    float point[3];  float t;             /* t = FLT_MAX on a miss */
    float normal[3]; uint32_t triangle;   /* shading normal as the renderer resolves it (interpolated, facing the side the ray came
                                           * from: the sign of 1/det); triangle = index into the mesh's array given to st_mesh_insert */
    float uv[2]; float barycentric[2];    /* texture coordinates at the hit; Triangle::hit's (u, v): point = (1-u-v) p0 + u p1 + v p2 */
    StHandle instance;                    /* the st_instance_insert handle */
    uint32_t hit; uint32_t _pad;          /* 1 = hit */
} StRayHit;
enum { ST_RAY_COHERENT = 1,    /* the caller promises runs of 64 consecutive rays are coherent (camera-like): they are walked as one
                                * packet per wave. Correct for any rays; the flag changes only speed. */
       ST_RAY_MAPPED_NORMAL = 2 }; /* StRayHit.normal is the normal bent by the material's normal map ("normal mapping" below: n'), whatever the
                                * engine's switch says; every other field is as without the flag. st_scene_trace_rays_host takes no flags.
                                * A host-only engine, which has nothing to map with, answers the bit as an unknown one (ST_ERR_INVALID_ARGUMENT). */
int st_scene_trace_rays(StEngine* e, const StRay* rays_device, uint32_t count, StRayHit* hits_device, uint32_t flags, void* hip_stream);
int st_scene_occluded(StEngine* e, const StRay* rays_device, uint32_t count, uint32_t* occluded_device, void* hip_stream);
int st_camera_pick(StEngine* e, StHandle camera, const uint32_t* pixels_xy_device /* (x, y) pairs */, uint32_t count,
                   StRayHit* hits_device, void* hip_stream);
/* Blocking convenience: host arrays in and out (staged through engine-owned buffers on a stream of the engine's own). */
int st_scene_trace_rays_host(StEngine* e, const StRay* rays, uint32_t count, StRayHit* hits);

/* ---- per-pixel AOVs (NEW seam): what an external denoiser, a temporal upscaler or an editor asks of each pixel besides its colour
 * (k_aov.hip). One launch writes every requested plane; each plane is device memory of the engine's device, width x height
 * elements in row-major order (y * width + x), of the element type given per kind below.
 * Pixel ray. Pixel (x, y) is the camera ray (Camera::ray, the pixel centre) of the camera as its last st_render_camera saw it, as
 *   st_camera_pick casts it: the frame on screen, not a later st_camera_update. A camera that has not rendered yet uses its
 *   current description. width x height is that frame's size.
 * Previous camera. MOTION compares with the camera of the frame before that one, exactly as that render's velocity plane did.
 * Scene. The scene of the last st_tick, enqueued on `hip_stream` after that tick's uploads (as queries are); the call returns at
 *   once, like st_render_camera. It works in every camera mode (Reference and BVH heatmap included): it casts its own rays.
 * Tiles. The camera's window (st_camera_set_window, st_dist_set_partition) is honoured: only pixels inside it are written, the
 *   rest of every plane is left as it was, so a rank of a tiled frame produces its own tile's AOVs.
 * Sky. A pixel whose ray hits nothing gets the value each kind gives for the sky.
 * Errors. A host-only engine returns ST_ERR_NO_DEVICE. A call before the first st_tick, a null `targets`, a wrong struct_size
 *   or no plane requested is ST_ERR_INVALID_ARGUMENT; an unknown camera is ST_ERR_UNKNOWN_CAMERA. In the exact build
 *   (ST_ARITH_EXACT) a live scene copy whose tree was built on the device is ST_ERR_INVALID_ARGUMENT, as for the queries.
 * Stack overflow. A walk whose stack overflows sets the engine's sticky walk word, as the queries do. */
enum StAovKind {
    ST_AOV_DEPTH = 0,     /* f32:  distance from the camera ray's origin to the hit (the G-buffer's depth, d0.x); FLT_MAX on sky */
    ST_AOV_NORMAL = 1,    /* f32x4: shading normal as StRayHit.normal (xyz), w = 0; 0 on sky. Like DEPTH and MOTION it comes from the primary hit as the
                           * frame resolved it: in the fast build that is the exact arithmetic of primary visibility, an ulp from st_camera_pick's;
                           * with st_engine_set_normal_mapping on it is the mapped normal ("normal mapping") */
    ST_AOV_ALBEDO = 2,    /* f32x4: linear base colour at the hit's uv, texture applied (what primary visibility samples), alpha in w; 0 on sky */
    ST_AOV_MOTION = 3,    /* f32x2: the renderer's velocity (current minus previous screen position in pixels, instance motion included;
                           * 0 where its squared length is below 0.001, as the velocity plane); 0 on sky */
    ST_AOV_INSTANCE = 4,  /* u64:  st_instance_insert handle; 0 on sky */
    ST_AOV_TRIANGLE = 5,  /* u32:  index into the mesh's st_mesh_insert array; 0xffffffff on sky */
    ST_AOV_COUNT = 6
};
typedef struct StAovTargets {         /* 56 B */
    uint32_t struct_size;             /* sizeof(StAovTargets) */
    uint32_t _pad;
    void* planes[ST_AOV_COUNT];       /* indexed by StAovKind: device pointers, width x height elements each; NULL = not wanted */
} StAovTargets;
int st_camera_render_aovs(StEngine* e, StHandle camera, const StAovTargets* targets, void* hip_stream);

/* ---- skinned meshes (NEW seam): per-instance joint poses skinned on the device (k_skin.hip, linear blend skinning).
 * A skin belongs to a mesh, a pose to an instance: instances share a skinned mesh and each has joints of its own (Bevy's SkinnedMesh
 * per entity; glTF's node with a skin that refers to a mesh). An instance of a skinned mesh without a pose renders the bind pose.
 * - When a pose takes effect: at the next st_tick, like any scene edit. Frames, scene queries and AOVs see it only after that tick;
 *   of two poses set before one tick the last wins.
 * - Joint matrices: joint transform x inverse bind matrix, mapping the bind pose into the INSTANCE's object space; the instance transform
 *   is applied after it. (Bevy's skin matrices are world-space: a facade passes them relative to the instance transform, or sets the
 *   instance transform to identity.)
 * - Lifecycle: st_mesh_insert on a skinned handle drops the skin and the pose of every instance of that mesh; st_mesh_remove drops the
 *   skin. st_instance_insert on an existing id keeps its pose only if the mesh handle is unchanged; st_instance_remove drops the pose.
 * - Errors: st_mesh_set_skin returns ST_ERR_INVALID_ARGUMENT for an unknown mesh, a null pointer, a wrong corner_count, a joint_count
 *   outside 1..256, a joint index >= joint_count, or a weight that is negative, not finite or part of an all-zero set; a host-only
 *   engine accepts a skin (host work). st_instance_set_pose returns ST_ERR_NO_DEVICE on a host-only engine (there is no CPU skinning)
 *   and ST_ERR_INVALID_ARGUMENT for an unknown instance, an instance whose mesh has no skin, a joint_count other than the skin's, or
 *   a matrix element that is not finite.
 * - Motion of a deformation (st_engine_set_deformation_motion, OFF by default). Off, the velocity plane, reprojection and ST_AOV_MOTION
 *   follow instance transforms only: a bending limb reports the motion of its instance. On, a primary hit on an instance whose pose the
 *   LAST st_tick re-skinned takes its previous position from the previous pose: with the hit on triangle k of the instance's mesh and
 *   Triangle::hit's barycentrics (u, v) — StRayHit.barycentric —
 *       prev_point = prev_xform x ((1 - u - v) q0 + u q1 + v q2)
 *   where q0..q2 are the object-space positions of triangle k as the posed store held them BEFORE that tick (what st_debug_read_posed
 *   returned then) and prev_xform is the instance's previous transform, the matrix the rigid formula uses. The velocity is
 *   screen(camera, point) - screen(previous camera, prev_point), with the same 0.001 squared-length threshold, and feeds the reprojection
 *   map and ST_AOV_MOTION (bit-equal to the velocity plane wherever both are written) the same way.
 *   Every other hit keeps the rigid formula, bit for bit what the switch off gives: an unskinned instance, a posed instance the last tick
 *   did not re-skin, and two cases that show ONE frame without a deformation term — the first tick that gives an instance a pose (there
 *   are no earlier posed positions: the bind pose is not kept as one) and a tick that returns it to the bind pose
 *   (st_instance_set_pose(NULL) drops the pose and its previous positions with it). Likewise the first tick after the switch is turned
 *   on only records the poses it skins; deformation terms start with the next re-skin. The previous positions are dropped wherever the
 *   pose is (see Lifecycle). Scene queries and the other AOVs are unaffected.
 *   Cost: a second region of the posed store (96 B per triangle) for every instance re-posed while the switch is on, one 4-B table word
 *   per primary hit, and 4 + 36 B more per deforming hit. st_tick and st_render_camera gain no host synchronisation. */
typedef struct StSkinVertex {   /* 24 B */
    uint16_t joints[4];         /* indices into the skin's joint palette, < joint_count */
    float weights[4];           /* used as given (not renormalised); finite, >= 0, not all zero */
} StSkinVertex;
/* corners[3 t + v] = corner v of triangle t of the mesh as given to st_mesh_insert; corner_count = 3 x its triangles; 1 <= joint_count <= 256 */
int st_mesh_set_skin(StEngine* e, StHandle mesh, const StSkinVertex* corners, size_t corner_count, uint32_t joint_count);
/* joint_count x 12 floats, each an Affine3A column-major like st_instance_insert's xform: joint transform x inverse bind matrix,
 * mapping the bind pose into the INSTANCE's object space (the instance transform is applied after it). NULL / 0 = back to the bind pose. */
int st_instance_set_pose(StEngine* e, StHandle instance, const float* joint_xforms, uint32_t joint_count);
/* Skin launches so far (one per tick at most), the triangles they skinned, and the batched read-backs of posed triangles the host
 * needed (host-path refresh modes, heatmap observers, debug reads of the scene). */
int st_debug_skinning(StEngine* e, uint64_t* launches, uint64_t* triangles, uint64_t* host_readbacks);
/* The instance's posed object-space triangles as the device holds them: 24 floats per triangle (positions 9, normals 9, uvs 6: the device
 * mesh store's layout). Blocking. An instance with neither a pose nor morph weights is ST_ERR_INVALID_ARGUMENT. out == NULL only reports the size. */
int st_debug_read_posed(StEngine* e, StHandle instance, float* out, size_t capacity_floats, size_t* written_floats);
/* Deformation motion (above). Host work: valid on a host-only engine (which never has a pose). Takes effect at the next st_tick. */
int st_engine_set_deformation_motion(StEngine* e, int enabled);
int st_engine_get_deformation_motion(StEngine* e, int* enabled);
/* What the last st_tick left: the instances whose hits take the deformation term in the frames after it, and the device memory the
 * second regions of the posed store hold. 0 / 0 while the switch is off. A host-only engine is ST_ERR_NO_DEVICE. */
int st_debug_deformation(StEngine* e, uint64_t* instances_with_previous, uint64_t* previous_bytes);

/* ---- normal mapping (NEW seam): StMaterial.normal_map_texture bends the normal of PRIMARY hits (st_traverse.h normal_map_apply).
 * OFF by default (st_engine_set_normal_mapping). Off — and on, while no material's normal_map_texture resolves to a live image — every
 * frame, AOV, pick and query is what it was before the seam existed, bit for bit: the launches get the same null argument.
 * - When it takes effect: the switch with the next st_render_camera, st_camera_render_aovs, st_camera_pick or query; a material's map, or
 *   an image that is inserted or removed, with the next st_tick like any scene edit.
 * - Where it applies: primary visibility (the G-buffer's normal, the surface planes the denoiser's edge-stopping and the reprojection read —
 *   they must carry the mapped normal, or the denoiser blurs the bump shading away), ST_AOV_NORMAL and st_camera_pick follow the switch;
 *   st_scene_trace_rays follows ST_RAY_MAPPED_NORMAL and not the switch.
 * - Out of scope: the hits of GI bounce rays, ST_MODE_REFERENCE and heatmap frames, shadow rays, a per-material normal scale (glTF's
 *   normalTexture.scale is ignored), and vertex tangents.
 * - The tangent frame is DERIVED from the winning triangle's world-space edges and uv corners — the frame three.js and the glTF sample
 *   viewer use for a mesh without tangents. StMeshTriangle.tangents stay unused. The device keeps edges and uv corners current under every
 *   refresh mode, skinning and morphing, so mapped normals follow deforming meshes at no extra store. Because supplied (MikkTSpace)
 *   tangents are ignored, a map baked against them can show faint seams.
 * - The texel: bilinear over the image, with the wrap, rectangle mapping, texel centres and clamp of every other texture; each byte decodes
 *   as byte / 255. The sRGB curve is never applied to a normal map (st_image_insert_rgba8's `srgb` argument is ignored, as everywhere).
 * - The definition, float32, no fused multiply-add, the same operations in both arithmetic builds. n: the hit's resolved normal (facing the
 *   ray); s = copysign(1, 1/det), the flip that made it face the ray, so nf = s n is the front normal; uv: the hit's uv; e1, e2: the
 *   triangle's world-space edges p1 - p0, p2 - p0; uv0..uv2 its uv corners; R the map's atlas rectangle.
 *       (du1, dv1) = uv1 - uv0   (du2, dv2) = uv2 - uv0   d = du1 dv2 - du2 dv1
 *       Pu = (e1 dv2 - e2 dv1) / d          Pv = (e2 du1 - e1 du2) / d
 *       T  = normalize(Pu - nf (nf . Pu))   C = nf x T
 *       h  = (C . Pv <= 0) ? +1 : -1        B = h C          (glTF's v runs down the image: an unmirrored layout has h = +1)
 *       m  = the texel at uv                t = (2 m.x - 1, 2 m.y - 1, max(2 m.z - 1, 0))   (a texel pointing below the tangent plane is flattened onto it)
 *       n' = s normalize(t.x T + t.y B + t.z nf)
 *   normalize(v) is v * (1 / sqrt(v . v)); a dot product is ((x x + y y) + z z). n' is n itself, with identical bits, where R is zero (no
 *   map, or a handle whose image is gone) or where |d| lies outside [1e-30, FLT_MAX] or |Pu - nf (nf . Pu)| or the last length outside [1e-18, 1e18] (zero and
 *   not-finite values included: a length's bounds keep its square inside float32's normal range).
 *   Pinned by hand: a quad in the xy-plane facing +z with u along +x and v along -y — texel (255, 128, 128) tilts the normal towards +x,
 *   texel (128, 255, 128) towards +y.
 * - Cost: off, one scalar test of a null kernel argument. On, per primary hit the material's rectangle; per mapped hit two 16-B edge records,
 *   the triangle's attribute record again and four atlas texels. A scene copy whose tree the host built under a mode that keeps no edge
 *   records on the device (ST_BVH_REBUILD, ST_BVH_REFIT, and ST_BVH_AUTO while the host's tree is in use) gets them with st_tick's own
 *   upload while the switch is on and a material has a map: no host join. Where the switch, or a query with ST_RAY_MAPPED_NORMAL, comes
 *   after that tick, the first call that maps normals sends them once and joins its stream. */
int st_engine_set_normal_mapping(StEngine* e, int enabled);   /* host work: valid on a host-only engine */
int st_engine_get_normal_mapping(StEngine* e, int* enabled);

/* ---- morph targets (NEW seam): per-instance blend-shape weights applied on the device (k_skin.hip k_morph; glTF `targets` / `weights`).
 * Targets belong to a mesh, weights to an instance: instances share a morphed mesh and each carries weights of its own (Bevy's
 * MorphWeights per entity). A mesh may have targets, a skin, both, or neither. An instance without weights renders the base mesh.
 * - When weights take effect: at the next st_tick, like a pose. Frames, scene queries and AOVs see them only after that tick; of two
 *   weight sets given before one tick the last wins.
 * - Arithmetic: float32, evaluated left to right, no fused multiply-add; the kernel is built once with the exact build's flags (like
 *   skinning), so fast and exact engines give the same bits. The ACTIVE targets are those whose weight is not exactly 0, in ascending
 *   index; a zero-weight target is skipped, not multiplied in ((-0) + 0 * d would flip a sign bit, and a skipped target costs no
 *   bandwidth). Per component of every corner:
 *       p = base position;  for k in active: p = p + w[k] * position delta[k]
 *       n = base normal;    for k in active: n = n + w[k] * normal delta[k]
 *   With at least one active target, len = sqrt(dot(n, n)) (st_math.h dot: (x x + y y) + z z); if len is 0 or not finite the normal is
 *   the base normal as given, else n * (1 / len) (st_math.h normalize). With no active target the triangle is the base triangle, bit
 *   for bit. uvs are copied. Tangents are not morphed: the device arrays hold none (as for skinning) and tangent deltas are not taken.
 * - Morph, then skin (glTF's and Bevy's order): if the instance also has a joint pose, the morphed (p, n) replace the bind-pose values
 *   at the input of the skin stage, which is exactly skinning's blend, position and normal steps; the morphed triangle is never written
 *   to memory in between. An instance with a pose and no non-zero weight is skinned exactly as without targets.
 * - Lifecycle (the skin's rules): st_mesh_insert on a morphed handle drops the targets and the weights of every instance of that mesh;
 *   st_mesh_remove drops the targets. st_mesh_set_morph_targets on a mesh that has targets replaces them and drops those instances'
 *   weights; their joint poses stay. st_mesh_set_skin keeps weights (it drops poses). st_instance_insert on an existing id keeps its
 *   weights only if the mesh handle is unchanged; st_instance_remove drops them. Weights NULL / 0, or all exactly zero, on an instance
 *   without a pose: it returns to the base mesh and its regions of the posed store are freed, as st_instance_set_pose(NULL) does.
 * - Errors: st_mesh_set_morph_targets returns ST_ERR_INVALID_ARGUMENT for an unknown mesh, a null pointer, a wrong corner_count, a
 *   target_count outside 1..64, or a delta component that is not finite; a host-only engine accepts targets (host work).
 *   st_instance_set_morph_weights returns ST_ERR_NO_DEVICE on a host-only engine (there is no CPU morphing) and
 *   ST_ERR_INVALID_ARGUMENT for an unknown instance, an instance whose mesh has no targets, a target_count other than the mesh's, or a
 *   weight that is not finite. Negative weights and weights above 1 are valid.
 * - Deformation motion: a tick that applies changed weights counts as "re-skinned" in the contract above — with the switch on, the
 *   previous region keeps the positions from before that tick and the velocity formula is the one written there. The one-frame
 *   exceptions carry over: the first tick that deforms an instance has no previous positions, a tick that returns it to the base shape
 *   has none either, and the first tick after the switch is turned on only records what it deforms.
 * - Counters: st_debug_skinning keeps its meaning — ticks and triangles that went through a skin stage, in whichever kernel, at most
 *   one per tick — and st_debug_morphing counts the morph stage the same way.
 * - Not here: the glTF loader ignores `targets` as it ignores skins; loading rigged and morphed glTF is a separate piece of work.
 *   Cost: 72 B of device memory per triangle and target (triangles rounded up to 128 per mesh), sent once when a tick first needs
 *   them (a one-off upload wait, as for a new skin); per tick and morphed instance 72 B read per triangle and ACTIVE target. */
typedef struct StMorphDelta { float position[3]; float normal[3]; } StMorphDelta;   /* 24 B */
/* deltas[k * corner_count + 3 t + v] = target k's displacement of corner v of triangle t of the mesh as given to st_mesh_insert;
 * corner_count = 3 x its triangles; 1 <= target_count <= 64 */
int st_mesh_set_morph_targets(StEngine* e, StHandle mesh, const StMorphDelta* deltas, size_t corner_count, uint32_t target_count);
/* target_count floats; NULL / 0 = back to the base shape */
int st_instance_set_morph_weights(StEngine* e, StHandle instance, const float* weights, uint32_t target_count);
/* ticks that ran a morph stage, the triangles morphed, and the bytes of deltas the device store holds (padding included) */
int st_debug_morphing(StEngine* e, uint64_t* ticks, uint64_t* triangles, uint64_t* delta_bytes);

/* ---- environment lighting (NEW seam): an equirectangular HDR map in place of the procedural atmosphere (k_env.hip, st_env.cpp).
 * - Timing: a change takes effect at the next st_tick, like every scene edit. Frames, scene queries and AOVs before that tick see the old
 *   sky; a frame already enqueued keeps reading the map it started with. The old map's memory is released only after the frames that read
 *   it are done (an event recorded behind them; the engine waits for the device instead when cameras render on several streams).
 * - Mapping: the world direction is rotated by -yaw about +Y, giving d; u = 0.5 + atan2(d.x, -d.z) / 2 pi, v = acos(clamp(d.y)) / pi.
 *   Row 0 is the zenith, the image centre looks down -Z (Bevy's forward). Look-up is bilinear at texel centres, wrapping in u and clamping
 *   in v, at full resolution; the value is multiplied by `intensity`.
 * - What it replaces: the whole atmosphere, the sky LUT and the sun disk with its bloom, wherever a ray leaves the scene (primary sky
 *   pixels, GI bounces and GI's sky pick, Reference-mode misses). Light 0, the analytic sun, gets zero colour while a map is set unless
 *   ST_ENV_KEEP_SUN is given. GI's sky pick probability is 0.25 whenever a map is set (for the atmosphere it is 0 while the sun's altitude
 *   is <= -1). GI draws sky directions from the map's importance table (a Vose alias table over a luminance grid of at most 512 x 256
 *   cells) mixed one-to-one with its usual draws, so the estimate keeps its expectation; ST_ENV_UNIFORM_SAMPLING draws as for the atmosphere.
 * - Errors: ST_ERR_INVALID_ARGUMENT for a null pointer, a side outside 1..16384 or width x height > 2^25, channels other than 3 or 4, a
 *   negative or non-finite host texel, a wrong struct_size, unknown flag bits, a negative or non-finite intensity or yaw, and (device
 *   variant) a row pitch that is not a multiple of 4 or shorter than a row. The device variant cannot check texels on the host: its upload
 *   kernel sets NaN, infinite and negative channels to 0 and counts those texels (st_debug_environment_sanitized). A host-only engine
 *   accepts st_environment_set, _update and _clear (validating and storing is host work; light 0 follows them at st_tick) and returns
 *   ST_ERR_NO_DEVICE for st_environment_set_device and the debug seams.
 * - Unaffected: AOVs and StRayHit — "sky" in them means "no hit", as before. History is not reset when the map changes (nor when the sun
 *   moves). */
enum { ST_ENV_KEEP_SUN = 1,            /* the analytic sun light (light 0) stays on; by default it is off while a map is set */
       ST_ENV_UNIFORM_SAMPLING = 2 };  /* no importance sampling: GI draws sky directions exactly as for the atmosphere (tests, A/B) */
typedef struct StEnvironmentDesc {     /* 16 B */
    uint32_t struct_size;              /* sizeof(StEnvironmentDesc) */
    uint32_t flags;                    /* ST_ENV_* */
    float intensity;                   /* linear scale of every texel; finite, >= 0 */
    float yaw;                         /* radians, rotation of the map about +Y; finite */
} StEnvironmentDesc;
/* texels: width x height x channels floats (3 = RGB, 4 = RGBA with alpha ignored), linear, row 0 the zenith; host memory, copied before the
 * call returns */
int st_environment_set(StEngine* e, const float* texels, uint32_t width, uint32_t height, uint32_t channels, const StEnvironmentDesc* desc);
/* the same from device memory, rows `row_pitch_bytes` apart (0 = packed): the contract of st_image_insert_device_rgba8 for a static image —
 * the caller keeps the buffer alive and its writes ordered before the next st_tick, which copies it */
int st_environment_set_device(StEngine* e, const void* texels_device, uint32_t width, uint32_t height, uint32_t channels,
                              size_t row_pitch_bytes, const StEnvironmentDesc* desc);
int st_environment_update(StEngine* e, const StEnvironmentDesc* desc);   /* intensity, yaw and flags; no re-upload */
int st_environment_clear(StEngine* e);                                    /* back to the atmosphere */
/* Radiance .hdr (RGBE) bytes -> width x height x 3 floats, row 0 the top of the image. Header "#?RADIANCE" or "#?RGBE" with
 * FORMAT=32-bit_rle_rgbe (other header lines such as EXPOSURE are ignored); resolution "-Y H +X W" only; flat and new-style run-length
 * scanlines. Texel = m * 2^(e - 136), e == 0 -> 0 (Ward's rgbe.c without the +0.5). Other orientations, 32-bit_rle_xyze and old-style
 * runs are ST_ERR_UNSUPPORTED, and so is an image of more than 2^26 texels; truncated or malformed data is ST_ERR_PARSE, and so is a
 * resolution the remaining bytes cannot hold (every scanline takes at least 12 bytes, flat ones 4 per texel). out_rgb == NULL only
 * reports the size. Needs no engine. */
int st_decode_hdr(const void* bytes, size_t size, float* out_rgb, size_t capacity_floats, uint32_t* width, uint32_t* height);
/* Debug seams: the kernels' own functions over device arrays, enqueued on the stream like the scene queries; they read the live map (the
 * one of the last st_tick; ST_ERR_INVALID_ARGUMENT when there is none). eval: n directions (xyz) -> n rgb; sample: n uniform triples in
 * [0, 1) -> n (xyz, solid-angle pdf) — the first picks the cell, the other two place the direction across and down it, as GI draws them;
 * pdf: n directions -> n pdfs. */
int st_debug_environment_eval(StEngine* e, const float* dirs_device, uint32_t n, float* rgb_device, void* hip_stream);
int st_debug_environment_sample(StEngine* e, const float* u_device /* triples */, uint32_t n, float* dir_pdf_device, void* hip_stream);
int st_debug_environment_pdf(StEngine* e, const float* dirs_device, uint32_t n, float* pdf_device, void* hip_stream);
/* Texels the device uploads have sanitised so far, and the importance table of the live map: cells_x x cells_y cells of (q, alias, p)
 * (12 B each; table == NULL only reports the size). Blocking. */
int st_debug_environment_sanitized(StEngine* e, uint64_t* texels);
int st_debug_environment_table(StEngine* e, void* table, size_t capacity_bytes, uint32_t* cells_x, uint32_t* cells_y);

/* ---- display transforms (NEW seam): exposure, tone mapping and auto-exposure of what a camera writes to its output (st_display.cpp,
 * k_display.hip). What a swap chain, a PPM or an LDR view target shows: without it the 8-bit formats clamp the HDR colour at 1.
 * - Scope: the setting belongs to the camera and takes effect at its next st_render_camera. Only what is written to `out_device` changes:
 *   AOVs, scene queries, the internal planes and the HDR history are not affected. BVH-heatmap frames are false colour and stored as
 *   without a display; every other mode (Reference included) passes through it. desc == NULL turns it off: the output is then exactly
 *   what it is without a display, and the composing kernels are the same ones. The setting survives st_camera_update and
 *   st_engine_set_arithmetic.
 * - Input: c = the composed colour the RGBA32F output holds without a display. Luminance Y = 0.2126 r + 0.7152 g + 0.0722 b, evaluated left
 *   to right in float32 (no fused multiply-add in either build; so is everything below).
 * - Exposure: manual: s = 2^exposure_ev, computed on the host in double and rounded to float. Auto: s = 0.18 * 2^(exposure_ev - adapted_ev),
 *   in float on the device. e = c * s per channel.
 * - Operators (float32, in this order; every operator except NONE first takes max(x, 0) per channel, which turns NaN into 0):
 *     NONE: e. The float formats store it unclamped; the 8-bit formats clamp as always.
 *     REINHARD: e / (1 + e) per channel.   REINHARD_LUMINANCE: e / (1 + Y(e)).
 *     ACES_FITTED (Hill's RRT + ODT fit): v = M_in e; v = (v (v + 0.0245786) - 0.000090537) / (v (0.983729 v + 0.4329510) + 0.238081);
 *       clamp(M_out v, 0, 1). Matrices applied row by row, each row's sum left to right: M_in = [[0.59719, 0.35458, 0.04823],
 *       [0.07600, 0.90834, 0.01566], [0.02840, 0.13383, 0.83777]], M_out = [[1.60475, -0.53108, -0.07367], [-0.10208, 1.10813, -0.00605],
 *       [-0.00327, -0.07276, 1.07602]].
 *     PBR_NEUTRAL (Khronos): x = min(r, g, b); offset = x < 0.08 ? x - 6.25 x x : 0.04; e -= offset; peak = max(r, g, b); if peak < 0.76
 *       the result is e. Else np = 1 - 0.24 * 0.24 / (peak + 0.24 - 0.76); e *= np / peak; g = 1 - 1 / (0.15 (peak - np) + 1); the
 *       result is e (1 - g) + np g.
 *   The result then goes through the camera's output format as always (st_camera_set_output_format); alpha stays 1.
 * - Auto-exposure metering: every pixel the frame composes. Bin k of 64 spans log2 Y in ev_min + [k, k + 1) (ev_max - ev_min) / 64, the
 *   bin index being floor((log2 Y - ev_min) * (64 / (ev_max - ev_min))) in float; Y not > 0 (NaN included) is bin 0, values out of range
 *   (+inf included) go to bin 0 or 63. With N pixels sorted by bin, those of rank [floor(low_fraction N), ceil(high_fraction N)) are kept,
 *   a bin at either end in part; metered_ev = the count-weighted mean of the kept bins' centres (in double, rounded to float). The first
 *   metered frame after st_camera_set_display turns auto on (from off) sets adapted_ev = metered_ev; later frames move adapted_ev to
 *   metered_ev, by at most max_ev_step_up up and max_ev_step_down down per rendered frame (0: no limit; a move within the limit lands on
 *   metered_ev exactly). Frame N's metering sets the s of frame N + 1 (one frame of lag); the first frame after auto is turned on uses
 *   adapted_ev = log2(0.18), so s = 2^exposure_ev. A frame that keeps no pixel changes nothing. Changing other fields while auto stays on
 *   keeps the adapted state. The metering is a histogram per workgroup in LDS, added to (one of 64 replicas of) the camera's device histogram
 *   with integer atomics (reproducible bit for bit), and a one-workgroup kernel behind the frame on the same stream: no host sync, no read-back. Frames of one
 *   camera finalize in order also when the caller changes streams between them.
 * - Tiles: manual exposure works with windows (st_camera_set_window, st_dist_set_partition, st_dist_set_grid): gathered tiles equal the
 *   single-engine frame bit for bit. Auto-exposure would meter each rank's tile on its own, so auto together with a window is
 *   ST_ERR_INVALID_ARGUMENT from whichever of the two setters comes second. To share one exposure, rank 0 runs auto on a full-frame
 *   camera, reads st_camera_exposure and hands scale's EV (log2 scale) to the other ranks, which set it manually.
 * - Errors: ST_ERR_INVALID_ARGUMENT for a null pointer (except desc), a wrong struct_size, an unknown tonemap value or unknown flag bits, a
 *   non-finite field, and with auto on: ev_min >= ev_max, fractions outside 0 <= low_fraction < high_fraction <= 1, or a negative step
 *   limit (with auto off those fields are stored unchecked). An unknown camera is ST_ERR_UNKNOWN_CAMERA. Setting and getting are host work
 *   and valid on a host-only engine; st_camera_exposure and st_debug_camera_histogram return ST_ERR_NO_DEVICE there. */
enum StTonemap { ST_TONEMAP_NONE = 0, ST_TONEMAP_REINHARD = 1, ST_TONEMAP_REINHARD_LUMINANCE = 2, ST_TONEMAP_ACES_FITTED = 3,
                 ST_TONEMAP_PBR_NEUTRAL = 4 };
enum { ST_DISPLAY_AUTO_EXPOSURE = 1 };
typedef struct StDisplayDesc {             /* 40 B */
    uint32_t struct_size;                  /* sizeof(StDisplayDesc) */
    uint32_t tonemap;                      /* StTonemap */
    uint32_t flags;                        /* ST_DISPLAY_* */
    float exposure_ev;                     /* manual: s = 2^exposure_ev; auto: compensation in EV */
    float ev_min, ev_max;                  /* auto: histogram range of log2 luminance */
    float low_fraction, high_fraction;     /* auto: pixels kept are those ranked in [low, high) of the sorted luminances */
    float max_ev_step_up, max_ev_step_down;   /* auto: most the adapted EV may rise / fall per rendered frame; 0 = no limit */
} StDisplayDesc;
int st_camera_set_display(StEngine* e, StHandle camera, const StDisplayDesc* desc);   /* NULL = off */
/* the last desc set (a zeroed desc with struct_size when none was) and whether the display is on; either pointer may be NULL */
int st_camera_get_display(StEngine* e, StHandle camera, StDisplayDesc* out, int* enabled);
/* Blocking: the camera's exposure as the device holds it after its last render (any pointer may be NULL). Display off: scale 1, metered
 * and adapted NaN. Manual: 2^exposure_ev, NaN, NaN. Auto: the scale the next frame uses, the last metered EV (NaN before the first
 * metered frame) and the adapted EV. */
int st_camera_exposure(StEngine* e, StHandle camera, float* scale, float* metered_ev, float* adapted_ev);
/* Blocking debug seam: the 64 bins metered from the camera's last rendered auto-exposure frame (zeros before one). */
int st_debug_camera_histogram(StEngine* e, StHandle camera, uint32_t bins[64]);

/* ---- post-processing (NEW seam): FXAA anti-aliasing and resampling of what a camera writes to its output (st_post.cpp, k_post.hip). The
 * last two nodes of the reference's per-camera graph (bevy-strolle/src/graph.rs: rendering, fxaa, tonemapping, upscaling).
 * - Order: rendering -> display transform -> FXAA -> resample -> output format. The reference runs its FXAA node before tone mapping;
 *   FXAA's thresholds are defined for display-referred values in [0, 1], and on unbounded HDR radiance every light-source edge is an "edge
 *   of contrast infinity", so here (as in Bevy's own main graph) FXAA sees the colour the display transform produced.
 * - Scope: the setting belongs to the camera and takes effect at its next st_render_camera. It changes only what is written to `out_device`
 *   and how large that buffer must be (st_camera_output_size). AOVs, picks, scene queries, st_camera_read_buffer, the auto-exposure metering
 *   (it meters the render-size composed frame) and the HDR history are unchanged; picks and AOVs stay in render-size pixel coordinates.
 *   desc == NULL, or a desc with no flag and an output size equal to the render size, launches nothing new: the frame is the one the same
 *   composing kernels write without post-processing. Otherwise the composing launch writes a camera-owned render-size RGBA32F plane and at
 *   most two launches follow it on the caller's stream (ST_PASS_POST): the frame is complete when that stream has drained, as always. The
 *   setting survives st_camera_update and st_engine_set_arithmetic; an explicit output size is kept when st_camera_update changes the render
 *   size. BVH-heatmap frames are false colour: they skip FXAA but are resampled, so the buffer contract does not depend on the mode.
 * - Arithmetic: float32, evaluated left to right as written, no fused multiply-add, division and square root correctly rounded, in BOTH
 *   builds: tests/post_ref.py restates all of it in numpy and the kernels match it bit for bit. min(a, b) below is a when a < b or b is
 *   NaN, else b; max likewise with >. Colours are r, g, b; alpha is written as 1.
 * - Look-ups: pixel (x, y) has its centre at (x + 0.5, y + 0.5). Along one axis a continuous position p has q = p - 0.5, i0 = floor(q),
 *   f = q - i0. BILINEAR reads the texels i0 and i0 + 1 (indices clamped to the image) and blends a + (b - a) * f, x first, then y;
 *   an axis with f == 0 takes texel a itself (so infinities next door do not leak in as NaN). CATMULL_ROM reads i0 - 1 .. i0 + 2 with the
 *   weights (a = -0.5) w0 = ((-0.5 f + 1) f - 0.5) f, w1 = ((1.5 f - 2.5) f) f + 1, w2 = ((-1.5 f + 2) f + 0.5) f, w3 = ((0.5 f - 0.5) f) f,
 *   summed ((t0 w0 + t1 w1) + t2 w2) + t3 w3, rows first, then the four row results along y (f == 0: the texel i0 itself); the result is
 *   clamped per channel to the min / max of the inner 2 x 2 texels (no ringing around light sources): min(max(v, lo), hi). A position
 *   with f == 0 on both axes takes the texel itself.
 * - Resampling: output pixel (ox, oy) of OW x OH samples the W x H source at ((ox + 0.5) W / OW, (oy + 0.5) H / OH). Per axis this is
 *   evaluated in integers, n = (2 ox + 1) W - OW and d = 2 OW: i0 = floor(n / d), f = float(n - i0 d) / float(d) (one rounding; the
 *   float product (ox + 0.5) * W is not exact above 2^24); NEAREST takes floor((2 ox + 1) W / d). Equal sizes make every filter the
 *   identity, bit for bit. Downscaling is allowed and is point-sampled reconstruction, without a prefilter (exact 2 : 1 bilinear happens to
 *   be the 2 x 2 mean); a prefiltered downscale is not offered.
 * - FXAA (Lottes' FXAA 3.11 quality path, preset 39's 12 steps):
 *     luma L = sqrt(0.2126 r' + 0.7152 g' + 0.0722 b') with x' = x > 0 ? (x < 1 ? x : 1) : 0 (NaN -> 0). M is the pixel's, N S E W NW NE SW SE
 *     its neighbours' (indices clamped at the borders; N is y - 1). range = max - min over M, N, S, E, W; when range < max(edge_threshold_min,
 *     max * edge_threshold) the pixel is copied unchanged. edgeH = |(NW + SW) - 2 W| + 2 |(N + S) - 2 M| + |(NE + SE) - 2 E|, edgeV =
 *     |(NW + NE) - 2 N| + 2 |(W + E) - 2 M| + |(SW + SE) - 2 S|; horizontal when edgeH >= edgeV. Across the edge (N / S when horizontal, W / E
 *     else) the steeper of |neg - M| and |pos - M| picks the side, a tie the negative one (N or W); gradient g = that difference, local
 *     average A = 0.5 (side + M). From the centre moved half a pixel across the edge to that side, walk both ways along the edge to the
 *     distances 1, 2, 3, 4, 5, 6.5, 8.5, 10.5, 12.5, 14.5, 18.5, 26.5 (steps 1 1 1 1 1 1.5 2 2 2 2 4 8) with bilinear look-ups of L; a side
 *     ends at the first distance where |L - A| >= 0.25 g (or at 26.5). With d1, d2 the two distances, edge offset = 0.5 - min(d1, d2) /
 *     (d1 + d2), used only when (L_end - A < 0) differs from (M - A < 0) at the nearer end (d1 < d2: the negative end, else the positive one),
 *     else 0. Subpixel term: a = |((((N + S) + (E + W)) 2 + ((NW + NE) + (SW + SE))) / 12 - M| / range, clamped to at most 1; s = ((-2 a + 3) a) a;
 *     offset_sub = (s s) fxaa_subpixel. The result is the bilinear colour look-up at the centre moved across the edge, to the chosen side, by
 *     max(edge offset, offset_sub).
 * - Tiles: FXAA's edge search and the resampler read neighbours across tile edges, so a camera cannot have post-processing (any desc) and
 *   a window (st_camera_set_window, st_dist_set_partition, st_dist_set_grid) at once: ST_ERR_INVALID_ARGUMENT from whichever setter comes
 *   second. For tiled frames the ranks render RGBA32F without post-processing, st_dist_gather assembles the frame on rank 0, and rank 0
 *   runs st_post_process on it. Tiled frames carry no upscaling either ("upscaling" below): rank 0 runs st_upscale_process on the
 *   gathered frame, behind st_post_process when FXAA is wanted.
 * - Errors: ST_ERR_INVALID_ARGUMENT for a wrong struct_size, unknown flags or filter, exactly one of the two output sides 0, a side above
 *   16384, a threshold that is not finite or is negative, fxaa_subpixel outside [0, 1] (NaN included) and null pointers where they are not
 *   allowed. An unknown camera is ST_ERR_UNKNOWN_CAMERA. Set, get and st_camera_output_size are host work and valid on a host-only engine;
 *   st_post_process returns ST_ERR_NO_DEVICE there. */
enum StResampleFilter { ST_RESAMPLE_NEAREST = 0, ST_RESAMPLE_BILINEAR = 1, ST_RESAMPLE_CATMULL_ROM = 2 };
enum { ST_POST_FXAA = 1 };
typedef struct StPostDesc {                /* 32 B */
    uint32_t struct_size;                  /* sizeof(StPostDesc) */
    uint32_t flags;                        /* ST_POST_* */
    uint32_t output_width, output_height;  /* 0, 0 = the camera's render size (no resampling) */
    uint32_t filter;                       /* StResampleFilter; ignored when the sizes are equal */
    float fxaa_edge_threshold;             /* 0 = default 0.166 */
    float fxaa_edge_threshold_min;         /* 0 = default 0.0833 */
    float fxaa_subpixel;                   /* 0..1; NaN is an error; no "0 = default": the caller writes 0.75 for FXAA 3.11's default */
} StPostDesc;
int st_camera_set_post(StEngine* e, StHandle camera, const StPostDesc* desc);   /* NULL = off */
/* the last desc set (a zeroed desc with struct_size when none was) and whether post-processing is on; either pointer may be NULL */
int st_camera_get_post(StEngine* e, StHandle camera, StPostDesc* out, int* enabled);
/* what st_render_camera's buffer must hold, in pixels of the camera's output format; either pointer may be NULL */
int st_camera_output_size(StEngine* e, StHandle camera, uint32_t* width, uint32_t* height);
/* Stateless: the same two kernels over any RGBA32F device image of width x height, written to dst_device (the desc's output size, or
 * width x height) in dst_format. Needs a device engine; no camera, no tick. Enqueued on hip_stream without a host sync. A call
 * that runs FXAA and then resamples uses an engine-owned intermediate plane: it is allocated (with a device sync) only when a call needs a
 * larger one than any before it, and calls that use it on different streams are ordered by the engine. src and dst must not overlap. */
int st_post_process(StEngine* e, const StPostDesc* desc, const void* src_rgba32f_device, uint32_t width, uint32_t height,
                    void* dst_device, int dst_format /* StOutputFormat */, void* hip_stream);

/* ---- upscaling (NEW seam): an edge-adaptive upscaler and contrast-adaptive sharpening behind FXAA (st_upscale.cpp, k_upscale.hip). The
 * construction of FidelityFX Super Resolution 1.0 (EASU and RCAS, publicly documented), restated here in this library's arithmetic rules;
 * the sharpening step is what Bevy calls ContrastAdaptiveSharpening. The separable Catmull-Rom resampler of the post-processing section
 * treats every edge as axis-aligned; the upscaler turns its kernel along the local edge, so slanted edges stay edges.
 * - Order: rendering -> display transform -> FXAA -> upscale -> sharpen -> output format. With FXAA on (st_camera_set_post), the FXAA
 *   launch writes the render-size RGBA32F plane the upscaler reads. The stage takes the resampler's place: a StPostDesc whose explicit
 *   output size differs from the render size and this stage exclude each other (one stage owns the resize), ST_ERR_INVALID_ARGUMENT from
 *   whichever setter comes second; FXAA alone is fine.
 * - Output size: st_camera_output_size reports the descriptor's output size while the stage is on. output_width, output_height = 0, 0 (or
 *   the render size) skips the upscale step: sharpen only. sharpness = 0 skips the sharpening step: upscale only. A descriptor that asks
 *   for neither, like desc == NULL, launches nothing new and changes no argument of any existing launch. This is an upscaler: an output
 *   side smaller than the render side is an error, and st_camera_update to a render size larger than a live descriptor's output size
 *   (or, with this stage on, to one that would make a StPostDesc's explicit output size a resize) is refused and leaves the camera as it was.
 * - Scope: the setting belongs to the camera, takes effect at its next st_render_camera and survives st_camera_update and
 *   st_engine_set_arithmetic. It changes only what reaches `out_device`: AOVs, picks, planes, exposure metering and history are unchanged.
 *   BVH-heatmap frames are false colour: they skip both steps and are brought to the output size by the NEAREST resampler, so the buffer
 *   contract does not depend on the mode. Reference and orthographic frames go through the stage.
 * - Display-referred: every texel either step reads goes through x' = x > 0 ? (x < 1 ? x : 1) : 0 first (NaN -> 0; the FXAA luma's
 *   clamp). With ST_DISPLAY_NONE and an HDR output format the stage therefore clips at 1: HDR callers use ST_RESAMPLE_CATMULL_ROM instead.
 *   Indices are clamped to the image. Alpha is written as 1.
 * - Arithmetic: float32, evaluated left to right as written, no fused multiply-add, division and square root correctly rounded (plain
 *   / and sqrt, where FSR uses approximate reciprocals), min and max the post-processing section's, in BOTH builds: tests/upscale_ref.py
 *   restates all of it in numpy, is normative where this prose leaves a choice, and the kernels match it bit for bit.
 * - Upscale: per axis i0 and f are the post-processing section's integer evaluation ("Resampling"); (x0, y0), (fx, fy) below. Twelve taps:
 *         b c            b = (x0, y0 - 1), c = (x0 + 1, y0 - 1)
 *       e f g h          e = (x0 - 1, y0), f = (x0, y0), g = (x0 + 1, y0), h = (x0 + 2, y0)
 *       i j k l          i = (x0 - 1, y0 + 1), j = (x0, y0 + 1), k = (x0 + 1, y0 + 1), l = (x0 + 2, y0 + 1)
 *         n o            n = (x0, y0 + 2), o = (x0 + 1, y0 + 2)
 *   Luma L = 0.5 B + (0.5 R + G). Four plus-shaped stencils, in the order f, g, j, k, with weights w = (1 - fx)(1 - fy), fx (1 - fy),
 *   (1 - fx) fy, fx fy and arms (top, left, right, bottom) = (b, e, g, j), (c, f, h, k), (f, i, k, n), (g, j, l, o), add to dir = (0, 0)
 *   and len = 0; each along x first (p left, q centre, r right), then along y (p top, q centre, r bottom):
 *     dir.x (dir.y) += (r - p) w;  m = max(|r - q|, |q - p|);  t = m > 0 ? min(|r - p| / m, 1) : 0;  len += (t t) w.
 *   r2 = dir.x dir.x + dir.y dir.y; r2 < 1 / 32768: dir = (1, 0), else s = sqrt(r2), dir = (dir.x / s, dir.y / s). len = 0.5 len, then
 *   len = len len. stretch = (dir.x dir.x + dir.y dir.y) / max(|dir.x|, |dir.y|); len2 = (1 + (stretch - 1) len, 1 - 0.5 len);
 *   lob = 0.5 + ((0.25 - 0.04) - 0.5) len (the constant folded in float32); clp = 1 / lob.
 *   A tap at (x0 + dx, y0 + dy) has o = (float(dx) - fx, float(dy) - fy); v = ((o.x dir.x + o.y dir.y) len2.x, (-o.x dir.y + o.y dir.x) len2.y);
 *   d2 = min(v.x v.x + v.y v.y, clp); tb = 0.4 d2 - 1; wB = 1.5625 (tb tb) - 0.5625; ta = lob d2 - 1; wA = ta ta; w = wB wA.
 *   Per channel sum = sum + c w and wsum = wsum + w, from 0, over the taps in the order b c e f g h i j k l n o; the result is
 *   sum / wsum when wsum > 0, else tap f's channel, then clamped to the min / max of f, g, j, k: min(max(v, lo), hi).
 * - Sharpen, at the output size: e the pixel, b, d, f, h its N (y - 1), W, E, S neighbours. Per channel: mn4 = min(min(min(b, d), f), h),
 *   mx4 likewise; hitMin = mx4 == 0 ? 0 : min(mn4, e) / (4 mx4); den = 4 mn4 - 4; hitMax = den == 0 ? 0 : (1 - max(mx4, e)) / den;
 *   lobe_c = max(-hitMin, hitMax). lobe = max(-0.1875, min(max(max(lobe_r, lobe_g), lobe_b), 0)) sharpness. With ST_UPSCALE_DENOISE, on
 *   the lumas (L as above): range = max(max(max(max(bL, dL), fL), hL), eL) - the min likewise; nz = range == 0 ? 0 :
 *   min(|(((0.25 bL + 0.25 dL) + 0.25 fL) + 0.25 hL) - eL| / range, 1); lobe = lobe (1 - 0.5 nz). Per channel the result is
 *   ((((lobe b + lobe d) + lobe h) + lobe f) + e) / (4 lobe + 1).
 * - Tiles: both steps read across tile edges, so the stage and a window (st_camera_set_window, st_dist_set_partition, st_dist_set_grid)
 *   exclude each other like post-processing does. For tiled frames rank 0 runs st_upscale_process on the gathered frame.
 * - Errors: ST_ERR_INVALID_ARGUMENT for a wrong struct_size, unknown flags, non-zero pads, exactly one output side 0, a side above 16384,
 *   an output side smaller than the render side, sharpness outside [0, 1] (NaN included), null pointers where they are not allowed, and
 *   src and dst overlapping. An unknown camera is ST_ERR_UNKNOWN_CAMERA. Set and get are host work and valid on a host-only engine;
 *   st_upscale_process returns ST_ERR_NO_DEVICE there. */
enum { ST_UPSCALE_DENOISE = 1 };           /* the sharpening step's noise limiter */
typedef struct StUpscaleDesc {             /* 32 B */
    uint32_t struct_size;                  /* sizeof(StUpscaleDesc) */
    uint32_t flags;                        /* ST_UPSCALE_* */
    uint32_t output_width, output_height;  /* 0, 0 = the render size: sharpen only */
    float sharpness;                       /* 0..1; 0 = no sharpening step; NaN is an error */
    uint32_t _pad[3];                      /* zero */
} StUpscaleDesc;
int st_camera_set_upscale(StEngine* e, StHandle camera, const StUpscaleDesc* desc);   /* NULL = off */
/* the last desc set (a zeroed desc with struct_size when none was) and whether the stage is on; either pointer may be NULL */
int st_camera_get_upscale(StEngine* e, StHandle camera, StUpscaleDesc* out, int* enabled);
/* Stateless, like st_post_process: the same kernels over any RGBA32F device image of width x height, written to dst_device (the desc's
 * output size, or width x height) in dst_format; a desc that asks for neither step copies the image into the format (unclamped, alpha 1) as
 * st_post_process without flags does. src and dst must not overlap. A call that runs both steps uses an engine-owned output-size plane, allocated
 * (with a device sync) only when a call needs a larger one than any before it; calls that use it on different streams are ordered by the
 * engine. */
int st_upscale_process(StEngine* e, const StUpscaleDesc* desc, const void* src_rgba32f_device, uint32_t width, uint32_t height,
                       void* dst_device, int dst_format /* StOutputFormat */, void* hip_stream);

/* Debug seam: how the stage runs when both steps are on. 0: two launches with an output-size RGBA32F plane between them; 1, 2, 3: one
 * launch whose workgroups upscale an output tile of 64 x 8, 32 x 32 or 64 x 16 pixels plus a one-pixel ring into LDS and sharpen from
 * there. The result is the same bit for bit (the per-pixel arithmetic is the same); the ring is computed twice. The environment
 * variable ST_UPSCALE_FUSED sets the same at st_engine_create. Takes effect at the next frame or call. */
int st_debug_set_upscale_fused(StEngine* e, int tile);

/* ---- bloom (NEW seam): an HDR mip-pyramid glow in front of the display transform (st_bloom.cpp, k_bloom.hip). The first node of Bevy's
 * HDR post chain (bloom -> tonemapping -> FXAA -> upscaling): what tells a viewer how bright a clipped light is.
 * - Order: rendering -> bloom -> display transform -> FXAA -> resample -> output format.
 * - Scope: the setting belongs to the camera and takes effect at its next st_render_camera. It changes only what is written to
 *   `out_device`: AOVs, picks, scene queries, st_camera_read_buffer, the HDR history and the auto-exposure metering (it keeps metering the
 *   composed frame before bloom: st_camera_exposure is the same with bloom on or off) are unchanged. BVH-heatmap frames are false colour and
 *   skip bloom; every other mode (Reference included) passes through it. desc == NULL turns it off: the frame then launches the kernels it
 *   launches without bloom, with the same arguments. The setting survives st_camera_update and st_engine_set_arithmetic. While a frame
 *   blooms, the composing launch writes the composed colour, untransformed, into a camera-owned render-size RGBA32F plane (and meters it);
 *   2 L launches (ST_PASS_POST, in front of FXAA and the resampler) follow on the caller's stream: L downsamples, L - 1 upsamples
 *   and the composite, which also runs the display transform and writes the output format (or the post-processing plane; with colour
 *   grading on, below, the composite stores its colour untransformed into the grade's RGBA32F plane instead). The pyramid is one
 *   allocation, made by the first frame that needs it and again only when a larger render size or level count needs a larger one.
 * - Arithmetic: float32, evaluated left to right as written, no fused multiply-add, division correctly rounded, in BOTH builds;
 *   tests/bloom_ref.py restates all of it in numpy and the kernels match it bit for bit. min / max are the post-processing section's
 *   (min(a, b) is a when a < b or b is NaN, else b; max likewise with >). Colours are r, g, b; alpha is written as 1. t(x, y) below is a
 *   texel with both indices clamped to its image.
 * - Plan (st_bloom_plan): mip 0 is ceil(W / 2) x ceil(H / 2), mip k halves mip k - 1 the same way. The level count L is the requested one
 *   (0 = 6) reduced until mip L - 1 has both sides >= 2; a frame that cannot hold one level (a side below 3) has L = 0 and is not bloomed
 *   (st_bloom_process then only applies the display transform and the format). Blend factor of level k, with x = k / max(L - 1, 1), in double
 *   on the host and rounded to float: lf = (1 - (1 - x)^(1 / (1 - curvature))) low_frequency_boost, times (1 - intensity) unless
 *   ST_BLOOM_ADDITIVE; hp = 1 - clamp((x - f) / f, 0, 1) with f = high_pass_frequency; b_k = (intensity + lf) hp.
 * - Prefilter P of a frame texel: per channel v = min(max(x, 0), clamp) (NaN -> 0, +inf -> clamp: the pyramid is finite whatever the frame
 *   holds). With threshold > 0: knee = threshold softness, m = max(max(r, g), b), s = min(max(m - (threshold - knee), 0), 2 knee),
 *   s = (s s) / (4 knee + 1e-4), w = max(m - threshold, s) / max(m, 1e-4), and each channel is v w. (knee, threshold - knee, 2 knee and
 *   4 knee + 1e-4 are float32 values computed once.)
 * - Downsample (13 taps on the texel grid): for destination pixel (x, y), S(dx, dy) = ((t(X, Y) + t(X + 1, Y)) + (t(X, Y + 1) + t(X + 1, Y + 1))) 0.25
 *   with (X, Y) = (2 x + dx, 2 y + dy). a b c = S(-2, -2) S(0, -2) S(2, -2), d e f = S(-2, 0) S(0, 0) S(2, 0), g h i = S(-2, 2) S(0, 2) S(2, 2),
 *   j k = S(-1, -1) S(1, -1), l m = S(-1, 1) S(1, 1). G0 = (((a + b) + d) + e) 0.25, G1 = (((b + c) + e) + f) 0.25, G2 = (((d + e) + g) + h) 0.25,
 *   G3 = (((e + f) + h) + i) 0.25, G4 = (((j + k) + l) + m) 0.25, weights W0..3 = 0.125, W4 = 0.5. The result is
 *   (((G0 W0 + G1 W1) + G2 W2) + G3 W3) + G4 W4. The first downsample (frame -> mip 0) reads P(t). With ST_BLOOM_FIREFLY_SUPPRESS it uses
 *   Wi' = Wi (1 / (1 + Y(Gi))) (Y: the display section's luminance) and divides that sum by (((W0' + W1') + W2') + W3') + W4'.
 * - Upsample U(x, y) of a mip to a destination twice its size (or one less): the destination pixel sits at ((x + 0.5) / 2, (y + 0.5) / 2)
 *   in source texels, so by the post-processing section's look-up rule i0 = floor((x + 1) / 2) - 1 and f = 0.75 for even x, 0.25 for odd x
 *   (likewise y). B(ox, oy) is the bilinear look-up at texels (i0 + ox, j0 + oy): top = t(i, j) + (t(i + 1, j) - t(i, j)) fx, bottom likewise
 *   on row j + 1, B = top + (bottom - top) fy. U = B(-1, -1) / 16 + B(0, -1) / 8 + B(1, -1) / 16 + B(-1, 0) / 8 + B(0, 0) / 4 + B(1, 0) / 8 +
 *   B(-1, 1) / 16 + B(0, 1) / 8 + B(1, 1) / 16, summed left to right in this order.
 * - Chain: for k = L - 1 .. 1: mip[k - 1] = mip[k - 1] (1 - b_k) + U_k b_k, or mip[k - 1] + U_k b_k with ST_BLOOM_ADDITIVE.
 * - Composite: c' = c (1 - b_0) + U_0 b_0, or c + U_0 b_0 with ST_BLOOM_ADDITIVE, c being the composed colour as it is: an infinite pixel
 *   stays infinite and reaches no other pixel. c' goes through the display transform (the camera's operator and its manual or metered
 *   scale) and the output format.
 * - Tiles: bloom reads far across tile edges, so a camera cannot have bloom and a window (st_camera_set_window, st_dist_set_partition,
 *   st_dist_set_grid) at once: ST_ERR_INVALID_ARGUMENT from whichever setter comes second. For tiled frames the ranks render RGBA32F with
 *   display and bloom off, st_dist_gather assembles the frame on rank 0, and rank 0 runs st_bloom_process (with the display descriptor) and
 *   then st_post_process on it.
 * - Errors: ST_ERR_INVALID_ARGUMENT for a wrong struct_size, unknown flags, a field outside the ranges below (NaN included), a null pointer
 *   where one is not allowed, a frame side above 16384 (st_bloom_plan, st_bloom_process; 0 too for st_bloom_process), and an auto-exposure
 *   display passed to st_bloom_process. An unknown camera is ST_ERR_UNKNOWN_CAMERA. Set, get
 *   and st_bloom_plan are host work and valid on a host-only engine; st_bloom_process returns ST_ERR_NO_DEVICE there. */
enum { ST_BLOOM_ADDITIVE = 1, ST_BLOOM_FIREFLY_SUPPRESS = 2 };
typedef struct StBloomDesc {               /* 40 B */
    uint32_t struct_size;                  /* sizeof(StBloomDesc) */
    uint32_t flags;                        /* ST_BLOOM_* */
    uint32_t levels;                       /* 1..8; 0 = default 6 */
    float intensity;                       /* finite, >= 0; <= 1 unless ST_BLOOM_ADDITIVE */
    float low_frequency_boost;             /* 0..1 */
    float low_frequency_boost_curvature;   /* 0 <= curvature < 1 */
    float high_pass_frequency;             /* 0 < f <= 1 */
    float threshold;                       /* >= 0, finite; 0 = no prefilter threshold */
    float threshold_softness;              /* 0..1 */
    float clamp;                           /* > 0, finite; 0 = default 65504 */
} StBloomDesc;
int st_camera_set_bloom(StEngine* e, StHandle camera, const StBloomDesc* desc);   /* NULL = off */
/* the last desc set (a zeroed desc with struct_size when none was) and whether bloom is on; either pointer may be NULL */
int st_camera_get_bloom(StEngine* e, StHandle camera, StBloomDesc* out, int* enabled);
/* Pure host arithmetic, no engine: the effective level count, each mip's size (width, height pairs) and the per-level blend factors for a
 * width x height frame. Entries past the level count are 0. Any of the three outputs may be NULL. */
int st_bloom_plan(const StBloomDesc* desc, uint32_t width, uint32_t height, uint32_t* levels, uint32_t sizes_wh[16], float factors[8]);
/* Stateless, like st_post_process: src (RGBA32F, HDR) -> bloom -> the display transform (NULL = none; manual exposure only) -> dst_device
 * (width x height) in dst_format. Needs a device engine; no camera, no tick. Enqueued on hip_stream without a host sync. The pyramid is
 * engine-owned: it is allocated (with a device sync) only when a call needs a larger one than any before it, and calls on different
 * streams are ordered by the engine. src and dst must not overlap. */
int st_bloom_process(StEngine* e, const StBloomDesc* desc, const StDisplayDesc* display, const void* src_rgba32f_device,
                     uint32_t width, uint32_t height, void* dst_device, int dst_format /* StOutputFormat */, void* hip_stream);
/* Debug / measurement seam: the fused tail of the bloom chain, OFF by default (it measured slower than the launches it replaces:
 * tools/experiments/bloom_fused_tail.md). With it the last levels of the pyramid, those whose mips fit one workgroup's LDS together at three
 * floats per texel, go down and back up in ONE single-workgroup launch instead of two launches per level; the bits are those of the
 * straightforward chain. lds_bytes: 0 = no fused tail (the default), -1 = what the device grants, n = at most n bytes. The
 * environment variable ST_BLOOM_TAIL_BYTES sets the same when an engine is created. *in_force (may be NULL): the byte budget now in force
 * (0 on a host-only engine). */
int st_debug_set_bloom_tail(StEngine* e, int lds_bytes, uint32_t* in_force);

/* ---- motion blur (NEW seam): a velocity-driven gather in front of bloom (st_motion_blur.cpp, k_motion_blur.hip). The node Bevy's graph
 * places directly before bloom (motion blur -> bloom -> tonemapping -> FXAA -> upscaling), and the first user-visible consumer of the
 * renderer's per-pixel motion (the velocity map, ST_AOV_MOTION, deformation motion).
 * - Order: rendering -> motion blur -> bloom -> display transform -> FXAA -> resample -> output format.
 * - Scope: the setting belongs to the camera and takes effect at its next st_render_camera. It changes only what is written to
 *   `out_device`: AOVs, picks, scene queries, the HDR history, every plane st_camera_read_buffer returns (with the one exception below) and
 *   the auto-exposure metering (it keeps metering the composed frame in the composing launch, before the blur) are unchanged. desc == NULL
 *   turns it off: the frame then launches the kernels it launches without the setting, with the same arguments, and st_debug_last_launches
 *   is unchanged. The setting survives st_camera_update and st_engine_set_arithmetic. Modes without a velocity map skip the blur:
 *   ST_MODE_REFERENCE and ST_MODE_BVH_HEATMAP run no primary-visibility pass, and their frames are bit for bit the frames without the
 *   setting. Sky pixels have velocity 0 in the renderer's map, so the sky is not blurred by camera rotation; moving geometry still blurs
 *   over it (sky velocity from the camera matrices is not offered). The one plane whose contents the setting changes is
 *   ST_BUF_VELOCITY_MAP: the default frame (fast build, Image{denoise}) keeps the velocity in registers and leaves that plane stale; while
 *   a camera blurs, primary visibility stores it (16 B per pixel) and st_camera_buffer_stale reports it as current. Nothing else about that
 *   frame changes. What "at rest" means is per tile neighbourhood (step 4): a static pixel in a tile next to a moving one goes through the
 *   gather, where its weights make it c(X), so it comes back clamped to [0, 65504] (NaN as 0) with alpha 1, not with C(X)'s own bits;
 *   only pixels of tiles whose 3 x 3 neighbourhood is at rest pass through untouched. While a frame blurs, the composing launch writes the composed colour, untransformed, into a camera-owned render-size
 *   RGBA32F plane (and meters it); three launches (ST_PASS_POST) belong to the blur: pack (with the tile maximum) as soon as primary
 *   visibility is through, and the neighbour maximum and the gather behind the composing launch, in front of bloom, FXAA and the resampler.
 * - Arithmetic: float32, evaluated left to right as written, no fused multiply-add, division and square root correctly rounded, in BOTH
 *   builds; tests/motion_blur_ref.py restates all of it in numpy and the kernels match it bit for bit. min, max and
 *   clamp01(x) = min(max(x, 0), 1) use the post-processing section's NaN rule (min(a, b) is a when a < b or b is NaN, else b; max likewise
 *   with >). The frame is W x H. C is the composed HDR colour, V the velocity in pixels (current minus previous screen position), Z the
 *   distance along the camera ray. In a frame, V is the velocity map's xy and Z is PRIM_GBUFFER_D0.x of the frame's parity, with 0 (sky) read
 *   as FLT_MAX; in st_motion_blur_process V and Z are the given planes as they are. R = max_radius, S = samples, e_s = depth_softness, each
 *   after its default is applied.
 * - 1. Pack (per pixel): h = 0.5 shutter (one float). v = (V.x h, V.y h); r = sqrt(v.x v.x + v.y v.y). If not r >= 0.5 (NaN included):
 *   v = 0, r = 0. Else if r > R: k = R / r; v = (v.x k, v.y k); r = R. (r, Z) is stored as a float2 plane; v feeds step 2.
 * - 2. Tile maximum: tiles are 32 x 32 pixels, ceil(W / 32) x ceil(H / 32) of them. A tile's vector is the v of its pixel with the largest
 *   r; among equal r the first pixel in row-major order wins; a tile with all r = 0 has vector 0. (A 64-bit key, r's bits above the complement
 *   of the pixel's index in the tile, makes this one unsigned max, reduced with cross-lane operations and one LDS step per workgroup.) Pack
 *   and tile maximum are one launch.
 * - 3. Neighbour maximum: n(tile) is the tile vector with the largest r over the 3 x 3 tiles around it that exist; ties go to the first in
 *   row-major order of (dy, dx); r_n is its length as stored, not recomputed. One small launch.
 * - 4. Gather (per pixel X = (x, y), with n and r_n of its tile): if r_n < 0.5, the result is C(X) with its own bits: NaN and infinities pass
 *   through. Otherwise let c(Y) be C(Y) with each of r, g, b as min(max(., 0), 65504), so that one infinite pixel cannot poison a streak, and
 *   (r_X, Z_X), (r_Y, Z_Y) the packed values. j = 0 with ST_MOTION_BLUR_NO_JITTER; otherwise j = (B[y & 3][x & 3] + 0.5) / 16 - 0.5, with B
 *   the 4 x 4 Bayer matrix {0 8 2 10 / 12 4 14 6 / 3 11 1 9 / 15 7 13 5}. w_0 = 1 / max(r_X, 0.5); sum = c(X) w_0; wsum = w_0. For
 *   i = 0 .. S - 1, in order: t = ((i + 0.5 + j) 2) / S - 1; p = (x + 0.5 + n.x t, y + 0.5 + n.y t); Y = (floor p.x, floor p.y), each
 *   clamped to the image (in float, as min(max(floor p, 0), side - 1): NaN reads texel 0); d = |t| r_n; e = max(e_s min(Z_X, Z_Y), 1e-6);
 *   f = clamp01(1 - (Z_Y - Z_X) / e); b = clamp01(1 - (Z_X - Z_Y) / e); cone(d, r) = r > 0 ? clamp01(1 - d / r) : 0; cyl(d, r) = 0 for
 *   r = 0, else 1 - q q (3 - 2 q) with q = clamp01((d - 0.95 r) / (1.05 r - 0.95 r));
 *   w = (f cone(d, r_Y) + b cone(d, r_X)) + (cyl(d, r_Y) cyl(d, r_X)) 2; sum += c(Y) w per channel; wsum += w. The result is sum / wsum per
 *   channel, alpha 1. This is the reconstruction filter of McGuire et al. 2012 with nearest-texel taps. The result goes through the display
 *   transform and the output format when the blur is the last HDR node; with bloom on it is stored untransformed as RGBA32F into the plane
 *   bloom reads.
 * - Tiles: the gather reads up to 32 pixels across tile edges, and the tile grid is the frame's, so a camera cannot have motion blur and a
 *   window (st_camera_set_window, st_dist_set_partition, st_dist_set_grid) at once: ST_ERR_INVALID_ARGUMENT from whichever setter comes
 *   second, as for bloom. For tiled frames rank 0 runs st_motion_blur_process on the gathered colour, MOTION and DEPTH planes.
 * - Errors: ST_ERR_INVALID_ARGUMENT for a wrong struct_size, unknown flags, an odd samples or one outside 2..32 other than 0, a field
 *   outside its range (NaN included), null pointers where they are not allowed, a frame side of 0 or above 16384 in the process call, and an
 *   auto-exposure display passed to the process call. An unknown camera is ST_ERR_UNKNOWN_CAMERA. Set and get are host work and valid on a
 *   host-only engine; st_motion_blur_process returns ST_ERR_NO_DEVICE there. */
enum { ST_MOTION_BLUR_NO_JITTER = 1 };
typedef struct StMotionBlurDesc {          /* 24 B */
    uint32_t struct_size;                  /* sizeof(StMotionBlurDesc) */
    uint32_t flags;                        /* ST_MOTION_BLUR_* */
    uint32_t samples;                      /* even, 2..32; 0 = default 8 */
    float shutter;                         /* fraction of the frame interval the shutter is open: finite, 0 <= shutter <= 4; Bevy's default is 0.5 */
    float max_radius;                      /* pixels, 0 < r <= 32; 0 = default 32 */
    float depth_softness;                  /* relative depth extent of the soft depth test, 0 < s <= 1; 0 = default 0.05 */
} StMotionBlurDesc;
int st_camera_set_motion_blur(StEngine* e, StHandle camera, const StMotionBlurDesc* desc);   /* NULL = off */
/* the last desc set (a zeroed desc with struct_size when none was) and whether the blur is on; either pointer may be NULL */
int st_camera_get_motion_blur(StEngine* e, StHandle camera, StMotionBlurDesc* out, int* enabled);
/* Stateless, like st_bloom_process. color: RGBA32F; velocity: f32x2 (ST_AOV_MOTION's layout); depth: f32 (ST_AOV_DEPTH's layout, FLT_MAX on
 * sky); display NULL = none, manual exposure only; dst in dst_format, width x height. Needs a device engine; no camera, no tick. Enqueued
 * on hip_stream without a host sync. The packed plane and the tile vectors are engine-owned: allocated (with a device sync) only when a call
 * needs larger ones than any before it, and calls on different streams are ordered by the engine. No input may overlap dst. */
int st_motion_blur_process(StEngine* e, const StMotionBlurDesc* desc, const StDisplayDesc* display, const void* color_device,
                           const void* velocity_device, const void* depth_device, uint32_t width, uint32_t height,
                           void* dst_device, int dst_format /* StOutputFormat */, void* hip_stream);

/* ---- depth of field (NEW seam): a thin-lens circle-of-confusion gather in front of motion blur (st_dof.cpp, k_dof.hip). The HDR node
 * Bevy's graph places directly before motion blur (DepthOfField -> motion blur -> bloom -> tonemapping -> FXAA -> upscaling): a camera
 * with a physical lens (focal length from the projection and the sensor height, an aperture in f-stops) focused at a distance or on a
 * point of the frame.
 * - Order: rendering -> depth of field -> motion blur -> bloom -> display transform -> FXAA -> resample -> output format.
 * - Scope: the setting belongs to the camera and takes effect at its next st_render_camera. It changes only what is written to
 *   `out_device`: AOVs, picks, scene queries, the HDR history, every plane st_camera_read_buffer returns and the auto-exposure metering (it
 *   keeps metering the composed frame in the composing launch, before the blur) are unchanged. desc == NULL turns it off: the frame then
 *   launches the kernels it launches without the setting, with the same arguments, and st_debug_last_launches is unchanged. The setting
 *   survives st_camera_update and st_engine_set_arithmetic. Frames that skip it, bit for bit the frames without the setting:
 *   ST_MODE_REFERENCE and ST_MODE_BVH_HEATMAP, which have no G-buffer, and a frame whose projection is not a perspective one
 *   (projection[15] != 0; also a projection whose [5] is not positive and finite or whose [0] is 0 or not finite), because the focal
 *   length is derived from the projection. Unlike motion blur, the sky is blurred, as geometry at infinity. While a frame focuses, the
 *   composing launch writes the composed colour, untransformed, into a camera-owned render-size RGBA32F plane (and meters it); three
 *   launches (ST_PASS_POST) belong to the filter: pack (with the tile maximum) as soon as primary visibility is through, and the neighbour
 *   maximum and the gather behind the composing launch, in front of motion blur, bloom, FXAA and the resampler. The gather writes motion
 *   blur's HDR plane (untransformed) when motion blur is on, otherwise bloom's when bloom is on, otherwise what the composing launch would
 *   have written, through the display transform and the output format. Focus smoothing over time is not offered: with ST_DOF_AUTOFOCUS the
 *   focus distance is this frame's depth under the focus point, and it jumps when that does.
 * - Arithmetic: float32, evaluated left to right as written, no fused multiply-add, division and square root correctly rounded, in BOTH
 *   builds; tests/dof_ref.py restates all of it in numpy and the kernels match it bit for bit. min, max and clamp01 use the post-processing
 *   section's NaN rule. The frame is W x H. C is the composed HDR colour, D the distance along the camera ray, P the column-major
 *   projection. In a frame, D is PRIM_GBUFFER_D0.x of the frame's parity (ST_AOV_DEPTH's value), with 0 (sky) read as FLT_MAX, and P is the
 *   camera's; in st_dof_process D and P are the given ones as they are. N = aperture_f_stops, h_s = sensor_height, R = max_radius,
 *   S = samples, each after its default is applied.
 * - 0. Host constants, per frame, in double (every operand converted to double first, left to right), each rounded to float once:
 *   f_d = 0.5 h_s P[5]; K_d = 0.5 f_d f_d / (N h_s) H; f = (float)f_d, the focal length in metres; K = (float)K_d, in pixel-metres. The
 *   tap table T[k], k < S: rho = sqrt((k + 0.5) / S), th = k 2.399963229728653 (the golden angle), T[k] = (rho cos th, rho sin th, rho),
 *   computed in double and rounded to float; st_dof_plan returns it.
 * - 1. Planar depth (per pixel (x, y)): a lens focuses on a plane and D is radial. The pixel centre maps to NDC as the camera's rays do:
 *   ndc_x = (x + 0.5) 2 / W - 1; ndc_y = -((y + 0.5) 2 / H - 1), with W and H as floats. ax = (ndc_x + P[8]) / P[0];
 *   ay = (ndc_y + P[9]) / P[5]; c = 1 / sqrt((ax ax + ay ay) + 1); Z = D c. If D >= FLT_MAX (sky, +inf), Z = FLT_MAX. With
 *   ST_DOF_PLANAR_DEPTH, which only st_dof_process honours (D is then a planar depth already), c = 1: Z = D.
 * - 2. Focus: s = focal_distance. With ST_DOF_AUTOFOCUS, let Z_f be the Z of pixel (min(floor(focus_x W), W - 1),
 *   min(floor(focus_y H), H - 1)) of this same frame (the products in float); if 0 < Z_f < FLT_MAX, s = Z_f, otherwise (sky, NaN) s stays
 *   focal_distance. Every workgroup of the pack launch reads that pixel with one uniform load: no extra launch, no host read-back.
 *   m = max(s - f, 1e-6); A = K / m.
 * - 3. Pack (per pixel): coc = Z > 0 ? A (1 - s / Z) : 0, the signed radius in pixels of the circle of confusion: negative in front of the
 *   focal plane, tending to A at infinity. coc = min(max(coc, -R), R). (coc, Z) is stored as a float2 plane.
 * - 4. Near-field tile maximum: tiles are 32 x 32 pixels, ceil(W / 32) x ceil(H / 32) of them. A tile's value is the largest -coc over its
 *   pixels with coc < 0, or 0 when it has none. (Non-negative floats order like their bits: one unsigned max, reduced with cross-lane
 *   operations and one LDS step per workgroup; no device atomic.) Pack and tile maximum are one launch.
 * - 5. Neighbour maximum: n(tile) is the largest tile value over the 3 x 3 tiles around it that exist. One small launch.
 * - 6. Gather (per pixel X = (x, y)): r_X = |coc_X|; r_g = max(r_X, n(tile of X)). If r_g < 0.5 the result is C(X) with its own four
 *   words: NaN, infinities and alpha pass through. Otherwise let c(Y) be C(Y) with each of r, g, b as min(max(., 0), 65504).
 *   sum = c(X); wsum = 1. For k = 0 .. S - 1, in order: p = (x + 0.5 + T[k].x r_g, y + 0.5 + T[k].y r_g); Y = (floor p.x, floor p.y),
 *   each clamped to the image (in float, as min(max(floor p, 0), side - 1)); d = T[k].z r_g; r_Y = |coc_Y|; if Z_Y > Z_X then
 *   r_Y = min(r_Y, r_X), so that a blurred background does not bleed over a sharper foreground; q = clamp01((r_Y - d) + 0.5);
 *   w = q q (3 - 2 q); sum += c(Y) w per channel; wsum += w. The result is sum / wsum per channel, alpha 1. The gather radius is the
 *   pixel's own, widened only by the near field around it: a tap that is closer than X and has a larger radius than r_X is necessarily in
 *   front of the focal plane, and that is what n bounds (DESIGN.md "Depth of field").
 * - Known limits: this is the scatter-as-gather disk filter with nearest-texel taps. Nearest taps undersample large radii at small S (at
 *   R = 32 a disk holds 3,200 texels: S = 32 visits one in a hundred, which shows as noise on high-contrast bokeh); foreground bleed is
 *   not area-normalised (a near-field texel weighs the same whatever the area of its own disk, so a thin near object spreads brighter
 *   than a lens would spread it); Y clamps at the frame's edges, so the border repeats outwards.
 * - Tiles: the gather reads up to 32 pixels across tile edges, and the tile grid is the frame's, so a camera cannot have depth of field and
 *   a window (st_camera_set_window, st_dist_set_partition, st_dist_set_grid) at once: ST_ERR_INVALID_ARGUMENT from whichever setter comes
 *   second. For tiled frames rank 0 runs st_dof_process on the gathered colour and ST_AOV_DEPTH planes, in front of
 *   st_motion_blur_process, st_bloom_process and st_post_process.
 * - Errors: ST_ERR_INVALID_ARGUMENT for a wrong struct_size, unknown flag bits, a field outside its range (NaN included), focus_x or
 *   focus_y outside [0, 1] when ST_DOF_AUTOFOCUS is set (they are not looked at otherwise), null pointers where they are not allowed, a
 *   side of 0 or above 16384 in the process call, and an auto-exposure display or a non-perspective projection given to the process call.
 *   An unknown camera is ST_ERR_UNKNOWN_CAMERA. Set, get and plan are host work and valid on a host-only engine; st_dof_process returns
 *   ST_ERR_NO_DEVICE there. */
enum { ST_DOF_AUTOFOCUS = 1, ST_DOF_PLANAR_DEPTH = 2 };
typedef struct StDofDesc {                 /* 40 B */
    uint32_t struct_size;                  /* sizeof(StDofDesc) */
    uint32_t flags;                        /* ST_DOF_* */
    uint32_t samples;                      /* 4..64; 0 = default 32 */
    float focal_distance;                  /* metres along the optical axis, finite, > 0; Bevy's default is 10 */
    float aperture_f_stops;                /* N, finite, > 0; 0 = default 1 */
    float sensor_height;                   /* metres, finite, > 0; 0 = default 0.01866 (Super 35) */
    float max_radius;                      /* pixels, 0 < R <= 32; 0 = default 32 (Bevy's 64-pixel diameter) */
    float focus_x, focus_y;                /* ST_DOF_AUTOFOCUS: the focus point in [0, 1]^2 of the frame, (0, 0) the top left corner */
    uint32_t _pad;                         /* ignored */
} StDofDesc;
int st_camera_set_dof(StEngine* e, StHandle camera, const StDofDesc* desc);   /* NULL = off */
/* the last desc set (a zeroed desc with struct_size when none was) and whether depth of field is on; either pointer may be NULL */
int st_camera_get_dof(StEngine* e, StHandle camera, StDofDesc* out, int* enabled);
/* Pure host work, no engine: the sample count after its default, the tile counts of a width x height frame and the tap table (samples x
 * (x, y, rho); the rest of the 192 floats is 0). Any of the three outputs may be NULL. The desc is checked as in the setter; a side above
 * 16384 is ST_ERR_INVALID_ARGUMENT. */
int st_dof_plan(const StDofDesc* desc, uint32_t width, uint32_t height, uint32_t* samples, uint32_t tiles_xy[2], float taps_xyr[64 * 3]);
/* Stateless, like st_motion_blur_process. color: RGBA32F; depth: f32 (ST_AOV_DEPTH's layout, FLT_MAX on sky; with ST_DOF_PLANAR_DEPTH a
 * planar depth); projection: the 16 floats of the column-major perspective projection the planes were rendered with (host memory, read
 * during the call); display NULL = none, manual exposure only; dst in dst_format, width x height. Needs a device engine; no camera, no
 * tick. Enqueued on hip_stream without a host sync. The packed plane and the tile values are engine-owned: allocated (with a device sync)
 * only when a call needs larger ones than any before it, and calls on different streams are ordered by the engine. No input may overlap
 * dst. */
int st_dof_process(StEngine* e, const StDofDesc* desc, const StDisplayDesc* display, const float projection[16], const void* color_device,
                   const void* depth_device, uint32_t width, uint32_t height, void* dst_device, int dst_format /* StOutputFormat */,
                   void* hip_stream);

/* ---- fog (NEW seam): distance and height fog in front of depth of field (st_fog.cpp, k_fog.hip). In Bevy fog (FogSettings / DistanceFog)
 * is part of the PBR fragment shader, which this engine replaces, so it has to be served here: it needs the primary hit's distance and the
 * pixel's world-space ray. It is the first node of the output chain: scene-referred radiance along the primary ray, in front of the lens
 * (depth of field), the shutter (motion blur) and the glare (bloom). A participating medium seen from the camera only.
 * - Order: rendering -> fog -> (light shafts, below) -> depth of field -> motion blur -> bloom -> display transform -> FXAA -> resample ->
 *   output format.
 * - Scope: the setting belongs to the camera and takes effect at its next st_render_camera. It changes only what is written to
 *   `out_device`: AOVs, picks, scene queries, the HDR history, every plane st_camera_read_buffer returns and the auto-exposure metering are
 *   unchanged. desc == NULL turns it off: the frame then launches the kernels it launches without the setting, with the same arguments, and
 *   st_debug_last_launches is unchanged. The setting survives st_camera_update and st_engine_set_arithmetic. Frames that skip it, bit for
 *   bit the frames without the setting: ST_MODE_REFERENCE and ST_MODE_BVH_HEATMAP, which have no G-buffer, and a frame whose projection is
 *   not a perspective one (depth of field's test: projection[15] != 0, a [5] that is not positive and finite, a [0] that is 0 or not
 *   finite). While a frame is fogged, the composing launch writes the composed colour, untransformed, into a camera-owned render-size
 *   RGBA32F plane (and meters it); one launch (ST_PASS_POST) behind the composing launch writes the HDR plane of the next node that is on
 *   (depth of field's, else motion blur's, else bloom's), untransformed, or what the composing launch would have written, through the
 *   display transform and the output format.
 * - Windows: fog is pointwise, so unlike depth of field, motion blur and post-processing it works on a camera with a window
 *   (st_camera_set_window, st_dist_set_partition, st_dist_set_grid), in either order of the setters. Pixels keep their absolute
 *   coordinates and only the pixels inside the window are written; tiled frames keep the fog on the ranks' cameras and need no process call
 *   on rank 0.
 * - Arithmetic: float32, evaluated left to right as written, no fused multiply-add, division and square root correctly rounded, in BOTH
 *   builds; tests/fog_ref.py restates all of it in numpy and the kernel matches it bit for bit. min, max and clamp01 use the
 *   post-processing section's NaN rule (min(a, b) = a when a < b or b is NaN, else b; max likewise with >). The only transcendentals are
 *   exp2p and log2p below, in both builds (never the hardware's exponential and logarithm instructions):
 *   exp(x) = exp2p(x 1.44269504088896341); pow(s, p) = s == 0 ? 0 : exp2p(p log2p(s)).
 *   exp2p(x): NaN -> x; x > 127.999 -> +inf; x < -150 -> 0; px = floor(x); i = (int)px; x = x - px; if x > 0.5 then i = i + 1, x = x - 1;
 *   p = (((((1.535336188319500e-4 x + 1.339887440266574e-3) x + 9.618437357674640e-3) x + 5.550332471162809e-2) x
 *   + 2.402264791363012e-1) x + 6.931472028550421e-1) x + 1; the result is scale2(p, i), where scale2(z, n) = z 2^n in float with two
 *   multiplications when n leaves [-126, 127]: n > 127: z = z 2^127, n = min(n - 127, 127); n < -126: z = z 2^-126, n = max(n + 126, -126);
 *   then z 2^n.
 *   log2p(x), x > 0 finite: if x is subnormal, x = x 2^23 and e = -23, else e = 0; e = e + (biased exponent of x) - 126; m = the
 *   significand of x in [0.5, 1); if m < 0.707106781186547524 then e = e - 1, m = (m + m) - 1, else m = m - 1; z = m m;
 *   y = ((((((((7.0376836292e-2 m - 1.1514610310e-1) m + 1.1676998740e-1) m - 1.2420140846e-1) m + 1.4249322787e-1) m - 1.6668057665e-1) m
 *   + 2.0000714765e-1) m - 2.4999993993e-1) m + 3.3333331174e-1) m z; y = y - 0.5 z; r = y 0.44269504088896340736;
 *   r = r + m 0.44269504088896340736; r = r + y; r = r + m; r = r + (float)e.
 *   C is the composed HDR colour, D the distance along the pixel's ray, P the column-major projection, M the column-major camera transform
 *   (M[12..14] the camera position), b = height_falloff, a = color[3]. In a frame, D is PRIM_GBUFFER_D0.x of the frame's parity
 *   (ST_AOV_DEPTH's value), with 0 (sky) read as FLT_MAX, and P and M are the camera's; in st_fog_process they are the given ones.
 * - 0. Host constants, in double, each rounded to float once: L = light_direction normalised (each component converted to double, divided
 *   by the length); with ST_FOG_FOLLOW_SUN the engine's sun direction of the last st_tick (st_sun_update takes effect at the next tick).
 *   y0 = M[13]. E0 = exp(clamp(-b (y0 - height_reference), -80, 80)).
 * - 1. Ray (per pixel (x, y), absolute coordinates in the W x H frame): ndc_x = (x + 0.5) 2 / W - 1; ndc_y = -((y + 0.5) 2 / H - 1);
 *   ax = (ndc_x + P[8]) / P[0]; ay = (ndc_y + P[9]) / P[5]; c = 1 / sqrt((ax ax + ay ay) + 1), exactly as in depth of field's step 1.
 *   v = (ax c, ay c, -c). w = M.col0 v.x + M.col1 v.y + M.col2 v.z per component, left to right. w is not normalised again: a camera
 *   transform with scale scales the height term and the glow's cosine with it, which is the caller's business. dy = w.y.
 * - 2. Distance: if D is not > 0 (NaN included) the pixel passes through: it keeps its own four words, NaN, infinities and alpha. If
 *   D >= FLT_MAX (sky, +inf): without ST_FOG_SKY the pixel passes through, with it d = sky_distance. Otherwise d = D.
 * - 3. Height: if b = 0, d_e = d. Else k = min(max((b dy) d, -80), 80); G = |k| < 0.03125 ? 1 - k (0.5 - k 0.16666667)
 *   : (1 - exp(-k)) / k; d_e = min(d (E0 G), FLT_MAX). This is the closed-form optical depth, as an equivalent distance at the stated
 *   density, of a density that falls off as exp(-b (y - height_reference)). With the series switch at 1 / 32, G stays within 4e-6 relative
 *   of float64 over |k| <= 80.
 * - 4. Factors: LINEAR: g = clamp01((d_e - start) / (end - start)). EXPONENTIAL: g = 1 - exp(-(density d_e)). EXPONENTIAL_SQUARED:
 *   u = density d_e; g = 1 - exp(-(u u)). For these three ge = gi = g a, the same for every channel. ATMOSPHERIC, per channel:
 *   ge = (1 - exp(-(extinction d_e))) a; gi = (1 - exp(-(inscattering d_e))) a. If every ge and gi is 0, the pixel passes through.
 * - 5. Colour: s = min(max((w.x L.x + w.y L.y) + w.z L.z, 0), 1); F = min(color.rgb + light_color pow(s, light_exponent), FLT_MAX) per
 *   channel, or color.rgb when light_color is all 0 (the lobe is skipped). c' = min(max(C, 0), 65504) per channel.
 *   out = c' (1 - ge) + F gi per channel, alpha 1.
 * - Deviations from the first statement of this arithmetic, found ill-defined while building it: (1) s is also clamped to 1 from above: a
 *   transform with scale gives w L > 1, pow overflows to +inf and a zero channel of light_color times +inf is NaN; (2) F is held at
 *   FLT_MAX: color.rgb + light_color may overflow to +inf, and +inf times a zero gi (ATMOSPHERIC with one channel's inscattering 0) is NaN.
 *   With both, no finite input produces NaN (a non-finite entry of P or M is cleaned by the NaN rule of min and max: s = 0, k = -80).
 * - Known limits: the ray's origin is taken as the camera position M[12..14], while the renderer's rays start on the near plane, so D is
 *   short by the near distance along the ray; the auto-exposure metering stays in the composing launch, in front of the fog, so it meters
 *   the unfogged frame; the medium is seen from the camera only: it neither shadows the glow (shadowed in-scattering is the next node's, "light shafts") nor attenuates the light
 *   that reaches surfaces or GI paths.
 * - Errors: ST_ERR_INVALID_ARGUMENT for a wrong struct_size, an unknown falloff or flag bit, a field outside its stated range (NaN
 *   included; only the fields the falloff and the flags name are looked at: start and end with LINEAR, density with the two exponentials,
 *   extinction and inscattering with ATMOSPHERIC, sky_distance with ST_FOG_SKY, light_exponent and light_direction when light_color is
 *   not all 0, light_direction not with ST_FOG_FOLLOW_SUN; height_reference is finite; light_color is finite and >= 0), null pointers where
 *   they are not allowed, a side of 0 or above 16384, an auto-exposure display, ST_FOG_FOLLOW_SUN (a stateless call has no engine sun) or a
 *   non-perspective projection given to the process call. An unknown camera is ST_ERR_UNKNOWN_CAMERA. Set and get are host work and valid
 *   on a host-only engine; st_fog_process returns ST_ERR_NO_DEVICE there. */
enum StFogFalloff { ST_FOG_LINEAR = 0, ST_FOG_EXPONENTIAL = 1, ST_FOG_EXPONENTIAL_SQUARED = 2, ST_FOG_ATMOSPHERIC = 3 };
enum { ST_FOG_SKY = 1, ST_FOG_FOLLOW_SUN = 2 };
typedef struct StFogDesc {                 /* 112 B */
    uint32_t struct_size, falloff, flags, _pad;   /* sizeof(StFogDesc), StFogFalloff, ST_FOG_*, ignored */
    float color[4];                        /* linear rgb, finite, >= 0; a in [0, 1] = the most the fog may cover (Bevy's fog colour alpha) */
    float start, end;                      /* LINEAR: metres, finite, start < end */
    float density;                         /* EXPONENTIAL, EXPONENTIAL_SQUARED: per metre, finite, >= 0 */
    float height_falloff;                  /* b, per metre, finite, >= 0; 0 = density does not depend on height */
    float height_reference;                /* world y at which the density is the stated one */
    float sky_distance;                    /* ST_FOG_SKY: the distance sky pixels are fogged at, finite, > 0 */
    float extinction[3];                   /* ATMOSPHERIC: per metre and channel, finite, >= 0 */
    float inscattering[3];
    float light_color[3];                  /* the glow towards a directional light; all 0 = none */
    float light_exponent;                  /* finite, > 0 when light_color is not all 0; Bevy's default 8 */
    float light_direction[3];              /* towards the light, any non-zero length (normalised on the host in double); ignored with ST_FOG_FOLLOW_SUN */
    float _pad2;                           /* ignored */
} StFogDesc;
int st_camera_set_fog(StEngine* e, StHandle camera, const StFogDesc* desc);   /* NULL = off */
/* the last desc set (a zeroed desc with struct_size when none was) and whether fog is on; either pointer may be NULL */
int st_camera_get_fog(StEngine* e, StHandle camera, StFogDesc* out, int* enabled);
/* Stateless, like st_dof_process. color: RGBA32F; depth: f32 (ST_AOV_DEPTH's layout, FLT_MAX on sky); transform and projection: the 16
 * floats each of the column-major camera transform and perspective projection the planes were rendered with (host memory, read during the
 * call); display NULL = none, manual exposure only; dst in dst_format, width x height. Needs a device engine; no camera, no tick.
 * Enqueued on hip_stream without a host sync; the node needs no scratch memory, so nothing is allocated. ST_FOG_FOLLOW_SUN is refused. No
 * input may overlap dst. */
int st_fog_process(StEngine* e, const StFogDesc* desc, const StDisplayDesc* display, const float transform[16], const float projection[16],
                   const void* color_device, const void* depth_device, uint32_t width, uint32_t height, void* dst_device,
                   int dst_format /* StOutputFormat */, void* hip_stream);

/* ---- light shafts (NEW seam): shadowed single in-scattering marched through the BVH, between fog and depth of field (st_shafts.cpp,
 * k_shafts.hip). Fog attenuates what lies behind the medium; this node adds the light the medium scatters towards the camera in front of
 * the surface, with one shadow ray per sample and light, so occluders cut shafts into it. The caller names the lights by handle.
 * - Order: rendering -> fog -> light shafts -> depth of field -> motion blur -> bloom -> display transform -> FXAA -> resample -> format.
 * - Scope: as fog's. The setting belongs to the camera, takes effect at its next st_render_camera, survives st_camera_update and
 *   st_engine_set_arithmetic, and changes only what is written to `out_device` (and st_camera_ray_count, which grows by the march's shadow
 *   rays). desc == NULL turns it off: the frame then launches the kernels it launches without the setting, with the same arguments.
 *   Frames that skip it are fog's: ST_MODE_REFERENCE, ST_MODE_BVH_HEATMAP and non-perspective projections. While a frame carries shafts,
 *   the node in front (fog, else the composing launch) writes a camera-owned render-size RGBA32F plane; two launches (ST_PASS_POST) behind
 *   it, the march into a camera-owned cell plane and the apply launch, write the next node's plane or what the composing launch would have.
 * - Windows: the apply launch reads neighbouring cells, so the node is excluded together with a window exactly as depth of field is
 *   (st_camera_set_window, st_dist_set_partition, st_dist_set_grid refuse, as does the setter on a windowed camera). A tiled frame carries
 *   no shafts: st_light_shafts_process over the gathered planes needs the whole scene on rank 0, which is a limit.
 * - Lights: `lights[0 .. light_count)` are StHandles of st_light_insert. A handle that names no light in the light table of the last
 *   st_tick is skipped and is not an error (a light removed between frames drops out at the tick that removes it). The sun is not a
 *   table light here: sun_color (all 0 = no sun) arrives from direction L and is shadowed by a ray of unbounded length.
 * - Arithmetic: fog's discipline. This node's own arithmetic is float32, left to right, no fused multiply-add, division and square root
 *   correctly rounded, in BOTH builds; min, max, clamp01 with the post-processing section's NaN rule; exp(x) = exp2p(x 1.44269504088896341)
 *   with fog's exp2p; acos is glam's acos_approx: x = |v|; r = ((((((-0.0012624911 x + 0.0066700901) x - 0.0170881256) x + 0.0308918810) x
 *   - 0.0501743046) x + 0.0889789874) x - 0.2145988016) x + 1.5707963050; r = r sqrt(max(1 - x, 0)); v >= 0 ? r : 3.14159265358979 - r.
 *   tests/shafts_ref.py restates all of it in numpy and both builds match it bit for bit GIVEN the visibility bits. A visibility bit V of
 *   the StRay {origin, t_max, direction} is by definition 1 - (what st_scene_occluded answers for that ray), so alpha-tested materials
 *   and the t_max <= 0 / zero-direction contract behave as they do there; the fast build's walk is its own st_scene_occluded's.
 *   C, D, P, M as in fog. o = M[12..14].
 * - 0. Host constants, in double, each rounded to float once: g = anisotropy; k1 = (1 - g g) / (4 pi); k2 = 1 + g g; k3 = 2 g.
 *   L = sun_direction normalised as fog normalises its light direction; with ST_SHAFTS_FOLLOW_SUN the engine's sun direction of the last
 *   st_tick. st_light_shafts_plan returns the cell grid, ceil(W / divisor) x ceil(H / divisor), and the jitter table
 *   j[cy & 3][cx & 3] = (B + 0.5) / 16 with the 4 x 4 Bayer matrix B = {0 8 2 10 / 12 4 14 6 / 3 11 1 9 / 15 7 13 5}: frame-independent.
 * - 1. Cell (cx, cy): the pixels [cx divisor, (cx + 1) divisor) x [cy divisor, (cy + 1) divisor) inside the frame. Its depth d_c: over the
 *   block's pixels with D > 0 (sky counts, as FLT_MAX), the minimum where cx + cy is even and the maximum where it is odd (divisor 1: the
 *   pixel's D). A block without such a pixel is empty: the cell is (0, 0, 0, 0). Its ray goes through the block's nominal centre,
 *   (cx divisor + 0.5 divisor, cy divisor + 0.5 divisor) in pixels, with fog's step 1 (w is not renormalised).
 * - 2. March: d_end = min(d_c, max_distance); delta = d_end / steps; for k = 0 .. steps - 1: t = (k + j) delta; p = o + w t per component;
 *   A = 0; the sun, then the lights in the desc's order, add E phase to A where the sample sees them; m = (exp(-(density t)) delta) density;
 *   S = S + (m scatter) A per channel. phase(c) = k1 / (q sqrt(q)), q = k2 - k3 c, c = min(max((w.x l.x + w.y l.y) + w.z l.z, -1), 1).
 *   Sun: l = L, E = sun_color, ray {p, FLT_MAX, L}. Light: v = centre - p; l2 = (v.x v.x + v.y v.y) + v.z v.z; len = sqrt(l2); a sample
 *   with len not > radius contributes nothing; l = v / len; f_angle = 1 for a point light, else clamp01(1 - (r r) r) with
 *   r = acos(((n.x u.x + n.y u.y) + n.z u.z) / sqrt(n2 l2)) / angle, u = -v, n the light's octahedral direction decoded as the renderer
 *   decodes it but not normalised (the quotient takes the length out), n2 its squared length; f_dist = 1 for an infinite range, else
 *   (sm sm) / max(l2, 1e-4), sm = clamp01(1 - f f), f = l2 (1 / (range range)); fe = f_angle f_dist, times exp(-(density len)) with
 *   ST_SHAFTS_LIGHT_EXTINCTION; E phase = (colour fe) phase per channel; ray {p, len - radius, l}. No cosine and no BRDF: the medium
 *   is isotropic but for the phase function. NO SHADOW RAY IS CAST where E phase is 0 in all three channels (out of range, outside the
 *   cone, a black light, a sample inside the light): the ray count is part of this specification.
 *   The cell is (min(max(S, 0), FLT_MAX) per channel, d_c).
 * - 3. Apply, per pixel: a D that is not > 0 passes the pixel's own four words through. Divisor 1: S_p is the cell's S. Divisor 2:
 *   u = ((x + 0.5) 0.5 - 0.5, (y + 0.5) 0.5 - 0.5); the four cells around u, clamped to the grid, in the order (0,0) (1,0) (0,1) (1,1);
 *   d_p = min(D, max_distance); weight = bilinear (1 / (0.001 + |min(d_i, max_distance) - d_p| / d_p)); empty cells are skipped;
 *   S_p = (sum of weight S_i) / (sum of weights), or 0 when that sum is not > 0. If intensity S_p is 0 in all three channels the pixel
 *   passes through; otherwise out.rgb = min(min(max(C, 0), 65504) + intensity S_p, FLT_MAX) with the pixel's own alpha.
 * - Deviations from the first statement, found ill-defined while building it: (1) S is held in [0, FLT_MAX] when the cell is stored (an
 *   overflowed S times a zero weight is NaN; the NaN rule of max also cleans a NaN from lights of opposite signs); (2) d_p is clamped to
 *   max_distance like d_i, or a sky pixel would weigh every cell 0; (3) the arccosine is restated with the correctly rounded square root,
 *   because the renderer's own goes to the hardware's in the fast build. With these no finite input produces NaN.
 * - Known limits: single scattering in a homogeneous medium; the light reaching a sample is attenuated by the medium only with
 *   ST_SHAFTS_LIGHT_EXTINCTION and never for the sun; the ray's origin is M[12..14] as in fog; stratified samples with an ordered 4 x 4
 *   jitter and no temporal filter: banding shows below about 8 steps; tiled frames carry no shafts (above).
 * - Errors: ST_ERR_INVALID_ARGUMENT for a wrong struct_size, an unknown flag bit, a field outside its stated range (NaN included;
 *   sun_direction is looked at only when sun_color is not all 0 and ST_SHAFTS_FOLLOW_SUN is not set), null pointers where they are not
 *   allowed, a side of 0 or above 16384, an auto-exposure display or a non-perspective projection given to the process call, a window
 *   (above); st_light_shafts_process before the first st_tick. An unknown camera is ST_ERR_UNKNOWN_CAMERA. Set, get and plan are host
 *   work and valid on a host-only engine; st_light_shafts_process returns ST_ERR_NO_DEVICE there. */
enum { ST_SHAFTS_FOLLOW_SUN = 1, ST_SHAFTS_LIGHT_EXTINCTION = 2 };
enum { ST_SHAFTS_MAX_LIGHTS = 8 };
typedef struct StLightShaftsDesc {         /* 144 B */
    uint32_t struct_size, flags, steps, divisor;   /* sizeof(StLightShaftsDesc), ST_SHAFTS_*, 1..64 samples per ray, 1 or 2 pixels per cell side */
    float density;                         /* extinction per metre, finite, >= 0 */
    float anisotropy;                      /* Henyey-Greenstein g in [-0.95, 0.95]; 0 = isotropic, > 0 = forward */
    float max_distance;                    /* the march ends there, finite, > 0 */
    float intensity;                       /* finite, >= 0 */
    float scatter[3]; float _pad;          /* single-scattering albedo per channel in [0, 1]; ignored */
    float sun_color[3]; float _pad2;       /* finite, >= 0; all 0 = no sun; ignored */
    float sun_direction[3];                /* towards the sun, any non-zero length; ignored with ST_SHAFTS_FOLLOW_SUN */
    uint32_t light_count;                  /* <= 8 */
    StHandle lights[8];
} StLightShaftsDesc;
int st_camera_set_light_shafts(StEngine* e, StHandle camera, const StLightShaftsDesc* desc);   /* NULL = off */
/* the last desc set (a zeroed desc with struct_size when none was) and whether the node is on; either pointer may be NULL */
int st_camera_get_light_shafts(StEngine* e, StHandle camera, StLightShaftsDesc* out, int* enabled);
/* host only: the cell grid and the jitter table (row cy & 3, column cx & 3) of step 0; either pointer may be NULL */
int st_light_shafts_plan(const StLightShaftsDesc* desc, uint32_t width, uint32_t height, uint32_t cells_wh[2], float jitter[16]);
/* Like st_fog_process, but it reads the engine's live scene copy and light table: it needs a preceding st_tick, counts as a reader of
 * that copy as st_scene_occluded does, and takes ST_SHAFTS_FOLLOW_SUN. The cell plane is engine-owned scratch, grown, never shrunk. */
int st_light_shafts_process(StEngine* e, const StLightShaftsDesc* desc, const StDisplayDesc* display, const float transform[16],
                            const float projection[16], const void* color_device, const void* depth_device, uint32_t width, uint32_t height,
                            void* dst_device, int dst_format /* StOutputFormat */, void* hip_stream);

/* ---- colour grading (NEW seam): white balance, contrast, saturation, an ASC CDL, a 3-D look-up table and deband dither around the display
 * transform (st_grade.cpp, k_grade.hip, st_cube.h). What Bevy's tone-mapping node does around the operator itself: ColorGrading in front
 * of it, the LUT-based tone mappers (AgX, BlenderFilmic, TonyMcMapface: 3-D tables over a log2 shaper) in place of it, DebandDither behind
 * it. The sixth and last HDR node: it reads its render-size RGBA32F plane, grades the scene-referred colour (A), applies the camera's
 * display transform as the last node of the chain always does (B), grades the display-referred result (C) and writes the frame's target
 * in its format: `out`, or the post-processing plane in front of FXAA. One pointwise launch (ST_PASS_POST, profile slot "color_grading").
 * - Order: rendering -> fog -> light shafts -> depth of field -> motion blur -> bloom -> lens effects ("lens effects" below) -> colour
 *   grading (A, display transform, C) -> FXAA -> resample -> output format.
 * - Scope: as fog's. The setting belongs to the camera, takes effect at its next st_render_camera, survives st_camera_update and
 *   st_engine_set_arithmetic and changes only what is written to `out_device`: AOVs, picks, scene queries, st_camera_read_buffer, the HDR
 *   history and the auto-exposure metering (it meters the composed frame) are unchanged. desc == NULL turns it off: the frame then launches
 *   the kernels it launches without the setting, with the same arguments. ST_MODE_BVH_HEATMAP frames skip the node (false colour);
 *   ST_MODE_REFERENCE frames and non-perspective projections pass through it: nothing here depends on a G-buffer or on the projection.
 * - Windows and tiles: the node is pointwise in frame coordinates (dither takes the pixel's coordinates in the whole frame), so a camera
 *   with a window may grade, in either order of the setters, and gathered graded tiles are the grade of the gathered tiles bit for bit
 *   (the single engine's frame wherever the renderer's own taps do not cross a tile border). When rank 0 blooms the gathered
 *   frame instead (bloom excludes windows), the ranks render without a display and without grading and rank 0 calls
 *   st_color_grading_process behind st_bloom_process: bloom without a display into an RGBA32F plane, then grading with the display.
 * - Look-up tables: st_lut_insert keeps a table of side N (2..65), N^3 rgb triples, red fastest as in a .cube file; the next st_tick copies
 *   it to the device on its stream without a host sync, one float4 per texel so that a corner is one 16-B load. A descriptor names a table
 *   by handle; a handle that names no live table (0, never inserted, removed, or inserted after the last st_tick) skips the LUT step and is
 *   not an error. Inserting over a live id replaces the table at the next tick. A table removed or replaced while frames that read it are in
 *   flight stays alive until they have drained (a fence, no host sync in st_render_camera).
 * - Arithmetic: everything is float32, evaluated left to right as written, no fused multiply-add, division correctly rounded, in BOTH
 *   builds; tests/grade_ref.py restates all of it in numpy (grade_f32) and the kernel matches it bit for bit. min, max and clamp01 are the
 *   post-processing section's (NaN rule), Y(r, g, b) = 0.2126 r + 0.7152 g + 0.0722 b is the display section's luminance,
 *   pw(x, p) = x == 0 ? 0 : exp2p(p log2p(x)) for x >= 0 and lg(x) = log2p(x) with fog's two polynomials (never the hardware's exponential
 *   and logarithm instructions). A step whose parameters are neutral is skipped and leaves the value's bits untouched: a descriptor that is
 *   neutral everywhere is on but writes exactly what off writes. Alpha is written as 1 by every step that runs. c is the node's texel.
 * - A. Scene-referred; runs only when one of its three steps is active, each of which is skipped on its own when neutral.
 *   v = min(max(c, 0), 65504) per channel (NaN becomes 0).
 *   White balance (temperature or tint != 0): v = M v, each row summed left to right, then max(., 0). The host computes M in double and
 *   rounds it once: M = LMS2LIN diag(k) LIN2LMS (the two products formed in that order), k = w1 / w2 per component,
 *   w1 = (0.949237, 1.03542, 1.08728), w2 the CAT02 LMS of the CIE xy point x = 0.31271 - t (t < 0 ? 0.1 : 0.05),
 *   y = 2.87 x - 3 x^2 - 0.27509507 + 0.05 u with t = temperature, u = tint: with Y = 1, X = x / y, Z = (1 - x - y) / y,
 *   L = 0.7328 X + 0.4296 Y - 0.1624 Z, M = -0.7036 X + 1.6975 Y + 0.0061 Z, S = 0.0030 X + 0.0136 Y + 0.9834 Z.
 *   LIN2LMS = {0.390405 0.549941 0.00892632 / 0.0708416 0.963172 0.00135775 / 0.0231082 0.128021 0.936245},
 *   LMS2LIN = {2.85847 -1.62879 -0.0248910 / -0.210182 1.15820 0.000324281 / -0.0418120 -0.118169 1.06867} (Unity's and Bevy's).
 *   Contrast (!= 1), about mid-grey: v = 0.18 pw(v / 0.18, contrast).
 *   Saturation (!= 1): y = Y(v); v = max(y + (v - y) saturation, 0).
 *   Stage A ends with min(v, 65504).
 * - B. Display transform: the camera's operator and its manual or metered scale, exactly the transform every node's last store applies
 *   (alpha 1). Without a display the colour passes as it is.
 * - C. Display-referred.
 *   CDL (skipped when slope = 1, offset = 0, power = 1 in all channels and cdl_saturation = 1): per channel v = max(v slope + offset, 0);
 *   v = pw(v, power) in the channels whose power != 1; then, when cdl_saturation != 1, y = Y(v); v = max(y + (v - y) cdl_saturation, 0).
 *   LUT (a handle that names a live table of side N): per channel u = clamp01(v) in ST_LUT_DOMAIN_UNIT (NaN becomes 0); in
 *   ST_LUT_DOMAIN_LOG2 u = v > 0 ? clamp01((lg(v) - lut_ev_min) inv_range) : 0 with inv_range = 1 / (lut_ev_max - lut_ev_min) computed in
 *   double and rounded once. p = u float(N - 1); i = min(int(floor(p)), N - 2); f = p - float(i). Texel (ir, ig, ib) lies at index
 *   (ib N + ig) N + ir. The interpolation is tetrahedral: the three axes ordered by descending f, ties in the order r, g, b, give a, b, c;
 *   t0 is the cell's low corner, t1 = t0 stepped along a, t2 = t1 stepped along b, t3 the high corner;
 *   L = ((t0 (1 - fa) + t1 (fa - fb)) + t2 (fb - fc)) + t3 fc per channel. The result is L when lut_strength == 1, else
 *   v + (L - v) lut_strength.
 *   Dither (ST_GRADE_DITHER; Bevy's screen_space_dither): (x, y) the pixel's coordinates in the whole frame; n = 171 x + 231 y in integers
 *   (exact in float up to 16384^2); d = float(n); for channel k with q = (103, 71, 97): t = d / q; t = t - floor(t);
 *   delta = (t - 0.5) / 255; v = pw(max(pw(max(v, 0), g1) + delta, 0), 2.2f) with g1 the float nearest 1 / 2.2.
 *   Then the target's format.
 * - Reading of the first statement where it left a choice: (1) the CDL's power is looked at per channel, so a channel whose power is 1
 *   keeps the bits of max(v slope + offset, 0); (2) i is also held at 0 from below, which changes no value (u is in [0, 1]) and keeps a
 *   corner load inside the table whatever the arithmetic in front of it does; (3) st_lut_insert after the last st_tick is "no live table"
 *   for the frames until the next one, like every other scene edit.
 * - Known limits: the LOG2 domain takes lut_strength 1 only (a blend of display-referred L with the scene-referred v has no meaning);
 *   with ST_TONEMAP_NONE and no stage A an exposed value may overflow to +inf before stage C, and a half-strength LUT then gives NaN;
 *   dither is sized for 8-bit targets (1 / 255) whatever the format; no 1-D or shaper LUT other than log2; no table data ships.
 * - Errors: ST_ERR_INVALID_ARGUMENT for a wrong struct_size, unknown flags or an unknown domain, any non-finite field, temperature or tint
 *   outside [-1, 1], contrast outside (0, 4], saturation or cdl_saturation outside [0, 4], a slope outside [0, 16], an offset outside
 *   [-1, 1], a power outside (0, 8], lut_strength outside [0, 1], in the LOG2 domain lut_ev_min >= lut_ev_max or lut_strength != 1, null
 *   pointers where they are not allowed, image sides outside 1..16384, a LUT side outside 2..65 or a non-finite LUT value, an
 *   auto-exposure display given to the process call. An unknown camera is ST_ERR_UNKNOWN_CAMERA. Set, get, plan, st_lut_insert and
 *   st_lut_remove are host work and valid on a host-only engine; st_color_grading_process returns ST_ERR_NO_DEVICE there. */
enum { ST_GRADE_DITHER = 1 };
enum StLutDomain { ST_LUT_DOMAIN_UNIT = 0, ST_LUT_DOMAIN_LOG2 = 1 };
enum { ST_GRADE_STEP_WHITE_BALANCE = 1, ST_GRADE_STEP_CONTRAST = 2, ST_GRADE_STEP_SATURATION = 4, ST_GRADE_STEP_CDL = 8, ST_GRADE_STEP_LUT = 16,
       ST_GRADE_STEP_DITHER = 32 };
typedef struct StColorGradingDesc {        /* 96 B */
    uint32_t struct_size, flags;           /* sizeof(StColorGradingDesc), ST_GRADE_* */
    float temperature, tint;               /* [-1, 1]; 0 = neutral (Bevy's ColorGrading / Unity's white balance, divided by 100) */
    float contrast, saturation;            /* (0, 4] and [0, 4]; 1 = neutral; scene-referred */
    float slope[3], offset[3], power[3];   /* ASC CDL, display-referred: [0, 16], [-1, 1], (0, 8]; 1, 0, 1 = neutral */
    float cdl_saturation;                  /* [0, 4]; 1 = neutral */
    StHandle lut;                          /* of st_lut_insert; 0 = none */
    uint32_t lut_domain;                   /* StLutDomain */
    float lut_ev_min, lut_ev_max;          /* LOG2: the table spans log2(v) in [lut_ev_min, lut_ev_max], finite, min < max */
    float lut_strength;                    /* [0, 1]; LOG2: 1 */
    uint32_t _pad[2];                      /* ignored */
} StColorGradingDesc;
typedef struct StColorGradingPlan {        /* 48 B */
    uint32_t steps;                        /* ST_GRADE_STEP_*: the steps a frame with this descriptor runs (LUT: the handle is not 0) */
    float white_balance[9];                /* M, row major; the identity when the step is not active */
    float lut_inv_range;                   /* 1 / (lut_ev_max - lut_ev_min) in the LOG2 domain, else 0 */
    uint32_t _pad;
} StColorGradingPlan;
int st_camera_set_color_grading(StEngine* e, StHandle camera, const StColorGradingDesc* desc);   /* NULL = off */
/* the last desc set (a zeroed desc with struct_size when none was) and whether the node is on; either pointer may be NULL */
int st_camera_get_color_grading(StEngine* e, StHandle camera, StColorGradingDesc* out, int* enabled);
/* rgb: size^3 x 3 floats in host memory, red fastest, copied during the call; size in 2..65; every value finite */
int st_lut_insert(StEngine* e, StHandle id, uint32_t size, const float* rgb);
int st_lut_remove(StEngine* e, StHandle id);   /* an id that names no table is not an error */
/* host only: the host constants of a descriptor */
int st_color_grading_plan(const StColorGradingDesc* desc, StColorGradingPlan* out);
/* Stateless, like st_bloom_process: the same launch over any RGBA32F device plane. lut_rgba_device: lut_size^3 float4 (rgb, anything) in
 * device memory, red fastest, or NULL for no LUT step; the desc's handle is not consulted. display NULL = none, manual exposure only.
 * Needs a device engine; no camera, no tick, no scratch memory. Enqueued on hip_stream without a host sync. src may not overlap dst. */
int st_color_grading_process(StEngine* e, const StColorGradingDesc* desc, const StDisplayDesc* display, const void* lut_rgba_device,
                             uint32_t lut_size, const void* src_rgba32f_device, uint32_t width, uint32_t height, void* dst_device,
                             int dst_format /* StOutputFormat */, void* hip_stream);
/* A .cube file's 3-D table, shaped like st_decode_hdr: out_rgb NULL reports lut_size only; else lut_size^3 x 3 floats, red fastest. Reads
 * TITLE, # comments, blank lines, LUT_3D_SIZE N, DOMAIN_MIN 0 0 0 / DOMAIN_MAX 1 1 1, then exactly N^3 rows of three numbers; CR LF and
 * tabs are fine. ST_ERR_UNSUPPORTED: LUT_1D_SIZE, any other domain, an unknown keyword. ST_ERR_PARSE: too few or too many rows, a
 * non-number, a non-finite value, a size outside 2..65. Own code (st_cube.h); no engine needed. */
int st_decode_cube(const void* bytes, size_t size, float* out_rgb, size_t capacity_floats, uint32_t* lut_size);

/* ---- lens effects (NEW seam): radial distortion, chromatic fringing, vignette and film grain between bloom and colour grading
 * (st_lens.cpp, k_lens.hip). What Unity's and Unreal's stacks do in the pass between bloom and grading, and Bevy's ChromaticAberration: the
 * seventh HDR node. It reads its render-size RGBA32F plane and writes the plane colour grading reads, else the frame's target in its format
 * through the display transform: `out`, or the post-processing plane in front of FXAA. One launch (ST_PASS_POST, profile slot "lens"):
 * a gather of up to 16 bilinear look-ups per pixel with the distortion or the fringe step, a pointwise pass without them.
 * - Order: rendering -> fog -> light shafts -> depth of field -> motion blur -> bloom -> lens effects -> colour grading (A, display
 *   transform, C) -> FXAA -> resample / upscale -> output format. The lens sees the glow bloom added (a real lens bends the bloomed
 *   image) and grading sees the lens's result (grain is scene-referred and is graded like the light it rides on).
 * - Scope: as fog's and grading's. The setting belongs to the camera, takes effect at its next st_render_camera, survives st_camera_update
 *   and st_engine_set_arithmetic and changes only what is written to `out_device`: AOVs, picks, scene queries, st_camera_read_buffer, the
 *   HDR history and the auto-exposure metering (it meters the composed frame) are unchanged. desc == NULL turns it off: the frame then
 *   launches the kernels it launches without the setting, with the same arguments. A descriptor that is neutral in every step is on, but
 *   writes what off writes: a skipped step leaves the bits alone. ST_MODE_BVH_HEATMAP frames skip the node (false colour);
 *   ST_MODE_REFERENCE frames and non-perspective projections pass through it: it needs neither a G-buffer nor a projection.
 * - Windows and tiles: distortion and fringing read far across tile edges, so a camera cannot have lens effects (any desc) and a window
 *   (st_camera_set_window / st_camera_set_rows, st_dist_set_partition, st_dist_set_grid) at once: ST_ERR_INVALID_ARGUMENT from whichever
 *   setter comes second. For tiled frames the ranks render without it, st_dist_gather assembles the frame on rank 0, and rank 0 runs
 *   st_lens_process on the gathered plane (behind st_bloom_process, in front of st_color_grading_process). It needs the colour plane only.
 * - Arithmetic: everything is float32, evaluated left to right as written, no fused multiply-add, division correctly rounded, in BOTH
 *   builds; there is no transcendental. tests/lens_ref.py restates all of it in numpy (lens_f32) and the kernel matches it bit for bit.
 *   min, max and clamp01 are the post-processing section's (NaN rule), BILINEAR is that section's look-up (indices clamped to the image, an
 *   axis with f == 0 takes texel a itself), colour(c) = min(max(c, 0), 65504) per channel (NaN becomes 0).
 * - Host constants (st_lens_plan; in double from the float fields, each rounded to float once): cx = W / 2, cy = H / 2,
 *   inv_hd2 = 1 / (cx^2 + cy^2). Tap table: without the fringe step one tap, tap_scale 1, weights (1, 1, 1). With it n = fringe_taps,
 *   t_i = i / (n - 1), tap_scale[i] = 1 + fringe (2 t_i - 1); the spectral tents wR = max(1 - 2 t, 0), wG = 1 - |2 t - 1|,
 *   wB = max(2 t - 1, 0), each divided by its sum over the taps (summed in index order): n = 3 gives the classic three single-channel
 *   taps, and a constant image stays constant within the weights' rounding. fit = 1 without ST_LENS_FIT. With it, over the centres of
 *   the frame's border pixels and both axes, fit = min of cx / (|u| f(r2) scale T) for u != 0 and cy / (|v| f(r2) scale T) for v != 0,
 *   with u, v, r2, f as below evaluated in double and T the largest tap_scale (as rounded): the largest factor at which no tap of any
 *   output pixel has its source position outside [0, W] x [0, H]; the bound on k1, k2 makes |u| f(r2) grow with |u| along a row, so the
 *   border binds. An axis with offset 0 constrains nothing: a 1 x 1 frame has fit 1. scale_eff = scale fit. steps = the steps whose
 *   parameters are not neutral: distortion (k1 != 0 or k2 != 0 or scale_eff != 1), fringe (fringe != 0), vignette (vignette_intensity
 *   != 0), grain (grain_intensity != 0).
 * - Per output pixel (x, y), absolute coordinates: u = (x + 0.5) - cx, v = (y + 0.5) - cy (both exact in float);
 *   r2 = (u u + v v) inv_hd2 (1 at the frame's corner); f = (k2 r2 + k1) r2 + 1; g = f scale_eff, and g = 1 without the distortion step.
 * - Taps (distortion or fringe step): tap i reads BILINEAR of colour(texel) at the continuous position (u s + cx, v s + cy) with
 *   s = g tap_scale[i]. Each channel's sum starts at 0 and runs over the taps in index order, sum = sum + tap weight; taps whose three
 *   weights are all 0 are skipped. With g = 1 and tap_scale 1 the position is (x + 0.5, y + 0.5) exactly, both fractions are 0 and the
 *   tap is colour(the pixel's own texel). With neither step the pixel takes its own texel, and keeps its four words, alpha and NaN
 *   included, unless a later step runs; a later step starts from colour(texel).
 * - Vignette, at the output pixel: m = r2 with ST_LENS_VIGNETTE_ROUND, else m = ((u / cx) (u / cx) + (v / cy) (v / cy)) 0.5, an ellipse
 *   that follows the frame (both are 1 at the corner). q = 1 + m vignette_falloff; fall = 1 / (q q) (the cos^4 law with
 *   tan^2 theta = m vignette_falloff); colour = colour ((1 - a) + a fall) per channel, a = vignette_intensity.
 * - Grain, multiplicative in scene-referred light (photographic noise is relative to exposure): the cell is (x / grain_size,
 *   y / grain_size) in integers; s = grain_seed, plus the camera's frame counter (the one the pass seeds take; st_debug_world's
 *   next_frame - 1 behind a tick) under ST_LENS_GRAIN_ANIMATE, modulo 2^32; h = pcg(cell_x + pcg(cell_y + s)) in 32-bit unsigned
 *   arithmetic with one PCG round pcg(v): v = v 747796405 + 2891336453; w = ((v >> ((v >> 28) + 4)) ^ v) 277803737; (w >> 22) ^ w.
 *   eta = ((float(h & 0xffff) + float(h >> 16)) - 65535) / 65536: triangular in (-1, 1), exact. colour = colour (1 + grain_intensity eta).
 * - Finish: alpha is 1 when any step ran. The colour is held at min(., 65504) and stored: the raw plane when grading follows, else the
 *   frame's target through the display transform.
 * - Deviations from the first statement, where building it showed a choice: (1) fit is rounded towards zero, not to nearest, so its own
 *   rounding cannot push a tap out of the frame, and scale_eff is rounded from scale times that float; (2) the grain's hash nests two PCG
 *   rounds, one per cell coordinate: one round over a linear mix of the two leaves visible diagonals; (3) BILINEAR's f == 0 rule needs
 *   no branch here: every texel is clamped to a finite colour first, so a + (b - a) 0 is a itself; (4) a tap position just outside the
 *   frame by float rounding of u s + cx reads the clamped border texel: harmless, and the plan's fit is stated for exact arithmetic.
 * - Known limits: picks and AOVs stay in undistorted render-size pixel coordinates; there is no prefilter where distortion minifies
 *   (scale_eff f > 1 undersamples and may alias); fringing is radial only (no lateral / axial split, no per-channel distortion
 *   coefficients); grain is white per cell (no spatial correlation beyond grain_size, the same value in all three channels).
 * - Errors: ST_ERR_INVALID_ARGUMENT for a wrong struct_size, unknown flags, k1 or k2 not finite or 3 |k1| + 5 |k2| > 0.95, scale outside
 *   [0.25, 4], fringe outside [0, 0.1], fringe_taps outside 3..16 when fringe != 0, vignette_intensity outside [0, 1], vignette_falloff
 *   not finite or <= 0 when the intensity is not 0, grain_intensity outside [0, 1), grain_size outside 1..8 when the intensity is not 0
 *   (NaN is outside every range), null pointers where they are not allowed, image sides outside 1..16384, and for st_lens_process
 *   ST_LENS_GRAIN_ANIMATE (a stateless call has no frame counter) and an auto-exposure display. An unknown camera is
 *   ST_ERR_UNKNOWN_CAMERA. Set, get and plan are host work and valid on a host-only engine; st_lens_process returns ST_ERR_NO_DEVICE there. */
enum { ST_LENS_FIT = 1, ST_LENS_VIGNETTE_ROUND = 2, ST_LENS_GRAIN_ANIMATE = 4 };
enum { ST_LENS_STEP_DISTORTION = 1, ST_LENS_STEP_FRINGE = 2, ST_LENS_STEP_VIGNETTE = 4, ST_LENS_STEP_GRAIN = 8 };
enum { ST_LENS_MAX_TAPS = 16 };
typedef struct StLensDesc {                /* 48 B: twelve 4-B words, a multiple of 8 B without a pad */
    uint32_t struct_size, flags;           /* sizeof(StLensDesc), ST_LENS_* */
    float k1, k2;                          /* radial distortion; 0, 0 = none; finite, 3 |k1| + 5 |k2| <= 0.95 (keeps r f(r^2) increasing: no fold-over) */
    float scale;                           /* source zoom, in [0.25, 4]; 1 = none; with ST_LENS_FIT multiplied by the plan's fit */
    float fringe;                          /* [0, 0.1]; 0 = none: relative radial spread between the red and the blue end */
    uint32_t fringe_taps;                  /* 3..16 when fringe != 0, else ignored */
    float vignette_intensity;              /* [0, 1]; 0 = none */
    float vignette_falloff;                /* finite, > 0 when the intensity is not 0 */
    float grain_intensity;                 /* [0, 1); 0 = none */
    uint32_t grain_size;                   /* 1..8 pixels per grain cell when the intensity is not 0 */
    uint32_t grain_seed;
} StLensDesc;
typedef struct StLensPlan {                /* 284 B; host constants, each computed in double and rounded once */
    uint32_t steps, taps;                  /* ST_LENS_STEP_*; taps = 1 without the fringe step */
    float cx, cy, inv_hd2;                 /* W / 2, H / 2, 1 / (cx^2 + cy^2) */
    float fit, scale_eff;                  /* fit = 1 without ST_LENS_FIT */
    float tap_scale[16];                   /* [ST_LENS_MAX_TAPS]; entries past `taps` are 0 */
    float tap_weight[16][3];               /* r, g, b */
} StLensPlan;
int st_camera_set_lens(StEngine* e, StHandle camera, const StLensDesc* desc);   /* NULL = off */
/* the last desc set (a zeroed desc with struct_size when none was) and whether the node is on; either pointer may be NULL */
int st_camera_get_lens(StEngine* e, StHandle camera, StLensDesc* out, int* enabled);
/* host only, no engine: the host constants of a descriptor for a width x height frame; out may be NULL (the checks alone) */
int st_lens_plan(const StLensDesc* desc, uint32_t width, uint32_t height, StLensPlan* out);
/* Stateless, like st_bloom_process: the same launch over any RGBA32F device plane. display NULL = none, manual exposure only. Needs a
 * device engine; no camera, no tick, no scratch memory. Enqueued on hip_stream without a host sync. src may not overlap dst. */
int st_lens_process(StEngine* e, const StLensDesc* desc, const StDisplayDesc* display, const void* src_rgba32f_device, uint32_t width,
                    uint32_t height, void* dst_device, int dst_format /* StOutputFormat */, void* hip_stream);
/* measurement and tests: force != 0 sends descriptors without the distortion and the fringe step through the gather instantiation (one
 * tap at the pixel's own centre) instead of the pointwise one; steps that run give the same bits either way */
int st_debug_set_lens_gather(StEngine* e, int force);

/* ---- multi-GPU behind the boundary (NEW seam; SURVEY.md section 8e, BASELINE.json configs 4 and 5). One process per GPU, one
 * engine per process, the scene replicated; the frame is cut into tiles, every rank renders its tile (+ an apron of redundant
 * pixels in Image mode, whose passes read neighbours) with absolute pixel coordinates, and the ONE collective of the path
 * gathers the composed tiles to rank 0: grouped ncclSend / ncclRecv over RCCL — one point-to-point message per xGMI link into
 * the root, not a ring — on a communication stream the engine owns, ordered behind the frame by an event and overlapped with
 * the next frame. librccl is opened at run time (a process that already loaded it, e.g. through torch, shares that copy). */
typedef struct StDistRect { uint32_t x0, y0, x1, y1; } StDistRect;          /* [x0, x1) x [y0, y1) in pixels */
typedef struct StDistUniqueId { char internal[128]; } StDistUniqueId;      /* ncclUniqueId */
/* The partition rule (a pure function; `e` is not needed): `world` tiles in a grid of `cols` columns (0: the default grid — 1x1,
 * two row bands, 2x2, 3x2, 4x2, ... columns >= rows; a prime world gives row bands) whose edges sit on multiples of 16 pixels in
 * x and 8 in y; rank r owns tile (r % cols, r / cols). */
int st_dist_partition(uint32_t width, uint32_t height, uint32_t world, uint32_t cols, uint32_t rank, StDistRect* owned);
/* `owned` widened by `apron` pixels on every side that has a neighbour, outward to the same 16 / 8 grid: what a rank renders. */
int st_dist_window(uint32_t width, uint32_t height, const StDistRect* owned, uint32_t apron, StDistRect* window);
/* Cost-weighted tiles (round 5). The equal split gives BASELINE config 5's eight tiles unequal work (one GPU rendering each tile window in
 * turn: max / mean 1.10, profiles/r05_tile_balance.json), so a grid's row edges and — per row — its column edges can be moved. A StDistGrid is
 * plain data that every rank holds identically: rank r owns column r % cols of row r / cols. st_dist_grid: the equal split (the tiles
 * st_dist_partition returns). st_dist_grid_rebalance: from the current grid and ONE cost per tile in rank order (a rank's frame time: the host
 * gathers them its own way), the grid whose rows — then each row's tiles — would cost the same if a tile's cost were spread evenly over its
 * pixels; edges stay on the 16 x 8 pixel grid, tiles stay at least 64 x 32 pixels, and with max_step != 0 no edge moves further than that per
 * call (max_step <= apron: every pixel a rank newly owns was already rendered by it, as apron, so its history is warm). The tiles of a valid
 * grid are disjoint and cover the frame. st_dist_set_grid: like st_dist_set_partition, with the grid's tiles; every rank must set the same
 * grid between the same two frames (the root sizes its receives from it). */
#define ST_DIST_MAX_SIDE 16
typedef struct StDistGrid {
    uint32_t cols, rows;
    uint32_t row_edge[ST_DIST_MAX_SIDE + 1];                    /* rows + 1 values, 0 ... height, multiples of 8 */
    uint32_t col_edge[ST_DIST_MAX_SIDE][ST_DIST_MAX_SIDE + 1];  /* per row: cols + 1 values, 0 ... width, multiples of 16 */
} StDistGrid;
int st_dist_grid(uint32_t width, uint32_t height, uint32_t world, uint32_t cols, StDistGrid* out);
int st_dist_grid_tile(const StDistGrid* grid, uint32_t rank, StDistRect* owned);
int st_dist_grid_rebalance(uint32_t width, uint32_t height, const StDistGrid* current, const float* tile_cost, uint32_t max_step, StDistGrid* out);
/* RCCL transport: rank 0 makes an id (ncclGetUniqueId) and hands it to the other processes by its own means (the Rust host: a
 * pipe or MPI; bench.py: torch.distributed's store); every rank then joins with st_dist_init on its engine's device. */
int st_dist_unique_id(StDistUniqueId* out);
int st_dist_init(StEngine* e, int rank, int world, const StDistUniqueId* id);
/* In-process transport (tests; a single-GPU box): the engines of one process that share `group` exchange tiles through a
 * mailbox — same partition, pack / unpack and stream ordering, no RCCL. Works on host-only engines too (host frames). Within a
 * frame the non-root ranks call st_dist_gather before rank 0 does. */
int st_dist_init_local(StEngine* e, int rank, int world, uint64_t group);
int st_dist_shutdown(StEngine* e);
int st_dist_rank(StEngine* e, int* rank, int* world);
/* Sets the camera's window (st_camera_set_window) to this rank's tile + apron; reports both rectangles (either may be NULL). */
int st_dist_set_partition(StEngine* e, StHandle camera, uint32_t cols, uint32_t apron, StDistRect* owned, StDistRect* window);
int st_dist_set_grid(StEngine* e, StHandle camera, const StDistGrid* grid, uint32_t apron, StDistRect* owned, StDistRect* window);
/* `frame`: the buffer st_render_camera just composed into on `hip_stream` (full-frame sized, the camera's output format; this
 * rank's tile of it is what travels). `full_on_root`: where rank 0 assembles the frame (may be `frame` itself: its own tile is
 * then already in place); ignored on other ranks. Returns at once; the caller alternates two frame buffers so that frame N is
 * gathered while frame N+1 renders; st_render_camera into a buffer whose gather is still in flight is ordered behind that gather by the
 * engine. st_dist_wait orders `hip_stream` behind the gather that read `frame` (NULL: every gather in flight); host_wait != 0 blocks
 * the caller instead. st_dist_gather_ms: duration of the camera's last gather on the communication stream (blocks until it is through). */
int st_dist_gather(StEngine* e, StHandle camera, const void* frame, void* full_on_root, void* hip_stream);
int st_dist_wait(StEngine* e, StHandle camera, const void* frame, void* hip_stream, int host_wait);
int st_dist_gather_ms(StEngine* e, StHandle camera, float* ms);

/* camera.rs:170-175 `viewport.format`: the reference renders into a texture view of that format and the hardware converts
 * on store; here the composition kernel does. RGBA32F (default, 16 B/pixel), RGBA16F (8 B, round to nearest even),
 * RGBA8 / BGRA8 sRGB (4 B: clamp, IEC 61966-2-1 encode, round to nearest; alpha 255). The buffer handed to
 * st_render_camera must hold width x height pixels of the chosen format. */
enum StOutputFormat { ST_FORMAT_RGBA32F = 0, ST_FORMAT_RGBA16F = 1, ST_FORMAT_RGBA8_UNORM_SRGB = 2, ST_FORMAT_BGRA8_UNORM_SRGB = 3 };
int st_camera_set_output_format(StEngine* e, StHandle camera, int format);

/* ---- scheduling / tuning switches of one engine (NEW seam). Every field selects another launch structure or host policy for
 * the SAME pass graph: in the exact build every combination renders the same bits (tests/test_gpu_parity.py runs several
 * against the oracle). Defaults are what bench.py times. Get, change, set — between frames; `struct_size` must be
 * sizeof(StTuning). Environment variables (read once, when the engine is created) override the defaults:
 *   ST_NO_OVERLAP ST_NO_FUSE ST_NO_FUSE_DI_HEAD ST_NO_FUSE_SPATIAL ST_NO_FUSE_GI_SAMPLING ST_NO_FUSE_GI_VALIDATION
 *   ST_NO_FUSE_GI_REPROJECTION ST_NO_FUSE_WAVELET ST_NO_FUSE_COMPOSE ST_NO_PREVIEW_BOTH ST_NO_VARIANCE_IN_REPROJECT
 *   ST_KEEP_ALL_PLANES ST_KEEP_SCRATCH ST_NO_GI_ALIAS ST_NO_STAGING ST_NO_DOUBLE_BUFFER ST_NO_PACKED_BASE
 *   ST_NO_ANYHIT_FAST ST_NO_COMPACT_BVH (=1 clears the field), ST_ALLOW_DEEP_BVH ST_DI_HEAD_ON_MAIN ST_TILE_MAP ST_TILE_MAP_DENOISE ST_SIDE_PRIORITY
 *   ST_TICK_TIMING ST_DEVICE_BAKE ST_SIDE_START (= value). */
typedef struct StTuning {
    uint32_t struct_size;
    uint32_t overlap;               /* 1: two HIP streams per camera, software-pipelined across frames */
    uint32_t fuse;                  /* 1: own-pixel consumer passes ride in their producer's launch (0: one launch per reference pass) */
    uint32_t fuse_di_head;          /* DI sampling + temporal resampling in one launch */
    uint32_t fuse_spatial;          /* DI / GI spatial resampling: pick + trace + sample per 2x1 cell in one launch */
    uint32_t fuse_gi_sampling;      /* GI sampling passes a + b in one launch */
    uint32_t fuse_gi_validation;    /* validation frames: gi_reprojection done by its two readers */
    uint32_t fuse_gi_reprojection;  /* tracing frames: gi_reprojection inside gi_temporal */
    uint32_t fuse_wavelet;          /* a-trous strides 1 and 2 as one launch */
    uint32_t fuse_compose;          /* fast build: frame composition inside the last a-trous pass */
    uint32_t preview_both;          /* both GI preview passes + resolving in one launch, flagged pixels served afterwards */
    uint32_t variance_in_reproject; /* estimate_variance's long-history branch inside the reproject stages */
    uint32_t lean_frame;            /* fast build: planes nothing reads again are not stored (st_debug_keep_all_planes) */
    uint32_t skip_scratch_stores;   /* fused DI spatial launch keeps its scratch records in registers */
    uint32_t di_head_on_main;       /* DI sampling + temporal on the caller's stream (0: on the side stream) */
    uint32_t alias_gi_history;      /* fast build: GI history hand-over by pointer swap instead of gi_resolving's copy */
    uint32_t tile_map;              /* blockIdx -> 8x8 tile mapping of the ReSTIR passes: 0 XCD bands, 1 hardware order, 2 chunks of 4 tile rows */
    uint32_t tile_map_denoise;      /* the same for the SVGF passes */
    int32_t side_priority;          /* > 0: the side stream gets the device's highest stream priority, < 0 the lowest */
    uint32_t staging;               /* st_tick uploads through page-locked staging slots (0: from pageable memory, joining the stream) */
    uint32_t double_buffer;         /* scene / light arrays exist twice on the device; a change fills the copy no frame in flight reads */
    uint32_t packed_base;           /* per-material packed base colour (0: primary visibility packs it per pixel) */
    uint32_t tick_timing;           /* 1: host-side cost of a scene refresh on stderr */
    uint32_t anyhit_fast;           /* fast build: shadow rays (boolean result only, ray.rs:84-112) walk with fast arithmetic
                                     * (st_traverse.h any_hit_fast); 0: the contract loop. Always 0 while traversal bytes are counted */
    uint32_t compact_bvh;           /* fast build: shadow rays walk a second, compact form of the BVH stream (48-B entries with conservative f16 child
                                     * boxes, regenerated on the device after every change: k_bvh.hip k_bvh_compact) — 2 / 3 texels per step instead of 4 */
    uint32_t allow_deep_bvh;        /* 1: a tree deeper than the traversal stack is a warning on stderr, not ST_ERR_BVH_TOO_DEEP */
    uint32_t device_bake;           /* 1: instances are baked into world space ON THE DEVICE from object-space meshes uploaded once
                                     * (k_bvh.hip k_bvh_bake) when only transforms changed under ST_BVH_REFIT_DEVICE; 0: on the host */
    uint32_t wide_bvh;              /* fast build, scenes that do not fit LDS: every ray outside the heatmap pass walks a 4-WIDE form of the BVH — four conservative
                                     * f16 child boxes + four links per aligned 64-B line (k_bvh.hip k_bvh_wide; the host collapses the binary tree once per build,
                                     * the device refills the boxes after every change) — half the dependent round trips and lines of the compact binary stream */
    uint32_t wide_stack_entries;    /* pending entries per ray of the wide walk's stack: 0 = 24 (strolle-gpu/src/lib.rs:76); tests render with 48 to show that 24 drops no push */
    uint32_t primary_packets;       /* with the wide stream: primary visibility walks it as ONE packet per wave — uniform node pointer and stack, scalar node
                                     * fetches, per-lane box and triangle tests, ballots decide the descent (st_traverse.h closest_hit_packet) */
    uint32_t side_start;            /* two streams: where the NEXT frame's side-stream work (primary visibility, the GI chain) may start. 0: behind this frame's DI
                                     * passes; 1 / 2 (default) / 3: also behind the a-trous launch of strides 1+2 / stride 4 / stride 8 — the LDS-staged launches fill a CU's
                                     * LDS, and a tracing block beside them waits for a CU instead of sharing one. Only waits move: the same launches in the same
                                     * order, the same bits. Frames without the fused a-trous chain behave as 0 */
} StTuning;
int st_engine_get_tuning(StEngine* e, StTuning* out);
int st_engine_set_tuning(StEngine* e, const StTuning* tuning);

/* Arithmetic of the per-pixel kernels. Both builds of every kernel live in the library (csrc/Makefile):
 * ST_ARITH_FAST (default) uses the hardware's reciprocal / square root / exp2 / log2 / sin / cos (1 ulp each) and lets the
 * compiler contract a*b+c into FMAs, everywhere except the ray-generation + BVH-traversal compare chain (Camera::ray,
 * Ray::traverse, intersect_box, Triangle::hit: strolle-gpu/src/camera.rs:32-51, ray.rs:114-302, triangle.rs:64-113),
 * which stays IEEE-exact so that BVH-heatmap integers are bit-identical to the reference restatement. The reference itself
 * leaves these functions to the SPIR-V driver's precision. Output is checked against the oracle within the per-plane
 * tolerances stated in tests/test_gpu_fast_tolerance.py.
 * ST_ARITH_EXACT evaluates everything with correctly rounded + - * / sqrt, no contraction and fixed polynomial
 * transcendentals: every buffer of every pass is then bit-identical to the CPU oracle (tests/test_gpu_parity.py).
 * ST_EXACT=1 in the environment makes new engines start in the exact build. Switching keeps all camera state. */
enum StArithmetic { ST_ARITH_FAST = 0, ST_ARITH_EXACT = 1 };
int st_engine_set_arithmetic(StEngine* e, int arithmetic);
int st_engine_get_arithmetic(StEngine* e, int* out);

/* ---- parity / measurement read-back */
enum StBufferId {
    ST_BUF_PRIM_GBUFFER_D0_A = 0, ST_BUF_PRIM_GBUFFER_D0_B = 1, ST_BUF_PRIM_GBUFFER_D1_A = 2, ST_BUF_PRIM_GBUFFER_D1_B = 3,
    ST_BUF_PRIM_SURFACE_MAP_A = 4, ST_BUF_PRIM_SURFACE_MAP_B = 5, ST_BUF_REPROJECTION_MAP = 6, ST_BUF_VELOCITY_MAP = 7,
    ST_BUF_DI_RESERVOIRS_0 = 8, ST_BUF_DI_RESERVOIRS_1 = 9, ST_BUF_DI_RESERVOIRS_2 = 10,
    ST_BUF_DI_DIFF_SAMPLES = 11, ST_BUF_DI_DIFF_PREV_COLORS = 12, ST_BUF_DI_DIFF_CURR_COLORS = 13,
    ST_BUF_DI_DIFF_MOMENTS_A = 14, ST_BUF_DI_DIFF_MOMENTS_B = 15, ST_BUF_DI_DIFF_STASH = 16, ST_BUF_DI_SPEC_SAMPLES = 17,
    ST_BUF_GI_D0 = 18, ST_BUF_GI_D1 = 19, ST_BUF_GI_D2 = 20,
    ST_BUF_GI_RESERVOIRS_0 = 21, ST_BUF_GI_RESERVOIRS_1 = 22, ST_BUF_GI_RESERVOIRS_2 = 23, ST_BUF_GI_RESERVOIRS_3 = 24,
    ST_BUF_GI_DIFF_SAMPLES = 25, ST_BUF_GI_DIFF_PREV_COLORS = 26, ST_BUF_GI_DIFF_CURR_COLORS = 27,
    ST_BUF_GI_DIFF_MOMENTS_A = 28, ST_BUF_GI_DIFF_MOMENTS_B = 29, ST_BUF_GI_DIFF_STASH = 30, ST_BUF_GI_SPEC_SAMPLES = 31,
    ST_BUF_REF_HITS = 32, ST_BUF_REF_RAYS = 33, ST_BUF_REF_COLORS = 34,
    ST_BUF_DBG_USED_MEMORY = 35, /* u32 per pixel: Ray::traverse's `used_memory` of the heatmap pass (ray.rs:125-264) */
    ST_BUF_COUNT = 36
};
/* Synchronises the device, then copies a per-camera buffer (camera_controller/buffers.rs:7-51) to host
 * memory. out == NULL: only report the size in *written.
 * After a frame every buffer holds what the reference's pass graph leaves in it — bit for bit in the exact build, within
 * the documented tolerance in the fast build, with one stated difference there: on frames whose GI source is the temporal
 * pass's output the history plane GI_RESERVOIRS_0 is that output itself (a pointer swap) instead of the reference's
 * decoded-and-re-encoded copy of it, so a few normals per frame differ by an ulp between the two planes' read-backs. */
int st_camera_read_buffer(StEngine* e, StHandle camera, int buffer_id, void* out, size_t capacity, size_t* written);
/* The inverse of st_camera_read_buffer: overwrite a per-camera buffer with host data (`bytes` must be the buffer's size).
 * With st_debug_set_pass_mask this lets a test hand one launch exactly the inputs the oracle's pass saw, so the fast
 * build is compared pass by pass instead of through ReSTIR's chaotic temporal feedback. Planes this library derives from
 * the reference's (decoded surface twins, sqrt-luma planes) are regenerated before the next render. Synchronises. */
int st_camera_write_buffer(StEngine* e, StHandle camera, int buffer_id, const void* data, size_t bytes);
/* The lean frame. In the fast build, when the whole pass graph of an Image{denoise} frame runs, planes that nothing reads
 * again — not a later pass of the frame, not the next frame — are not stored: the velocity map and the encoded surface map
 * (every kernel reads the decoded twin this library keeps), both diffuse-sample planes (the fused denoise-reproject stages
 * consume them in registers), the reprojected GI reservoirs of tracing frames, the first GI preview pass's result where it
 * is a plain normalisation of its input (the second pass rebuilds it where it reads one), and the last a-trous pass's colour
 * planes (frame composition runs inside that launch). st_camera_read_buffer of ST_BUF_VELOCITY_MAP, PRIM_SURFACE_MAP_*,
 * DI/GI_DIFF_SAMPLES, GI_RESERVOIRS_2, GI_RESERVOIRS_3 and DI/GI_DIFF_CURR_COLORS then returns what an earlier launch left.
 * keep != 0 (or ST_KEEP_ALL_PLANES=1 in the environment) makes every frame store all planes as the reference does; the exact
 * build, a pass mask and the partial camera modes always do. */
int st_debug_keep_all_planes(StEngine* e, int keep);
/* *stale = 1 when the camera's last frame left `buffer_id` unwritten (one of the planes listed above, in a lean frame): what
 * st_camera_read_buffer returns for it is an earlier launch's or frame's content. strolle_amd.api read_buffer(strict=True) refuses such a read. */
int st_camera_buffer_stale(StEngine* e, StHandle camera, int buffer_id, int* stale);
/* One bit per reference pass (strolle/src/camera_controller.rs:87-174 order). st_render_camera executes a launch only when
 * ALL the passes it covers are in the mask (a fused launch covers several); a mask that splits a fused launch is an
 * ST_ERR_INVALID_ARGUMENT. Default: all ones. Frame counters, seeds and plane ping-pong are unaffected. */
enum StPassBit {
    ST_PASS_PRIM_VISIBILITY = 1u << 0, ST_PASS_FRAME_REPROJECTION = 1u << 1,
    ST_PASS_DI_SAMPLING = 1u << 2, ST_PASS_DI_TEMPORAL = 1u << 3, ST_PASS_DI_SPATIAL_PICK = 1u << 4, ST_PASS_DI_SPATIAL_TRACE = 1u << 5,
    ST_PASS_DI_SPATIAL_SAMPLE = 1u << 6, ST_PASS_DI_RESOLVING = 1u << 7,
    ST_PASS_GI_REPROJECTION = 1u << 8, ST_PASS_GI_SAMPLING_A = 1u << 9, ST_PASS_GI_SAMPLING_B = 1u << 10, ST_PASS_GI_TEMPORAL = 1u << 11,
    ST_PASS_GI_SPATIAL_PICK = 1u << 12, ST_PASS_GI_SPATIAL_TRACE = 1u << 13, ST_PASS_GI_SPATIAL_SAMPLE = 1u << 14,
    ST_PASS_GI_PREVIEW_0 = 1u << 15, ST_PASS_GI_PREVIEW_1 = 1u << 16, ST_PASS_GI_RESOLVING = 1u << 17,
    ST_PASS_DENOISE_REPROJECT_DI = 1u << 18, ST_PASS_DENOISE_REPROJECT_GI = 1u << 19, ST_PASS_DENOISE_VARIANCE = 1u << 20,
    ST_PASS_DENOISE_WAVELET_0 = 1u << 21, /* ... wavelet pass n = ST_PASS_DENOISE_WAVELET_0 << n, n < 5 */
    ST_PASS_COMPOSITION = 1u << 26, ST_PASS_BVH_HEATMAP = 1u << 27, ST_PASS_REF_TRACING = 1u << 28, ST_PASS_REF_SHADING = 1u << 29,
    ST_PASS_POST = 1u << 30   /* the launches behind composition, one launch group: fog ("fog" above), light shafts ("light shafts"), depth of field ("depth of field"), motion blur ("motion blur"), bloom ("bloom"), lens effects ("lens effects"), colour grading ("colour grading"), then FXAA and / or the resampler ("post-processing"), then the upscaler and / or the sharpening step ("upscaling") */
};
int st_debug_set_pass_mask(StEngine* e, uint64_t mask);
/* Measurement only (tools/pair_matrix.py): the frame's graph is built as always — every fusion of the whole frame — but only the launches
 * whose ordinal in the frame's serial order has its bit set are enqueued, all on the caller's stream. ~0 (default): everything, as shipped.
 * What the planes hold after a filtered frame is unspecified. */
int st_debug_set_launch_filter(StEngine* e, uint64_t filter);
/* The variance pass's short-history flags after the last frame (StTuning::variance_in_reproject): one 64-bit word per 8x8 tile, bit =
 * pixel of the tile — the pixels whose estimate_variance takes the 29-tap spatial branch (frame_denoising.rs:128-189). out == NULL: only
 * the tile count. (Steady state, 1080p: 8 % of the pixels on the Cornell box, 84 % in the dungeon — DI samples without confidence reset
 * their history every frame.) */
int st_debug_variance_flags(StEngine* e, StHandle camera, uint64_t* tile_mask_out, size_t capacity_tiles, size_t* tiles);
/* The pass bits of every launch the last st_render_camera considered, in launch order (executed or not): lets a test walk
 * the shipped launch structure without knowing it. Returns the count; writes at most `capacity` entries. */
int st_debug_last_launches(StEngine* e, uint64_t* out_bits, size_t capacity, size_t* count);
/* Rays traced for this camera since the last reset (device counters, closest-hit + any-hit). */
int st_camera_ray_count(StEngine* e, StHandle camera, uint64_t* out, int reset);
/* Host-side copies of what st_tick uploads: what = 0 BVH stream as the reference's serializer writes it (float4), 1
 * triangles in the reference's 144-B layout, 2 lights (112 B), 3 materials (112 B), 4 the BVH stream in its device form
 * (every entry four float4: internal nodes with the far child's byte offset, leaf entries followed by the triangle's
 * hit-test record; st_types.h), 6 the device form read back FROM the device (live copy),
 * 7-13 the inputs of the device refit (k_bvh.hip; uint32 unless noted): 7 parent of every entry (entry << 1 | child slot),
 * 8 LDS slot of every internal entry (bit 31: a task's root), 9 work items (bit 31: root of a finished task), 10 batch offsets
 * into 9, 11 (first batch, batches) per launch, 12 leaf entry of every triangle slot, 13 triangle bounds (two float4 per slot);
 * 14-17 the WIDE stream (StTuning::wide_bvh; uint32 unless noted): 14 its topology as the host builds it — one word with the root's
 * link in bits 0-7 and the most entries a walk over it can have pending in bits 8.., then 8 words per node: where each of the four child boxes lives in the device form (entry << 1 | 0 left box, 1 right box;
 * 0xffffffff = empty slot) and the four links (index << 1 | is a leaf record) —, 15 the device-form entry of every leaf record,
 * 16 / 17 its nodes (64 B each) and leaf records (48 B each) read back FROM the device (live copy; float4).
 * All but 6, 16 and 17 work on host-only engines. */
int st_debug_read_scene(StEngine* e, int what, void* out, size_t capacity, size_t* written);
int st_debug_world(StEngine* e, uint32_t* light_count, uint32_t* next_frame);
/* Where an image sits in the 8192-wide atlas: x, y, width, height in texels (images.rs:115-124 `lookup`). */
int st_debug_image_rect(StEngine* e, StHandle id, uint32_t out_xywh[4]);
/* The last BVH refresh (strolle/src/bvh/builder.rs:35-124 reuses subtrees whose primitives did not change): how many
 * primitives the tree holds and how many of them came over inside subtrees copied from the previous tree. The
 * uploaded stream is the one a from-scratch build of the same primitives gives, reuse or not. */
int st_debug_bvh_refresh(StEngine* e, uint64_t* primitives, uint64_t* reused);
/* Atmosphere LUTs as generated on the device (strolle-shaders/src/atmosphere): what = 0 transmittance 256x64,
 * 1 multi-scattering 32x32, 2 sky 256x256; RGBA32F texels holding f16-rounded values (the reference stores Rgba16Float). */
int st_debug_read_lut(StEngine* e, int what, float* out, size_t capacity_floats, size_t* written_floats);

/* ---- scene ingest. In the reference this step is Bevy's glTF loader plus bevy-strolle's
 * stages (bevy-strolle/src/stages/prepare.rs:20-122 meshes, :124-180 materials, :182-260 images; extract.rs instances);
 * here it is a convenience layered on the entry points above and nothing else. One mesh + instance per triangle-list
 * primitive of the default scene, numbered in depth-first node order: mesh / instance handle = first_handle + i,
 * material handle = first_handle + material index, image handle = first_image_handle + image index; KHR_lights_punctual
 * point and spot lights become lights the way bevy_gltf + bevy-strolle's extract stage would make them
 * (extract.rs:283-327), light handle = first_handle + k. Materials follow
 * prepare.rs:132-175 (Opaque forces alpha 1, Mask becomes Blend with alpha 0/1, reflectance 0.5, ior 1). PNG (all colour
 * types and bit depths, Adam7 too) and JPEG textures are decoded here; KTX2 / WebP, Draco and sparse accessors give
 * ST_ERR_UNSUPPORTED. Host-only work: valid on host-only engines. */
enum { ST_GLTF_OVERRIDE_REFLECTANCE = 1, ST_GLTF_OVERRIDE_PERCEPTUAL_ROUGHNESS = 2 };
typedef struct StGltfOptions {
    StHandle first_handle;        /* default 1 */
    StHandle first_image_handle;  /* default 1000 */
    uint32_t override_mask;       /* ST_GLTF_OVERRIDE_*: replace that field of every material (demo.rs:254-258 does this) */
    float reflectance;
    float perceptual_roughness;
    uint32_t subdivide;           /* k: every triangle is split into 4^k by midpoint subdivision (synthetic scaling), k <= 6 */
    float light_radius;           /* radius given to KHR_lights_punctual lights, which have none. 0 is what arrives through Bevy
                                   * (PointLight::radius defaults to 0) — but the reference's ReSTIR loses about half of a
                                   * zero-radius light's energy (reservoir/di.rs:105-116 tests `light.contains(point)`), which is
                                   * why its own examples set 0.15 (cornell.rs:45-54, demo.rs:169-191) */
    uint32_t _pad;
} StGltfOptions;
typedef struct StGltfSummary {
    uint32_t meshes, triangles, materials, images;
    uint32_t images_dropped;      /* did not fit the atlas: the reference warns and drops them (images.rs:71-79) */
    uint32_t primitives_skipped;  /* points, lines, strips, fans, or primitives without a single triangle */
    uint32_t lights;              /* KHR_lights_punctual point / spot lights inserted, handles first_handle + k in node order */
    uint32_t lights_skipped;      /* directional ones (strolle's sun is st_sun_update) and ones fainter than 0.0001 cd */
} StGltfSummary;
/* options == NULL: the defaults above; summary may be NULL. External buffers / images are read relative to the file. */
int st_scene_load_gltf(StEngine* e, const char* path, const StGltfOptions* options, StGltfSummary* summary);
int st_scene_load_gltf_memory(StEngine* e, const void* bytes, size_t size, const char* base_dir, const StGltfOptions* options, StGltfSummary* summary);
/* PNG -> RGBA8 (straight alpha; 16-bit samples keep their high byte), the decoder the loader uses. out_rgba == NULL
 * only reports the size. */
int st_decode_png(const void* bytes, size_t size, uint8_t* out_rgba, size_t capacity, uint32_t* width, uint32_t* height);
/* The same for either of glTF's two image formats, told apart by signature: PNG, or JPEG (baseline, extended and
 * progressive DCT; 8-bit; grey or three components). */
int st_decode_image(const void* bytes, size_t size, uint8_t* out_rgba, size_t capacity, uint32_t* width, uint32_t* height);

/* This device's streaming ceiling measured with the library's own grid-stride float4 copy kernel (k_util.hip): best of `iters`
 * copies of `bytes`, (bytes read + bytes written) / time in GB/s. bench.py reports it beside the 8 TB/s spec peak. */
int st_debug_copy_bandwidth(StEngine* e, size_t bytes, int iters, double* out_gbps);

/* Per-kernel measurement. st_profile_enable(e, flags): bit 0 (ST_PROFILE_TIMING) = HIP events around every launch on the
 * launch stream; while it is set the pass graph runs serially on the caller's stream (no two-stream overlap), so that an
 * event pair times its kernel alone. Bit 1 (ST_PROFILE_TRAVERSAL_BYTES) = the tracing kernels also sum the reference's
 * `used_memory` counter over their rays (a cross-lane reduction per ray: ~10 us per full-screen launch, which is why it
 * is not always on; rays themselves are always counted, st_camera_ray_count). The rendered bits are the same in every
 * mode. st_profile_read returns, per kernel slot i < *count: name, launches, total milliseconds (0 without bit 0),
 * algorithmic bytes (DESIGN.md "bytes per unit" x units launched; the traversal part is 0 without bit 1). */
enum { ST_PROFILE_TIMING = 1, ST_PROFILE_TRAVERSAL_BYTES = 2,
       ST_PROFILE_GROUP_ATROUS = 4 /* with TIMING: the a-trous chain's launches (4 per frame, back to back on one stream) are timed as ONE
                                      interval under the slot "a-trous chain (one timed interval)" instead of one event pair per slot */,
       ST_PROFILE_KERNEL_EVENTS = 8 /* with TIMING: every launch carries its own start / stop events (hipExtLaunchKernelGGL: the dispatch's
                                       timestamps, what rocprofv3's kernel trace reports) instead of events recorded between kernels */ };
enum { ST_PROFILE_MAX_KERNELS = 64 };  /* >= the number of kernel slots (st_kernels.h) */
typedef struct StKernelProfile {
    char name[48];
    uint32_t launches;
    float total_ms;
    double algorithmic_bytes; /* summed over launches: screen-space bytes (B) + traversal bytes (A), SURVEY.md 8(d) */
    double traversal_bytes;   /* the A part alone: the reference's used_memory counter summed over the kernel's rays */
} StKernelProfile;
int st_profile_enable(StEngine* e, int enabled);
int st_profile_read(StEngine* e, StKernelProfile* out, size_t capacity, size_t* count, int reset);

#ifdef __cplusplus
}
#endif
#endif /* STROLLE_HIP_H */
