// st_kernels.h — launch interface between the host engine (st_engine.cpp) and the HIP kernels.
// Each launcher enqueues exactly one kernel on `stream`; `KArgs` travels by value in the kernarg segment.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "st_types.h"

namespace st {

// Per-kernel timing without event packets between kernels (ST_PROFILE_KERNEL_EVENTS): when the engine sets this pair, the next
// launch goes through hipExtLaunchKernelGGL, which writes the dispatch's own start / stop timestamps into the two events — what
// rocprofv3's kernel trace reads too. An event RECORDED between two kernels instead makes the second wait for a barrier packet
// (3-15 us each, measured), which is how the default profiling mode times runs of launches.
// `consumed` tells the engine that a launch really took the pair (a launcher whose grid is empty enqueues nothing: its events must go
// back to the pool unrecorded — hipEventElapsedTime on a pair no dispatch wrote fails).
struct LaunchEvents { hipEvent_t start = nullptr, stop = nullptr; bool consumed = false; };
extern thread_local LaunchEvents g_launch_events;  // st_engine.cpp
#define ST_KLAUNCH_SMEM(kernel, grid, block, smem, stream, ...)                                                                                  \
    do {                                                                                                                                         \
        if (::st::g_launch_events.start && !::st::g_launch_events.consumed) {                                                                    \
            hipExtLaunchKernelGGL(kernel, grid, block, smem, stream, ::st::g_launch_events.start, ::st::g_launch_events.stop, 0, __VA_ARGS__);   \
            ::st::g_launch_events.consumed = true;                                                                                               \
        } else hipLaunchKernelGGL(kernel, grid, block, smem, stream, __VA_ARGS__);                                                               \
    } while (0)
#define ST_KLAUNCH(kernel, grid, block, stream, ...) ST_KLAUNCH_SMEM(kernel, grid, block, 0, stream, __VA_ARGS__)

// Kernel slots: index into the per-camera counter array (2 x u64 per slot: rays, traversal bytes) and into the
// profiler's table. `bytes_per_unit` = compulsory screen-space bytes one launch unit (pixel or 2x1 cell) reads +
// writes through the planes the reference binds for that pass (neighbour taps assumed cache-served).
enum KernelSlot {
    KS_BVH_HEATMAP, KS_REF_TRACING, KS_REF_SHADING, KS_PRIM_VISIBILITY, KS_FRAME_REPROJECTION,
    KS_DI_SAMPLING, KS_DI_TEMPORAL, KS_DI_SPATIAL_PICK, KS_DI_SPATIAL_TRACE, KS_DI_SPATIAL_SAMPLE, KS_DI_RESOLVING,
    KS_GI_REPROJECTION, KS_GI_SAMPLING_A, KS_GI_SAMPLING_B, KS_GI_TEMPORAL, KS_GI_SPATIAL_PICK, KS_GI_SPATIAL_TRACE,
    KS_GI_SPATIAL_SAMPLE, KS_GI_PREVIEW, KS_GI_RESOLVING, KS_DENOISE_REPROJECT, KS_DENOISE_VARIANCE, KS_DENOISE_WAVELET,
    KS_COMPOSITION,
    // fused launches (own-pixel consumer passes appended to their producer); bytes = sum of the reference passes they execute
    KS_PRIM_VISIBILITY_REPROJECTION, KS_DI_RESOLVING_REPROJECT, KS_GI_PREVIEW_RESOLVE, KS_GI_PREVIEW_RESOLVE_REPROJECT, KS_DENOISE_WAVELET_12,
    KS_GI_REPROJECTION_TEMPORAL, KS_DI_SAMPLING_TEMPORAL, KS_DI_SPATIAL_FUSED, KS_GI_SPATIAL_FUSED,
    KS_GI_PREVIEW_BOTH, KS_GI_PREVIEW_BOTH_NO_REPROJECT, KS_GI_PREVIEW_LATE, KS_DENOISE_WAVELET_COMPOSE, KS_GI_SAMPLING_AB,
    KS_DENOISE_WAVELET_FAMILY,  // profiling only (ST_PROFILE_GROUP_ATROUS): the a-trous chain's launches timed as ONE interval
    KS_POST_FXAA, KS_POST_RESAMPLE,  // output post-processing behind composition (k_post.hip); their bytes depend on the output size and format: render() credits them itself
    KS_BLOOM_DOWN, KS_BLOOM_UP, KS_BLOOM_COMPOSITE, KS_BLOOM_TAIL,  // bloom in front of the display transform (k_bloom.hip); bytes depend on the level: render() credits them itself
    KS_MBLUR_PACK, KS_MBLUR_NEIGHBOUR, KS_MBLUR_GATHER,  // motion blur in front of bloom (k_motion_blur.hip); render() credits their bytes itself
    KS_DOF_PACK, KS_DOF_NEIGHBOUR, KS_DOF_GATHER,  // depth of field in front of motion blur (k_dof.hip); render() credits their bytes itself
    KS_FOG,  // fog in front of depth of field (k_fog.hip); render() credits its bytes itself
    KS_SHAFTS_MARCH, KS_SHAFTS_APPLY,  // light shafts between fog and depth of field (k_shafts.hip); render() credits their bytes itself
    KS_GRADE,  // colour grading behind bloom (k_grade.hip); render() credits its bytes itself
    KS_UPSCALE, KS_SHARPEN, KS_UPSCALE_SHARPEN,  // the upscale stage behind FXAA (k_upscale.hip); their bytes depend on the output size and format: render() credits them itself
    KS_LENS,  // lens effects between bloom and colour grading (k_lens.hip); render() credits its bytes itself
    KS_COUNT
};
struct KernelInfo { const char* name; float bytes_per_unit; bool half; };
inline const KernelInfo& kernel_info(int slot) {
    static const KernelInfo k[KS_COUNT] = {
        {"bvh_heatmap", 16.f, false},        {"ref_tracing", 64.f, false},         {"ref_shading", 128.f, false},
        {"prim_visibility", 64.f, false},    {"frame_reprojection", 64.f, false},  {"di_sampling", 68.f, false},
        {"di_temporal", 176.f, false},       {"di_spatial_pick", 128.f, true},     {"di_spatial_trace", 48.f, false},
        {"di_spatial_sample", 192.f, true},  {"di_resolving", 128.f, false},       {"gi_reprojection", 176.f, false},
        {"gi_sampling_a", 80.f, true},       {"gi_sampling_b", 144.f, true},       {"gi_temporal", 272.f, false},
        {"gi_spatial_pick", 160.f, true},    {"gi_spatial_trace", 48.f, false},    {"gi_spatial_sample", 352.f, true},
        {"gi_preview", 160.f, false},        {"gi_resolving", 256.f, false},       {"denoise_reproject", 112.f, false},
        {"denoise_variance", 112.f, false},  {"denoise_wavelet", 84.f, false},     {"composition", 112.f, false},
        {"prim_visibility+frame_reprojection", 64.f + 64.f, false},
        {"di_resolving+denoise_reproject", 128.f + 112.f, false},
        {"gi_preview+gi_resolving", 160.f + 256.f, false},
        {"gi_preview+gi_resolving+denoise_reproject", 160.f + 256.f + 112.f, false},
        {"denoise_wavelet x2 (strides 1+2)", 84.f + 84.f, false},
        {"gi_reprojection+gi_temporal", 176.f + 272.f, false},
        {"di_sampling+di_temporal", 68.f + 176.f, false},
        {"di_spatial_pick+trace+sample", 128.f + 2.f * 48.f + 192.f, true},  // per cell: the trace pass covers both of its pixels
        {"gi_spatial_pick+trace+sample", 160.f + 2.f * 48.f + 352.f, true},
        {"gi_preview x2+gi_resolving+denoise_reproject", 160.f + 160.f + 256.f + 112.f, false},
        {"gi_preview x2+gi_resolving", 160.f + 160.f + 256.f, false},
        {"gi_preview 2nd pass (pixels that resample)", 0.f, false},  // its bytes are credited to the launch above
        {"denoise_wavelet+composition", 84.f + 112.f, false},
        {"gi_sampling_a+b", 80.f + 144.f, true},
        {"a-trous chain (one timed interval)", 0.f, false},  // bytes: the sum its member launches are credited
        {"post_fxaa", 0.f, false},           {"post_resample", 0.f, false},
        {"bloom_down", 0.f, false},          {"bloom_up", 0.f, false},             {"bloom_composite", 0.f, false},
        {"bloom_tail", 0.f, false},
        {"motion_blur_pack", 0.f, false},    {"motion_blur_neighbour", 0.f, false}, {"motion_blur_gather", 0.f, false},
        {"dof_pack", 0.f, false},            {"dof_neighbour", 0.f, false},        {"dof_gather", 0.f, false},
        {"fog", 0.f, false},
        {"shafts_march", 0.f, false},        {"shafts_apply", 0.f, false},
        {"color_grading", 0.f, false},
        {"upscale", 0.f, false},             {"sharpen", 0.f, false},              {"upscale+sharpen", 0.f, false},
        {"lens", 0.f, false},
    };
    return k[slot];
}

// Skinning (k_skin.hip): built once with the exact flags, like the device BVH builder. One job per posed instance; job_start (n_jobs + 1
// entries, in triangles) pads every job to kSkinBlock so that a workgroup serves one job. Triangles index the skin store (skin_first) and the
// posed store (posed_first), 24 floats each; palette_first counts 12-float joint matrices.
constexpr uint32_t kSkinBlock = 128u, kSkinMaxJoints = 256u;
struct SkinJob { uint32_t skin_first, count, posed_first, palette_first, joint_count, pad[3]; };
static_assert(sizeof(SkinJob) == 32, "one skin job is 32 B");
void launch_skin(const SkinJob* jobs, const uint32_t* job_start, uint32_t n_jobs, uint32_t padded_total, const float* bind, const void* corners,
                 const float* palettes, float* posed, hipStream_t s);
// Morph targets (k_skin.hip k_morph; include/strolle_hip.h "morph targets"): the jobs with at least one active target, the skin stage behind
// the morph stage when joint_count is not 0 (skin_first then names the skin's corners too; without a skin it names bind triangles only).
// The target store is counted in units of 18 floats (one triangle of one target): target k of a mesh lies at unit target_first + k * padded,
// `padded` being the mesh's triangles rounded up to kSkinBlock, as four planes of float4 and one of float2 (floats 4q .. 4q + 3 and 16, 17 of
// each triangle's 18: position deltas 9, normal deltas 9), so that a wave's load for one target is one contiguous run. active_first /
// active_count: the job's non-zero weights with their target indices, ascending, in the tick's MorphActive list.
struct MorphJob { uint32_t skin_first, count, posed_first, palette_first, joint_count, target_first, padded, active_first, active_count, pad[3]; };
static_assert(sizeof(MorphJob) == 48, "one morph job is 48 B");
struct MorphActive { uint32_t target; float weight; };
constexpr uint32_t kMorphMaxTargets = 64u, kMorphUnitFloats = 18u;
void launch_morph(const MorphJob* jobs, const uint32_t* job_start, uint32_t n_jobs, uint32_t padded_total, const float* bind, const void* corners,
                  const float* palettes, const float* targets, const MorphActive* active, float* posed, hipStream_t s);

// The launchers exist twice, in namespaces st::exact and st::fast (the two arithmetic builds of the kernel files, Makefile);
// the engine calls them through a table picked per engine (st_engine_set_arithmetic).
#define ST_LAUNCHER(name, args) void name args;
namespace exact {
#include "st_launchers.inc"
}
namespace fast {
#include "st_launchers.inc"
}
#undef ST_LAUNCHER
struct Launchers {
#define ST_LAUNCHER(name, args) void (*name) args;
#include "st_launchers.inc"
#undef ST_LAUNCHER
};
inline Launchers launchers_exact() {
    Launchers t;
#define ST_LAUNCHER(name, args) t.name = &exact::name;
#include "st_launchers.inc"
#undef ST_LAUNCHER
    return t;
}
inline Launchers launchers_fast() {
    Launchers t;
#define ST_LAUNCHER(name, args) t.name = &fast::name;
#include "st_launchers.inc"
#undef ST_LAUNCHER
    return t;
}

}  // namespace st
