// k_skin.hip — linear blend skinning of posed instances on the device (include/strolle_hip.h "skinned meshes"; st_deform.cpp).
//
// One launch per tick covers every instance whose pose changed (and, after the posed store was reallocated, every posed instance). It reads
// the skin store (a skinned mesh's bind-pose triangles in the device mesh store's layout — 24 floats: positions 9, normals 9, uvs 6 — and
// one StSkinVertex per corner) and writes the instance's posed object-space triangles, in that same layout, into its region of the posed
// store, from which k_bvh.hip k_bvh_bake bakes the instance like any moved one.
//
// Built ONCE, with the exact build's flags (Makefile: k_skin.o, like k_lbvh.o), whatever arithmetic the frames use: a fast and an exact
// engine produce the same posed bits, and the host baking the posed triangles of a host-path refresh gets the device's bits.
// The operations and their order (tests/test_skin_abi.py and tests/test_gpu_skinning.py restate them in numpy float32):
//   blend     M[e] = ((w0 * J0[e] + w1 * J1[e]) + w2 * J2[e]) + w3 * J3[e] for each of the 12 floats (Affine3A columns x, y, z, t);
//             slots of weight 0 take part like the others
//   position  p' = ((x * p.x + y * p.y) + z * p.z) + t                     (glam Affine3A::transform_point3, k_bvh_bake's order)
//   normal    c0 = cross(y, z), c1 = cross(z, x), c2 = cross(x, y), det = dot(z, c2) (glam Affine3A::inverse);
//             det == 0: the bind normal as it is; else n' = normalize(((c0 / det) * n.x + (c1 / det) * n.y) + (c2 / det) * n.z)
//             (the inverse transpose of M's 3x3, as bevy_pbr's skin_normals; st_math.h cross, dot, normalize)
//   uvs       copied
//
// Shape: a workgroup serves one job (the start table pads every job to kSkinBlock triangles), so the job's palette — at most 256 joints x
// 48 B = 12 KB — is staged in LDS once and every corner's four joint reads hit LDS. One thread per triangle: it reads 96 B of bind pose and
// 72 B of skin and writes 96 B. (kernel-resource-usage, gfx950: no scratch; the figures are in DESIGN.md "Skinned meshes".)
#include <hip/hip_runtime.h>

#include "st_math.h"
#include "st_kernels.h"

namespace st {

struct SkinVertexDevice { uint16_t joints[4]; float weights[4]; };
static_assert(sizeof(SkinVertexDevice) == 24, "StSkinVertex is 24 B");

// The skin stage of one corner: the blend of its four joints from the staged palette, then position and normal (the header's operations).
static __device__ __forceinline__ void skin_corner(const float* pal, const SkinVertexDevice& c, V3 q, V3 nn, V3* p_out, V3* n_out) {
    float M[12];
    {
        const float* J0 = pal + 12u * c.joints[0];
#pragma unroll
        for (int e = 0; e < 12; e++) M[e] = c.weights[0] * J0[e];
    }
#pragma unroll
    for (int s = 1; s < 4; s++) {
        const float* Js = pal + 12u * c.joints[s];
#pragma unroll
        for (int e = 0; e < 12; e++) M[e] = M[e] + c.weights[s] * Js[e];
    }
    const V3 ax = v3(M[0], M[1], M[2]), ay = v3(M[3], M[4], M[5]), az = v3(M[6], M[7], M[8]), at = v3(M[9], M[10], M[11]);
    *p_out = ((ax * q.x) + (ay * q.y) + (az * q.z)) + at;
    const V3 c0 = cross(ay, az), c1 = cross(az, ax), c2 = cross(ax, ay);
    const float det = dot(az, c2);
    V3 n = nn;
    if (det != 0.0f) {
        V3 acc = (c0 / det) * nn.x; acc = acc + (c1 / det) * nn.y; acc = acc + (c2 / det) * nn.z;
        n = normalize(acc);
    }
    *n_out = n;
}

// the job whose padded [job_start[j], job_start[j + 1]) holds the workgroup that starts at triangle `first` of the launch
static __device__ __forceinline__ uint32_t job_of(const uint32_t* job_start, uint32_t n_jobs, uint32_t first) {
    uint32_t lo = 0u, hi = n_jobs;
    while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (job_start[mid] <= first) lo = mid; else hi = mid; }
    return lo;
}

// What both kernels begin with: the workgroup's job, its palette staged in LDS (`pal`) behind a barrier, and the thread's triangle `k` of the job —
// false for the threads of the padding, which are done.
template <class Job>
static __device__ __forceinline__ bool begin_job(const Job* jobs, const uint32_t* job_start, uint32_t n_jobs, const float* palettes, float* pal, Job* job, uint32_t* k) {
    const uint32_t first = blockIdx.x * kSkinBlock;
    const uint32_t lo = job_of(job_start, n_jobs, first);
    const Job j = jobs[lo];
    const float* src = palettes + 12u * (size_t)j.palette_first;
    for (uint32_t i = threadIdx.x; i < 12u * j.joint_count; i += kSkinBlock) pal[i] = src[i];
    __syncthreads();
    *job = j;
    *k = first - job_start[lo] + threadIdx.x;
    return *k < j.count;
}
// ... and end with: corner v's position and normal into the posed triangle, and the uvs copied from the bind triangle
static __device__ __forceinline__ void store_corner(float* out, int v, V3 p, V3 n) {
    out[3 * v] = p.x; out[3 * v + 1] = p.y; out[3 * v + 2] = p.z;
    out[9 + 3 * v] = n.x; out[9 + 3 * v + 1] = n.y; out[9 + 3 * v + 2] = n.z;
}
static __device__ __forceinline__ void copy_uvs(float* out, const float* m) {
#pragma unroll
    for (int u = 0; u < 6; u++) out[18 + u] = m[18 + u];
}

__global__ __launch_bounds__(kSkinBlock) void k_skin(const SkinJob* jobs, const uint32_t* job_start, uint32_t n_jobs, const float* bind,
                                                     const SkinVertexDevice* corners, const float* palettes, float* posed) {
    __shared__ float pal[kSkinMaxJoints * 12u];
    SkinJob j; uint32_t k;
    if (!begin_job(jobs, job_start, n_jobs, palettes, pal, &j, &k)) return;
    const float* m = bind + 24u * (size_t)(j.skin_first + k);
    const SkinVertexDevice* sv = corners + 3u * (size_t)(j.skin_first + k);
    float* out = posed + 24u * (size_t)(j.posed_first + k);
#pragma unroll
    for (int v = 0; v < 3; v++) {
        const SkinVertexDevice c = sv[v];
        V3 p, n;
        skin_corner(pal, c, v3(m[3 * v], m[3 * v + 1], m[3 * v + 2]), v3(m[9 + 3 * v], m[9 + 3 * v + 1], m[9 + 3 * v + 2]), &p, &n);
        store_corner(out, v, p, n);
    }
    copy_uvs(out, m);
}

// Morph targets (include/strolle_hip.h "morph targets"): the jobs of a tick that have at least one active target, the skin stage above behind
// the morph stage where the job has a palette — the morphed triangle stays in registers in between. Same shape as k_skin: a workgroup serves
// one job, one thread one triangle. The operations and their order (tests/morph_ref.py restates them):
//   for each active target k, ascending (weights that are exactly 0 are not in the list): x = x + w[k] * d[k] for the 9 position and the 9
//   normal components; then per corner len = sqrt(dot(n, n)): 0 or not finite keeps the base normal, else n * (1 / len) (st_math.h normalize)
// Delta traffic: a thread's 18 floats of one target come as four float4 and one float2 from five planes of the target (st_kernels.h MorphJob),
// so that a wave's load is 1 KB (512 B) of consecutive addresses of which every byte is used; the weight and the target index are the same for
// the whole workgroup and are read through uniform addresses (scalar loads).
__global__ __launch_bounds__(kSkinBlock) void k_morph(const MorphJob* jobs, const uint32_t* job_start, uint32_t n_jobs, const float* bind,
                                                      const SkinVertexDevice* corners, const float* palettes, const float* targets,
                                                      const MorphActive* active, float* posed) {
    __shared__ float pal[kSkinMaxJoints * 12u];
    MorphJob j; uint32_t k;
    if (!begin_job(jobs, job_start, n_jobs, palettes, pal, &j, &k)) return;
    const float* m = bind + 24u * (size_t)(j.skin_first + k);
    float* out = posed + 24u * (size_t)(j.posed_first + k);
    float x[18];
#pragma unroll
    for (int i = 0; i < 18; i++) x[i] = m[i];
    const MorphActive* act = active + j.active_first;
    const size_t plane = (size_t)j.padded;   // float4s per plane
    // (the next target's loads are issued before this one's sums: two targets in flight per thread — a tick's launch is a few thousand waves)
    struct Delta { float4 d0, d1, d2, d3; float2 d4; float w; };
    auto fetch = [&](uint32_t a) {
        const float4* t4 = reinterpret_cast<const float4*>(targets + kMorphUnitFloats * ((size_t)j.target_first + (size_t)act[a].target * plane));
        return Delta{t4[k], t4[plane + k], t4[2u * plane + k], t4[3u * plane + k], reinterpret_cast<const float2*>(t4 + 4u * plane)[k], act[a].weight};
    };
    Delta next{};
    if (j.active_count != 0u) next = fetch(0u);
    for (uint32_t a = 0; a < j.active_count; a++) {
        const Delta c = next;
        if (a + 1u < j.active_count) next = fetch(a + 1u);
        const float d[18] = {c.d0.x, c.d0.y, c.d0.z, c.d0.w, c.d1.x, c.d1.y, c.d1.z, c.d1.w, c.d2.x, c.d2.y, c.d2.z, c.d2.w, c.d3.x, c.d3.y, c.d3.z, c.d3.w, c.d4.x, c.d4.y};
#pragma unroll
        for (int i = 0; i < 18; i++) x[i] = x[i] + c.w * d[i];
    }
    const bool skinned = j.joint_count != 0u;
    const SkinVertexDevice* sv = corners + 3u * (size_t)(j.skin_first + k);
#pragma unroll
    for (int v = 0; v < 3; v++) {
        V3 p = v3(x[3 * v], x[3 * v + 1], x[3 * v + 2]);
        V3 n = v3(x[9 + 3 * v], x[9 + 3 * v + 1], x[9 + 3 * v + 2]);
        if (j.active_count != 0u) {
            const float len = length(n);
            if (len == 0.0f || !(len <= 3.402823466e+38f)) n = v3(m[9 + 3 * v], m[9 + 3 * v + 1], m[9 + 3 * v + 2]);
            else n = n * (1.0f / len);
        }
        if (skinned) {
            const SkinVertexDevice c = sv[v];
            skin_corner(pal, c, p, n, &p, &n);
        }
        store_corner(out, v, p, n);
    }
    copy_uvs(out, m);
}

void launch_skin(const SkinJob* jobs, const uint32_t* job_start, uint32_t n_jobs, uint32_t padded_total, const float* bind, const void* corners,
                 const float* palettes, float* posed, hipStream_t s) {
    if (n_jobs && padded_total)
        ST_KLAUNCH(k_skin, dim3(padded_total / kSkinBlock), dim3(kSkinBlock), s, jobs, job_start, n_jobs, bind, static_cast<const SkinVertexDevice*>(corners), palettes, posed);
}

void launch_morph(const MorphJob* jobs, const uint32_t* job_start, uint32_t n_jobs, uint32_t padded_total, const float* bind, const void* corners,
                  const float* palettes, const float* targets, const MorphActive* active, float* posed, hipStream_t s) {
    if (n_jobs && padded_total)
        ST_KLAUNCH(k_morph, dim3(padded_total / kSkinBlock), dim3(kSkinBlock), s, jobs, job_start, n_jobs, bind, static_cast<const SkinVertexDevice*>(corners), palettes, targets, active, posed);
}

}  // namespace st
