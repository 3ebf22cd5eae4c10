// k_skin.hip — linear blend skinning of posed instances on the device (include/strolle_hip.h "skinned meshes"; st_skin.cpp).
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

__global__ __launch_bounds__(kSkinBlock) void k_skin(const SkinJob* jobs, const uint32_t* job_start, uint32_t n_jobs, const float* bind,
                                                     const SkinVertexDevice* corners, const float* palettes, float* posed) {
    __shared__ float pal[kSkinMaxJoints * 12u];
    const uint32_t first = blockIdx.x * kSkinBlock;
    uint32_t lo = 0u, hi = n_jobs;          // the job whose padded [job_start[j], job_start[j + 1]) holds this workgroup
    while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (job_start[mid] <= first) lo = mid; else hi = mid; }
    const SkinJob j = jobs[lo];
    const float* src = palettes + 12u * (size_t)j.palette_first;
    for (uint32_t i = threadIdx.x; i < 12u * j.joint_count; i += kSkinBlock) pal[i] = src[i];
    __syncthreads();
    const uint32_t k = first - job_start[lo] + threadIdx.x;
    if (k >= j.count) return;
    const float* m = bind + 24u * (size_t)(j.skin_first + k);
    const SkinVertexDevice* sv = corners + 3u * (size_t)(j.skin_first + k);
    float* out = posed + 24u * (size_t)(j.posed_first + k);
#pragma unroll
    for (int v = 0; v < 3; v++) {
        const SkinVertexDevice c = sv[v];
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
        const V3 q = v3(m[3 * v], m[3 * v + 1], m[3 * v + 2]);
        const V3 p = ((ax * q.x) + (ay * q.y) + (az * q.z)) + at;
        const V3 nn = v3(m[9 + 3 * v], m[9 + 3 * v + 1], m[9 + 3 * v + 2]);
        const V3 c0 = cross(ay, az), c1 = cross(az, ax), c2 = cross(ax, ay);
        const float det = dot(az, c2);
        V3 n = nn;
        if (det != 0.0f) {
            V3 acc = (c0 / det) * nn.x; acc = acc + (c1 / det) * nn.y; acc = acc + (c2 / det) * nn.z;
            n = normalize(acc);
        }
        out[3 * v] = p.x; out[3 * v + 1] = p.y; out[3 * v + 2] = p.z;
        out[9 + 3 * v] = n.x; out[9 + 3 * v + 1] = n.y; out[9 + 3 * v + 2] = n.z;
    }
#pragma unroll
    for (int u = 0; u < 6; u++) out[18 + u] = m[18 + u];
}

void launch_skin(const SkinJob* jobs, const uint32_t* job_start, uint32_t n_jobs, uint32_t padded_total, const float* bind, const void* corners,
                 const float* palettes, float* posed, hipStream_t s) {
    if (n_jobs && padded_total)
        ST_KLAUNCH(k_skin, dim3(padded_total / kSkinBlock), dim3(kSkinBlock), s, jobs, job_start, n_jobs, bind, static_cast<const SkinVertexDevice*>(corners), palettes, posed);
}

}  // namespace st
