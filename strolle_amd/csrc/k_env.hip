// k_env.hip — environment lighting (include/strolle_hip.h "environment lighting"; st_env.cpp): the upload of a map from device memory, the
// luminance grid its importance table is built from, and the debug seams that run the kernels' own look-up and sampling functions
// (st_device.h env_eval / env_pdf / env_sample).
#include "k_common.h"

namespace st {
namespace ST_KNS {

// A channel that is NaN, +-inf or negative becomes 0; `bad` counts the texels that had one (integer atomics only).
__global__ void k_env_upload(const unsigned char* src, size_t pitch, uint32_t w, uint32_t h, uint32_t channels, float4* texels, uint32_t* bad) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= w || y >= h) return;
    const float* p = reinterpret_cast<const float*>(src + (size_t)y * pitch) + (size_t)x * channels;
    float c[3];
    bool sanitised = false;
    for (int k = 0; k < 3; k++) {
        const float v = p[k];
        const bool ok = v >= 0.0f && v <= 3.402823466e38f;
        c[k] = ok ? v : 0.0f;
        sanitised |= !ok;
    }
    texels[(size_t)y * w + x] = make_float4(c[0], c[1], c[2], 0.0f);
    if (sanitised) atomicAdd(bad, 1u);
}
void launch_env_upload(const void* src, size_t pitch, uint32_t w, uint32_t h, uint32_t channels, float4* texels, uint32_t* bad, hipStream_t s) {
    if (!w || !h) return;
    ST_KLAUNCH(k_env_upload, dim3((w + 255u) / 256u, h), dim3(256), s, static_cast<const unsigned char*>(src), pitch, w, h, channels, texels, bad);
}

// One thread per cell of the gw x gh grid: the Rec. 709 luminance of the cell's texel average times sin theta of the cell's centre. The
// sum runs in a fixed order (no atomics): the grid, and the table built from it, are the same bits on every run.
__global__ void k_env_grid(const float4* texels, uint32_t w, uint32_t h, uint32_t gw, uint32_t gh, float* weights) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= gw * gh) return;
    const uint32_t cy = i / gw, cx = i - cy * gw;
    const uint32_t x0 = (uint32_t)((uint64_t)cx * w / gw), x1 = (uint32_t)((uint64_t)(cx + 1u) * w / gw);
    const uint32_t y0 = (uint32_t)((uint64_t)cy * h / gh), y1 = (uint32_t)((uint64_t)(cy + 1u) * h / gh);
    float r = 0.0f, g = 0.0f, b = 0.0f;
    for (uint32_t y = y0; y < y1; y++)
        for (uint32_t x = x0; x < x1; x++) { const float4 t = texels[(size_t)y * w + x]; r += t.x; g += t.y; b += t.z; }
    const float n = (float)((x1 - x0) * (y1 - y0));
    const float lum = fdiv(0.2126f * r + 0.7152f * g + 0.0722f * b, n);
    weights[i] = lum * sin_(kPi * fdiv((float)cy + 0.5f, (float)gh));
}
void launch_env_grid(const float4* texels, uint32_t w, uint32_t h, uint32_t gw, uint32_t gh, float* weights, hipStream_t s) {
    ST_KLAUNCH(k_env_grid, dim3((gw * gh + 255u) / 256u), dim3(256), s, texels, w, h, gw, gh, weights);
}

// what = 0: in = n directions (xyz) -> out = n rgb; 1: in = n uniform triples -> out = n (xyz, pdf); 2: in = n directions -> out = n pdfs
__global__ void k_env_debug(const KArgs a, uint32_t what, const float* in, uint32_t n, float* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (what == 1u) {
        const EnvSample s = env_sample(a, in[3u * i], in[3u * i + 1u], in[3u * i + 2u]);
        out[4u * i] = s.dir.x; out[4u * i + 1u] = s.dir.y; out[4u * i + 2u] = s.dir.z; out[4u * i + 3u] = s.pdf;
        return;
    }
    const V3 d = v3(in[3u * i], in[3u * i + 1u], in[3u * i + 2u]);
    if (what == 0u) { const V3 c = env_eval(a, d); out[3u * i] = c.x; out[3u * i + 1u] = c.y; out[3u * i + 2u] = c.z; }
    else out[i] = env_pdf(a, d);
}
void launch_env_debug(const KArgs& a, uint32_t what, const float* in, uint32_t n, float* out, hipStream_t s) {
    if (!n) return;
    ST_KLAUNCH(k_env_debug, dim3((n + 255u) / 256u), dim3(256), s, a, what, in, n, out);
}

}  // namespace ST_KNS
}  // namespace st
