// k_output.h — what the kernels of the HDR output chain and of post-processing (k_fog, k_shafts, k_dof, k_motion_blur, k_bloom, k_post) spell
// alike: the device twins of st_output_chain.h. Include it after k_common.h. Everything is force-inlined float32, left to right, under the
// same contract(off) the including files set for their own arithmetic, so a kernel's code is what it was with its own copy (compared in
// assembly, both builds). display_transform and store_output stay in st_passes.h.
#pragma once
#include "k_common.h"

#pragma clang fp contract(off)

namespace st {

constexpr float kFltMax = 3.402823466e+38f;
constexpr float kColourMax = 65504.0f;   // the largest half: what a colour is held to before a node weighs it

// min / max as include/strolle_hip.h defines them: the first operand unless the second is smaller / larger or NaN
ST_D float out_min(float a, float b) { return (a < b || b != b) ? a : b; }
ST_D float out_max(float a, float b) { return (a > b || b != b) ? a : b; }
ST_D float out_clamp01(float x) { return out_min(out_max(x, 0.0f), 1.0f); }
ST_D int out_clampi(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }
ST_D float out_exp(float x) { return exp2_poly_(x * 1.44269504088896341f); }
ST_D V3 out_colour(float4 c) { return v3(out_min(out_max(c.x, 0.0f), kColourMax), out_min(out_max(c.y, 0.0f), kColourMax), out_min(out_max(c.z, 0.0f), kColourMax)); }

// What k_post.hip and k_upscale.hip both read a display-referred texel and an output pixel's source position with (include/strolle_hip.h
// "post-processing"): the clamp into [0, 1], the integer evaluation of (o + 0.5) n_src / n_dst, the clamp to four texels' min / max
ST_D float post_unit(float x) { return x > 0.0f ? (x < 1.0f ? x : 1.0f) : 0.0f; }   // NaN -> 0
ST_D void post_resample_axis(uint32_t o, uint32_t n_src, uint32_t n_dst, int* i0, float* f) {
    const int n = (int)((2u * o + 1u) * n_src) - (int)n_dst, d = (int)(2u * n_dst);   // n > -d: floor(n / d) is -1 for every negative n
    *i0 = n >= 0 ? n / d : -1;
    *f = (float)(n - *i0 * d) / (float)d;
}
ST_D float post_box(float v, float a, float b, float c, float d) {
    const float lo = out_min(out_min(out_min(a, b), c), d), hi = out_max(out_max(out_max(a, b), c), d);
    return out_min(out_max(v, lo), hi);
}

// D of a pixel: in a frame PRIM_GBUFFER_D0.x alone (4 of the texel's 16 B), 0 (sky) read as FLT_MAX; otherwise the float plane as it is
ST_D float out_frame_depth(const void* depth, size_t at, bool frame) {
    if (frame) { const float d = reinterpret_cast<const float*>(static_cast<const float4*>(depth) + at)[0]; return d == 0.0f ? kFltMax : d; }
    return static_cast<const float*>(depth)[at];
}
// A node's last store: the raw plane, the camera's format, or the format through the display. (Without a display the colour is stored as it
// is, not through display_transform at NONE and scale 1 as the bloom composite does: that path writes alpha 1, and a pixel a node leaves
// alone keeps its own four words, alpha included.)
template <class Args>
ST_D void out_store(const Args& p, size_t at, float4 c) {
    if (p.raw) static_cast<float4*>(p.dst)[at] = c;
    else if (!p.display.on) store_output(p.dst, (uint32_t)at, c, p.format);
    else store_output(p.dst, (uint32_t)at, display_transform(c, p.display.tonemap, display_scale(p.display)), p.format);
}

}  // namespace st
