// k_display.hip — camera display transforms (include/strolle_hip.h "display transforms"; st_display.cpp): the camera's device exposure
// state. The composing launches (k_trace.hip k_composition<true>, k_denoise.hip k_denoise_wavelet_far<true, true>) meter the frame into
// its histogram; the finalize kernel here runs behind them on the same stream and turns the histogram into the next frame's scale. No
// host sync, no read-back.
// Layout of the state (kDisplayBytes): hist[kDisplayReplicas][64] (what the composing launches add to, workgroup b to replica b % 64),
// last[64] (the last finalized frame's histogram, for st_debug_camera_histogram), then DisplayState.
#include "k_common.h"

namespace st {
namespace ST_KNS {

ST_D DisplayState* display_state(void* base) { return reinterpret_cast<DisplayState*>(static_cast<char*>(base) + kDisplayStateOffset); }

// st_camera_set_display turned auto-exposure on: the first frame uses `scale` (2^exposure_ev), the adaptation starts from `adapted_ev`
// (log2 0.18) and the first metered frame is taken as it is
__global__ void k_display_reset(void* base, float scale, float adapted_ev) {
    uint32_t* hist = static_cast<uint32_t*>(base);
    const uint32_t t = threadIdx.x;
    for (uint32_t r = 0; r <= kDisplayReplicas; r++) hist[r * kDisplayBins + t] = 0u;   // the replicas and `last`
    if (t == 0u) {
        DisplayState* st = display_state(base);
        st->scale = scale; st->metered_ev = __builtin_nanf(""); st->adapted_ev = adapted_ev; st->primed = 0u; st->frames = 0u;
    }
}
void launch_display_reset(void* state, float scale, float adapted_ev, hipStream_t s) {
    hipLaunchKernelGGL(k_display_reset, dim3(1), dim3(kDisplayBins), 0, s, state, scale, adapted_ev);
}

// One workgroup of 64 lanes, one bin each. With N metered pixels sorted by bin, the ranks [floor(low N), ceil(high N)) are kept (a bin at
// either end only in part); metered_ev = the count-weighted mean of the kept bins' centres (double). adapted_ev moves to it by at most the
// step limits (0 = none); the next frame's scale = 0.18 * 2^(compensation - adapted_ev), in float. Nothing kept: the state stays.
__global__ void k_display_finalize(void* base, float ev_min, float ev_max, float low, float high, float step_up, float step_down, float compensation) {
    __shared__ uint32_t s_count[kDisplayBins];
    uint32_t* hist = static_cast<uint32_t*>(base);
    const uint32_t t = threadIdx.x;
    uint32_t n = 0u;
    for (uint32_t r = 0; r < kDisplayReplicas; r++) { n += hist[r * kDisplayBins + t]; hist[r * kDisplayBins + t] = 0u; }   // (the next frame's composing launch comes after this kernel in stream order)
    s_count[t] = n;
    hist[kDisplayReplicas * kDisplayBins + t] = n;
    __syncthreads();
    if (t != 0u) return;
    uint64_t total = 0u;
    for (uint32_t k = 0; k < kDisplayBins; k++) total += s_count[k];
    const uint64_t lo = (uint64_t)floor((double)low * (double)total), hi = (uint64_t)ceil((double)high * (double)total);
    const double width = ((double)ev_max - (double)ev_min) / (double)kDisplayBins;
    uint64_t cum = 0u, kept = 0u;
    double sum = 0.0;
    for (uint32_t k = 0; k < kDisplayBins; k++) {
        const uint64_t b0 = cum, b1 = cum + s_count[k];
        cum = b1;
        const uint64_t k0 = b0 > lo ? b0 : lo, k1 = b1 < hi ? b1 : hi;
        if (k1 <= k0) continue;
        kept += k1 - k0;
        sum += (double)(k1 - k0) * ((double)ev_min + ((double)k + 0.5) * width);
    }
    DisplayState* st = display_state(base);
    if (kept == 0u) return;
    const float metered = (float)(sum / (double)kept);
    float adapted = st->adapted_ev;
    if (st->primed == 0u) adapted = metered;
    else if (step_up > 0.0f && metered - adapted > step_up) adapted = adapted + step_up;
    else if (step_down > 0.0f && adapted - metered > step_down) adapted = adapted - step_down;
    else adapted = metered;
    st->metered_ev = metered; st->adapted_ev = adapted; st->primed = 1u; st->frames = st->frames + 1u;
    st->scale = 0.18f * exp2f(compensation - adapted);
}
void launch_display_finalize(void* state, float ev_min, float ev_max, float low_fraction, float high_fraction, float step_up, float step_down, float compensation_ev,
                             hipStream_t s) {
    hipLaunchKernelGGL(k_display_finalize, dim3(1), dim3(kDisplayBins), 0, s, state, ev_min, ev_max, low_fraction, high_fraction, step_up, step_down, compensation_ev);
}

}  // namespace ST_KNS
}  // namespace st
