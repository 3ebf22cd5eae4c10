// st_display.cpp — camera display transforms (include/strolle_hip.h "display transforms"): the setter's checks, the per-frame DisplayArgs
// and the order of the camera's device exposure state (k_display.hip) across frames and streams. See st_engine.h CameraState.
#include <cmath>

#include "st_engine.h"

namespace st {

static constexpr double kMidGrey = 0.18;

int check_display(const StDisplayDesc& d) {
    if (d.struct_size != sizeof(StDisplayDesc)) return fail(ST_ERR_INVALID_ARGUMENT, "StDisplayDesc.struct_size is not sizeof(StDisplayDesc)");
    if (d.tonemap > ST_TONEMAP_PBR_NEUTRAL) return fail(ST_ERR_INVALID_ARGUMENT, "unknown tonemap");
    if ((d.flags & ~(uint32_t)ST_DISPLAY_AUTO_EXPOSURE) != 0u) return fail(ST_ERR_INVALID_ARGUMENT, "unknown display flag bits");
    for (float v : {d.exposure_ev, d.ev_min, d.ev_max, d.low_fraction, d.high_fraction, d.max_ev_step_up, d.max_ev_step_down})
        if (!std::isfinite(v)) return fail(ST_ERR_INVALID_ARGUMENT, "a display field is not finite");
    if (d.flags & ST_DISPLAY_AUTO_EXPOSURE) {
        if (!(d.ev_min < d.ev_max)) return fail(ST_ERR_INVALID_ARGUMENT, "auto-exposure: ev_min must be below ev_max");
        if (!(0.0f <= d.low_fraction && d.low_fraction < d.high_fraction && d.high_fraction <= 1.0f))
            return fail(ST_ERR_INVALID_ARGUMENT, "auto-exposure: fractions must satisfy 0 <= low < high <= 1");
        if (d.max_ev_step_up < 0.0f || d.max_ev_step_down < 0.0f) return fail(ST_ERR_INVALID_ARGUMENT, "auto-exposure: step limits must be >= 0");
    }
    return ST_OK;
}

// no display: NONE at scale 1, which stores the colour's own bits
int process_target(const char* call, const StDisplayDesc* display, void* dst, int format, NodeTarget& out) {
    out = NodeTarget{dst, (uint32_t)format, false, DisplayArgs{}};
    out.display.scale = 1.0f;
    if (display) {
        if (int rc = check_display(*display)) return rc;
        if (display->flags & ST_DISPLAY_AUTO_EXPOSURE) return fail(ST_ERR_INVALID_ARGUMENT, std::string(call) + " takes a manual display: auto-exposure is a camera's state");
        out.display.on = 1u; out.display.tonemap = display->tonemap; out.display.scale = (float)std::exp2((double)display->exposure_ev);
    }
    if (format < ST_FORMAT_RGBA32F || format > ST_FORMAT_BGRA8_UNORM_SRGB) return fail(ST_ERR_INVALID_ARGUMENT, "unknown output format");
    return ST_OK;
}

int Engine::set_display(CameraState& c, const StDisplayDesc* desc) {
    if (!desc) { c.display_on = false; return ST_OK; }
    if (int rc = check_display(*desc)) return rc;
    const bool auto_now = (desc->flags & ST_DISPLAY_AUTO_EXPOSURE) != 0u;
    if (auto_now && c.windowed()) return fail(ST_ERR_INVALID_ARGUMENT, "auto-exposure on a camera with a window would meter the tile alone (include/strolle_hip.h \"display transforms\")");
    if (auto_now && !c.display_auto()) c.display_reset = true;   // off -> on: the adaptation starts over at the next frame
    c.display = *desc; c.display_on = true;
    c.display_scale = (float)std::exp2((double)desc->exposure_ev);
    return ST_OK;
}

// Before the frame's first launch. Heatmap frames are stored as they are.
int Engine::display_begin(CameraState& c, hipStream_t stream, bool heatmap, DisplayArgs& d) {
    d = DisplayArgs{};
    if (!c.display_on || heatmap) return ST_OK;
    d.on = 1u; d.tonemap = c.display.tonemap; d.scale = c.display_scale;
    if (!c.display_auto()) return ST_OK;
    if (!c.display_state.ptr) {
        if (int rc = c.display_state.reserve(kDisplayBytes, kDisplayBytes)) return rc;
        c.display_reset = true;
    }
    // the previous metered frame's finalize ran on another stream: this frame's reads of the state and adds to the histogram come after it
    // (on the same stream they do anyway: no event between the two frames' kernels)
    if (int rc = c.display_done.wait(stream, Fence::OtherStreams, Fence::Keep)) return rc;
    if (c.display_reset) {
        L.launch_display_reset(c.display_state.ptr, c.display_scale, (float)std::log2(kMidGrey), stream);
        c.display_reset = false;
    }
    d.meter = 1u;
    d.state = reinterpret_cast<const float*>(c.display_state.as<const char>() + kDisplayStateOffset);
    d.hist = c.display_state.as<uint32_t>();
    d.ev_min = c.display.ev_min;
    d.bins_per_ev = (float)kDisplayBins / (c.display.ev_max - c.display.ev_min);
    return ST_OK;
}

int Engine::display_finalize(CameraState& c, hipStream_t stream) {
    const StDisplayDesc& s = c.display;
    L.launch_display_finalize(c.display_state.ptr, s.ev_min, s.ev_max, s.low_fraction, s.high_fraction, s.max_ev_step_up, s.max_ev_step_down, s.exposure_ev, stream);
    return c.display_done.record(stream);
}

int Engine::display_exposure(CameraState& c, float* scale, float* metered_ev, float* adapted_ev) {
    if (!has_device) return fail(ST_ERR_NO_DEVICE, "st_camera_exposure on a host-only engine");
    float v[3] = {1.0f, NAN, NAN};
    if (c.display_on) v[0] = c.display_scale;
    if (c.display_auto()) {
        v[2] = (float)std::log2(kMidGrey);
        if (c.display_state.ptr && !c.display_reset) {
            ST_HIP(hipSetDevice(device));
            ST_HIP(hipDeviceSynchronize());
            DisplayState st{};
            ST_HIP(hipMemcpy(&st, c.display_state.as<const char>() + kDisplayStateOffset, sizeof(st), hipMemcpyDeviceToHost));
            v[0] = st.scale; v[1] = st.metered_ev; v[2] = st.adapted_ev;
        }
    }
    if (scale) *scale = v[0];
    if (metered_ev) *metered_ev = v[1];
    if (adapted_ev) *adapted_ev = v[2];
    return ST_OK;
}

int Engine::display_histogram(CameraState& c, uint32_t* bins) {
    if (!has_device) return fail(ST_ERR_NO_DEVICE, "st_debug_camera_histogram on a host-only engine");
    memset(bins, 0, kDisplayBins * sizeof(uint32_t));
    if (!c.display_state.ptr) return ST_OK;
    ST_HIP(hipSetDevice(device));
    ST_HIP(hipDeviceSynchronize());
    ST_HIP(hipMemcpy(bins, c.display_state.as<const char>() + kDisplayLastOffset, kDisplayBins * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return ST_OK;
}

}  // namespace st
