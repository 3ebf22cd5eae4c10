// st_output_chain.h — what the nodes of the HDR output chain (fog, light shafts, depth of field, motion blur, bloom: st_fog.cpp, st_shafts.cpp,
// st_dof.cpp, st_motion_blur.cpp, st_bloom.cpp) and post-processing share on the host: the shape of a camera's setting, where a node reads
// and writes, what a launch is credited, and the checks and host constants more than one of them needs. Included by st_engine.h (it uses
// FencedPlanes, fail and format_bytes); the table that orders the nodes within a frame is st_render.cpp's.
#pragma once
#include <cfloat>

namespace st {

constexpr uint32_t kMaxImageSide = 16384u;   // of a frame, and of an image a stateless call takes

// Why a node cannot serve a camera that renders a window of its frame. The node's setter and st_camera_set_window state the same rule:
//   "<node> on a camera with a window<why>"   /   "a window on a camera with <node><why>"
struct WindowRule { const char* node; const char* why; };
inline std::string refuses_window(const WindowRule& r) { return std::string(r.node) + " on a camera with a window" + r.why; }
inline std::string window_refused_by(const WindowRule& r) { return std::string("a window on a camera with ") + r.node + r.why; }
constexpr WindowRule kPostWindow{"post-processing", ": FXAA and the resampler read across tile edges (include/strolle_hip.h \"post-processing\")"};
constexpr WindowRule kUpscaleWindow{"upscaling", ": both steps read across tile edges (include/strolle_hip.h \"upscaling\")"};
constexpr WindowRule kBloomWindow{"bloom", ": the pyramid reads far across tile edges (include/strolle_hip.h \"bloom\")"};
constexpr WindowRule kLensWindow{"lens effects", ": distortion and fringing read far across tile edges (include/strolle_hip.h \"lens effects\")"};
constexpr WindowRule kMBlurWindow{"motion blur", ": the gather reads up to 32 pixels across tile edges (include/strolle_hip.h \"motion blur\")"};
constexpr WindowRule kDofWindow{"depth of field", ": the gather reads up to 32 pixels across tile edges (include/strolle_hip.h \"depth of field\")"};
constexpr WindowRule kShaftsWindow{"light shafts", ": the apply launch reads neighbouring cells across tile edges (include/strolle_hip.h \"light shafts\")"};

// Why upscaling cannot serve a camera whose post-processing resizes, stated alike by st_camera_set_upscale and st_camera_set_post
constexpr const char* kOneResizeWhy = ": one stage owns the resize (include/strolle_hip.h \"upscaling\")";
inline std::string upscale_refuses_resize() { return std::string("upscaling on a camera with post-processing that resizes") + kOneResizeWhy; }
inline std::string resize_refused_by_upscale() { return std::string("post-processing that resizes on a camera with upscaling") + kOneResizeWhy; }

// A camera's setting of one stage of the output chain: the last descriptor set, whether it is on, and the scratch planes its frames use
// (plane[0] of an HDR node: the render-size RGBA32F plane it reads). It survives st_camera_update; the planes are made by the first frame
// that needs them, and their fence is recorded behind each frame's launches of the stage. `window`: null for a stage that honours windows.
template <class Desc, int N> struct NodeSetting {
    Desc desc{}; bool on = false; FencedPlanes<N> planes; const WindowRule* window;
    explicit NodeSetting(const WindowRule* w) : window(w) {}
};
// The setters' skeleton: null means off; `check`; a windowed camera is refused by the stage's rule; the descriptor is copied (the caller zeroes its pads)
template <class Desc, int N, class Check> int set_node(bool windowed, NodeSetting<Desc, N>& s, const Desc* desc, Check check) {
    if (!desc) { s.on = false; return ST_OK; }
    if (int rc = check(*desc)) return rc;
    if (s.window && windowed) return fail(ST_ERR_INVALID_ARGUMENT, refuses_window(*s.window));
    s.desc = *desc; s.on = true;
    return ST_OK;
}

// Where a node writes: the RGBA32F plane the next HDR node reads, untransformed (`raw`), or the frame's (the call's) target in `format`
// through `display`.
struct NodeTarget { void* dst; uint32_t format; bool raw; DisplayArgs display; };
template <class Args> void apply_target(const NodeTarget& t, Args& a) {
    a.dst = t.dst; a.format = t.raw ? (uint32_t)ST_FORMAT_RGBA32F : t.format; a.raw = t.raw ? 1u : 0u; a.display = t.display;
}
// What a node reads. `frame`: depth is PRIM_GBUFFER_D0 (float4, x; 0 = sky) and velocity the velocity map (float4, xy); otherwise a float
// and a float2 plane. velocity: motion blur's alone.
struct NodeSource { const void* color; const void* depth; const void* velocity; bool frame; uint32_t w, h; };
// The camera the image was rendered with (16 floats each, column major) and the engine's sun direction, for the descriptors that follow it
struct NodeView { const float* transform; const float* projection; const float* sun; };
template <class Args> void apply_projection(const float* p, Args& a) { a.p0 = p[0]; a.p5 = p[5]; a.p8 = p[8]; a.p9 = p[9]; }   // the view-space slopes of a pixel's ray
template <class Args> void apply_axes(const float* m, Args& a) { for (int i = 0; i < 3; i++) { a.m0[i] = m[i]; a.m1[i] = m[4 + i]; a.m2[i] = m[8 + i]; } }
// One launch of a node: its kernel slot and the compulsory bytes it is credited
struct OutputStep { int slot; double bytes; };

inline bool finite(float x) { return x >= -FLT_MAX && x <= FLT_MAX; }
inline bool finite_not_negative(float x) { return x >= 0.0f && x <= FLT_MAX; }
inline bool positive_finite(float x) { return x > 0.0f && x <= FLT_MAX; }
inline bool finite_direction(const float* v) { return finite(v[0]) && finite(v[1]) && finite(v[2]) && !(v[0] == 0.0f && v[1] == 0.0f && v[2] == 0.0f); }
// v / |v| in double, rounded once; false (and `out` untouched) for a vector of length 0
inline bool unit_direction(const float* v, float out[3]) {
    const double x = (double)v[0], y = (double)v[1], z = (double)v[2], len = std::sqrt(x * x + y * y + z * z);
    if (!(len > 0.0)) return false;
    out[0] = (float)(x / len); out[1] = (float)(y / len); out[2] = (float)(z / len);
    return true;
}

int check_display(const StDisplayDesc& d);   // st_display.cpp: the setter's checks
// The stateless calls' common ending of their checks (st_display.cpp): the optional manual display, then the output format -> where `call` writes
int process_target(const char* call, const StDisplayDesc* display, void* dst, int format, NodeTarget& out);

}  // namespace st
