// st_engine.h — the host engine of libstrolle_hip.so: state and interfaces shared by its translation units
//   st_engine.cpp       construction, tuning (StTuning + environment), destruction
//   st_scene.cpp        the scene stores (st_stores.h): lights, materials, the image atlas, meshes, instances, triangle slots; the tick's phases that connect them (baking)
//   st_bvh_refresh.cpp  the scene's BVH (st_bvh_refresh.h): the host's tree and its streams, refits, the wide topology, the device builder's input, the tick's tree plan
//   st_tick.cpp         Engine::tick: refresh of the stores + uploads (page-locked staging); the tick's device copies (st_copies.h): double-buffered scene / light copies, their readers, retirement
//   st_render.cpp       per-camera buffers and Engine::render: the per-frame pass graph in phases, on two HIP streams; present hand-over
//   st_display.cpp      display transforms: exposure, tone mapping, the auto-exposure state
//   st_post.cpp         output post-processing: FXAA and the resampler
//   st_upscale.cpp      the upscale stage behind FXAA: the edge-adaptive upscaler and the sharpening step
//   st_bloom.cpp        bloom: the plan, the chain of launches
//   st_motion_blur.cpp  motion blur: the plan, its three launches
//   st_dof.cpp          depth of field: the plan (host constants, tap table), its three launches
//   st_fog.cpp          fog: the checks, the host constants, its one launch
//   st_shafts.cpp       light shafts: the checks, the plan, the host constants, its two launches
//   st_deform.cpp       mesh deformation (st_deform.h): skinned meshes, morph targets, deformation motion; the tick's launches
//   st_env.cpp          environment lighting: the map, its importance table
//   st_query.cpp        scene queries: closest hit, occlusion, picks
//   st_aov.cpp          per-pixel AOVs
//   st_gltf.cpp         scene ingest: glTF 2.0 (.gltf / .glb), image decoding
//   st_dist.cpp         multi-GPU: partitions, transport, gather
//   st_profile.cpp      per-kernel event timing
//   st_abi.cpp          the C ABI (include/strolle_hip.h)
// Behavioural contract: strolle/src/lib.rs (Engine), camera_controller.rs (pass order), lights.rs / materials.rs /
// instances.rs / triangles.rs (stores), camera.rs (camera uniform). The wgpu plumbing of the reference (bind groups, mapped
// buffers, textures) is replaced by plain device allocations and pointer swaps.
// Ownership: every device allocation, event, stream and page-locked buffer of the host engine is a member of a move-only type that frees it
// in its destructor (DeviceArray, Event, Stream, PinnedBuffer, below) — teardown lists nothing. A destructor runs with whatever device is
// current, so whoever lets one of them go first makes the engine's device current and, where work may still use the resource, joins it
// (~Engine, st_camera_delete, st_camera_update; st_tick for everything a tick replaces: st_copies.h CopyPair, Retired). st_dist.cpp keeps its own protocol.
// Stream order between users of one resource on different streams is a Fence (below): record / record_chained behind the users, wait
// (from any stream or only from other streams than the recorder; keeping or clearing the recording), host_wait, poll, settled.
#pragma once
#include <algorithm>
#include <cstdio>
#include <chrono>
#include <cmath>
#include <cstring>
#include <initializer_list>
#include <map>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/strolle_hip.h"
#include "st_lbvh.h"
#include "st_atlas.h"
#include "st_bvh.h"
#include "st_kernels.h"
#include "st_ranges.h"

#include <thread>

namespace st {

extern thread_local std::string g_last_error;  // st_engine.cpp
inline int fail(int status, const std::string& msg) { g_last_error = msg; return status; }
// StTuning::tick_timing's clock: the milliseconds between two readings of TickClock::now()
using TickClock = std::chrono::steady_clock;
inline double ms_between(TickClock::time_point a, TickClock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

#define ST_HIP(call)                                                                                      \
    do {                                                                                                  \
        hipError_t err_ = (call);                                                                         \
        if (err_ != hipSuccess) return fail(ST_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(err_)); \
    } while (0)

// ------------------------------------------------------------------ host maths (glam order; see st_math.h)
inline M4 m4_from_cols(const float* a) { M4 m; for (int i = 0; i < 4; i++) m.c[i] = make_float4(a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3]); return m; }
inline M4 m4_mul(const M4& a, const M4& b) { M4 r; for (int i = 0; i < 4; i++) r.c[i] = mul(a, b.c[i]); return r; }
inline M4 m4_inverse(const M4& m) {  // glam 0.24 Mat4::inverse, scalar path
    const float m00 = m.c[0].x, m01 = m.c[0].y, m02 = m.c[0].z, m03 = m.c[0].w;
    const float m10 = m.c[1].x, m11 = m.c[1].y, m12 = m.c[1].z, m13 = m.c[1].w;
    const float m20 = m.c[2].x, m21 = m.c[2].y, m22 = m.c[2].z, m23 = m.c[2].w;
    const float m30 = m.c[3].x, m31 = m.c[3].y, m32 = m.c[3].z, m33 = m.c[3].w;
    const float c00 = m22 * m33 - m32 * m23, c02 = m12 * m33 - m32 * m13, c03 = m12 * m23 - m22 * m13;
    const float c04 = m21 * m33 - m31 * m23, c06 = m11 * m33 - m31 * m13, c07 = m11 * m23 - m21 * m13;
    const float c08 = m21 * m32 - m31 * m22, c10 = m11 * m32 - m31 * m12, c11 = m11 * m22 - m21 * m12;
    const float c12 = m20 * m33 - m30 * m23, c14 = m10 * m33 - m30 * m13, c15 = m10 * m23 - m20 * m13;
    const float c16 = m20 * m32 - m30 * m22, c18 = m10 * m32 - m30 * m12, c19 = m10 * m22 - m20 * m12;
    const float c20 = m20 * m31 - m30 * m21, c22 = m10 * m31 - m30 * m11, c23 = m10 * m21 - m20 * m11;
    const float4 f0 = make_float4(c00, c00, c02, c03), f1 = make_float4(c04, c04, c06, c07), f2 = make_float4(c08, c08, c10, c11);
    const float4 f3 = make_float4(c12, c12, c14, c15), f4_ = make_float4(c16, c16, c18, c19), f5 = make_float4(c20, c20, c22, c23);
    const float4 v0 = make_float4(m10, m00, m00, m00), v1 = make_float4(m11, m01, m01, m01), v2_ = make_float4(m12, m02, m02, m02), v3_ = make_float4(m13, m03, m03, m03);
    const float4 i0 = (v1 * f0 - v2_ * f1) + v3_ * f2;
    const float4 i1 = (v0 * f0 - v2_ * f3) + v3_ * f4_;
    const float4 i2_ = (v0 * f1 - v1 * f3) + v3_ * f5;
    const float4 i3 = (v0 * f2 - v1 * f4_) + v2_ * f5;
    const float4 sa = make_float4(1.0f, -1.0f, 1.0f, -1.0f), sb = make_float4(-1.0f, 1.0f, -1.0f, 1.0f);
    M4 inv;
    inv.c[0] = i0 * sa; inv.c[1] = i1 * sb; inv.c[2] = i2_ * sa; inv.c[3] = i3 * sb;
    const float4 col0 = make_float4(inv.c[0].x, inv.c[1].x, inv.c[2].x, inv.c[3].x);
    const float4 d0 = m.c[0] * col0;
    const float det = d0.x + d0.y + d0.z + d0.w;
    const float rcp = 1.0f / det;
    for (int i = 0; i < 4; i++) inv.c[i] = inv.c[i] * rcp;
    return inv;
}
struct Affine { V3 x, y, z, t; };
inline Affine affine_from12(const float* a) { Affine r; r.x = v3(a[0], a[1], a[2]); r.y = v3(a[3], a[4], a[5]); r.z = v3(a[6], a[7], a[8]); r.t = v3(a[9], a[10], a[11]); return r; }
inline V3 affine_vec(const Affine& a, V3 v) { V3 r = a.x * v.x; r = r + a.y * v.y; r = r + a.z * v.z; return r; }
inline V3 affine_point(const Affine& a, V3 p) { return ((a.x * p.x) + (a.y * p.y) + (a.z * p.z)) + a.t; }
inline Affine affine_inverse(const Affine& a) {  // glam Affine3A::inverse
    const V3 t0 = cross(a.y, a.z), t1 = cross(a.z, a.x), t2 = cross(a.x, a.y);
    const float det = dot(a.z, t2);
    const float inv_det = 1.0f / det;
    const V3 c0 = t0 * inv_det, c1 = t1 * inv_det, c2 = t2 * inv_det;
    Affine r;
    r.x = v3(c0.x, c1.x, c2.x); r.y = v3(c0.y, c1.y, c2.y); r.z = v3(c0.z, c1.z, c2.z);
    r.t = -affine_vec(r, a.t);
    return r;
}

// per-pass seeds (NEW seam): the same definition is stated in DESIGN.md
inline uint32_t seed_hash(uint32_t v) {
    v = v * 747796405u + 2891336453u;
    const uint32_t w = ((v >> ((v >> 28) + 4u)) ^ v) * 277803737u;
    return (w >> 22) ^ w;
}
inline uint32_t pass_seed(uint64_t base, uint32_t frame, uint32_t pass_id) {
    return seed_hash((uint32_t)base ^ seed_hash((uint32_t)(base >> 32) ^ seed_hash(frame ^ seed_hash(pass_id))));
}
enum PassSeedId { SEED_DI_SAMPLING = 1, SEED_DI_TEMPORAL = 2, SEED_DI_SPATIAL_PICK = 3, SEED_DI_SPATIAL_SAMPLE = 5, SEED_GI_SAMPLING_A = 8,
                  SEED_GI_SAMPLING_B = 9, SEED_GI_TEMPORAL = 10, SEED_GI_SPATIAL_PICK = 11, SEED_GI_SPATIAL_SAMPLE = 13, SEED_GI_PREVIEW = 14,
                  SEED_REF_SHADING = 200 };

// sun light colour: atmosphere/generate_transmittance_lut.rs:32-59 evaluated on the host (lights.rs:80-95)
inline V3 sun_transmittance(V3 pos, V3 sun_dir) {
    auto sphere = [&](float radius) {
        const float b = dot(pos, sun_dir), c = dot(pos, pos) - radius * radius;
        if (c > 0.0f && b > 0.0f) return -1.0f;
        const float discr = b * b - c;
        if (discr < 0.0f) return -1.0f;
        return discr > b * b ? -b + sqrtf(discr) : -b - sqrtf(discr);
    };
    if (sphere(6.360f) > 0.0f) return v3s(0.0f);
    const float atmosphere_distance = sphere(6.460f);
    float t = 0.0f, i = 0.0f;
    V3 transmittance = v3s(1.0f);
    while (i < 40.0f) {
        const float new_t = ((i + 0.3f) / 40.0f) * atmosphere_distance;
        const float dt = new_t - t;
        t = new_t;
        const V3 new_pos = pos + t * sun_dir;
        const float altitude_km = (length(new_pos) - 6.360f) * 1000.0f;
        const float rayleigh_density = exp_(-altitude_km / 8.0f), mie_density = exp_(-altitude_km / 1.2f);
        const V3 rayleigh_scattering = v3(5.802f, 13.558f, 33.1f) * rayleigh_density;
        const float rayleigh_absorption = 0.0f;  // RAYLEIGH_ABSORPTION_BASE (0.0) * density, folded: 0 * inf must not poison the LUT (DESIGN.md deviation 9)
        const float mie_scattering = 3.996f * mie_density, mie_absorption = 4.4f * mie_density;
        const V3 ozone_absorption = v3(0.650f, 1.881f, 0.085f) * fmax_(1.0f - fabsf(altitude_km - 25.0f) / 15.0f, 0.0f);
        const V3 extinction = rayleigh_scattering + v3s(rayleigh_absorption) + v3s(mie_scattering) + v3s(mie_absorption) + ozone_absorption;
        const V3 arg = -dt * extinction;
        transmittance = transmittance * v3(exp_(arg.x), exp_(arg.y), exp_(arg.z));
        i += 1.0f;
    }
    return transmittance;
}

// ------------------------------------------------------------------ small containers
// The device's object-space triangle (mesh store, bind store, posed store): positions 9, normals 9, uvs 6
constexpr size_t kTriangleFloats = 24u;
inline void pack_triangle(const StMeshTriangle& t, float* f) { memcpy(f, t.positions, 9 * sizeof(float)); memcpy(f + 9, t.normals, 9 * sizeof(float)); memcpy(f + 18, t.uvs, 6 * sizeof(float)); }
inline void unpack_triangle(const float* f, StMeshTriangle& t) { memcpy(t.positions, f, 9 * sizeof(float)); memcpy(t.normals, f + 9, 9 * sizeof(float)); memcpy(t.uvs, f + 18, 6 * sizeof(float)); }   // (tangents stay)

// ------------------------------------------------------------------ owners of HIP resources (the rule: this file's header comment)
// Each is move-only (a declared move makes a copy a compile error) and lets go in its destructor; `h` / `ptr` stay readable for the calls that use them.
struct Event {   // made by its first recording, without timing unless told otherwise (the profiler's are timed)
    hipEvent_t h = nullptr; unsigned flags = hipEventDisableTiming;
    Event() = default;
    explicit Event(unsigned f) : flags(f) {}
    Event(Event&& o) noexcept : h(o.h), flags(o.flags) { o.h = nullptr; }
    Event& operator=(Event&& o) noexcept { std::swap(h, o.h); std::swap(flags, o.flags); return *this; }
    ~Event() { reset(); }
    void reset() { if (h) (void)hipEventDestroy(h); h = nullptr; }
    hipEvent_t get() { if (!h) (void)hipEventCreateWithFlags(&h, flags); return h; }
    int record(hipStream_t s) { if (!h) ST_HIP(hipEventCreateWithFlags(&h, flags)); ST_HIP(hipEventRecord(h, s)); return ST_OK; }
    int wait(hipStream_t s) const { if (h) ST_HIP(hipStreamWaitEvent(s, h, 0)); return ST_OK; }   // (never recorded: nothing to wait for)
};
struct Stream {   // created where it is first needed — flags and priority are that site's business — and used as the handle it converts to
    hipStream_t h = nullptr;
    Stream() = default;
    Stream(Stream&& o) noexcept : h(o.h) { o.h = nullptr; }
    Stream& operator=(Stream&& o) noexcept { std::swap(h, o.h); return *this; }
    ~Stream() { reset(); }
    void reset() { if (h) (void)hipStreamDestroy(h); h = nullptr; }   // destroys only: a site that must drain it first says so
    operator hipStream_t() const { return h; }
};
struct PinnedBuffer {   // page-locked host memory
    void* ptr = nullptr; size_t capacity = 0;
    PinnedBuffer() = default;
    PinnedBuffer(PinnedBuffer&& o) noexcept : ptr(o.ptr), capacity(o.capacity) { o.ptr = nullptr; o.capacity = 0; }
    PinnedBuffer& operator=(PinnedBuffer&& o) noexcept { std::swap(ptr, o.ptr); std::swap(capacity, o.capacity); return *this; }
    ~PinnedBuffer() { release(); }
    // room for `bytes`: a smaller buffer is replaced by one of exactly that size (what it held is not kept)
    int reserve(size_t bytes, unsigned flags = hipHostMallocDefault) {
        if (bytes <= capacity) return ST_OK;
        release();
        ST_HIP(hipHostMalloc(&ptr, bytes, flags)); capacity = bytes;
        return ST_OK;
    }
    void release() { if (ptr) (void)hipHostFree(ptr); ptr = nullptr; capacity = 0; }
};

// "X is in use up to here on stream S; its next user on another stream comes after that": an event, whether a recording may still have to be
// waited for (`pending`), and the stream of the last recording. The sites differ in real ways, so each one names its variant:
//   record(s)            the users of X enqueued on `s` so far end here
//   record_chained(s)    the same, behind a wait for the fence's own earlier recording: one event then covers users on several streams
//   wait(s, from, then)  `s` continues behind the recording. from = OtherStreams skips the wait when `s` itself made the recording (stream order
//                        says as much, and an event between two kernels costs the second one 3-15 us: st_kernels.h); AnyStream queues it
//                        regardless. then = Clear forgets the recording (its one next user, a writer, has waited); Keep leaves it to later waiters.
//   host_wait()          the host waits for it; clears
//   poll()               whether nothing is pending any more; a recording that has completed is cleared (not ready is left in hipGetLastError)
//   settled()            the caller has joined the whole device: nothing is pending (no HIP call)
struct Fence {
    enum From { AnyStream, OtherStreams };
    enum Then { Keep, Clear };
    Event ev; hipStream_t last = nullptr; bool pending = false;
    int record(hipStream_t s) { if (int rc = ev.record(s)) return rc; last = s; pending = true; return ST_OK; }
    int record_chained(hipStream_t s) { if (int rc = wait(s, AnyStream, Keep)) return rc; return record(s); }
    int wait(hipStream_t s, From from, Then then) {
        if (pending && (from == AnyStream || last != s)) ST_HIP(hipStreamWaitEvent(s, ev.h, 0));
        if (then == Clear) pending = false;
        return ST_OK;
    }
    int host_wait() { if (pending) ST_HIP(hipEventSynchronize(ev.h)); pending = false; return ST_OK; }
    bool poll() { if (pending && hipEventQuery(ev.h) == hipSuccess) pending = false; return !pending; }
    void settled() { pending = false; }
};

// Pinned staging for the uploads of st_tick: what a tick sends is copied into one slot of page-locked memory and goes to
// the device from there, so st_tick does not have to wait for the stream before the caller may touch the scene again —
// with a scene that changes every frame the host then runs a frame ahead of the GPU instead of in lock-step with it.
// Three slots: a slot is reused only after the copies issued from it have finished (its fence).
struct StagingRing {
    static constexpr int kSlots = 3;
    static constexpr size_t kMaxSlotBytes = (size_t)256 << 20;  // larger ticks go from pageable memory and join the stream
    struct Slot { PinnedBuffer mem; size_t used = 0; Fence done; };
    Slot slots[kSlots];
    int cur = 0;
    size_t wanted = 0;   // bytes the last tick asked for: the next slot is grown to hold that much
    bool enabled = true;

    void begin_tick() {
        if (!enabled) return;
        cur = (cur + 1) % kSlots;
        Slot& s = slots[cur];
        (void)s.done.host_wait();
        s.used = 0;
        const size_t want = std::min(kMaxSlotBytes, std::max<size_t>(wanted + wanted / 4, (size_t)1 << 20));
        if (s.mem.reserve(want) != ST_OK) (void)hipGetLastError();   // (no slot: this tick's uploads go from pageable memory)
        wanted = 0;
    }
    // a page-locked copy of [src, src + bytes), or nullptr when the slot cannot take it (the caller then uploads from `src`
    // and joins the stream)
    const void* stage(const void* src, size_t bytes) {
        wanted += (bytes + 255) & ~(size_t)255;
        if (!enabled) return nullptr;
        Slot& s = slots[cur];
        const size_t at = (s.used + 255) & ~(size_t)255;
        if (!s.mem.ptr || at + bytes > s.mem.capacity) return nullptr;
        char* to = static_cast<char*>(s.mem.ptr) + at;
        memcpy(to, src, bytes);
        s.used = at + bytes;
        return to;
    }
    int end_tick(hipStream_t stream) {
        if (!enabled) return ST_OK;
        Slot& s = slots[cur];
        return s.used == 0 ? ST_OK : s.done.record(stream);
    }
    ~StagingRing() { for (Slot& s : slots) (void)s.done.host_wait(); }   // a slot's copies end before its memory goes
};

struct DeviceArray {
    void* ptr = nullptr; size_t capacity = 0;
    DeviceArray() = default;
    DeviceArray(DeviceArray&& o) noexcept : ptr(o.ptr), capacity(o.capacity) { o.ptr = nullptr; o.capacity = 0; }
    DeviceArray& operator=(DeviceArray&& o) noexcept { std::swap(ptr, o.ptr); std::swap(capacity, o.capacity); return *this; }
    ~DeviceArray() { release(); }
    template <class T> T* as() const { return static_cast<T*>(ptr); }
    // `pageable` is set when the copy had to be issued straight from `src`: the caller joins the stream before `src` changes
    int upload(const void* src, size_t bytes, hipStream_t stream, StagingRing& ring, bool* pageable) {
        if (int rc = reserve(bytes, std::max<size_t>(bytes * 3 / 2, 4096))) return rc;
        return upload_range(src, 0, bytes, stream, ring, pageable);
    }
    // room for `bytes`: a smaller allocation is replaced by one of `alloc` bytes (what it held is not kept)
    int reserve(size_t bytes, size_t alloc) {
        if (bytes <= capacity) return ST_OK;
        if (ptr) ST_HIP(hipFree(ptr));
        ptr = nullptr; capacity = 0;
        ST_HIP(hipMalloc(&ptr, alloc)); capacity = alloc;
        return ST_OK;
    }
    // part of an array that is already on the device: bytes [offset, offset + bytes) of `base`
    int upload_range(const void* base, size_t offset, size_t bytes, hipStream_t stream, StagingRing& ring, bool* pageable) {
        if (!bytes) return ST_OK;
        const void* src = static_cast<const char*>(base) + offset;
        const void* staged = ring.stage(src, bytes);
        if (!staged) *pageable = true;
        ST_HIP(hipMemcpyAsync(static_cast<char*>(ptr) + offset, staged ? staged : src, bytes, hipMemcpyHostToDevice, stream));
        return ST_OK;
    }
    void release() { if (ptr) (void)hipFree(ptr); ptr = nullptr; capacity = 0; }
};
// Scratch planes one frame (or call) writes and the launches behind it read, with the Fence of those last readers: N planes used together share one fence.
template <int N> struct FencedPlanes {
    enum Fit { Exact /* replaced whenever the size differs: it shrinks too */, Grow /* replaced only by a larger one */ };
    DeviceArray plane[N]; Fence read;
    // Plane i at bytes[i] (0: not needed now, it stays as it is), and `stream` ordered behind the last readers on other streams (on the same stream the next writer follows
    // them anyway: no event between two frames' kernels). A plane is replaced with the whole device joined — launches in flight may still use the one that goes.
    int acquire(const size_t (&bytes)[N], Fit fit, hipStream_t stream) {
        for (int i = 0; i < N; i++) {
            DeviceArray& p = plane[i];
            if (!bytes[i] || (fit == Exact ? p.capacity == bytes[i] : p.capacity >= bytes[i])) continue;
            if (p.ptr) { ST_HIP(hipDeviceSynchronize()); read.settled(); p.release(); }
            if (int rc = p.reserve(bytes[i], bytes[i])) return rc;
        }
        return read.wait(stream, Fence::OtherStreams, Fence::Keep);
    }
    int done(hipStream_t stream) { return read.record(stream); }   // behind the launches that read the planes
};
// Room for `bytes` in a store that grows by half: *fresh says it is a new allocation — what the old one held is gone, the caller sends it again.
// `readers` of the old one are waited for on the host first (hipFree waits too; said there).
inline int grow_store(DeviceArray& a, size_t bytes, bool* fresh, std::initializer_list<Fence*> readers = {}) {
    *fresh = bytes > a.capacity;
    if (!*fresh) return ST_OK;
    for (Fence* f : readers) if (int rc = f->host_wait()) return rc;
    return a.reserve(bytes, bytes + bytes / 2);
}
inline double format_bytes(uint32_t format) { return format == ST_FORMAT_RGBA32F ? 16.0 : (format == ST_FORMAT_RGBA16F ? 8.0 : 4.0); }   // of one pixel (StOutputFormat)

}  // namespace st
#include "st_stores.h"
#include "st_deform.h"
#include "st_bvh_refresh.h"
#include "st_copies.h"
#include "st_output_chain.h"
namespace st {

// ------------------------------------------------------------------ per-camera state (camera_controller/buffers.rs)
constexpr int kInternalPlanes = 4;  // decoded-surface twins A/B (KArgs::sn / psn) + the pair the variance pass writes ahead of the strides-1+2 wavelet launch
// Depth of field derives the focal length from projection[5] and the view-space slopes from [0], [5], [8], [9]: a perspective projection
// ([15] == 0) whose [5] is positive and finite and whose [0] is finite and not 0 (include/strolle_hip.h "depth of field")
inline bool dof_perspective(const float* p) { return p[15] == 0.0f && p[5] > 0.0f && p[5] <= 3.402823466e+38f && std::fabs(p[0]) > 0.0f && std::fabs(p[0]) <= 3.402823466e+38f; }

struct CameraState {
    StCamera desc{};
    GpuCamera curr{}, prev{};
    uint64_t handle = 0;   // the StHandle this camera is known by (st_dist.cpp keys its partitions by it)
    uint32_t frame = 0, row0 = 0, row1 = 0, col0 = 0, col1 = 0;   // [row0,row1) x [col0,col1): the window this engine renders (st_camera_set_window)
    uint32_t out_format = 0;  // StOutputFormat (camera.rs:170-175 viewport.format)
    DeviceArray slab;   // every plane in one allocation, each at a 256-byte boundary
    float4* plane[ST_BUF_COUNT + kInternalPlanes] = {};   // + the two decoded-surface twins (KArgs::sn / psn), internal only
    size_t plane_bytes[ST_BUF_COUNT + kInternalPlanes] = {};
    DeviceArray tile_mask;  // two arrays of one u64 per 8x8 tile (KArgs::tile_mask, KArgs::gi_late_mask)
    size_t tile_mask_tiles() const { return tile_mask.capacity / (2 * sizeof(unsigned long long)); }
    DeviceArray counters;   // KS_COUNT x kCounterLines x 8 u64 (one 64-B line each: {rays, traversal bytes, pad})
    unsigned long long profiled_traversal_bytes[KS_COUNT] = {};  // part of counters[..][1] already reported by st_profile_read
    // The two-stream frame pipeline (render()) belongs to the camera: its side stream and the events that order frame N+1's
    // passes behind frame N's are per camera, so cameras rendered on different caller streams never wait on — or race
    // with — each other's frames.
    Stream side_stream;
    Event ev_di_head, ev_gi_done, ev_prim_ok, ev_frame_done, ev_setup, ev_lds_done;
    bool have_prev_frame_events = false;
    bool have_lds_done = false;   // the last frame recorded ev_lds_done inside its a-trous chain (StTuning::side_start): the next primary visibility waits for it too
    // GI history hand-over without the copy. gi_resolving ends every frame by copying the frame's source reservoirs into
    // GI_RESERVOIRS_0, next frame's history (gi_resolving.rs:60-66): 128 B per pixel of pure copy. When the source is the
    // temporal pass's output (GI_RESERVOIRS_1, four frames in six) and the whole pass graph runs, the engine swaps the two
    // plane pointers instead: GI_RESERVOIRS_0 takes over the storage temporal resampling wrote, and GI_RESERVOIRS_1 — which
    // the next temporal pass overwrites completely before anything reads it — gets the old history's storage. Until then
    // reading GI_RESERVOIRS_1 back returns GI_RESERVOIRS_0's storage (`gi_aliased`; st_camera_read_buffer), and anything
    // that could observe the difference (a pass mask, st_camera_write_buffer) first makes the copy for real
    // (`materialize_gi_history`).
    uint32_t last_lean = 0; bool last_lean_composed = false;   // KArgs::lean of the last frame: which planes it left unwritten (st_camera_buffer_stale)
    bool gi_aliased = false;
    bool surface_map_replaced[2] = {false, false};  // st_camera_write_buffer replaced PRIM_SURFACE_MAP_A / _B: regenerate its decoded twin before the next frame
    // Present hand-over (st_camera_present_copy): composed frames leave for host memory on a stream of their own, behind the
    // frame that produced them, while the next frame's kernels run. Two copies may be in flight (the caller alternates two
    // output buffers); a render into a buffer whose copy is still pending is ordered behind that copy.
    struct PresentSlot { const void* src = nullptr; void* dst = nullptr; Event ev_src, ev_done; bool pending = false; };
    Stream present_stream;
    PresentSlot present[2];
    uint32_t present_next = 0;
    // the camera as the last render saw it (st_camera_pick casts through the frame on screen, not a later st_camera_update)
    GpuCamera shown{}; uint32_t shown_width = 0, shown_height = 0; bool has_shown = false;
    GpuCamera shown_prev{};   // ... and the camera of the frame before it (that render's KArgs::prev_cam: st_camera_render_aovs' MOTION)
    // Display transform (st_display.cpp; include/strolle_hip.h "display transforms"). Not part of the per-camera buffers: it survives the
    // reallocation of st_camera_update. `display_state` (auto-exposure only) is kDisplayBytes of device memory — the histogram the composing
    // launches add to, the last finalized one, DisplayState — allocated by the first auto frame; `display_reset` asks the next render to
    // put it back to its first-frame values. `display_done` is recorded behind each finalize: a frame on another stream waits for it first.
    StDisplayDesc display{}; bool display_on = false, display_reset = false;
    float display_scale = 1.0f;   // manual: 2^exposure_ev (host double, rounded)
    DeviceArray display_state; Fence display_done;
    bool display_auto() const { return display_on && (display.flags & ST_DISPLAY_AUTO_EXPOSURE) != 0u; }
    bool windowed() const { return row0 != 0u || col0 != 0u || row1 != desc.height || col1 != desc.width; }
    // The output chain (st_output_chain.h NodeSetting: descriptor, on, planes; each survives st_camera_update). Post-processing (st_post.cpp):
    // while a frame needs it, the composing launch writes planes[0] (render size, RGBA32F) instead of the caller's buffer; planes[1] carries
    // FXAA's output to the resampler when both run; replaced only when the render size changed. In front of it the five HDR nodes, in
    // chain order (DESIGN.md "The output chain"; the order and what a frame does with each is st_render.cpp's node table): while a node is
    // on, whatever is in front of it — the composing launch, else the node before — writes the node's HDR plane, and its own last launch
    // writes where that one would have. Their planes are grown, never shrunk.
    NodeSetting<StPostDesc, 2> post{&kPostWindow};
    NodeSetting<StFogDesc, 1> fog{nullptr};                  // st_fog.cpp. [0] the HDR plane. Pointwise: a window does not exclude it
    NodeSetting<StLightShaftsDesc, 2> shafts{&kShaftsWindow};   // st_shafts.cpp. [0] the HDR plane, [1] the cell plane (S.rgb, d_c)
    NodeSetting<StDofDesc, 4> dof{&kDofWindow};              // st_dof.cpp. [0] the HDR plane, [1] (coc, Z) per pixel, [2] the tiles' near-field maxima, [3] their 3 x 3 neighbour maxima
    NodeSetting<StMotionBlurDesc, 4> mblur{&kMBlurWindow};   // st_motion_blur.cpp. [0] the HDR plane, [1] (r, Z) per pixel, [2] the tile vectors, [3] their 3 x 3 neighbour maxima
    NodeSetting<StBloomDesc, 2> bloom{&kBloomWindow};        // st_bloom.cpp. [0] the HDR plane, [1] the pyramid (one allocation of float4 mips)
    NodeSetting<StLensDesc, 1> lens{&kLensWindow};           // st_lens.cpp. [0] the HDR plane (between bloom and the grade)
    NodeSetting<StColorGradingDesc, 1> grade{nullptr};       // st_grade.cpp. [0] the HDR plane. Pointwise: a window does not exclude it
    // The upscale stage behind FXAA (st_upscale.cpp): it reads post.planes ([1] with FXAA on, else [0]); [0] here is the output-size RGBA32F plane
    // between the upscaler and the sharpening step, grown, never shrunk
    NodeSetting<StUpscaleDesc, 1> upscale{&kUpscaleWindow};
    bool upscale_resizes() const { return upscale.on && upscale.desc.output_width != 0u && (upscale.desc.output_width != desc.width || upscale.desc.output_height != desc.height); }
    bool upscale_sharpens() const { return upscale.on && upscale.desc.sharpness > 0.0f; }
    // Which frames run a node that is on. Heatmap frames are false colour; heatmap and reference frames run no primary-visibility pass, so they
    // have no G-buffer and no velocity map; the nodes that derive a pixel's ray or the focal length need a perspective projection.
    bool has_gbuffer() const { return desc.mode != ST_MODE_BVH_HEATMAP && desc.mode != ST_MODE_REFERENCE; }
    bool post_resizes() const { return post.on && post.desc.output_width != 0u && (post.desc.output_width != desc.width || post.desc.output_height != desc.height); }
    bool post_fxaa() const { return post.on && (post.desc.flags & ST_POST_FXAA) != 0u && desc.mode != ST_MODE_BVH_HEATMAP; }
    // The fog and light-shafts launches read the G-buffer of the frame's parity, which primary visibility of the frame after next rewrites:
    // gbuffer_depth_read[parity] is recorded behind the last of them and the next primary-visibility launch of that parity waits for it
    // (DESIGN.md "Fog", "Light shafts")
    Fence gbuffer_depth_read[2];
    uint32_t out_width() const { return upscale_resizes() ? upscale.desc.output_width : post.on && post.desc.output_width != 0u ? post.desc.output_width : desc.width; }
    uint32_t out_height() const { return upscale_resizes() ? upscale.desc.output_height : post.on && post.desc.output_width != 0u ? post.desc.output_height : desc.height; }
    // A present copy still in flight writes the caller's host memory: it lands before the stream goes. Everything else goes with its member —
    // the caller has made the device current and joined it (st_camera_delete, ~Engine).
    void join_present() { if (present_stream) (void)hipStreamSynchronize(present_stream); }
    ~CameraState() { join_present(); }
};
inline size_t plane_texels_per_pixel(int id) {
    if (id >= ST_BUF_DI_RESERVOIRS_0 && id <= ST_BUF_DI_RESERVOIRS_2) return 2;
    if (id >= ST_BUF_GI_RESERVOIRS_0 && id <= ST_BUF_GI_RESERVOIRS_3) return 4;
    if (id == ST_BUF_REF_HITS) return 2;
    if (id == ST_BUF_REF_RAYS) return 3;
    return 1;
}

constexpr size_t kCounterWordsPerSlot = (size_t)kCounterLines * 8;
constexpr size_t kCounterBytes = sizeof(unsigned long long) * kCounterWordsPerSlot * KS_COUNT;
inline int materialize_gi_history(CameraState& c) {
    if (!c.gi_aliased) return ST_OK;
    ST_HIP(hipDeviceSynchronize());
    ST_HIP(hipMemcpy(c.plane[ST_BUF_GI_RESERVOIRS_1], c.plane[ST_BUF_GI_RESERVOIRS_0], c.plane_bytes[ST_BUF_GI_RESERVOIRS_0], hipMemcpyDeviceToDevice));
    c.gi_aliased = false;
    return ST_OK;
}
// sums the per-line counters of every kernel slot into host[2*slot + {0: rays, 1: traversal bytes}]
inline int read_counters(const CameraState& c, unsigned long long* host /* 2*KS_COUNT */) {
    std::vector<unsigned long long> raw(kCounterWordsPerSlot * KS_COUNT);
    hipError_t err = hipMemcpy(raw.data(), c.counters.ptr, kCounterBytes, hipMemcpyDeviceToHost);
    if (err != hipSuccess) return fail(ST_ERR_HIP, std::string("hipMemcpy(counters): ") + hipGetErrorString(err));
    for (int s = 0; s < KS_COUNT; s++) {
        unsigned long long rays = 0, bytes = 0;
        for (uint32_t l = 0; l < kCounterLines; l++) { rays += raw[(size_t)s * kCounterWordsPerSlot + l * 8]; bytes += raw[(size_t)s * kCounterWordsPerSlot + l * 8 + 1]; }
        host[2 * s] = rays; host[2 * s + 1] = bytes;
    }
    return ST_OK;
}


struct ProfileRecord { int slot; hipEvent_t start, stop; double bytes; uint32_t launches; bool owns_start; };   // borrowed from Engine::profile_events

StTuning default_tuning();  // st_engine.cpp
struct DistState;           // st_dist.cpp: rank / world, transport, per-camera partition
int dist_partition(uint32_t width, uint32_t height, uint32_t world, uint32_t cols, uint32_t rank, StDistRect* owned);
int dist_window(uint32_t width, uint32_t height, const StDistRect* owned, uint32_t apron, StDistRect* window);
int dist_grid(uint32_t width, uint32_t height, uint32_t world, uint32_t cols, StDistGrid* out);
int dist_grid_tile(const StDistGrid* g, uint32_t rank, StDistRect* owned);
int dist_grid_rebalance(uint32_t width, uint32_t height, const StDistGrid* cur, const float* cost, uint32_t max_step, StDistGrid* out);

struct Engine {
    int device = -1;
    bool has_device = false;
    uint64_t base_seed = 0;
    uint32_t frame = 1;  // lib.rs:152

    // The scene stores (st_stores.h), one owner each; the members below connect them in a tick
    MeshStore meshes; MaterialStore materials; ImageAtlas images; LightStore lights; InstanceStore instances; TriangleSlots slots;
    bool moved_on_device = false;      // this tick's refresh left the moved instances to the device
    bool materials_changed_this_tick = false;
    uint64_t device_bakes = 0, device_baked_triangles = 0;
    void bake_stale_on_host();         // brings the host arrays up to date (rebuilds, host refits, full uploads and debug reads need them)

    // Mesh deformation — skinned meshes, morph targets, deformation motion — has one owner (st_deform.h)
    Deformer deform{*this};
    int deferred_status = ST_OK;      // a read-back that failed inside a refresh or bake_stale_on_host (message in g_last_error): st_tick / st_debug_read_scene return it
    int take_deferred_status() { const int rc = deferred_status; deferred_status = ST_OK; return rc; }

    // The scene's BVH — the host's tree, its streams, refits, the device builder, the tick's plan — has one owner (st_bvh_refresh.h)
    SceneTree tree{*this};

    StagingRing staging;

    bool sync_every_tick = false;
    float sun_azimuth = 0.0f, sun_altitude = 0.35f; bool sun_dirty = true;
    V3 sun_dir_ = v3s(0.0f);

    std::vector<uint8_t> blue_noise; bool blue_noise_dirty = true;
    bool atmosphere_initialized = false, sky_known = false; float known_sun_altitude = 0.0f;  // passes/atmosphere.rs:14-15,78-110

    // The tick's device copies — the scene's and the lights' pairs, their readers, the tick's streams and fences — have one owner (st_copies.h)
    SceneCopies copies{*this};
    // environment lighting (include/strolle_hip.h "environment lighting"; st_env.cpp). An edit waits in env_edit / env_desc_next for the next
    // tick (apply_environment on the host, upload_environment on the device). Every map the device holds is a fresh allocation (env_retired).
    struct EnvMap { DeviceArray texels, table; uint32_t w = 0, h = 0, gw = 0, gh = 0; Fence fence; };
    enum EnvEditKind { ENV_EDIT_NONE, ENV_EDIT_HOST, ENV_EDIT_DEVICE, ENV_EDIT_CLEAR };
    struct EnvEdit { EnvEditKind kind = ENV_EDIT_NONE; std::vector<float4> texels; const void* src = nullptr; size_t pitch = 0; uint32_t w = 0, h = 0, channels = 0; };
    EnvEdit env_edit;
    StEnvironmentDesc env_desc{}, env_desc_next{};
    bool env_set = false, env_sun_off = false;   // a map is live (host-only engines too: light 0 follows it); light 0 is dark because of it
    std::unique_ptr<EnvMap> env_live; Retired<EnvMap> env_retired{copies};
    DeviceArray d_env_grid, d_env_bad /* one u32: the texels the device upload sanitized */; uint64_t env_sanitized = 0;
    std::vector<float> env_grid_host; std::vector<EnvCell> env_table_host;

    // colour grading's look-up tables (include/strolle_hip.h "colour grading"; st_grade.cpp). st_lut_insert / st_lut_remove leave an edit
    // per id for the next tick (a host-only engine drops them there). Every table the device holds is a fresh allocation of size^3 float4 (luts_retired).
    struct Lut { DeviceArray texels; uint32_t size = 0; Fence fence; };
    struct LutEdit { uint32_t size = 0; std::vector<float4> texels; };   // size 0: remove
    std::map<StHandle, LutEdit> lut_edits;
    std::map<StHandle, std::unique_ptr<Lut>> luts_live; Retired<Lut> luts_retired{copies};

    DeviceArray d_byte_luts, d_atlas, d_blue_noise, d_transmittance, d_scattering, d_sky;

    std::unordered_map<uint64_t, std::unique_ptr<CameraState>> cameras; uint64_t next_camera = 0;

    // Which build of the kernels this engine launches (st_kernels.h): fast arithmetic by default, the bit-exact build on request
    // (st_engine_set_arithmetic, or ST_EXACT=1 in the environment when the engine is created).
    int arithmetic = ST_ARITH_FAST;
    Launchers L = launchers_fast();
    std::vector<uint64_t> last_launches;  // pass bits of every launch the last render considered (st_debug_last_launches)
    uint64_t launch_filter = ~0ull;  // st_debug_set_launch_filter: which launches of the whole frame's graph (by their ordinal in the serial order) are enqueued (tools/pair_matrix.py)
    uint64_t pass_mask = ~0ull;  // st_debug_set_pass_mask: which reference passes a render executes (parity tests run one launch at a time)
    // Scheduling / tuning switches (include/strolle_hip.h StTuning says what each selects; st_engine.cpp holds the defaults and
    // the environment overrides). Notes that belong to the implementation:
    //  * lean_frame: KArgs::lean, st_types.h kLean* — fast build + whole pass graph + Image{denoise}: planes nothing reads again are
    //    not stored; st_camera_read_buffer of those planes returns what an earlier frame or launch left there.
    //  * tile_map_denoise = 2 keeps the halo rows of the LDS windows and the a-trous taps in one XCD's L2. Measured on one box: with
    //    mode 1 the two-stream frame is 1.347 instead of 1.373 ms, but a wavelet launch moves 340 instead of 205 MB through the
    //    fabric (algorithmic: 174 MB) and takes 61 instead of 56 us on its own.
    //  * tile_map = 1 measured best on MI355X with the current kernels (2 was, before the LDS-staged denoiser).
    StTuning tuning;
    uint32_t exp_flags = 0;   // KArgs::exp_flags (ST_EXP): same-box A/B of an experiment before it is kept or archived
    bool profiling = false;       // st_profile_enable bit 0: per-kernel event timing (serial execution)
    bool count_bytes = false;     // st_profile_enable bit 1: traversal-byte counters
    bool profile_kernel_events = false;  // st_profile_enable bit 3: every launch carries its own start / stop events (hipExtLaunchKernelGGL): no event packets between kernels
    bool profile_group_atrous = false;  // st_profile_enable bit 2: the a-trous chain's back-to-back launches share ONE event pair (an event between two kernels costs the second one 3-15 us)
    std::vector<ProfileRecord> profile_records;
    std::vector<Event> profile_events; std::vector<hipEvent_t> event_pool;   // every event take_event() ever made; those of them that are free
    StKernelProfile profile_totals[KS_COUNT];

    Engine();
    int set_tuning(const StTuning& t);
    // multi-GPU (st_dist.cpp)
    DistState* dist = nullptr;
    void release_dist();
    void dist_forget_camera(uint64_t handle);
    int dist_set_partition(uint64_t handle, CameraState& c, uint32_t cols, uint32_t apron);
    int dist_set_grid(uint64_t handle, CameraState& c, const StDistGrid& grid, uint32_t apron);
    int dist_gather(uint64_t handle, CameraState& c, const void* frame, void* full, hipStream_t stream);
    int dist_wait(uint64_t handle, const void* frame, hipStream_t stream, bool host);
    void dist_guard(uint64_t handle, const void* out, hipStream_t s);
    int dist_gather_ms(uint64_t handle, float* ms);
    void reset_profile_totals();
    ~Engine();
    static void release_camera(CameraState& c);   // the per-size resources back to none: allocate_camera makes them again
    int present_copy(CameraState& c, const void* src, void* dst, size_t bytes, hipStream_t stream);
    int present_ready(CameraState& c, const void* dst, int wait, int* ready);

    // ---- the entry points that touch more than one owner (st_scene.cpp): a store and the deformer, the tree
    void insert_mesh(uint64_t id, const StMeshTriangle* t, size_t count);
    void remove_mesh(uint64_t id);
    void insert_instance(uint64_t id, uint64_t mesh, uint64_t material, const Affine& x);
    void remove_instance(uint64_t id);

    void drop_instance_triangles(uint64_t id);
    struct BakeJob { const std::vector<StMeshTriangle>* mesh; const InstanceRec* inst; uint32_t material; size_t first, count; };
    bool refresh_instances();
    void bake_jobs_on_host(const std::vector<BakeJob>& jobs, size_t total);
    int bake_on_device(SceneSet& t, hipStream_t up, bool* pageable);

    // Nothing observes the contract stream (a device-built tree can replace it) while every ray walks the wide stream: the fast build with the
    // wide stream and what it rests on, no traversal bytes counted (this part: wide_only_tuning) — and no camera draws the heatmap.
    bool wide_only_tuning() const { return arithmetic == ST_ARITH_FAST && tuning.wide_bvh && tuning.compact_bvh && tuning.anyhit_fast && !count_bytes; }
    bool heatmap_camera() const { for (const auto& kv : cameras) if (kv.second->desc.mode == ST_MODE_BVH_HEATMAP) return true; return false; }
    // A wide walk that found its stack full drops the push and says so in one of two sticky words of page-locked host memory (st_traverse.h
    // wide_walk_overflowed; KArgs::walk_flags). st_tick reads them: a per-lane walk's overflow re-arms every later launch with a deeper stack
    // (24 -> 32 -> 48 -> 56 entries: dynamic LDS, fewer waves per SIMD), the packet's (64 entries, one VGPR) hands primary visibility back to the
    // per-lane walk; either way that tick returns ST_ERR_BVH_TOO_DEEP once (StTuning::allow_deep_bvh: a line on stderr) — the frames rendered in
    // between may have missed geometry behind the dropped subtrees.
    PinnedBuffer walk_flags_mem; volatile uint32_t* walk_flags_host = nullptr; uint32_t* walk_flags_dev = nullptr;   // (the two views of walk_flags_mem)
    uint32_t wide_stack_rearmed = 0u;   // 0: StTuning::wide_stack_entries (0 = 24) as set; otherwise the entries an overflow re-armed the wide walks with
    bool packets_overflowed = false;    // the packet walk overflowed once on this engine: primary rays keep the per-lane walk
    uint64_t walk_overflows = 0; bool walk_overflow_unreported = false;
    uint32_t wide_stack_entries_now() const { return wide_stack_rearmed ? wide_stack_rearmed : (tuning.wide_stack_entries ? tuning.wide_stack_entries : (uint32_t)kBvhStackSize); }
    void note_walk_overflow();
    enum TriArrays : unsigned { TRI_GEO = 1u /* hit-test records + bounds */, TRI_ATTR = 2u /* attribute records */ };   // a copy's triangle-slot arrays
    bool tri_fits(const SceneSet& t, unsigned arrays) const;
    int upload_tri_slots(SceneSet& t, unsigned arrays, bool whole, hipStream_t up, bool* pageable);
    int tick(hipStream_t stream);
    TreePlan refresh_scene();
    void refresh_sun_and_lights();
    void apply_environment();
    int upload_environment(TickIo& io);
    void environment_args(KArgs& a) const;
    int environment_debug(uint32_t what, const float* in, uint32_t n, float* out, hipStream_t stream);
    int upload_scene(TreePlan plan, TickIo& io);
    int upload_images(TickIo& io);
    int upload_lights(TickIo& io);
    int report_deep_bvh();

    static GpuCamera serialize_camera(const StCamera& c);
    int allocate_camera(CameraState& c);

    hipEvent_t take_event();
    // One event pair per RUN of consecutive launches of the same slot on the same stream (the five a-trous launches, say):
    // an event between two kernels makes the second wait for a barrier packet, which adds microseconds to every launch
    // it brackets, so back-to-back launches of one slot are timed as one interval and divided by their count.
    // Consecutive runs on one stream share the event between them (the stop of one is the start of the next).
    struct OpenScope { int slot = -1; hipStream_t stream = nullptr; hipEvent_t start{}; bool owns_start = true; double bytes = 0; uint32_t launches = 0; } open_scope;
    void profile_begin(int slot, hipStream_t s, double bytes);
    hipEvent_t profile_close();
    int drain_profile();

    // a composition into a buffer whose present copy has not finished waits for that copy (callers that alternate two
    // buffers never meet this)
    static void present_guard(CameraState& c, const void* out, hipStream_t s) {
        for (auto& p : c.present) if (p.pending && p.src == out) (void)p.ev_done.wait(s);
    }

    int render(CameraState& c, void* out, hipStream_t stream);
    // ---- display transforms (st_display.cpp)
    int set_display(CameraState& c, const StDisplayDesc* desc);
    int display_begin(CameraState& c, hipStream_t stream, bool heatmap, DisplayArgs& d);   // this frame's DisplayArgs (+ the state's reset / stream order)
    int display_finalize(CameraState& c, hipStream_t stream);                              // behind a metered frame
    int display_exposure(CameraState& c, float* scale, float* metered_ev, float* adapted_ev);
    int display_histogram(CameraState& c, uint32_t* bins);
    // ---- output post-processing (st_post.cpp)
    struct PostPlan { bool fxaa = false, resample = false; PostArgs fx{}, rs{}; double fxaa_bytes = 0.0, resample_bytes = 0.0; };
    static PostPlan post_plan(const StPostDesc& d, bool fxaa, const void* src, uint32_t w, uint32_t h, void* mid, void* dst, uint32_t format);
    int set_post(CameraState& c, const StPostDesc* desc);
    int post_process(const StPostDesc* desc, const void* src, uint32_t w, uint32_t h, void* dst, int format, hipStream_t stream);
    FencedPlanes<1> post_scratch;   // st_post_process's intermediate plane (FXAA -> resampler): it only grows; calls on different streams take turns
    // ---- the upscale stage (st_upscale.cpp): the upscaler, then the sharpening step; `mid` (output size, RGBA32F) carries one to the other
    // `fused` (Engine::upscale_fused; 0 = two launches): both steps in one launch when both run — no plane between them
    struct UpscalePlan { bool upscale = false, sharpen = false; uint32_t fused = 0; UpscaleArgs up{}, sh{}, fu{}; double upscale_bytes = 0.0, sharpen_bytes = 0.0, fused_bytes = 0.0; size_t mid_bytes = 0; };
    static UpscalePlan upscale_plan(const StUpscaleDesc& d, const void* src, uint32_t w, uint32_t h, void* mid, void* dst, uint32_t format, uint32_t fused);
    int set_upscale(CameraState& c, const StUpscaleDesc* desc);
    static int upscale_camera_update(const CameraState& c, uint32_t new_width, uint32_t new_height);   // st_camera_update's question: may the render size become this?
    int upscale_process(const StUpscaleDesc* desc, const void* src, uint32_t w, uint32_t h, void* dst, int format, hipStream_t stream);
    uint32_t upscale_fused = 0u;   // st_debug_set_upscale_fused / ST_UPSCALE_FUSED: 0 two launches, 1 .. 3 the fused launch's tile (k_upscale.hip)
    FencedPlanes<1> upscale_scratch;   // st_upscale_process's plane between the two steps: it only grows; calls on different streams take turns
    // ---- the HDR nodes (st_output_chain.h). Each has its checks, a plan where frames of a size share host work, `*_steps`: the argument
    // block(s) and the OutputStep list of its launches from a NodeSource into a NodeTarget, `launch_*_step`, the setter, and the stateless call
    // ---- bloom (st_bloom.cpp)
    struct BloomPlan { uint32_t levels = 0; uint32_t w[8] = {}, h[8] = {}; float factor[8] = {}; size_t offset[8] = {}; size_t texels = 0; };
    struct BloomStep { OutputStep step; bool first; BloomArgs args; BloomTailArgs tail; };
    struct BloomSteps { BloomStep step[16]; uint32_t count = 0; };
    static int bloom_plan(const StBloomDesc& d, uint32_t w, uint32_t h, BloomPlan& plan);   // checks the desc; levels == 0: the frame holds no level
    // the frame's launches in order: `src` (w x h RGBA32F) -> the pyramid -> the target (raw when colour grading follows: untransformed RGBA32F)
    static BloomSteps bloom_steps(const StBloomDesc& d, const BloomPlan& plan, const void* src, uint32_t w, uint32_t h, float4* pyramid, const NodeTarget& target, uint32_t tail_lds_bytes);
    int set_bloom(CameraState& c, const StBloomDesc* desc);
    void launch_bloom_step(const BloomStep& s, hipStream_t stream);   // one of bloom_steps' launches
    int bloom_process(const StBloomDesc* desc, const StDisplayDesc* display, const void* src, uint32_t w, uint32_t h, void* dst, int format, hipStream_t stream);
    // The fused tail (k_bloom.hip k_bloom_tail), an experiment that measured slower and is OFF by default (tools/experiments/bloom_fused_tail.md): the LDS
    // its one workgroup may use. 0: no tail, the straightforward chain (the default); -1: what the device grants; n: at most n bytes
    // (ST_BLOOM_TAIL_BYTES in the environment, st_debug_set_bloom_tail). bloom_tail_bytes() is the figure in force.
    int bloom_tail_wanted = 0;
    uint32_t bloom_tail_bytes();
    static uint32_t bloom_tail_first(const BloomPlan& plan, uint32_t tail_lds_bytes);   // the first level the tail takes (== plan.levels: none)
    FencedPlanes<1> bloom_scratch;   // st_bloom_process's pyramid: likewise
    // ---- motion blur (st_motion_blur.cpp)
    struct MBlurPlan { uint32_t tiles_x = 0, tiles_y = 0; size_t packed_bytes = 0, tile_bytes = 0; };
    struct MBlurSteps { MBlurArgs args; OutputStep step[3]; };   // pack (+ tile maximum), neighbour maximum, gather: one argument block
    static int mblur_plan(const StMotionBlurDesc& d, uint32_t w, uint32_t h, MBlurPlan& plan);   // checks the desc
    static void mblur_steps(const StMotionBlurDesc& d, const MBlurPlan& plan, const NodeSource& src, float2* packed, float4* tile_max, float4* tile_n, const NodeTarget& target, MBlurSteps& out);
    int set_motion_blur(CameraState& c, const StMotionBlurDesc* desc);
    void launch_mblur_step(const MBlurSteps& s, uint32_t i, hipStream_t stream);
    int motion_blur_process(const StMotionBlurDesc* desc, const StDisplayDesc* display, const void* color, const void* velocity, const void* depth, uint32_t w, uint32_t h, void* dst, int format, hipStream_t stream);
    FencedPlanes<3> mblur_scratch;   // st_motion_blur_process's packed plane and tile vectors: grown, never shrunk
    // ---- depth of field (st_dof.cpp)
    struct DofPlan { uint32_t samples = 0, tiles_x = 0, tiles_y = 0; size_t packed_bytes = 0, tile_bytes = 0; float max_radius = 0.0f; float taps[kDofMaxSamples * 3u] = {}; };
    struct DofSteps { DofArgs args; OutputStep step[3]; };   // pack (+ tile maximum), neighbour maximum, gather: one argument block
    static int dof_plan(const StDofDesc& d, uint32_t w, uint32_t h, DofPlan& plan);   // checks the desc
    static void dof_steps(const StDofDesc& d, const DofPlan& plan, const float projection[16], const NodeSource& src, float2* packed, float* tile_max, float* tile_n, const NodeTarget& target, DofSteps& out);
    int set_dof(CameraState& c, const StDofDesc* desc);
    void launch_dof_step(const DofSteps& s, uint32_t i, hipStream_t stream);
    int dof_process(const StDofDesc* desc, const StDisplayDesc* display, const float* projection, const void* color, const void* depth, uint32_t w, uint32_t h, void* dst, int format, hipStream_t stream);
    FencedPlanes<3> dof_scratch;   // st_dof_process's packed plane and tile values: grown, never shrunk
    // ---- fog (st_fog.cpp)
    struct FogStep { FogArgs args; OutputStep step; };
    static void fog_step(const StFogDesc& d, const NodeView& view, const NodeSource& src, uint32_t row0, uint32_t row1, uint32_t col0, uint32_t col1, const NodeTarget& target, FogStep& out);
    int set_fog(CameraState& c, const StFogDesc* desc);
    int fog_process(const StFogDesc* desc, const StDisplayDesc* display, const float* transform, const float* projection, const void* color, const void* depth,
                    uint32_t w, uint32_t h, void* dst, int format, hipStream_t stream);
    // ---- colour grading (st_grade.cpp)
    struct GradePlan { uint32_t steps = 0; float M[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f}; float inv_range = 0.0f; };
    struct GradeStep { GradeArgs args; OutputStep step; };
    static int grade_plan(const StColorGradingDesc& d, GradePlan& out);   // checks the desc
    // `lut`: size^3 float4 or null (the step is then skipped, whatever the plan says)
    static void grade_step(const StColorGradingDesc& d, const GradePlan& plan, const float4* lut, uint32_t lut_size, const NodeSource& src, uint32_t row0, uint32_t row1,
                           uint32_t col0, uint32_t col1, const NodeTarget& target, GradeStep& out);
    int set_grade(CameraState& c, const StColorGradingDesc* desc);
    int grade_process(const StColorGradingDesc* desc, const StDisplayDesc* display, const void* lut, uint32_t lut_size, const void* src, uint32_t w, uint32_t h, void* dst,
                      int format, hipStream_t stream);
    int lut_insert(StHandle id, uint32_t size, const float* rgb);
    int lut_remove(StHandle id);
    int upload_luts(TickIo& io);   // the tick's: edits -> fresh device tables; retired ones are released behind their readers
    Lut* live_lut(StHandle id) const { auto it = luts_live.find(id); return it == luts_live.end() ? nullptr : it->second.get(); }
    // ---- lens effects (st_lens.cpp)
    struct LensStep { LensArgs args; OutputStep step; };
    static int lens_plan(const StLensDesc& d, uint32_t w, uint32_t h, StLensPlan& out);   // checks the desc and the sides
    // `frame`: the camera's frame counter (ST_LENS_GRAIN_ANIMATE adds it to the seed); `force_gather`: st_debug_set_lens_gather
    static void lens_step(const StLensDesc& d, const StLensPlan& plan, const NodeSource& src, uint32_t frame, bool force_gather, const NodeTarget& target, LensStep& out);
    int set_lens(CameraState& c, const StLensDesc* desc);
    int lens_process(const StLensDesc* desc, const StDisplayDesc* display, const void* src, uint32_t w, uint32_t h, void* dst, int format, hipStream_t stream);
    bool lens_force_gather = false;   // st_debug_set_lens_gather: a descriptor without taps runs the gather instantiation (one tap at the pixel's own centre)
    // ---- light shafts (st_shafts.cpp)
    struct ShaftsPlan { uint32_t cells_w = 0, cells_h = 0; size_t cell_bytes = 0; float jitter[16] = {}; };
    struct ShaftsSteps { ShaftsArgs args; OutputStep step[2]; };   // march, apply
    static int shafts_plan(const StLightShaftsDesc& d, uint32_t w, uint32_t h, ShaftsPlan& out);
    void shafts_steps(const StLightShaftsDesc& d, const ShaftsPlan& plan, const NodeView& view, const NodeSource& src, float4* cells, const NodeTarget& target, bool count, ShaftsSteps& out) const;
    void launch_shafts_step(const KArgs& scene, const ShaftsSteps& s, uint32_t i, hipStream_t stream);
    int set_shafts(CameraState& c, const StLightShaftsDesc* desc);
    int shafts_process(const StLightShaftsDesc* desc, const StDisplayDesc* display, const float* transform, const float* projection, const void* color, const void* depth,
                       uint32_t w, uint32_t h, void* dst, int format, hipStream_t stream);
    FencedPlanes<1> shafts_scratch;   // st_light_shafts_process's cell plane: grown, never shrunk
    // Normal mapping (include/strolle_hip.h "normal mapping"; st_traverse.h normal_map_apply). `normal_mapping` is the switch (MaterialStore::any_normal_map: whether
    // anything can be mapped). normal_map_geo: the argument primary visibility, the NORMAL AOV and
    // picks get (`flagged`: a query with ST_RAY_MAPPED_NORMAL, which does not ask the switch) — the live copy's hit-test records, or null where nothing can be mapped.
    bool normal_mapping = false;
    int normal_map_geo(hipStream_t stream, bool flagged, const float4** geo);
    int scene_args(KArgs& a, bool heatmap) const;   // the scene half of KArgs (st_render.cpp): render() and the scene queries
    void light_args(KArgs& a) const;                // its lights, LUT and environment half: render()

    // ---- scene queries (st_query.cpp; include/strolle_hip.h "scene queries")
    std::vector<uint32_t> instance_table_;   // host image of SceneSet::instance_table, rebuilt by every scene upload
    void fill_instance_table();
    int query_begin(hipStream_t stream, KArgs& a, unsigned reads);   // the checks, scene_args, copies.begin
    int trace_rays(const void* rays, uint32_t count, void* hits, uint32_t flags, hipStream_t stream, bool reader = true);
    int occluded(const void* rays, uint32_t count, uint32_t* out, hipStream_t stream);
    int pick(const CameraState& c, const uint32_t* pixels, uint32_t count, void* hits, hipStream_t stream);
    int trace_rays_host(const void* rays, uint32_t count, void* hits);
    int render_aovs(const CameraState& c, const StAovTargets& t, hipStream_t stream);   // per-pixel AOVs (st_aov.cpp)
    Stream query_stream; DeviceArray d_query_rays, d_query_hits; PinnedBuffer query_pinned;
};

}  // namespace st
