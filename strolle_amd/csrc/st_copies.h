// st_copies.h — the tick's device copies of the host engine: the protocol that lets the host run a frame ahead of the GPU (implementation: the end of
// st_tick.cpp). Part of st_engine.h, which includes it behind the owners of HIP resources and the tree's half of a scene copy it is made of.
//
// Engine::copies is the one owner of this protocol. The arrays a scene change rewrites exist twice (CopyPair). A tick that changes the scene fills the
// copy no frame in flight reads, on a stream of its own, while the previous frame still renders from the other one; the next frame switches over.
// (Updating in place would have to wait for the previous frame, and the next frame's primary rays with it.) The light table alternates the same way, on
// its own schedule: a light that moves every frame does not resend the scene. An allocation that is replaced whole — an environment map, a look-up
// table — is Retired: frames enqueued before the replacement keep reading theirs, which goes once its fence says they are done.
//   the writer (Engine::tick)   begin_tick; per pair: pick -> the uploads into the picked copy -> commit; end_uploads
//   a reader                    begin(stream, reads) -> its launches -> end(stream, reads): `reads` names, once, whose fences end on `stream`
//   mixed()                     readers on several streams: no single event ends their reads, so a writer and a retirement join the device instead
// One writer of a live copy stands outside a tick: Engine::normal_map_geo (st_render.cpp) fills the live scene copy's hit-test records from a reader's stream
// and joins that stream. That is safe because no launch in flight reads those records while SceneSet::geo_current is false — only the tick's device tree work
// on a copy does (such a copy is geo_current), and a mapping reader gets the pointer from normal_map_geo alone, behind the join.
#pragma once
namespace st {
struct SceneSet {
    DeviceArray tri_attr, xforms, materials, base_packed;
    TreeCopy tree;   // the tree's half (st_bvh_refresh.h): the streams, the refit's index arrays, the device builder's scratch
    // per triangle slot the hit-test record and the bounds (ST_BVH_REFIT_DEVICE, ST_BVH_BUILD_DEVICE: k_bvh.hip and k_lbvh.hip read them)
    DeviceArray tri_geo, tri_bounds;
    bool geo_current = false;   // tri_geo holds the hit-test record of every slot as this copy's tree has it (SceneTree::write); a host-tree path sends none — normal mapping asks (Engine::normal_map_geo)
    size_t dirty_lo = SIZE_MAX, dirty_hi = 0; bool tri_full = true;  // what this copy lacks of the host's triangle arrays
    std::vector<uint64_t> pending_moves;   // instances moved on the device whose current transform this copy has not baked yet
    DeviceArray bake_jobs, bake_starts;
    // per instance slot (tri_attr[4 t + 3].w): {StHandle lo, hi, first triangle slot, 0} — the scene queries' instance and mesh triangle (st_query.cpp)
    DeviceArray instance_table;
    Fence fence;   // reads of this copy enqueued since it was written end here (SceneCopies::end; pick waits before the copy is written again)
    bool valid = false;
};
struct LightSet { DeviceArray buf; Fence fence; };
// The two copies of a double-buffered resource; T carries a `Fence fence`. written: a tick has uploaded it, there is a live copy; alternating: a tick
// has written the other copy once, readers mark their end from then on
template <class T> struct CopyPair {
    T copy[2]; int live = 0;
    bool written = false, alternating = false;
    T& current() { return copy[live]; }
    const T& current() const { return copy[live]; }
    T& other() { return copy[live ^ 1]; }
};
struct TickIo { hipStream_t stream; bool pageable = false, pageable_copy = false, copied = false, uploaded = false; };   // one tick's uploads. copied: on copy_stream; uploaded: on `stream`
struct CopyTarget { int index; hipStream_t up; bool* pageable; bool other; };   // what pick chose: which copy, on which stream, which of TickIo's pageable flags
// What a reader reads (begin / end). kReadsNothing: no reader of its own — a call that is over when it returns, a frame's second stream
enum Reads : unsigned { kReadsNothing = 0u, kReadsScene = 1u, kReadsLights = 2u, kReadsEnvironment = 4u /* the live map */, kReadsShading = 6u,
                        kReadsPrevious = 8u /* previous regions of the posed store: deform_prev_point (frames, the MOTION AOV) */, kReadsFrame = 15u };

struct SceneCopies {
    Engine& e;   // its tuning, its staging ring, its live environment map, its deformer
    explicit SceneCopies(Engine& engine) : e(engine) {}
    CopyPair<SceneSet> scene; CopyPair<LightSet> lights;
    Stream copy_stream;   // the other copy is written here
    Fence tick_done;   // a tick queued copies without joining the stream: this marks their end, the next frame's streams wait for it
    Fence copy_done;   // behind a tick's copies on copy_stream, like tick_done
    hipStream_t last_render_stream = nullptr; bool rendered_before = false, mixed_render_streams = false;   // the readers' streams so far (begin)
    bool mixed() const { return mixed_render_streams; }
    int join_mixed() { if (mixed()) ST_HIP(hipDeviceSynchronize()); return ST_OK; }
    // ---- the writer. begin_tick: uploads of an earlier tick that no render has waited for yet stay pending until their event has completed — a tick
    // that uploads nothing must not make a later render on another stream forget them (hipErrorNotReady from the queries is not an error)
    void begin_tick() { (void)tick_done.poll(); (void)copy_done.poll(); (void)hipGetLastError(); }
    template <class T> int pick(TickIo& io, CopyPair<T>& pair, CopyTarget& c);
    template <class T> void commit(TickIo& io, CopyPair<T>& pair, const CopyTarget& c) {
        pair.live = c.index; pair.written = true;
        (c.other ? io.copied : io.uploaded) = true;   // (in-place uploads are work on the caller's stream)
    }
    int end_uploads(TickIo& io);
    // ---- what the refresh of the host's triangle slots leaves for both copies (st_scene.cpp)
    void owe_slots(size_t b, size_t end) { for (SceneSet& t : scene.copy) { t.dirty_lo = std::min(t.dirty_lo, b); t.dirty_hi = std::max(t.dirty_hi, end); } }   // slots [b, end) are owed to every copy
    void owe_whole_arrays() { for (SceneSet& t : scene.copy) t.tri_full = true; }   // the host's arrays grew: every copy's triangle arrays are sent whole
    void instance_moved(uint64_t id) { for (SceneSet& t : scene.copy) if (std::find(t.pending_moves.begin(), t.pending_moves.end(), id) == t.pending_moves.end()) t.pending_moves.push_back(id); }
    void void_pending_moves() { for (SceneSet& t : scene.copy) t.pending_moves.clear(); }   // the host baked what the device had moved
    // ---- the readers
    int begin(hipStream_t stream, unsigned reads);
    int end(hipStream_t stream, unsigned reads);
};
// Allocations replaced while frames may still read them; T carries a `Fence fence` its readers record
template <class T> struct Retired {
    SceneCopies& copies; std::vector<std::unique_ptr<T>> list;
    explicit Retired(SceneCopies& c) : copies(c) {}
    // `m` goes when this returns, unless one stream's event ends its reads: then it is kept for release()
    int retire(std::unique_ptr<T> m) {
        if (!m->fence.pending) return ST_OK;
        if (copies.mixed()) return copies.join_mixed();
        list.push_back(std::move(m));
        return ST_OK;
    }
    // lets go of those whose last reader has finished (st_tick: the device is current)
    void release() {
        for (size_t i = 0; i < list.size();) { if (list[i]->fence.poll()) list.erase(list.begin() + (long)i); else i++; }
        (void)hipGetLastError();   // hipErrorNotReady is not an error
    }
};
}  // namespace st
