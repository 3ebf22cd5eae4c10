// st_deform.h — mesh deformation of the host engine: skinned meshes, morph targets and deformation motion (include/strolle_hip.h "skinned meshes",
// "morph targets"; k_skin.hip; st_deform.cpp). Part of st_engine.h, which includes it behind the owners of HIP resources it is made of.
//
// Engine::deform is the one owner of this state. The rest of the engine asks it the questions below and never reads its records or stores.
#pragma once

namespace st {

struct Engine;

struct Deformer {
    Engine& e;   // its meshes, its instances (a deformation that changes marks one dirty), its staging ring, its device
    explicit Deformer(Engine& engine) : e(engine) {}

    // A skin per mesh: its bind-pose triangles (kTriangleFloats each, the mesh store's layout) and corners go to the bind store once.
    struct SkinRec { std::vector<StSkinVertex> corners; uint32_t joints = 0; size_t first = SIZE_MAX; };   // first: its triangles in the bind store (SIZE_MAX: not there yet)
    // A target set per mesh, kept in the device layout (st_kernels.h MorphJob: per target `padded` triangles of 18 floats as five planes), placed in
    // the target store when a tick first needs it. bind_first: a morph-only mesh's base triangles in the bind store (no corners there); a mesh
    // that also has a skin uses the skin's range.
    struct MorphRec { std::vector<float> planes; uint32_t targets = 0; size_t count = 0, padded = 0, first = SIZE_MAX, bind_first = SIZE_MAX; };
    // A deformation per instance: the last joint palette set (12 floats per joint; empty: none), the last morph weights set (one per target;
    // empty: none, or all zero), or both — never neither — and the instance's region of the posed store (kTriangleFloats per triangle), which the
    // tick's launches fill and k_bvh_bake reads. meshes[id] stays the bind pose.
    struct DeformRec {
        uint64_t mesh = 0; std::vector<float> palette, weights; size_t first = SIZE_MAX, count = 0;   // first: its region of the posed store (SIZE_MAX: none yet)
        bool reskin = true;          // the device region has to be (re)computed at the next tick: the pose or the weights changed, or the posed store was reallocated
        bool changed = true;         // they changed since the last launch (that launch makes the host image stale)
        bool host_current = false;   // `host` holds what the device region holds
        std::vector<StMeshTriangle> host;   // its host image (tangents from the bind mesh), read back only when a host bake needs it
        // deformation motion: `other` is the second region — a tick that deforms again writes it and swaps it with `first`, so that it then
        // holds the positions from before that tick; has_previous says the LAST tick did so. `skinned` / `previous` (+ `_w`) are the palettes and
        // weights the two regions were computed with (a posed store that grows computes both again into the new allocation); `recorded`: `first`
        // holds what a tick deformed while the switch was on. All empty / false while the switch is off.
        size_t other = SIZE_MAX; bool has_previous = false, recorded = false;
        std::vector<float> skinned, previous, skinned_w, previous_w;
    };
    std::unordered_map<uint64_t, SkinRec> skins;       // by mesh
    std::unordered_map<uint64_t, MorphRec> morphs;     // by mesh
    std::unordered_map<uint64_t, DeformRec> deforms;   // by instance

    // The three stores, each a RangeStore over its device allocation: ranges of what was dropped are reused (uploads into them are ordered behind
    // every launch on the skin stream). posed: triangles; binds: triangles of d_bind and, times three, corners of d_corners, with their host
    // images; targets: units of kMorphUnitFloats floats (its host image is the MorphRecs' planes).
    RangeStore posed, binds, targets;
    std::vector<float> bind_host; std::vector<StSkinVertex> corner_host;
    DeviceArray d_posed, d_bind, d_corners, d_targets;
    DeviceArray d_skin_jobs, d_skin_starts, d_palettes, d_morph_jobs, d_morph_starts, d_morph_active;   // one tick's jobs
    Stream skin_stream; Event ev_skinned;
    Fence posed_read;   // behind the bakes that read the posed regions (bake_on_device), on whichever streams: the next skin launch overwrites them
    // Deformation motion (st_traverse.h deform_prev_point): with the switch on, primary visibility and the AOV launch read the previous region of
    // every instance the last tick deformed again, through the free word of the scene copy's instance table (previous_word). `live`: how many
    // instances the last tick left one — the switch itself is read by the tick alone, so it takes effect at the next tick. deform_read is recorded
    // behind every reader that can reach deform_prev_point, behind a wait for its own earlier recording, so that one event covers readers on several
    // streams; the next skin launch, which overwrites previous regions, waits for it on the skin stream. No host wait (DESIGN.md "Deformation motion").
    bool motion_on = false; uint64_t live = 0;
    Fence deform_read;
    uint64_t skin_launches = 0, skinned_triangles = 0, posed_readbacks = 0, morph_ticks = 0, morphed_triangles = 0;

    // ---- the C ABI's entry points
    int set_skin(uint64_t mesh, const StSkinVertex* corners, size_t corner_count, uint32_t joint_count);
    int set_pose(uint64_t instance, const float* joint_xforms, uint32_t joint_count);
    int set_morph_targets(uint64_t mesh, const StMorphDelta* deltas, size_t corner_count, uint32_t target_count);
    int set_morph_weights(uint64_t instance, const float* weights, uint32_t target_count);
    int read_posed(uint64_t instance, float* out, size_t capacity_floats, size_t* written_floats);
    void skinning_stats(uint64_t* launches, uint64_t* triangles, uint64_t* host_readbacks) const { *launches = skin_launches; *triangles = skinned_triangles; *host_readbacks = posed_readbacks; }
    int morphing_stats(uint64_t* ticks, uint64_t* triangles, uint64_t* delta_bytes) const;
    int deformation_stats(uint64_t* instances_with_previous, uint64_t* previous_bytes) const;
    void drop_instance(uint64_t instance, bool make_dirty);   // the whole deformation: palette, weights and regions
    void drop_skin(uint64_t mesh);    // and the poses of the instances of that mesh
    void drop_morph(uint64_t mesh);   // and the weights of the instances of that mesh

    // ---- st_tick
    bool any() const { return !deforms.empty(); }
    void begin_tick();                // forgets last tick's previous poses (and, with the switch off, gives the second regions back)
    int tick(hipStream_t stream);     // before the refresh: one launch of each kernel at most for every deformation to (re)compute; `stream` follows them

    // ---- the host bake (st_scene.cpp)
    int read_back();                  // host images of every posed region they lag behind: one batch, one synchronisation
    // what a host bake of `instance` reads: the host image of its posed region, else its mesh (`mesh`)
    const std::vector<StMeshTriangle>* bake_source(uint64_t instance, const std::vector<StMeshTriangle>& mesh) const;

    // ---- the device bake (st_scene.cpp bake_on_device)
    // whether the bake of `instance`, whose slots hold `triangles`, reads its posed region, and which (a deformation is dropped with its mesh: its
    // triangle count is the one the instance's slots were baked for)
    bool bake_region(uint64_t instance, size_t triangles, size_t* first) const {
        const auto it = deforms.find(instance);
        if (it == deforms.end() || it->second.first == SIZE_MAX || it->second.count != triangles) return false;
        *first = it->second.first;
        return true;
    }
    const float* posed_store() const { return static_cast<const float*>(d_posed.ptr); }
    int wait_skinned(hipStream_t s) const { return ev_skinned.wait(s); }        // `s` reads posed regions next: behind the tick's launches (skin stream)
    int posed_read_by(hipStream_t s) { return posed_read.record_chained(s); }   // `s` read posed regions: the next launches overwrite them behind that

    // ---- the frames (st_query.cpp fill_instance_table, st_render.cpp, st_aov.cpp)
    // the instance table's free word: 0, or 1 + the previous region of `instance`, whose slots hold `triangles`
    uint32_t previous_word(uint64_t instance, size_t triangles) const {
        if (!live) return 0u;
        const auto it = deforms.find(instance);
        return it != deforms.end() && it->second.has_previous && it->second.count == triangles ? (uint32_t)it->second.other + 1u : 0u;
    }
    // what primary visibility and the MOTION AOV get as kernel arguments: null unless the last tick left some instance a previous pose (that tick wrote
    // the live copy's table: a deformation is a scene change)
    const uint4* deform_table() const;
    const float* deform_posed() const { return live ? posed_store() : nullptr; }
    int previous_read_by(hipStream_t s) { return live ? deform_read.record_chained(s) : ST_OK; }   // a reader that can reach deform_prev_point ends here on `s`
};

}  // namespace st
