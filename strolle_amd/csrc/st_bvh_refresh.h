// st_bvh_refresh.h — the scene's BVH of the host engine: the host's binned-SAH tree and its streams, the refit state, the wide topology, the device
// builder's input, every tree decision of a tick and its counter (include/strolle_hip.h st_set_bvh_refresh; k_bvh.hip, k_lbvh.hip; st_bvh_refresh.cpp).
// Part of st_engine.h, which includes it behind the owners of HIP resources it is made of.
//
// Engine::tree is the one owner of this state, and SceneSet::tree (a TreeCopy) of the half each device copy of the scene holds. The rest of the
// engine asks the questions below and never reads the records.
#pragma once

namespace st {

struct Engine;
struct SceneSet;

// What upload_scene does with the tree (SceneTree::plan decides, SceneTree::write carries it out)
enum class TreePlan { none, host_refit, host_rebuild, device_build, device_refit, host_to_observer };

// The tree's half of one device copy of the scene (st_copies.h SceneSet)
struct TreeCopy {
    DeviceArray bvh;   // the contract stream in its device form
    DeviceArray bvh_compact; uint32_t compact_entries = 0;   // k_bvh.hip k_bvh_compact: 48 B per entry, regenerated whenever `bvh` changed
    // k_bvh.hip k_bvh_wide: 4-wide nodes (64 B) + leaf records (48 B), regenerated whenever `bvh` changed; the topology arrays only when the tree was rebuilt
    DeviceArray bvh_wide /* the nodes, then the leaf records */, wide_topo, wide_leaf_entry; uint32_t wide_nodes = 0, wide_leaves = 0, wide_root = 0, wide_links16 = 0, wide_for_entries = 0;
    uint64_t wide_topology_serial = 0;   // which build_wide_topology() result this copy holds
    // ST_BVH_BUILD_DEVICE (k_lbvh.hip): this copy's wide stream was built on the device from its own triangle arrays; `bvh` (the contract
    // stream) is then stale and no launch may read it. lb_live: live triangles of that build. The rest is the builder's scratch.
    bool device_built = false; uint32_t lb_live = 0; uint64_t tri_info_serial = 0;
    uint64_t lb_serial = ~0ull; uint32_t lb_slots = 0;   // tri_info_serial_ / triangle slots of the copy's last device BUILD (a refit needs both unchanged)
    DeviceArray tri_info, lb_keys_a, lb_keys_b, lb_temp, lb_seg, lb_children, lb_node_box, lb_small;
    // ST_BVH_REFIT_DEVICE: what k_bvh.hip needs beside the stream and the copy's hit-test records and bounds — per triangle slot the
    // device entry that holds it; per entry its parent (entry << 1 | child slot); the leaf runs; an arrival counter per entry.
    // tree_version says which build of the tree these (and the stream's topology) belong to.
    DeviceArray entry_of_tri, parent, refit_local, refit_items, refit_batch_off;
    uint64_t tree_version = 0;

    // ---- the device bake (st_scene.cpp bake_on_device): what k_bvh_bake patches beside the triangle arrays — the stream's leaf entries, found
    // through the slot index; none on a copy whose tree was built on the device (it has no contract stream)
    float4* patch_stream() const { return bvh.as<float4>(); }
    const uint32_t* patch_index() const { return device_built ? nullptr : entry_of_tri.as<uint32_t>(); }
};

struct SceneTree {
    Engine& e;   // its triangle slots (read through TriangleSlots' accessors; set_live is the one call that changes them), its materials and instances, its scene copies and their fences, its tuning, its staging ring, its device
    explicit SceneTree(Engine& engine) : e(engine) {}

    // ---- the host's binned-SAH tree, its contract stream and the stream's device form
    BvhBuild bvh;
    std::vector<float4> bvh_stream, bvh_upload_;
    // BVH refresh policy (st_set_bvh_refresh). Refit: while the set of (triangle slot, material) pairs and the Blend flags
    // are what the last build saw — i.e. instances only moved — keep the tree and recompute the boxes bottom-up.
    int bvh_refresh_mode = ST_BVH_AUTO;   // (host-only engines, the exact build and observed contract streams: what ST_BVH_REBUILD does)
    bool have_topology = false; uint64_t topology_signature = 0;
    std::vector<uint32_t> internal_positions;  // stream offsets of the internal nodes, ascending (parents before children)
    uint64_t refits = 0, rebuilds = 0;
    uint64_t device_refits = 0;    // ticks whose boxes were recomputed on the device
    uint64_t tree_version = 0;     // bumped by every rebuild (ST_BVH_REFIT_DEVICE: a scene copy whose arrays are of this version can be refitted in place)
    bool host_stream_stale = false;  // device refits happened since bvh_stream's boxes were last recomputed (host_stream refits it first)
    std::vector<float4> readback_; uint32_t live_bvh_texels = 0;  // debug_read(Live*)
    std::vector<uint32_t> entry_of_tri_, parent_, refit_local_, refit_items_, refit_batch_off_;  // host images of the device refit's index arrays (index_device_tree)
    std::vector<uint32_t> readback_levels_;
    std::vector<std::pair<uint32_t, uint32_t>> refit_levels_;  // (first batch, batches) of each launch, leaves first
    // Deepest chain of internal nodes in the uploaded stream = the most entries a traversal can have pending (every internal
    // node on the path may push its far child). The kernels' per-lane stack holds kBvhStackSize entries (strolle-gpu/src/lib.rs:76;
    // the reference indexes past the end there, here a push beyond the end is dropped): a deeper tree is reported, not hidden.
    // (round 5) Up to kBvhStackSizeDeep the launches take a deeper stack instead (dynamic LDS): `stack_entries` is what this tree's launches hold.
    uint32_t bvh_stack_need = 0, stack_entries = (uint32_t)kBvhStackSize; bool bvh_depth_warned = false, bvh_too_deep_unreported = false;
    void measure_stack_need();
    // Device form of the stream (st_types.h "device BVH stream"): every entry four texels — an internal node as the
    // serializer wrote it (far pointer remapped), a leaf entry followed by its triangle's hit-test record — so that one
    // four-texel fetch serves a traversal step of either kind. Entry k starts at texel 4 k.
    std::vector<uint32_t> expand_map_;  // scratch: offset in bvh_stream -> texel pointer in bvh_upload_ (entry starts only)
    uint32_t device_bvh_len = 0; bool device_root_is_leaf = false;
    void expand_stream();
    void index_device_tree();
    std::vector<uint8_t> internal_start_;  // scratch of measure_stack_need: 1 where an internal node begins
    bool is_internal_start(size_t p) const { return p < internal_start_.size() && internal_start_[p]; }
    void mark_internal_starts();
    // the wide stream's topology (build_wide_topology), from bvh_upload_: 8 words per node (4 box sources, 4 links) and the
    // contract entry of every leaf record; wide_serial_ counts the builds
    std::vector<uint32_t> wide_topo_, wide_leaf_entry_; uint32_t wide_root_ = 0, wide_stack_need_ = 0; uint64_t wide_serial_ = 0; uint64_t wide_built_for_ = ~0ull;
    void build_wide_topology();
    int refresh_wide_stream(TreeCopy& t, hipStream_t up, bool topology_changed, bool* pageable);
    int refresh_compact_stream(TreeCopy& t, hipStream_t up);

    uint64_t topology_of(const std::vector<uint8_t>& blend) const;
    void index_stream();
    Aabb subtree_box(size_t p) const;
    void refit_node(size_t p);
    void refit_span(size_t begin, size_t end);
    // One thread: at 134 k triangles the sweep is about a millisecond, less than starting a worker pool for it would buy back.
    void refit_stream() { refit_span(0, bvh_stream.size()); }
    bool device_refit_possible() const;
    // ST_BVH_BUILD_DEVICE: the tree of a changed scene is built on the device (k_lbvh.hip) while nothing observes the contract stream
    bool host_tree_stale = false;    // the host's binned-SAH tree (bvh_stream and everything derived from it) is behind the scene
    uint64_t device_builds = 0, device_tree_refits = 0;   // ticks answered by a device build / by a refit of the device-built tree (moves only)
    static constexpr uint32_t kDeviceRefitsPerBuild = 15;   // moves-only ticks answered by a refit of the device-built tree between two builds
    bool device_tree_refit_now = false; uint32_t device_refits_since_build = 0;
    size_t info_dirty_lo_ = SIZE_MAX, info_dirty_hi_ = 0; bool info_full_ = true;   // slots whose word may have changed since tri_info_ was listed (spawned, removed); everything (materials changed)
    std::vector<uint32_t> tri_info_; uint32_t tri_info_live_ = 0; uint64_t tri_info_serial_ = 1, tri_info_built_for_ = 0;   // per slot: live | Blend << 1 | material << 2; the serial counts what can change it
    // ST_BVH_AUTO's choice of a scene's FIRST tree (device_build_possible): host_leaf_run_weight = the surface-area-weighted mean length of the host
    // tree's leaf runs (rebuild_host_tree); above kAutoLeafRunLimit the device builder's tree renders faster (profiles/r06_tree_choice*.txt)
    static constexpr float kAutoLeafRunLimit = 3.4f;
    float host_leaf_run_weight = 1.0f; bool auto_first_on_device = false;
    bool device_build_possible() const;
    int build_on_device(SceneSet& t, hipStream_t up, bool* pageable);
    int reserve_device_builder(TreeCopy& t, size_t slots, uint32_t live);
    void rebuild_host_tree(bool timing);

    // ---- st_tick: the refresh
    // the triangle slots [b, end) were taken or given back; slots, liveness, materials or Blend flags may have changed (`materials`: under any slot)
    void slots_changed(size_t b, size_t end) { info_dirty_lo_ = std::min(info_dirty_lo_, b); info_dirty_hi_ = std::max(info_dirty_hi_, end); }
    void slots_changed(bool materials) { if (materials) info_full_ = true; tri_info_serial_++; }
    // whether instances that only moved are left to the device's bake (st_scene.cpp refresh_instances): a tree that follows them there is on record
    bool moves_stay_on_device() const;
    // every tree decision of a tick and its counter, except `rebuilds` (rebuild_host_tree: a debug read rebuilds too) and `device_refits` (write:
    // whether the written copy can be refitted). t0: when the refresh began (StTuning::tick_timing's lines say what the bake took)
    TreePlan plan(bool instances_changed, bool moved_on_device, bool materials_changed, TickClock::time_point t0);
    // ---- st_tick: the upload. The tree half of copy `t`, as `plan` says: a device build or refit of its tree, a device refit of the host tree's boxes,
    // or the host's streams with their index arrays, compact and wide forms. *attr_sent: the copy's attribute records went with it.
    int write(SceneSet& t, TreePlan plan, hipStream_t up, bool* pageable, bool* attr_sent);
    void went_live(TreePlan plan) { live_bvh_texels = plan == TreePlan::device_build || plan == TreePlan::device_refit ? 0u : device_bvh_len; }   // the written copy is the live one now
    int report_too_deep();   // report_deep_bvh's half: ST_ERR_BVH_TOO_DEEP once per build

    // ---- the frames and the scene queries (st_render.cpp scene_args): which stream of copy `t` the rays walk (contract, compact or wide), its roots
    // and link mask, the stack they hold
    int walk_args(const TreeCopy& t, KArgs& a, bool heatmap) const;

    // ---- derived state, through accessors that bring it up to date
    const std::vector<float4>& host_stream() { if (host_stream_stale) { refit_stream(); host_stream_stale = false; } return bvh_stream; }   // with current boxes
    const std::vector<float4>& device_form() { host_stream(); expand_stream(); return bvh_upload_; }   // of the stream as it is now: as st_tick would upload it
    void refit_index() { index_device_tree(); }   // the device refit's index arrays, of the device form just taken
    void wide_topology(bool for_tick);            // of the device form just taken; a tick keeps its own (a debug read's is nobody's: a later tick builds its own)
    // st_debug_read_scene's tree cases (include/strolle_hip.h; the numbers are the ABI's)
    enum DebugRead { ContractStream = 0, DeviceForm = 4, LiveStream = 6, RefitParent = 7, RefitLocal = 8, RefitItems = 9, RefitBatchOff = 10, RefitLevels = 11,
                     RefitEntryOfTri = 12, RefitBounds = 13, WideTopology = 14, WideLeafEntry = 15, LiveWideNodes = 16, LiveWideLeaves = 17 };
    static bool debug_reads(int what) { return what == ContractStream || what == DeviceForm || (what >= LiveStream && what <= LiveWideLeaves); }
    int debug_read(int what, const void** p, size_t* bytes);

    // ---- the C ABI's counters and switches
    void set_refresh_mode(int mode) { if (bvh_refresh_mode != mode) { bvh_refresh_mode = mode; have_topology = false; } }
    void refit_stats(uint64_t* rebuilt, uint64_t* refitted) const { *rebuilt = rebuilds; *refitted = refits; }
    void depth(uint32_t* deepest_internal_chain, uint32_t* entries) const { *deepest_internal_chain = bvh_stack_need; *entries = stack_entries; }
    void auto_tree(float* leaf_run_weight, uint32_t* first_tree_on_device) const { *leaf_run_weight = host_leaf_run_weight; *first_tree_on_device = auto_first_on_device ? 1u : 0u; }
    void refresh_stats(uint64_t* primitives, uint64_t* reused) { *primitives = bvh.prims.size(); *reused = bvh.reused_primitives(); }
    uint64_t device_refit_ticks() const { return device_refits; }
    uint64_t device_build_ticks() const { return device_builds; }
    uint64_t device_tree_refit_ticks() const { return device_tree_refits; }
};

}  // namespace st
