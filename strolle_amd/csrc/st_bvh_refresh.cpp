// st_bvh_refresh.cpp — host engine of libstrolle_hip.so: the scene's BVH (st_bvh_refresh.h): the derivations (device form of the stream, host refit, the
// device refit's index arrays, wide topology, stack-depth check), the host tree and the device builder, the tick's plan and the tree half of its upload,
// the walks' arguments, the debug reads. See st_engine.h.
#include "st_engine.h"

#include <cstdlib>
namespace st {

void SceneTree::measure_stack_need() {
    std::vector<uint8_t> height(bvh_stream.size() + 1, 0);  // internal nodes only; a leaf run has height 0
    uint32_t deepest = 0;
    for (size_t p = bvh_stream.size(); p-- > 0;) {
        // walk backwards; an internal node starts where d0.w == 0 and the 3 texels after it are its own
        if (p + 3 < bvh_stream.size() && f2b(bvh_stream[p].w) == 0u && is_internal_start(p)) {
            const size_t l = p + 4, r = f2b(bvh_stream[p + 1].w);
            const uint32_t h = 1u + std::max<uint32_t>(l < height.size() ? height[l] : 0, r < height.size() ? height[r] : 0);
            height[p] = (uint8_t)std::min<uint32_t>(h, 255u);
            deepest = std::max(deepest, h);
        }
    }
    bvh_stack_need = deepest;
    // A ray's pending stack never holds more entries than the deepest chain of internal nodes (every node on the path pushes at most its far
    // child): up to kBvhStackSize (24, the reference's) the launches keep the reference's stack, up to kBvhStackSizeDeep (32) they take the
    // deep one — more LDS per block, no dropped push. Beyond that a tree is reported through st_tick's status (ST_ERR_BVH_TOO_DEEP, once per
    // build) — or, with StTuning::allow_deep_bvh, once on stderr.
    stack_entries = std::min<uint32_t>(std::max<uint32_t>(deepest, (uint32_t)kBvhStackSize), (uint32_t)kBvhStackSizeDeep);   // exactly what the tree needs: LDS per block decides occupancy
    bvh_too_deep_unreported = deepest > stack_entries;
    if (bvh_too_deep_unreported && e.tuning.allow_deep_bvh && !bvh_depth_warned) {
        bvh_depth_warned = true;
        fprintf(stderr, "[strolle-hip] warning: the BVH is %u internal nodes deep; traversal keeps %d pending entries per ray (as the reference does) and drops deeper ones — distant geometry may be missed. st_debug_bvh_depth reports this.\n", deepest, (int)stack_entries);
    }
}

void SceneTree::expand_stream() {
    const size_t n = bvh_stream.size();
    expand_map_.resize(n);
    size_t entries = 0;
    for (size_t p = 0; p < n; p += f2b(bvh_stream[p].w) == 0u ? 4 : 1) expand_map_[p] = (uint32_t)(4 * entries++);
    bvh_upload_.resize(4 * std::max<size_t>(entries, 1));
    if (!entries) for (float4& t : bvh_upload_) t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    size_t o = 0;
    for (size_t p = 0; p < n; o += 4) {
        if (f2b(bvh_stream[p].w) == 0u) {
            for (int k = 0; k < 4; k++) bvh_upload_[o + k] = bvh_stream[p + k];
            bvh_upload_[o + 1].w = b2f(expand_map_[f2b(bvh_stream[p + 1].w)] * 16u);  // far pointer as a byte offset
            p += 4;
        } else {
            const uint32_t tri = f2b(bvh_stream[p].y);
            bvh_upload_[o] = bvh_stream[p];
            for (int k = 0; k < 3; k++) bvh_upload_[o + 1 + k] = e.slots.geo()[3 * (size_t)tri + k];
            p += 1;
        }
    }
    device_bvh_len = (uint32_t)(4 * entries);
    device_root_is_leaf = entries != 0 && f2b(bvh_upload_[0].w) != 0u;
}

// Index arrays of the device refit, from the device form of the stream (bvh_upload_, entries of four texels): per triangle
// slot its leaf entry, per entry its parent (entry << 1 | child slot), and the work list of k_bvh_refit.
// The refit must not pass data between workgroups inside a launch (XCD L2s are not coherent; an agent-scope fence per node
// measured 2.1 ms for 208 k triangles), so the tree is cut into TASKS — maximal subtrees with at most kRefitBatch leaves —,
// each refitted bottom-up by one workgroup that keeps the child boxes in LDS. Finished task roots are the leaves of the next
// LEVEL (their boxes already sit in the stream, in their parent's entry), one launch per level: two for 208 k triangles.
// Small tasks share a workgroup (a batch: <= kRefitBatch items, LDS slots numbered within the batch).
// items: leaf entry of a run's first triangle, or (1 << 31 | entry) for a finished task root; refit_local_[entry]: the LDS slot
// of an internal node, bit 31 set on a task's root.
void SceneTree::index_device_tree() {
    const uint32_t n_entries = device_bvh_len / 4u;
    entry_of_tri_.assign(e.slots.size(), 0xffffffffu);
    parent_.assign(std::max<uint32_t>(n_entries, 1u), 0xffffffffu);
    refit_local_.assign(std::max<uint32_t>(n_entries, 1u), 0u);
    refit_items_.clear(); refit_batch_off_.assign(1, 0u); refit_levels_.clear();
    std::vector<uint32_t> internals;
    auto internal = [&](uint32_t k) { return f2b(bvh_upload_[4u * (size_t)k].w) == 0u; };
    auto child = [&](uint32_t k, int which) { return which ? f2b(bvh_upload_[4u * (size_t)k + 1u].w) / 64u : k + 1u; };
    for (uint32_t k = 0; k < n_entries; k++) {
        if (internal(k)) {
            parent_[child(k, 0)] = (k << 1) | 0u;
            parent_[child(k, 1)] = (k << 1) | 1u;
            internals.push_back(k);
        } else entry_of_tri_[f2b(bvh_upload_[4u * (size_t)k].y)] = k;
    }
    std::vector<uint32_t> leaves(n_entries, 0u);  // of an unfinished internal node: runs + finished task roots beneath it
    std::vector<uint8_t> finished(n_entries, 0);
    std::vector<uint32_t> stack;
    for (size_t left = internals.size(); left;) {
        for (size_t i = internals.size(); i-- > 0;) {   // children sit behind their parent
            const uint32_t k = internals[i];
            if (finished[k]) continue;
            uint32_t n = 0;
            for (int c = 0; c < 2; c++) { const uint32_t ck = child(k, c); n += internal(ck) && !finished[ck] ? leaves[ck] : 1u; }
            leaves[k] = n;
        }
        const uint32_t first_batch = (uint32_t)refit_batch_off_.size() - 1u;
        uint32_t in_batch = 0, slots = 0;
        for (const uint32_t k : internals) {
            if (finished[k] || leaves[k] > kRefitBatch) continue;
            // finished[] of a task's nodes is set when its root is met, so an unfinished node here has no parent in a task
            if (in_batch + leaves[k] > kRefitBatch) { refit_batch_off_.push_back((uint32_t)refit_items_.size()); in_batch = 0; slots = 0; }
            in_batch += leaves[k];
            stack.assign(1, k);
            while (!stack.empty()) {
                const uint32_t n = stack.back(); stack.pop_back();
                refit_local_[n] = slots++ | (n == k ? 0x80000000u : 0u);
                finished[n] = 1; left--;
                for (int c = 1; c >= 0; c--) {
                    const uint32_t ck = child(n, c);
                    if (!internal(ck)) refit_items_.push_back(ck);
                    else if (finished[ck]) refit_items_.push_back(ck | 0x80000000u);
                    else stack.push_back(ck);
                }
            }
        }
        if (in_batch) refit_batch_off_.push_back((uint32_t)refit_items_.size());
        refit_levels_.push_back({first_batch, (uint32_t)refit_batch_off_.size() - 1u - first_batch});
    }
}

// The WIDE stream's topology (k_bvh.hip k_bvh_wide; st_traverse.h closest_hit_wide): the binary tree of the device stream (bvh_upload_,
// entries of four texels) collapsed top-down into nodes of up to four children — a node's two children are replaced by their own children,
// largest surface area first, until there are four or only leaf runs are left (tools/bvh4_sim.py: 3.1 children per node on the dungeon,
// half the node steps per ray). Wide nodes are numbered in depth-first order, leaf records in stream order (a run's records stay
// consecutive). Only WHICH boxes a node holds is decided here; the boxes themselves are read on the device, from the device's stream.
void SceneTree::build_wide_topology() {
    const uint32_t n_entries = device_bvh_len / 4u;
    wide_topo_.clear(); wide_leaf_entry_.clear(); wide_root_ = 0u; wide_stack_need_ = 0u; wide_serial_++;
    if (!n_entries) return;
    auto internal = [&](uint32_t k) { return f2b(bvh_upload_[4u * (size_t)k].w) == 0u; };
    auto far_child = [&](uint32_t k) { return f2b(bvh_upload_[4u * (size_t)k + 1u].w) / 64u; };
    auto area = [&](uint32_t src) {   // of the box stored at (entry << 1 | slot)
        const float4 lo = bvh_upload_[4u * (size_t)(src >> 1) + 2u * (src & 1u)], hi = bvh_upload_[4u * (size_t)(src >> 1) + 2u * (src & 1u) + 1u];
        const float dx = std::max(hi.x - lo.x, 0.0f), dy = std::max(hi.y - lo.y, 0.0f), dz = std::max(hi.z - lo.z, 0.0f);
        return dx * dy + dy * dz + dz * dx;
    };
    std::vector<uint32_t> leaf_index(n_entries, 0u);
    for (uint32_t k = 0; k < n_entries; k++) if (!internal(k)) { leaf_index[k] = (uint32_t)wide_leaf_entry_.size(); wide_leaf_entry_.push_back(k); }
    if (!internal(0u)) { wide_root_ = 1u; return; }   // the whole tree is one leaf run: leaf record 0
    struct Child { uint32_t src, entry; };
    std::vector<uint32_t> head;             // binary entry that heads wide node i
    std::vector<Child> kids;                // 4 per node (src = ~0: empty)
    std::vector<uint32_t> node_of(n_entries, 0xffffffffu);
    std::vector<uint32_t> todo{0u};
    while (!todo.empty()) {
        const uint32_t k = todo.back(); todo.pop_back();
        node_of[k] = (uint32_t)head.size(); head.push_back(k);
        Child ch[4]; int n = 2;
        ch[0] = {(k << 1) | 0u, k + 1u}; ch[1] = {(k << 1) | 1u, far_child(k)};
        while (n < 4) {
            int pick = -1; float best = -1.0f;
            for (int i = 0; i < n; i++) if (internal(ch[i].entry)) { const float ar = area(ch[i].src); if (ar > best) { best = ar; pick = i; } }
            if (pick < 0) break;
            const uint32_t e = ch[pick].entry;
            for (int i = n; i > pick + 1; i--) ch[i] = ch[i - 1];   // the two grandchildren take the child's place, in order
            ch[pick] = {(e << 1) | 0u, e + 1u}; ch[pick + 1] = {(e << 1) | 1u, far_child(e)};
            n++;
        }
        for (int i = 0; i < 4; i++) kids.push_back(i < n ? ch[i] : Child{0xffffffffu, 0u});
        for (int i = n - 1; i >= 0; i--) if (internal(ch[i].entry)) todo.push_back(ch[i].entry);   // depth first: the first child's subtree follows its parent
    }
    // the most entries a walk over the wide nodes can have pending: descending into one of a node's n children leaves at most n - 1 behind
    // (children sit behind their parent in `head`, so a backward sweep sees finished children)
    {
        std::vector<uint32_t> need(head.size(), 0u);
        for (size_t i = head.size(); i-- > 0;) {
            uint32_t n = 0, below = 0;
            for (int c = 0; c < 4; c++) {
                const Child& q = kids[4u * i + c];
                if (q.src == 0xffffffffu) continue;
                n++;
                if (internal(q.entry)) below = std::max(below, need[node_of[q.entry]]);
            }
            need[i] = (n ? n - 1u : 0u) + below;
        }
        wide_stack_need_ = head.empty() ? 0u : need[0];
    }
    wide_topo_.resize(8u * head.size());
    for (size_t i = 0; i < head.size(); i++)
        for (int c = 0; c < 4; c++) {
            const Child& q = kids[4u * i + c];
            wide_topo_[8u * i + c] = q.src;
            wide_topo_[8u * i + 4u + c] = q.src == 0xffffffffu ? 0u : (internal(q.entry) ? (node_of[q.entry] << 1) : ((leaf_index[q.entry] << 1) | 1u));
        }
    wide_root_ = 0u;
}

void SceneTree::mark_internal_starts() {
    internal_start_.assign(bvh_stream.size(), 0);
    for (size_t p = 0; p < bvh_stream.size();) {
        if (f2b(bvh_stream[p].w) == 0u) { internal_start_[p] = 1; p += 4; } else p += 1;
    }
}

// ---- BVH refit (the alternative to a rebuild when instances only move)
// What the leaves of the current tree refer to: every live (triangle slot, material) pair, plus the Blend flags baked into
// the leaf entries. Equal signatures mean the stream's topology and leaf entries are still right; only boxes moved.
uint64_t SceneTree::topology_of(const std::vector<uint8_t>& blend) const {
    uint64_t h = 0x9e3779b97f4a7c15ull;
    auto mix = [&h](uint64_t v) { h = (h ^ v) * 0x100000001b3ull; h ^= h >> 29; };
    for (size_t i = 0; i < e.slots.size(); i++) if (e.slots.alive()[i]) mix(((uint64_t)i << 32) | e.slots.prims()[i].material_id);
    mix(0xffffffffffffffffull);
    for (uint8_t b : blend) mix(b);
    return h;
}

// offsets of the internal nodes of bvh_stream, in stream order (serializer.rs:20-110: a node is internal when d0.w == 0)
void SceneTree::index_stream() {
    internal_positions.clear();
    for (size_t p = 0; p < bvh_stream.size();) {
        if (f2b(bvh_stream[p].w) == 0u) { internal_positions.push_back((uint32_t)p); p += 4; }
        else p += 1;
    }
}

// box of the subtree that starts at stream offset p: a run of leaf entries (triangle bounds as baked) or an internal node
// (union of the two child boxes it stores)
Aabb SceneTree::subtree_box(size_t p) const {
    Aabb box;
    if (f2b(bvh_stream[p].w) == 0u) {
        box.grow(v3(bvh_stream[p].x, bvh_stream[p].y, bvh_stream[p].z)); box.grow(v3(bvh_stream[p + 1].x, bvh_stream[p + 1].y, bvh_stream[p + 1].z));
        box.grow(v3(bvh_stream[p + 2].x, bvh_stream[p + 2].y, bvh_stream[p + 2].z)); box.grow(v3(bvh_stream[p + 3].x, bvh_stream[p + 3].y, bvh_stream[p + 3].z));
        return box;
    }
    for (;; p++) {
        const float4* b = &e.slots.bounds()[2u * (size_t)f2b(bvh_stream[p].y)];  // = prims[...].bounds, 32 B apart instead of 56
        box.grow(v3(b[0].x, b[0].y, b[0].z)); box.grow(v3(b[1].x, b[1].y, b[1].z));
        if (!(f2b(bvh_stream[p].x) & 1u)) return box;
    }
}

void SceneTree::refit_node(size_t p) {
    const Aabb l = subtree_box(p + 4), r = subtree_box(f2b(bvh_stream[p + 1].w));
    bvh_stream[p] = make_float4(l.lo.x, l.lo.y, l.lo.z, bvh_stream[p].w);
    bvh_stream[p + 1] = make_float4(l.hi.x, l.hi.y, l.hi.z, bvh_stream[p + 1].w);
    bvh_stream[p + 2] = make_float4(r.lo.x, r.lo.y, r.lo.z, bvh_stream[p + 2].w);
    bvh_stream[p + 3] = make_float4(r.hi.x, r.hi.y, r.hi.z, bvh_stream[p + 3].w);
}

// internal nodes whose offsets lie in [begin, end), last to first: children sit behind their parent in the stream, so a
// backward sweep sees finished children
void SceneTree::refit_span(size_t begin, size_t end) {
    const auto lo = std::lower_bound(internal_positions.begin(), internal_positions.end(), (uint32_t)begin);
    auto hi = std::lower_bound(internal_positions.begin(), internal_positions.end(), (uint32_t)end);
    while (hi != lo) refit_node(*--hi);
}

// ---- the host tree and the device builder
// The host's binned-SAH tree of the scene as it is now (st_bvh.h: the reference's tree, with unchanged subtrees reused) and its flattened stream.
void SceneTree::rebuild_host_tree(bool timing) {
    if (e.instances.any_host_stale()) e.bake_stale_on_host();
    const std::vector<uint8_t> blend = e.materials.blend_flags();
    const auto t1 = TickClock::now();
    bvh.begin_refresh();  // keeps the previous tree: unchanged subtrees are copied, not rebuilt (same result as a fresh build)
    for (size_t i = 0; i < e.slots.size(); i++) if (e.slots.alive()[i]) bvh.prims.push_back(e.slots.prims()[i]);
    const auto t2 = TickClock::now();
    bvh.run();
    const auto t3 = TickClock::now();
    bvh.flatten(blend, bvh_stream);
    const auto t4 = TickClock::now();
    {   // what ST_BVH_AUTO's choice of the first tree rests on (device_build_possible): the surface-area-weighted mean length of this tree's leaf runs
        double weighted = 0.0, area = 0.0;
        std::vector<uint32_t> todo;
        if (!bvh.nodes.empty() && !bvh.prims.empty()) todo.push_back(0u);
        while (!todo.empty()) {
            const auto& n = bvh.nodes[todo.back()]; todo.pop_back();
            if (n.internal) { todo.push_back(n.left); todo.push_back(n.right); continue; }
            const double a = (double)n.bounds.half_area();
            if (a > 0.0 && a < 1e300) { weighted += a * (double)(n.end - n.begin); area += a; }
        }
        host_leaf_run_weight = area > 0.0 ? (float)(weighted / area) : 1.0f;
    }
    rebuilds++; tree_version++; host_stream_stale = false; host_tree_stale = false;
    mark_internal_starts(); measure_stack_need();
    have_topology = false;
    if (timing) fprintf(stderr, "[st_tick] gather %.2f ms, bvh build %.2f ms, flatten %.2f ms (%zu triangles, %zu reused)\n", ms_between(t1, t2), ms_between(t2, t3), ms_between(t3, t4), bvh.prims.size(), bvh.reused_primitives());
}
bool SceneTree::device_refit_possible() const { return bvh_refresh_mode == ST_BVH_REFIT_DEVICE && e.has_device; }
// ST_BVH_BUILD_DEVICE applies while nothing observes the contract stream (st_engine.h wide_only_tuning, heatmap_camera) — and there is a scene to sort.
bool SceneTree::device_build_possible() const {
    // ST_BVH_AUTO (the default since round 6): the FIRST tree of an engine is the host's — the reference's binned SAH, the better tree, paid once while a
    // scene loads. A scene that fits LDS keeps its contract stream there (k_common.h scene_fits_lds: a leaf entry per triangle, more than 112 never fit); a larger one sends its
    // CHANGES (spawn, despawn, move) to the device builder — and its FIRST tree too when the host's tree, built first, turns out to hang long leaf runs on large faces
    // (auto_first_on_device: plan sets it when rebuild_host_tree measured host_leaf_run_weight > kAutoLeafRunLimit). Measured on 17 scene x mode rows of 13 k to 537 k
    // triangles (tools/tree_choice.py, profiles/r06_tree_choice_auto.txt): at a weight of 3.0 or less the frames over the host's binned-SAH tree are up to 7 % faster than over
    // the device's LBVH (two rows: the device's by 1 and 6 %); at 3.7 the device's is 1-2 % faster; at 4.2-4.5 (the dungeon with its level split x16: runs of up to 140
    // coplanar triangles, a wide walk's step each) 5-17 % faster. A triangle COUNT does not separate them: 16 instanced copies of the level (139 k triangles, weight 1.8)
    // render 1-7 % faster on the host's tree, the x16-split level (134 k, weight 4.5) 12-17 % faster on the device's.
    const bool automatic = bvh_refresh_mode == ST_BVH_AUTO && (e.copies.scene.written || auto_first_on_device) && e.slots.live() > kLdsSceneTexels / 4u;
    if (!(bvh_refresh_mode == ST_BVH_BUILD_DEVICE || automatic) || !e.has_device || !e.wide_only_tuning() || e.heatmap_camera()) return false;
    return e.slots.live() >= 2u && e.slots.size() < (1u << 23);
}
bool SceneTree::moves_stay_on_device() const {
    // (ST_BVH_BUILD_DEVICE: the same, with the tree rebuilt on the device from the device-baked arrays instead of refitted)
    const bool build_mode = device_build_possible() && e.copies.scene.written;
    return (device_refit_possible() && have_topology) || build_mode;
}
// The device builder's scratch and output arrays of one scene copy, for `slots` triangle slots of which `live` are live: grown with headroom, never shrunk.
// Also called ahead of time (write, at the first upload of an engine whose later changes will be answered on the device): a spawn tick then allocates
// nothing (round 5: the first device build of each copy took 5-15 ms, all of it hipMalloc).
int SceneTree::reserve_device_builder(TreeCopy& t, size_t slots, uint32_t live) {
    if (live < 2u) return ST_OK;
    const uint32_t pow2 = lbvh_pow2(live);
    const size_t temp = lbvh_sort_temp_bytes((uint32_t)slots);
    auto need = [](DeviceArray& d, size_t bytes) { return d.reserve(bytes, bytes + bytes / 4); };
    int rc;
    if ((rc = need(t.lb_keys_a, slots * 8u)) || (rc = need(t.lb_keys_b, slots * 8u)) || (rc = need(t.lb_temp, std::max<size_t>(temp + temp / 4, 16u))) || (rc = need(t.lb_seg, (size_t)pow2 * 2u * 32u)) ||
        (rc = need(t.lb_children, (size_t)live * 8u)) || (rc = need(t.lb_node_box, (size_t)live * 32u)) ||
        (rc = need(t.lb_small, 64u)) || (rc = need(t.bvh_wide, (size_t)(live - 1u) * 64u + (size_t)live * 48u + 64u))) return rc;
    return ST_OK;
}
// This device copy's triangle arrays brought up to date, then k_lbvh.hip builds its wide stream from them.
int SceneTree::build_on_device(SceneSet& set, hipStream_t up, bool* pageable) {
    int rc;
    TreeCopy& t = set.tree;
    const size_t slots = e.slots.size();
    const auto t0 = TickClock::now();
    if (tri_info_built_for_ != tri_info_serial_ || tri_info_.size() != slots) {   // (a tick in which instances only moved changes none of this)
        auto word = [&](size_t i) {
            const uint32_t mat = e.slots.prims()[i].material_id;
            return (e.slots.alive()[i] ? 1u : 0u) | (e.materials.is_blend(mat) ? 2u : 0u) | (mat << 2);
        };
        if (info_full_ || tri_info_.size() != slots) {
            tri_info_.resize(slots);
            tri_info_live_ = 0;
            for (size_t i = 0; i < slots; i++) { tri_info_[i] = word(i); tri_info_live_ += tri_info_[i] & 1u; }
            e.slots.set_live(tri_info_live_);
        } else {   // only the slots an instance took or gave back since the last listing (208 k slots: the full listing was 0.25-0.35 ms of a 0.45-ms tick)
            for (size_t i = info_dirty_lo_; i < std::min(info_dirty_hi_, slots); i++) { const uint32_t w = word(i); tri_info_live_ += (w & 1u) - (tri_info_[i] & 1u); tri_info_[i] = w; }
        }
        info_full_ = false; info_dirty_lo_ = SIZE_MAX; info_dirty_hi_ = 0;
        tri_info_built_for_ = tri_info_serial_;
    }
    const uint32_t live = tri_info_live_;
    const auto t1 = TickClock::now();
    if ((rc = e.upload_tri_slots(set, Engine::TRI_GEO | Engine::TRI_ATTR, !set.valid || set.tri_full, up, pageable))) return rc;
    if (t.tri_info_serial != tri_info_serial_ || t.tri_info.capacity < slots * sizeof(uint32_t)) {
        if ((rc = t.tri_info.upload(tri_info_.data(), slots * sizeof(uint32_t), up, e.staging, pageable))) return rc;
        t.tri_info_serial = tri_info_serial_;
    }
    // instances that only moved are baked HERE from the object-space meshes (StTuning::device_bake, k_bvh.hip k_bvh_bake): the host bakes nothing for them
    const bool refit_tree = device_tree_refit_now && t.device_built && t.lb_live == live && t.lb_serial == tri_info_serial_ && t.lb_slots == (uint32_t)slots && live >= 2u;
    t.device_built = true;   // (bake_on_device: no contract stream to patch on this copy)
    const auto t2 = TickClock::now();
    if ((rc = e.bake_on_device(set, up, pageable))) return rc;
    const auto t3 = TickClock::now();
    const size_t temp = lbvh_sort_temp_bytes((uint32_t)slots);
    if ((rc = reserve_device_builder(t, slots, live))) return rc;
    LbvhArgs a{};
    a.tri_geo = static_cast<const float4*>(set.tri_geo.ptr); a.tri_bounds = static_cast<const float4*>(set.tri_bounds.ptr); a.tri_info = static_cast<const uint32_t*>(t.tri_info.ptr);
    a.slots = (uint32_t)slots; a.live = live; a.links16 = live < 32768u ? 1u : 0u;
    { static const char* v = getenv("ST_LBVH_CELL_ASPECT"); a.cell_aspect = v ? (float)atof(v) : kLbvhCellAspect; }
    a.nodes = static_cast<float4*>(t.bvh_wide.ptr); a.leaves = a.nodes + 4u * (size_t)(live - 1u);
    a.keys_in = static_cast<unsigned long long*>(t.lb_keys_a.ptr); a.keys_out = static_cast<unsigned long long*>(t.lb_keys_b.ptr);
    a.sort_temp = t.lb_temp.ptr; a.sort_temp_bytes = temp;
    a.seg = static_cast<float4*>(t.lb_seg.ptr); a.children = static_cast<uint2*>(t.lb_children.ptr); a.node_box = static_cast<float4*>(t.lb_node_box.ptr);
    a.bounds = static_cast<int*>(t.lb_small.ptr);
    // moves only, on a copy whose last build saw these very slots: the tree keeps its shape, every box follows (k_lbvh.hip lbvh_refit: 5 launches against 22)
    const char* what = refit_tree ? "refit" : "build";
    if ((refit_tree ? lbvh_refit(a, up) : lbvh_build(a, up)) != 0) return fail(ST_ERR_HIP, std::string("the device BVH ") + what + " failed to launch");
    if (e.tuning.tick_timing) fprintf(stderr, "[st_tick] device tree %s: slot words %.3f ms, uploads %.3f, bake launches %.3f, %s launches %.3f\n", what, ms_between(t0, t1), ms_between(t1, t2), ms_between(t2, t3), what, ms_between(t3, TickClock::now()));
    if (refit_tree) return ST_OK;
    t.lb_live = live; t.lb_serial = tri_info_serial_; t.lb_slots = (uint32_t)slots;
    t.wide_nodes = live - 1u; t.wide_leaves = live; t.wide_root = 0u; t.wide_links16 = a.links16; t.wide_for_entries = 0u; t.compact_entries = 0u;
    return ST_OK;
}

// ---- the tick's plan: what write does with the tree (st_tick.cpp refresh_scene has refreshed materials and instances)
TreePlan SceneTree::plan(bool instances_changed, bool moved_on_device, bool materials_changed, TickClock::time_point t0) {
    const bool timing = e.tuning.tick_timing;
    // ST_BVH_BUILD_DEVICE: while nothing observes the contract stream the changed scene's tree is built on the device (write, per device copy)
    // and the host's tree falls behind; the first tick that finds an observer brings it up to date like any rebuild.
    const bool build_now = device_build_possible();
    device_tree_refit_now = false;
    if (instances_changed && build_now) {
        // instances only moved (refresh_instances left them to the device's bake): the device-built tree is refitted, not rebuilt — at most
        // kDeviceRefitsPerBuild times in a row, then a rebuild restores the tree's quality (it costs 0.3 ms more at 208 k triangles)
        static const bool no_refit = getenv("ST_NO_DEVICE_TREE_REFIT") != nullptr;
        device_tree_refit_now = moved_on_device && !materials_changed && !no_refit && device_builds > 0 && device_refits_since_build < kDeviceRefitsPerBuild;
        if (device_tree_refit_now) { device_tree_refits++; device_refits_since_build++; } else { device_builds++; device_refits_since_build = 0; }
        host_tree_stale = true;
        if (timing) fprintf(stderr, "[st_tick] bake %.2f ms, tree: on the device\n", ms_between(t0, TickClock::now()));
        return device_tree_refit_now ? TreePlan::device_refit : TreePlan::device_build;
    }
    if (instances_changed || (host_tree_stale && !build_now)) {
        const auto t1 = TickClock::now();
        const bool refitting = bvh_refresh_mode == ST_BVH_REFIT || bvh_refresh_mode == ST_BVH_REFIT_DEVICE;
        // (moved_on_device: refresh_instances saw nothing but transforms change — slots, materials and Blend flags are what the last build saw)
        const uint64_t signature = moved_on_device ? topology_signature : (refitting ? topology_of(e.materials.blend_flags()) : 0);
        if (refitting && have_topology && !host_tree_stale && signature == topology_signature) {
            // ST_BVH_REFIT_DEVICE: the boxes are recomputed on the device from the moved triangles' bounds (k_bvh.hip); the host's
            // copy of the stream is brought up to date only when something reads it
            if (device_refit_possible()) host_stream_stale = true; else refit_stream();
            refits++;
            if (timing) fprintf(stderr, "[st_tick] bake %.2f ms, refit %.2f ms (%zu internal nodes)\n", ms_between(t0, t1), ms_between(t1, TickClock::now()), internal_positions.size());
            return TreePlan::host_refit;
        }
        rebuild_host_tree(timing);
        if (refitting) { index_stream(); topology_signature = signature; have_topology = true; }
        // the first tree of this scene: the host's, unless it hangs long leaf runs on large faces — then the device builder's, from this very tick on.
        // (finding 1: "first" is the first tick, !scene.written — also when the scene is still empty or half loaded then)
        if (!e.copies.scene.written && bvh_refresh_mode == ST_BVH_AUTO) {
            auto_first_on_device = host_leaf_run_weight > kAutoLeafRunLimit;
            if (auto_first_on_device && device_build_possible()) { device_builds++; device_refits_since_build = 0; return TreePlan::device_build; }
        }
        return TreePlan::host_rebuild;
    }
    // Nothing changed, the host's tree is current (a debug read rebuilt it) — but the live device copy still holds a device-built tree and no contract
    // stream, and an observer has appeared (heatmap camera, exact arithmetic, byte counting): the host's streams are uploaded now, so that the render
    // after THIS tick finds them (include/strolle_hip.h ST_BVH_BUILD_DEVICE: "a heatmap camera created later renders after the next st_tick").
    if (e.copies.scene.written && e.copies.scene.current().tree.device_built && !build_now) return TreePlan::host_to_observer;
    // The tree is as it was; a material or atlas edit (or the first upload) still sends the scene. (finding 2: under ST_BVH_AUTO a material-only edit replaces a current host tree by the device's, without device_builds++)
    return build_now && (materials_changed || !e.copies.scene.written) ? TreePlan::device_build : TreePlan::none;
}

// ---- the tree half of the scene's upload (st_tick.cpp upload_scene picked the copy and the stream)
int SceneTree::write(SceneSet& set, TreePlan plan, hipStream_t up, bool* pageable, bool* attr_sent) {
    int rc;
    TreeCopy& t = set.tree;
    const bool build_now = plan == TreePlan::device_build || plan == TreePlan::device_refit;
    // (finding 4: the reservation asks the tuning half of "nothing observes the contract stream", not the camera half)
    if (!e.copies.scene.written && (bvh_refresh_mode == ST_BVH_AUTO || bvh_refresh_mode == ST_BVH_BUILD_DEVICE) && e.wide_only_tuning() && e.slots.live() > kLdsSceneTexels / 4u && e.slots.size() < (1u << 23)) {
        // this scene's changes (and, for a large scene, its first tree: device_build_possible) go to the device builder: its arrays are allocated NOW, while the
        // scene loads, for both copies — BEFORE the wide stream of this copy is written below (its allocation is one of them: growing it afterwards would throw the stream away: round 6's
        // first version did, and rendered an empty world). A failure here is not an error: the build allocates what it finds missing.
        // ... and the host's triangle arrays get the same headroom now, so that the first spawn does not reallocate and copy them (60 MB at 208 k triangles: 7 ms)
        e.slots.reserve(e.slots.size() + e.slots.size() / 8u);
        bool reserved = true;
        for (SceneSet& s : e.copies.scene.copy)
            if (reserve_device_builder(s.tree, e.slots.size() + e.slots.size() / 8u, (uint32_t)std::min<size_t>(e.slots.live() + e.slots.live() / 8u, e.slots.size() + e.slots.size() / 8u)) != ST_OK) { (void)hipGetLastError(); reserved = false; break; }
        if (reserved && !build_now && e.copies.scene.copy[0].tree.lb_small.ptr) lbvh_warm(static_cast<int*>(e.copies.scene.copy[0].tree.lb_small.ptr), up);   // ... and the builder's code object is on the device before the first spawn
    }
    if (build_now) {
        // (instances the device moved stay stale on the host: this copy's pending list re-bakes them on the device even after a whole upload)
        if ((rc = build_on_device(set, up, pageable))) return rc;
        host_tree_stale = true;   // whatever made this tick upload (a material edit, too): the live copy's tree is no longer the host's
        t.tree_version = 0;       // ... and this copy's contract stream and refit arrays belong to no host tree any more
    } else t.device_built = false;
    const bool device_path = !build_now && device_refit_possible() && set.valid && !set.tri_full && t.tree_version == tree_version && e.tri_fits(set, Engine::TRI_GEO);
    *attr_sent = build_now;   // (build_on_device sent them)
    // a copy that cannot be brought up to date in place is sent whole, from the host's arrays: instances the device moved must be in them
    if (!device_path && !build_now && e.instances.any_host_stale()) e.bake_stale_on_host();
    if (device_path) {
        // This copy holds the current tree; only boxes and moved triangles are behind. Send the records and bounds of the
        // triangle slots baked since it was written and let the device patch its leaf entries and refit its boxes.
        if (set.dirty_lo < set.dirty_hi) {
            if ((rc = e.upload_tri_slots(set, Engine::TRI_GEO, false, up, pageable))) return rc;
            e.L.launch_bvh_patch_leaves(static_cast<float4*>(t.bvh.ptr), static_cast<const float4*>(set.tri_geo.ptr), static_cast<const uint32_t*>(t.entry_of_tri.ptr), (uint32_t)set.dirty_lo, (uint32_t)set.dirty_hi, up);
            if (e.tri_fits(set, Engine::TRI_ATTR)) {   // (an array that grew goes whole behind this, after the bake)
                if ((rc = e.upload_tri_slots(set, Engine::TRI_ATTR, false, up, pageable))) return rc;
                *attr_sent = true;
            }
        }
        // instances that only moved are baked HERE, from the object-space meshes (StTuning::device_bake; k_bvh.hip k_bvh_bake): this copy's
        // hit-test records (+ leaf entries), bounds and attribute records of every instance it has not followed yet
        if ((rc = e.bake_on_device(set, up, pageable))) return rc;
        for (const auto& level : refit_levels_)   // this copy holds the current tree, so the engine's work list is its own
            e.L.launch_bvh_refit(static_cast<float4*>(t.bvh.ptr), static_cast<const float4*>(set.tri_bounds.ptr), static_cast<const uint32_t*>(t.parent.ptr), static_cast<const uint32_t*>(t.refit_local.ptr),
                                 static_cast<const uint32_t*>(t.refit_items.ptr), static_cast<const uint32_t*>(t.refit_batch_off.ptr), level.first, level.second, up);
        device_refits++;
    } else if (!build_now) {
        device_form();
        // traversal pointers are 32-bit BYTE offsets into the device stream (64 B per entry) and stack slots hold entry numbers
        if ((size_t)device_bvh_len * sizeof(float4) > 0xffffffffull) return fail(ST_ERR_INVALID_ARGUMENT, "the BVH stream exceeds 4 GiB (2^26 entries): traversal pointers are 32-bit byte offsets");
        if ((rc = t.bvh.upload(bvh_upload_.data(), bvh_upload_.size() * sizeof(float4), up, e.staging, pageable))) return rc;
        if (device_refit_possible()) {  // what the device refit of later ticks needs beside the stream
            refit_index();
            if ((rc = e.upload_tri_slots(set, Engine::TRI_GEO, true, up, pageable))) return rc;
            const std::pair<DeviceArray*, const std::vector<uint32_t>*> index[] = {{&t.entry_of_tri, &entry_of_tri_}, {&t.parent, &parent_}, {&t.refit_local, &refit_local_}, {&t.refit_items, &refit_items_}, {&t.refit_batch_off, &refit_batch_off_}};
            for (const auto& [d, v] : index) if ((rc = d->upload(v->data(), v->size() * sizeof(uint32_t), up, e.staging, pageable))) return rc;
            t.tree_version = tree_version;
        }
    }
    if (!build_now) {
        if ((rc = refresh_compact_stream(t, up))) return rc;   // the shadow rays' compact form follows every change of the contract stream
        if ((rc = refresh_wide_stream(t, up, !device_path, pageable))) return rc;   // and so does the wide form (its topology only when the tree itself was sent)
    }
    // the hit-test records per slot are on this copy where the device builds, bakes or refits from them; a host tree under any other mode sent only its leaf entries
    set.geo_current = build_now || device_refit_possible();
    return ST_OK;
}
int SceneTree::report_too_deep() {
    if (bvh_too_deep_unreported) {   // once per build
        bvh_too_deep_unreported = false;
        if (!e.tuning.allow_deep_bvh)
            return fail(ST_ERR_BVH_TOO_DEEP, "the BVH is " + std::to_string(bvh_stack_need) + " internal nodes deep, the kernels' traversal stack holds " + std::to_string(stack_entries) +
                                             " pending entries (strolle-gpu/src/lib.rs:76): pushes beyond it are dropped and geometry behind them can be missed. The scene was uploaded and renders; StTuning::allow_deep_bvh = 1 accepts this");
    }
    return ST_OK;
}

void SceneTree::wide_topology(bool for_tick) {
    if (!for_tick || wide_built_for_ != tree_version || wide_topo_.empty()) build_wide_topology();
    wide_built_for_ = for_tick ? tree_version : ~0ull;
}
// The wide stream (k_bvh.hip k_bvh_wide) of device copy `t`: topology from the host when the tree was (re)sent, boxes and leaf records from that
// copy's contract stream as it is on the device right now.
int SceneTree::refresh_wide_stream(TreeCopy& t, hipStream_t up, bool topology_changed, bool* pageable) {
    if (!e.tuning.wide_bvh || !e.tuning.compact_bvh || device_bvh_len <= kLdsSceneTexels) { t.wide_nodes = t.wide_leaves = 0u; t.wide_for_entries = 0u; return ST_OK; }
    int rc;
    if (topology_changed || t.wide_for_entries != device_bvh_len / 4u) {
        if (!topology_changed && wide_built_for_ != tree_version) return ST_OK;   // (cannot happen: a copy on the device path holds this tree's topology)
        wide_topology(true);
        const uint32_t nodes = (uint32_t)(wide_topo_.size() / 8u), leaves = (uint32_t)wide_leaf_entry_.size();
        t.wide_nodes = t.wide_leaves = 0u; t.wide_for_entries = 0u;
        if (nodes >= (1u << 23) || leaves >= (1u << 23)) return ST_OK;   // v_mul_u32_u24 addressing and the << 5 of a node link: larger trees keep the binary streams
        if (nodes && (rc = t.wide_topo.upload(wide_topo_.data(), wide_topo_.size() * sizeof(uint32_t), up, e.staging, pageable))) return rc;
        if (leaves && (rc = t.wide_leaf_entry.upload(wide_leaf_entry_.data(), wide_leaf_entry_.size() * sizeof(uint32_t), up, e.staging, pageable))) return rc;
        // one allocation: nodes (64 B each), then the leaf records (48 B each) + one texel of slack (a node step's fourth texel is never read for a record)
        const size_t need = (size_t)nodes * 64u + (size_t)leaves * 48u + 64u;
        if (need > 0xfffffff0ull) return ST_OK;   // 32-bit byte offsets
        if ((rc = t.bvh_wide.reserve(need, need + need / 2))) return rc;
        t.wide_nodes = nodes; t.wide_leaves = leaves; t.wide_root = wide_root_; t.wide_for_entries = device_bvh_len / 4u;
        t.wide_links16 = (nodes < 32768u && leaves < 32768u) ? 1u : 0u;
        t.wide_topology_serial = wide_serial_;
    }
    if (!t.wide_for_entries) return ST_OK;
    launchers_exact().launch_bvh_wide(static_cast<const float4*>(t.bvh.ptr), static_cast<const uint32_t*>(t.wide_topo.ptr), t.wide_nodes, static_cast<const uint32_t*>(t.wide_leaf_entry.ptr), t.wide_leaves,
                                      t.wide_links16, static_cast<float4*>(t.bvh_wide.ptr), static_cast<float4*>(t.bvh_wide.ptr) + 4u * (size_t)t.wide_nodes, up);
    return ST_OK;
}

// The compact stream (k_bvh.hip k_bvh_compact) of device copy `t`, from that copy's contract stream as it is on the device right now.
int SceneTree::refresh_compact_stream(TreeCopy& t, hipStream_t up) {
    t.compact_entries = 0;
    if (!e.tuning.compact_bvh || device_bvh_len <= kLdsSceneTexels) return ST_OK;   // tiny scenes live in LDS as they are
    const uint32_t entries = device_bvh_len / 4u;
    // the compact walk addresses entries with v_mul_u32_u24 (st_traverse.h any_hit_compact): 24 bits of entry number. A larger stream (8 M+
    // triangles) keeps compact_entries = 0 and its rays walk the contract stream with any_hit_fast / traverse
    if (entries >= (1u << 24)) return ST_OK;
    const size_t bytes = (size_t)entries * 48u;
    if (int rc = t.bvh_compact.reserve(bytes, bytes + bytes / 2)) return rc;
    launchers_exact().launch_bvh_compact(static_cast<const float4*>(t.bvh.ptr), entries, static_cast<float4*>(t.bvh_compact.ptr), up);
    t.compact_entries = entries;
    return ST_OK;
}

// ---- the walks' arguments
int SceneTree::walk_args(const TreeCopy& scene, KArgs& a, bool heatmap) const {
    const StTuning& tuning = e.tuning;
    a.bvh = static_cast<const float4*>(scene.bvh.ptr);
    // the fast build's shadow rays walk the compact stream of this scene copy when it has one (k_bvh.hip k_bvh_compact)
    const bool compact = e.arithmetic == ST_ARITH_FAST && tuning.compact_bvh && tuning.anyhit_fast && !e.count_bytes && scene.compact_entries != 0u && scene.compact_entries * 4u == device_bvh_len;
    a.bvh_c = compact ? static_cast<const float4*>(scene.bvh_compact.ptr) : nullptr;
    a.bvh_c_root = (compact && device_root_is_leaf) ? 1u : 0u;
    // ... or, preferred, its wide form (k_bvh.hip k_bvh_wide)
    // (ST_BVH_BUILD_DEVICE: this copy's wide stream was built on the device and its contract stream is stale — every ray must walk the wide stream)
    if (scene.device_built && (!e.wide_only_tuning() || heatmap))
        return fail(ST_ERR_INVALID_ARGUMENT, "the live scene copy's tree was built on the device (ST_BVH_BUILD_DEVICE) and this frame needs the contract stream (heatmap camera, exact arithmetic, "
                                             "byte counting or a switched-off wide stream): st_tick builds it on the host once it sees the observer");
    const bool wide = scene.device_built || (compact && tuning.wide_bvh && scene.wide_for_entries != 0u && scene.wide_for_entries * 4u == device_bvh_len);
    a.bvh_w = wide ? static_cast<const float4*>(scene.bvh_wide.ptr) : nullptr;
    a.bvh_w_leaf_off = wide ? scene.wide_nodes * 64u : 0u;
    a.bvh_w_root = wide ? scene.wide_root : 0u; a.bvh_w_links16 = wide ? scene.wide_links16 : 0u;
    a.primary_packets = wide && tuning.primary_packets && !e.packets_overflowed ? 1u : 0u;
    {   // the largest link of this stream: (max(nodes, leaf records) - 1) << 1 | 1
        uint32_t bits = 16u;
        const uint32_t top = std::max(scene.wide_nodes, scene.wide_leaves);
        while (bits < 31u && (1ull << bits) <= (unsigned long long)top * 2ull + 1ull) bits++;
        a.bvh_w_link_mask = (1u << bits) - 1u;
    }
    // Walks over the CONTRACT stream (exact build, heatmap pass, byte-counting mode, the compact binary stream: the contract's tree) hold what
    // that tree's deepest chain can need — proven drop-free up to kBvhStackSizeDeep. The WIDE stream is another tree: its worst case (every
    // child of every node on a path hit: 35 pending entries for the 13 k-triangle dungeon, 45 at 208 k) does not fit LDS at full occupancy and
    // no ray comes near it (deepest stack measured: 11-13); it keeps kBvhStackSize entries, and test_the_wide_walk_drops_no_push renders
    // BASELINE config 3's scene with 24 and with 48 entries (StTuning::wide_stack_entries) and finds the same bits.
    // A walk that does find the stack full says so (KArgs::walk_flags) and the next st_tick re-arms the launches with a deeper one (st_engine.h walk_flags_host).
    a.stack_entries = wide ? e.wide_stack_entries_now() : stack_entries;
    a.bvh_len = scene.device_built ? 0x40000000u : device_bvh_len;   // (device-built: no contract stream; any value that is neither "empty" nor "fits LDS")
    if (scene.device_built) a.bvh = nullptr;
    return ST_OK;
}

// ---- st_debug_read_scene's tree cases
int SceneTree::debug_read(int what, const void** p, size_t* bytes) {
    const bool live_copy = what == LiveStream || what == LiveWideNodes || what == LiveWideLeaves;   // read from the device as it is: the host catches up with nothing
    if (!live_copy && e.instances.any_host_stale()) e.bake_stale_on_host();   // instances the device moved: the host arrays catch up
    if (int rc = e.take_deferred_status()) return rc;   // (their posed triangles could not be read back)
    if (!live_copy && host_tree_stale) rebuild_host_tree(false);   // ST_BVH_BUILD_DEVICE left the host's tree behind
    switch (what) {
        case ContractStream: { const auto& s = host_stream(); *p = s.data(); *bytes = s.size() * sizeof(float4); break; }
        case DeviceForm: *p = device_form().data(); *bytes = (size_t)device_bvh_len * sizeof(float4); break;  // as st_tick would upload it now
        case LiveStream: {  // the device stream as it is on the device right now (the live copy): what a device refit left there
            if (!e.has_device || !e.copies.scene.written) return fail(ST_ERR_NO_DEVICE, "no device copy of the scene");
            const TreeCopy& t = e.copies.scene.current().tree;
            const size_t n = t.bvh.capacity ? (size_t)live_bvh_texels : 0;
            readback_.resize(n);
            ST_HIP(hipSetDevice(e.device)); ST_HIP(hipDeviceSynchronize());
            if (n) ST_HIP(hipMemcpy(readback_.data(), t.bvh.ptr, n * sizeof(float4), hipMemcpyDeviceToHost));
            *p = readback_.data(); *bytes = n * sizeof(float4); break;
        }
        case RefitParent: case RefitLocal: case RefitItems: case RefitBatchOff: case RefitLevels: case RefitEntryOfTri: case RefitBounds: {  // the device refit's inputs (k_bvh.hip), built here for a host-side emulation
            device_form(); refit_index();
            readback_levels_.clear();
            for (const auto& l : refit_levels_) { readback_levels_.push_back(l.first); readback_levels_.push_back(l.second); }
            const std::vector<uint32_t>* v = what == RefitParent ? &parent_ : what == RefitLocal ? &refit_local_ : what == RefitItems ? &refit_items_ : what == RefitBatchOff ? &refit_batch_off_
                                           : what == RefitLevels ? &readback_levels_ : &entry_of_tri_;
            if (what == RefitBounds) { *p = e.slots.bounds().data(); *bytes = e.slots.bounds().size() * sizeof(float4); }
            else { *p = v->data(); *bytes = v->size() * sizeof(uint32_t); }
            break;
        }
        case WideTopology: case WideLeafEntry: {  // the wide stream's topology (k_bvh.hip k_bvh_wide), built here: WideTopology = 8 words per node (4 box sources, 4 links), preceded by
                                                  // one word holding the root's link; WideLeafEntry = the contract entry of every leaf record
            device_form(); wide_topology(false);
            readback_levels_.assign(1, wide_root_ | (wide_stack_need_ << 8));   // (bits 8..: the most entries a wide walk can have pending)
            readback_levels_.insert(readback_levels_.end(), wide_topo_.begin(), wide_topo_.end());
            const std::vector<uint32_t>* v = what == WideTopology ? &readback_levels_ : &wide_leaf_entry_;
            *p = v->data(); *bytes = v->size() * sizeof(uint32_t); break;
        }
        case LiveWideNodes: case LiveWideLeaves: {  // the wide stream as it is on the device right now (the live copy): nodes (64 B each) / leaf records (48 B each)
            if (!e.has_device || !e.copies.scene.written) return fail(ST_ERR_NO_DEVICE, "no device copy of the scene");
            const TreeCopy& t = e.copies.scene.current().tree;
            const size_t n = (t.wide_for_entries || t.device_built) ? (what == LiveWideNodes ? (size_t)t.wide_nodes * 4u : (size_t)t.wide_leaves * 3u) : 0;
            readback_.resize(n);
            ST_HIP(hipSetDevice(e.device)); ST_HIP(hipDeviceSynchronize());
            if (n) ST_HIP(hipMemcpy(readback_.data(), what == LiveWideNodes ? t.bvh_wide.ptr : static_cast<const void*>(static_cast<const float4*>(t.bvh_wide.ptr) + 4u * (size_t)t.wide_nodes), n * sizeof(float4), hipMemcpyDeviceToHost));
            *p = readback_.data(); *bytes = n * sizeof(float4); break;
        }
        default: return fail(ST_ERR_INVALID_ARGUMENT, "unknown scene buffer");
    }
    return ST_OK;
}

}  // namespace st
