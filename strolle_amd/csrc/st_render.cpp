// st_render.cpp — host engine of libstrolle_hip.so: per-camera buffers, present hand-over, and Engine::render: the per-frame pass graph (camera_controller.rs:87-174) in phases, on two HIP streams. See st_engine.h.
#include "st_engine.h"

namespace st {

void Engine::release_camera(CameraState& c) {
    c.slab.release(); c.counters.release(); c.tile_mask.release();
    c.side_stream.reset();
    for (Event* e : {&c.ev_di_head, &c.ev_gi_done, &c.ev_prim_ok, &c.ev_frame_done, &c.ev_setup, &c.ev_lds_done}) e->reset();
    c.have_prev_frame_events = c.have_lds_done = false;
    c.join_present(); c.present_stream.reset();
    for (auto& p : c.present) p = CameraState::PresentSlot();
}

// st_camera_present_copy: `src_device` (what st_render_camera composed into on `stream`) -> `dst_host`, asynchronously
int Engine::present_copy(CameraState& c, const void* src, void* dst, size_t bytes, hipStream_t stream) {
    if (!has_device) return fail(ST_ERR_NO_DEVICE, "present copy on a host-only engine");
    ST_HIP(hipSetDevice(device));
    if (!c.present_stream) ST_HIP(hipStreamCreateWithFlags(&c.present_stream.h, hipStreamNonBlocking));
    // the slot that already serves this destination, else the older one
    CameraState::PresentSlot* slot = nullptr;
    for (auto& p : c.present) if (p.dst == dst) slot = &p;
    if (!slot) { slot = &c.present[c.present_next & 1u]; c.present_next++; }
    if (slot->pending) ST_HIP(hipEventSynchronize(slot->ev_done.h));  // only when the caller runs more than two frames ahead
    slot->src = src; slot->dst = dst;
    if (int rc = slot->ev_src.record(stream)) return rc;             // the frame is composed
    if (int rc = slot->ev_src.wait(c.present_stream)) return rc;
    ST_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c.present_stream));
    if (int rc = slot->ev_done.record(c.present_stream)) return rc;
    slot->pending = true;
    return ST_OK;
}

// 1 = the copy into `dst` has landed (or none was asked for), 0 = still in flight; wait != 0 blocks until it has
int Engine::present_ready(CameraState& c, const void* dst, int wait, int* ready) {
    *ready = 1;
    for (auto& p : c.present) {
        if (p.dst != dst || !p.pending) continue;
        if (wait) { ST_HIP(hipEventSynchronize(p.ev_done.h)); p.pending = false; }
        else {
            const hipError_t q = hipEventQuery(p.ev_done.h);
            if (q == hipSuccess) p.pending = false;
            else if (q == hipErrorNotReady) { (void)hipGetLastError(); *ready = 0; }
            else return fail(ST_ERR_HIP, std::string("hipEventQuery: ") + hipGetErrorString(q));
        }
    }
    return ST_OK;
}

// ---- cameras (camera.rs:50-66, camera_controller.rs:27-86)
GpuCamera Engine::serialize_camera(const StCamera& c) {
    const M4 transform = m4_from_cols(c.transform), projection = m4_from_cols(c.projection);
    GpuCamera g;
    g.projection_view = m4_mul(projection, m4_inverse(transform));
    g.ndc_to_world = m4_mul(transform, m4_inverse(projection));
    g.origin = make_float4(transform.c[3].x, transform.c[3].y, transform.c[3].z, 0.0f);
    g.screen = make_float4((float)c.width, (float)c.height, 0.0f, 0.0f);
    return g;
}

int Engine::allocate_camera(CameraState& c) {
    c.row0 = 0; c.row1 = c.desc.height; c.col0 = 0; c.col1 = c.desc.width;
    if (!has_device) return ST_OK;
    ST_HIP(hipSetDevice(device));
    release_camera(c);
    const size_t n = (size_t)c.desc.width * c.desc.height;
    size_t total = 0;
    for (int i = 0; i < ST_BUF_COUNT + kInternalPlanes; i++) {
        c.plane_bytes[i] = i == ST_BUF_DBG_USED_MEMORY ? n * 4 : n * 16 * plane_texels_per_pixel(i);
        total += (c.plane_bytes[i] + 255) & ~size_t(255);
    }
    if (int rc = c.slab.reserve(total, total)) return rc;
    ST_HIP(hipMemset(c.slab.ptr, 0, total));  // wgpu zero-initialises resources; stale-data paths depend on it
    size_t off = 0;
    for (int i = 0; i < ST_BUF_COUNT + kInternalPlanes; i++) { c.plane[i] = reinterpret_cast<float4*>(c.slab.as<char>() + off); off += (c.plane_bytes[i] + 255) & ~size_t(255); }
    c.gi_aliased = false;
    if (int rc = c.counters.reserve(kCounterBytes, kCounterBytes)) return rc;
    ST_HIP(hipMemset(c.counters.ptr, 0, kCounterBytes));
    {
        const size_t tiles = (size_t)((c.desc.width + 7u) / 8u) * ((c.desc.height + 7u) / 8u), bytes = 2 * tiles * sizeof(unsigned long long);
        if (int rc = c.tile_mask.reserve(bytes, bytes)) return rc;
        ST_HIP(hipMemset(c.tile_mask.ptr, 0, bytes));  // [0, tiles): variance's, [tiles, 2 tiles): the GI preview's
    }
    memset(c.profiled_traversal_bytes, 0, sizeof(c.profiled_traversal_bytes));
    ST_HIP(hipDeviceSynchronize());  // the clears run on the null stream; renders may use any stream
    return ST_OK;
}

// The scene half of KArgs (st_engine.h scene_args): what every launch that walks the live scene copy reads — its arrays, the stream its rays
// walk (contract, compact or wide) and the stack they hold (SceneTree::walk_args), the walk flags. `heatmap`: the launch is a BVH heatmap pass, which observes the
// contract stream. Shared by render() and the scene queries (st_query.cpp).
// Normal mapping's launch argument (st_engine.h). The device keeps the hit-test records per slot wherever it bakes, refits or builds from them; a copy written from a
// host tree alone holds them only inside its leaf entries, so the first reader that maps normals sends the host's array (current: such a copy was written from it)
// and joins the stream — once per scene change, and only while a map is in use. It is the one writer of a live copy outside a tick; safe, because no launch in flight
// reads these records of a copy that is not geo_current, and the join ends the write before any reader is handed the pointer (st_copies.h).
int Engine::normal_map_geo(hipStream_t stream, bool flagged, const float4** geo) {
    *geo = nullptr;
    const std::vector<float4>& tri_geo = slots.geo();
    if (!(normal_mapping || flagged) || !materials.any_normal_map || tri_geo.empty()) return ST_OK;
    SceneSet& scene = copies.scene.current();
    if (!scene.geo_current) {
        const size_t bytes = tri_geo.size() * sizeof(float4);
        if (int rc = scene.tri_geo.reserve(bytes, std::max<size_t>(bytes * 3 / 2, 4096))) return rc;
        ST_HIP(hipMemcpyAsync(scene.tri_geo.ptr, tri_geo.data(), bytes, hipMemcpyHostToDevice, stream));
        ST_HIP(hipStreamSynchronize(stream));   // pageable source; and readers on other streams find the records there
        scene.geo_current = true;
    }
    if (scene.tri_geo.capacity < tri_geo.size() * sizeof(float4)) return fail(ST_ERR_INVALID_ARGUMENT, "normal mapping: the live scene copy's hit-test records are short of the scene's triangle slots");
    *geo = static_cast<const float4*>(scene.tri_geo.ptr);
    return ST_OK;
}
int Engine::scene_args(KArgs& a, bool heatmap) const {
    const SceneSet& scene = copies.scene.current();
    a.tri_attr = static_cast<const float4*>(scene.tri_attr.ptr); a.instance_xforms = static_cast<const float4*>(scene.xforms.ptr);
    a.materials = static_cast<const GpuMaterial*>(scene.materials.ptr); a.material_base_packed = tuning.packed_base ? static_cast<const uint32_t*>(scene.base_packed.ptr) : nullptr;
    a.atlas = static_cast<const uchar4*>(d_atlas.ptr); a.byte_luts = static_cast<const float*>(d_byte_luts.ptr);
    a.tri_slots = (uint32_t)slots.size();
    a.count_bytes = count_bytes ? 1u : 0u;
    a.exp_flags = exp_flags;
    if (int rc = tree.walk_args(scene.tree, a, heatmap)) return rc;   // which stream its rays walk, and with what stack
    a.walk_flags = walk_flags_dev;
    a.anyhit_contract = (count_bytes || !tuning.anyhit_fast) ? 1u : 0u;   // the reference's used_memory is the contract loop's
    a.atlas_w = images.width(); a.atlas_h = images.height();
    return ST_OK;
}
// The other half: the live copy of the lights, the blue noise, the atmosphere LUTs, the sun and the environment map — what a frame's shading reads.
void Engine::light_args(KArgs& a) const {
    a.lights = static_cast<const GpuLight*>(copies.lights.current().buf.ptr);
    a.blue_noise = static_cast<const uchar4*>(d_blue_noise.ptr);
    a.transmittance_lut = static_cast<const float4*>(d_transmittance.ptr); a.sky_lut = static_cast<const float4*>(d_sky.ptr);
    a.n_lights_buf = (uint32_t)lights.table().size(); a.light_count = lights.count();
    a.sun_altitude = sun_altitude; a.sun_dir[0] = sun_dir_.x; a.sun_dir[1] = sun_dir_.y; a.sun_dir[2] = sun_dir_.z;
    environment_args(a);
}

// ---- render (camera_controller.rs:87-174). Engine::render, at the end of this file, is a short sequence of phases over one Frame:
// route_output, bind_args, refresh_inputs, decide_switches, arm_output, one of the two schedules (two_streams, serial), finish_output.
namespace {
// ---- the node table: everything the frame knows about the single nodes is between here and "end of the node table" (and in Frame's
// node_* functions, which switch on the node). A new node: an HdrNode in chain order, a row here, its plan and steps in HdrWork, a case in each node_* function.
// early: its first `early` launches run in front of the ev_prim_ok record (pack_early): they read planes the NEXT frame's primary visibility
//        overwrites. Depth of field's pack reads this frame's G-buffer depth; motion blur's the velocity map (single-buffered) and the depth.
// reads_depth: its launches in finish_output read the G-buffer depth of the frame's parity, which the frame after next rewrites: the camera's
//        gbuffer_depth_read fence is recorded once, behind the last such node that is on, and prim() of that parity waits for it.
// reads_velocity: the lean frame keeps the velocity map for it (kLeanKeepVelocity).
enum HdrNode { kNodeFog, kNodeShafts, kNodeDof, kNodeMBlur, kNodeBloom, kNodeLens, kNodeGrade, kHdrNodes };   // chain order
struct HdrNodeRow { uint32_t early; bool reads_depth, reads_velocity; };
constexpr HdrNodeRow kHdrNode[kHdrNodes] = {
    /* fog (st_fog.cpp): one launch; pointwise, so windows are honoured */       {0u, true, false},
    /* light shafts (st_shafts.cpp): march, apply */                              {0u, true, false},
    /* depth of field (st_dof.cpp): pack | neighbour maximum, gather */           {1u, false, false},
    /* motion blur (st_motion_blur.cpp): pack | neighbour maximum, gather */      {1u, false, true},
    /* bloom (st_bloom.cpp): the pyramid's chain, the composite */                {0u, false, false},
    /* lens effects (st_lens.cpp): one launch; a gather over the whole plane */   {0u, false, false},
    /* colour grading (st_grade.cpp): one launch; pointwise, windows honoured */  {0u, false, false},
};
struct HdrWork {   // what the nodes that are on hold for one frame: node_plan's plans, node_arm's argument blocks and steps
    Engine::ShaftsPlan shafts_plan; Engine::DofPlan dof_plan; Engine::MBlurPlan mblur_plan; Engine::BloomPlan bloom_plan; Engine::GradePlan grade_plan; StLensPlan lens_plan;
    Engine::Lut* grade_lut = nullptr;   // the live table the descriptor names, if any: its fence is recorded behind the launch
    Engine::GradeStep grade; Engine::LensStep lens; Engine::FogStep fog; Engine::ShaftsSteps shafts; Engine::DofSteps dof; Engine::MBlurSteps mblur; Engine::BloomSteps bloom;
};
// ---- end of the node table
// The frame's output chain, decided once. Output post-processing (st_post.cpp): while the frame needs it, the frame's target is the camera's
// own render-size RGBA32F plane instead of `out`, and the post launches write `out` behind it. In front of it the HDR nodes (the node table,
// above) form an ordered list: the composing launch writes the plane of the first node that is on — the composed colour untransformed, and
// still metered —, each node writes the plane of the next one that is on, and the last one what the composing launch would have written:
// the frame's target, in its format, through the display transform (`target`).
struct OutputRoute {
    bool post_fxaa = false, post = false, keep_velocity = false /* a node that is on reads the velocity map */;
    bool up_steps = false /* the upscale stage runs behind FXAA (st_upscale.cpp) */, up_nearest = false /* a heatmap frame under it: the NEAREST resampler */;
    void* hdr_plane[kHdrNodes] = {};   // the render-size RGBA32F plane each node that is on reads, in chain order; null: the node is off
    Fence* planes_read[kHdrNodes] = {};   // ... and the fence of the node's planes
    bool on(int n) const { return hdr_plane[n] != nullptr; }
    // where node `n` writes (n = -1: the composing launch): the next node's plane, raw, or the frame's target
    NodeTarget target(int n) const {
        for (int k = n + 1; k < kHdrNodes; k++) if (hdr_plane[k]) return {hdr_plane[k], frame_format, true, frame_disp};
        return {frame_out, frame_format, false, frame_disp};
    }
    void* comp_out = nullptr; uint32_t comp_format = 0; DisplayArgs comp_disp{};      // the composing launch (either of the two): target, format, display transform
    void* frame_out = nullptr; uint32_t frame_format = 0; DisplayArgs frame_disp{};   // the frame's target: `out` or the post plane; no display: NONE at scale 1, which stores the colour's own bits
};
// Every per-frame decision, made once (decide_switches); the stages only read them.
struct FrameSwitches {
    bool needs_di, needs_gi, denoise, any_objects, tracing, whole_graph, gi_runs, swap_gi_history, gi_preview_both, even_tiles, compose_in_wavelet;
    bool fuse_gi_validation_now, fuse_gi_reprojection_now, two_streams;
    uint32_t gi_source, lean, variance_in_reproject, skip_dead_scratch, gi_skip_history_copy;   // (the last four: the KArgs fields of the same names)
};
// One frame of one camera: what its stages share. `cur` is the stream the next launches go to (the two-stream schedule diverts primary
// visibility and the GI chain to the camera's side stream); the rest below `s` is launch bookkeeping.
struct Frame {
    Engine& e; CameraState& c; void* const out; const hipStream_t stream; hipStream_t cur;
    const float4* nm_tri_geo = nullptr;   // normal mapping's argument of primary visibility (Engine::normal_map_geo): null while nothing is mapped
    KArgs a{}; OutputRoute route; FrameSwitches s{}; HdrWork work;
    const uint32_t mode, pseed;   // pseed: one seed for both preview passes (passes/gi_preview_resampling.rs:60-74)
    bool mask_split = false, di_reprojected = false, gi_reprojected = false, composed = false, luts_generated_now = false; uint32_t launch_ordinal = 0u;
    int side_rc = ST_OK;   // of recording ev_lds_done inside denoise()
    Frame(Engine& e_, CameraState& c_, void* out_, hipStream_t s_) : e(e_), c(c_), out(out_), stream(s_), cur(s_), mode(c_.desc.mode), pseed(pass_seed(e_.base_seed, c_.frame, SEED_GI_PREVIEW)) {}
    uint32_t seed(uint32_t pass) const { return pass_seed(e.base_seed, c.frame, pass); }
    auto gi_preview_src() const { return s.gi_source == 0 ? a.gi_res[1] : a.gi_res[2]; }
    double slot_bytes(int slot) const {
        const KernelInfo& ki = kernel_info(slot);
        const uint32_t cols = c.col1 - c.col0;
        return (double)(c.row1 - c.row0) * (ki.half ? (double)(((cols + 7u) / 8u / 2u) * 8u) : (double)cols) * ki.bytes_per_unit;
    }
    // `bits`: the reference passes this launch executes (StPassBit). Their unfused algorithmic bytes are what kernel_info(slot) credits to the
    // launch, so fusion shows up as a gain, not as a moved goalpost. `own_bytes`: the bytes of the output chain's launches depend on the
    // output size and format, so those launches state them.
    template <class F> void run(int slot, uint64_t bits, F&& launch, double own_bytes = -1.0) {
        if (e.last_launches.empty() || e.last_launches.back() != bits) e.last_launches.push_back(bits);  // a launch group is reported once
        if ((bits & e.pass_mask) != bits) { mask_split |= (bits & e.pass_mask) != 0; return; }
        if (e.launch_filter != ~0ull && !((e.launch_filter >> (launch_ordinal++ & 63u)) & 1ull)) return;  // measurement only: the frame's state is not meaningful afterwards
        const double bytes = own_bytes >= 0.0 ? own_bytes : slot_bytes(slot);
        a.ray_counter = c.counters.as<unsigned long long>() + kCounterWordsPerSlot * slot;
        if (e.profiling && e.profile_kernel_events) {  // the dispatch's own timestamps (what rocprofv3's kernel trace reads)
            (void)e.profile_close();   // a scope the run-of-launches mode left open belongs to that mode
            g_launch_events.start = e.take_event(); g_launch_events.stop = e.take_event(); g_launch_events.consumed = false;
            launch();
            if (g_launch_events.consumed) e.profile_records.push_back({slot, g_launch_events.start, g_launch_events.stop, bytes, 1u, true});
            else { e.event_pool.push_back(g_launch_events.start); e.event_pool.push_back(g_launch_events.stop); }   // nothing was enqueued (an empty grid)
            g_launch_events = LaunchEvents();
            return;
        }
        const bool atrous = slot == KS_DENOISE_WAVELET || slot == KS_DENOISE_WAVELET_12 || slot == KS_DENOISE_WAVELET_COMPOSE;
        e.profile_begin(e.profile_group_atrous && atrous ? (int)KS_DENOISE_WAVELET_FAMILY : slot, cur, bytes);
        launch();
    }
    // ---- the node table's functions (one case per node; the rest of the frame sees nodes by index only)
    // whether the camera wants the node this frame. Heatmap frames are false colour; heatmap and reference frames have no G-buffer and no
    // velocity map; fog, shafts and depth of field derive the pixel's ray or the focal length from a perspective projection
    bool node_wanted(int n) const {
        const bool perspective = c.has_gbuffer() && dof_perspective(c.desc.projection);
        switch (n) {
        case kNodeFog: return c.fog.on && perspective;
        case kNodeShafts: return c.shafts.on && perspective;
        case kNodeDof: return c.dof.on && perspective;
        case kNodeMBlur: return c.mblur.on && c.has_gbuffer();
        case kNodeGrade: return c.grade.on && c.desc.mode != ST_MODE_BVH_HEATMAP;   // (needs neither a G-buffer nor a projection)
        case kNodeLens: return c.lens.on && c.desc.mode != ST_MODE_BVH_HEATMAP;     // (likewise)
        default: return c.bloom.on && c.desc.mode != ST_MODE_BVH_HEATMAP;
        }
    }
    // the node's plan and its planes ([0]: the HDR plane; grown, never shrunk: a size that goes down and up again between frames costs no sync
    // and no allocation), `stream` ordered behind their last readers. The node is on when this leaves its HDR plane in the route.
    template <int N> int node_planes(int n, FencedPlanes<N>& p, const size_t (&bytes)[N]) {
        if (int rc = p.acquire(bytes, p.Grow, stream)) return rc;
        route.hdr_plane[n] = p.plane[0].ptr; route.planes_read[n] = &p.read;
        return ST_OK;
    }
    int node_plan(int n) {
        const uint32_t w = c.desc.width, h = c.desc.height;
        const size_t plane = (size_t)w * h * sizeof(float4);
        switch (n) {
        case kNodeFog: return node_planes(n, c.fog.planes, {plane});
        case kNodeShafts:
            if (int rc = Engine::shafts_plan(c.shafts.desc, w, h, work.shafts_plan)) return rc;
            return node_planes(n, c.shafts.planes, {plane, work.shafts_plan.cell_bytes});
        case kNodeDof:
            if (int rc = Engine::dof_plan(c.dof.desc, w, h, work.dof_plan)) return rc;
            return node_planes(n, c.dof.planes, {plane, work.dof_plan.packed_bytes, work.dof_plan.tile_bytes, work.dof_plan.tile_bytes});
        case kNodeMBlur:
            if (int rc = Engine::mblur_plan(c.mblur.desc, w, h, work.mblur_plan)) return rc;
            return node_planes(n, c.mblur.planes, {plane, work.mblur_plan.packed_bytes, work.mblur_plan.tile_bytes, work.mblur_plan.tile_bytes});
        case kNodeLens:
            if (int rc = Engine::lens_plan(c.lens.desc, w, h, work.lens_plan)) return rc;
            return node_planes(n, c.lens.planes, {plane});
        case kNodeGrade:
            if (int rc = Engine::grade_plan(c.grade.desc, work.grade_plan)) return rc;
            work.grade_lut = e.live_lut(c.grade.desc.lut);
            return node_planes(n, c.grade.planes, {plane});
        default:
            if (int rc = Engine::bloom_plan(c.bloom.desc, w, h, work.bloom_plan)) return rc;
            if (work.bloom_plan.levels == 0u) return ST_OK;   // the frame holds no level: off
            return node_planes(n, c.bloom.planes, {plane, work.bloom_plan.texels * sizeof(float4)});
        }
    }
    // the node's argument blocks and steps: from its HDR plane, this frame's G-buffer depth (and velocity map) into `t`
    void node_arm(int n, const NodeTarget& t) {
        const NodeSource src{route.hdr_plane[n], a.g0, a.velocity, true, c.desc.width, c.desc.height};
        const float sun[3] = {e.sun_dir_.x, e.sun_dir_.y, e.sun_dir_.z};   // as KArgs::sun_dir carries it (light_args)
        const NodeView view{c.desc.transform, c.desc.projection, sun};
        switch (n) {
        case kNodeFog: Engine::fog_step(c.fog.desc, view, src, c.row0, c.row1, c.col0, c.col1, t, work.fog); break;
        case kNodeShafts: e.shafts_steps(c.shafts.desc, work.shafts_plan, view, src, c.shafts.planes.plane[1].as<float4>(), t, true, work.shafts); break;
        case kNodeDof: { const auto& p = c.dof.planes.plane; Engine::dof_steps(c.dof.desc, work.dof_plan, c.desc.projection, src, p[1].as<float2>(), p[2].as<float>(), p[3].as<float>(), t, work.dof); break; }
        case kNodeLens: Engine::lens_step(c.lens.desc, work.lens_plan, src, c.frame, e.lens_force_gather, t, work.lens); break;
        case kNodeGrade:
            Engine::grade_step(c.grade.desc, work.grade_plan, work.grade_lut ? work.grade_lut->texels.as<float4>() : nullptr, work.grade_lut ? work.grade_lut->size : 0u, src,
                               c.row0, c.row1, c.col0, c.col1, t, work.grade);
            break;
        case kNodeMBlur: { const auto& p = c.mblur.planes.plane; Engine::mblur_steps(c.mblur.desc, work.mblur_plan, src, p[1].as<float2>(), p[2].as<float4>(), p[3].as<float4>(), t, work.mblur); break; }
        default: work.bloom = Engine::bloom_steps(c.bloom.desc, work.bloom_plan, src.color, src.w, src.h, c.bloom.planes.plane[1].as<float4>(), t, e.bloom_tail_bytes()); break;
        }
    }
    uint32_t node_steps(int n) const { return (n == kNodeFog || n == kNodeGrade || n == kNodeLens) ? 1u : n == kNodeShafts ? 2u : n == kNodeBloom ? work.bloom.count : 3u; }
    const OutputStep& node_step(int n, uint32_t i) const {
        switch (n) {
        case kNodeFog: return work.fog.step;
        case kNodeGrade: return work.grade.step;
        case kNodeLens: return work.lens.step;
        case kNodeShafts: return work.shafts.step[i];
        case kNodeDof: return work.dof.step[i];
        case kNodeMBlur: return work.mblur.step[i];
        default: return work.bloom.step[i].step;
        }
    }
    void node_launch(int n, uint32_t i) {
        switch (n) {
        case kNodeFog: e.L.launch_fog(work.fog.args, cur); break;
        case kNodeGrade: e.L.launch_grade(work.grade.args, cur); break;
        case kNodeLens: e.L.launch_lens(work.lens.args, cur); break;
        case kNodeShafts: e.launch_shafts_step(a, work.shafts, i, cur); break;   // the march reads the live scene copy and the light table too
        case kNodeDof: e.launch_dof_step(work.dof, i, cur); break;
        case kNodeMBlur: e.launch_mblur_step(work.mblur, i, cur); break;
        default: e.launch_bloom_step(work.bloom.step[i], cur); break;
        }
    }
    // ---- end of the node table's functions
    // launches [first, last) of node `n`, in the frame's one launch group behind the composing launch (ST_PASS_POST)
    void run_node(int n, uint32_t first, uint32_t last) {
        for (uint32_t i = first; i < last; i++) { const OutputStep& st = node_step(n, i); run(st.slot, ST_PASS_POST, [&] { node_launch(n, i); }, st.bytes); }
    }
    // ---- phases
    int route_output() {
        OutputRoute& r = route;
        DisplayArgs disp{};   // the camera's display transform (st_display.cpp)
        if (int rc = e.display_begin(c, stream, mode == ST_MODE_BVH_HEATMAP, disp)) return rc;
        const size_t plane = (size_t)c.desc.width * c.desc.height * sizeof(float4);
        const bool post_resample = out && c.post_resizes();
        r.up_steps = out && mode != ST_MODE_BVH_HEATMAP && (c.upscale_resizes() || c.upscale_sharpens());
        r.up_nearest = out && mode == ST_MODE_BVH_HEATMAP && c.upscale_resizes();
        r.post_fxaa = out && c.post_fxaa(); r.post = r.post_fxaa || post_resample || r.up_steps || r.up_nearest;
        if (r.post) if (int rc = c.post.planes.acquire({plane, r.post_fxaa && (post_resample || r.up_steps) ? plane : 0}, c.post.planes.Exact, stream)) return rc;
        if (r.up_steps) {   // the output-size plane between the two steps, when both run
            const size_t mid = Engine::upscale_plan(c.upscale.desc, nullptr, c.desc.width, c.desc.height, nullptr, nullptr, c.out_format, e.upscale_fused).mid_bytes;
            if (int rc = c.upscale.planes.acquire({mid}, c.upscale.planes.Grow, stream)) return rc;
        }
        for (int n = 0; n < kHdrNodes; n++) if (out && node_wanted(n)) if (int rc = node_plan(n)) return rc;
        for (int n = 0; n < kHdrNodes; n++) r.keep_velocity |= r.on(n) && kHdrNode[n].reads_velocity;
        r.frame_out = r.post ? c.post.planes.plane[0].ptr : out; r.frame_format = r.post ? (uint32_t)ST_FORMAT_RGBA32F : c.out_format;
        r.frame_disp = disp; if (!r.frame_disp.on) r.frame_disp.scale = 1.0f;
        const NodeTarget comp = r.target(-1);
        const bool hdr_chain = comp.raw;   // the composing launch feeds an HDR node: it stores the composed colour as it is
        r.comp_out = comp.dst; r.comp_format = hdr_chain ? (uint32_t)ST_FORMAT_RGBA32F : r.frame_format;
        if (hdr_chain) { if (disp.meter) disp.tonemap = kDisplayRaw; else disp = DisplayArgs{}; }   // the composing launch: meter, do not transform
        r.comp_disp = disp;
        return ST_OK;
    }
    // KArgs: the scene and light halves (scene_args, light_args), then the camera's planes — the `alt` ping-pong of the frame's parity, the
    // decoded-surface twins, the reservoir arrays — its window and the tile map
    int bind_args() {
        c.last_lean = 0u; c.last_lean_composed = false;
        a.cam = c.curr; a.prev_cam = c.prev;
        if (int rc = e.scene_args(a, mode == ST_MODE_BVH_HEATMAP)) return rc;
        if (mode != ST_MODE_BVH_HEATMAP && mode != ST_MODE_REFERENCE) if (int rc = e.normal_map_geo(stream, false, &nm_tri_geo)) return rc;   // (those two modes run no primary visibility)
        c.shown = c.curr; c.shown_prev = c.prev; c.shown_width = c.desc.width; c.shown_height = c.desc.height; c.has_shown = true;   // what st_camera_pick casts through
        e.light_args(a);
        const bool alt = c.frame % 2u == 1u;
        auto P = [&](int id) { return c.plane[id]; };
        a.g0 = P(alt ? ST_BUF_PRIM_GBUFFER_D0_B : ST_BUF_PRIM_GBUFFER_D0_A); a.pg0 = P(alt ? ST_BUF_PRIM_GBUFFER_D0_A : ST_BUF_PRIM_GBUFFER_D0_B);
        a.g1 = P(alt ? ST_BUF_PRIM_GBUFFER_D1_B : ST_BUF_PRIM_GBUFFER_D1_A); a.pg1 = P(alt ? ST_BUF_PRIM_GBUFFER_D1_A : ST_BUF_PRIM_GBUFFER_D1_B);
        a.sm = P(alt ? ST_BUF_PRIM_SURFACE_MAP_B : ST_BUF_PRIM_SURFACE_MAP_A); a.psm = P(alt ? ST_BUF_PRIM_SURFACE_MAP_A : ST_BUF_PRIM_SURFACE_MAP_B);
        a.sn = P(ST_BUF_COUNT + (alt ? 1 : 0)); a.psn = P(ST_BUF_COUNT + (alt ? 0 : 1));
        a.reprojection = P(ST_BUF_REPROJECTION_MAP); a.velocity = P(ST_BUF_VELOCITY_MAP);
        for (int i = 0; i < 3; i++) a.di_res[i] = P(ST_BUF_DI_RESERVOIRS_0 + i);
        a.di_diff_samples = P(ST_BUF_DI_DIFF_SAMPLES); a.di_diff_prev_colors = P(ST_BUF_DI_DIFF_PREV_COLORS); a.di_diff_curr_colors = P(ST_BUF_DI_DIFF_CURR_COLORS);
        a.di_diff_moments = P(alt ? ST_BUF_DI_DIFF_MOMENTS_B : ST_BUF_DI_DIFF_MOMENTS_A); a.di_diff_prev_moments = P(alt ? ST_BUF_DI_DIFF_MOMENTS_A : ST_BUF_DI_DIFF_MOMENTS_B);
        a.di_diff_stash = P(ST_BUF_DI_DIFF_STASH); a.di_spec_samples = P(ST_BUF_DI_SPEC_SAMPLES);
        a.gi_d0 = P(ST_BUF_GI_D0); a.gi_d1 = P(ST_BUF_GI_D1); a.gi_d2 = P(ST_BUF_GI_D2);
        for (int i = 0; i < 4; i++) a.gi_res[i] = P(ST_BUF_GI_RESERVOIRS_0 + i);
        a.gi_diff_samples = P(ST_BUF_GI_DIFF_SAMPLES); a.gi_diff_prev_colors = P(ST_BUF_GI_DIFF_PREV_COLORS); a.gi_diff_curr_colors = P(ST_BUF_GI_DIFF_CURR_COLORS);
        a.gi_diff_moments = P(alt ? ST_BUF_GI_DIFF_MOMENTS_B : ST_BUF_GI_DIFF_MOMENTS_A); a.gi_diff_prev_moments = P(alt ? ST_BUF_GI_DIFF_MOMENTS_A : ST_BUF_GI_DIFF_MOMENTS_B);
        a.gi_diff_stash = P(ST_BUF_GI_DIFF_STASH); a.gi_spec_samples = P(ST_BUF_GI_SPEC_SAMPLES);
        a.ref_hits = P(ST_BUF_REF_HITS); a.ref_rays = P(ST_BUF_REF_RAYS); a.ref_colors = P(ST_BUF_REF_COLORS);
        a.dbg_used_memory = reinterpret_cast<uint32_t*>(P(ST_BUF_DBG_USED_MEMORY));
        a.width = c.desc.width; a.height = c.desc.height; a.row0 = c.row0; a.row1 = c.row1; a.col0 = c.col0; a.col1 = c.col1;
        a.frame = c.frame; a.tile_map = e.tuning.tile_map;
        return ST_OK;
    }
    // Every switch of the path-traced graph (the heatmap and reference modes need neither DI nor GI: every fusion below is off for them).
    // The fused variants share `fused_denoised`; what each asks beyond it is spelled out, and where two differ by a term the comment says so.
    int decide_switches() {
        e.last_launches.clear();   // (from here on the frame lists its launch groups)
        if (mode != ST_MODE_BVH_HEATMAP && mode != ST_MODE_REFERENCE) {   // the path-traced modes' tile words: [0, tiles) variance's, [tiles, 2 tiles) the GI preview's
            a.tile_mask = c.tile_mask.as<unsigned long long>();
            a.gi_late_mask = a.tile_mask ? a.tile_mask + c.tile_mask_tiles() : nullptr;
        }
        const StTuning& t = e.tuning; const bool fast = e.arithmetic == ST_ARITH_FAST;
        s.needs_di = mode == ST_MODE_IMAGE || mode == ST_MODE_DI_DIFFUSE || mode == ST_MODE_DI_SPECULAR;
        s.needs_gi = mode == ST_MODE_IMAGE || mode == ST_MODE_GI_DIFFUSE || mode == ST_MODE_GI_SPECULAR;
        s.denoise = c.desc.denoise != 0u; s.any_objects = !e.instances.records.empty();
        s.tracing = c.frame % 6u < 4u; s.gi_source = (s.tracing && c.frame % 2u == 1u) ? 1u : 0u;
        s.whole_graph = e.pass_mask == ~0ull;  // a row window (multi-GPU band) changes which pixels a pass owns, not which passes follow it
        s.gi_runs = s.needs_gi && s.any_objects;
        // GI history hand-over by pointer swap instead of gi_resolving's copy (CameraState::gi_aliased says when). Fast build only: the reference's
        // copy is a decode + re-encode of every reservoir, which is not the identity on all bit patterns (the octahedral normal of a few records per
        // frame moves by an ulp), and the exact build owes the parity suite those bits.
        if (c.gi_aliased && s.gi_runs && !s.whole_graph) if (int rc = materialize_gi_history(c)) return rc;
        s.swap_gi_history = t.alias_gi_history && fast && s.gi_runs && s.whole_graph && s.gi_source == 0u;
        if (s.gi_runs && s.whole_graph) c.gi_aliased = false;  // this frame's temporal pass rewrites GI_RESERVOIRS_1 completely
        s.gi_skip_history_copy = s.swap_gi_history ? 1u : 0u;
        // both GI preview passes + resolving in one launch for the pixels whose second pass draws no neighbour (k_gi.hip k_gi_preview_both); the
        // second-pass launch then serves the flagged rest. (Not part of fused_denoised: it runs without the denoiser too.)
        s.gi_preview_both = t.preview_both && s.whole_graph && t.fuse && s.gi_runs && a.gi_late_mask;
        // the half-resolution grid drops the last tile column when the tile count is odd (`(size + 7) / 8 / (2, 1)`), while the stand-alone trace
        // pass still visits those pixels: only an even tile count lets one fused spatial launch cover all three
        s.even_tiles = (((a.width + 7u) / 8u) & 1u) == 0u;
        const bool fused_denoised = s.whole_graph && t.fuse && s.denoise && s.any_objects;
        // estimate_variance's long-history branch rides in the fused reproject stages (st_passes.h denoise_reproject_finish); the variance launch
        // then serves the short-history pixels only, in place, and the strides-1+2 launch reads curr_colors. (Both chains, in either build.)
        s.variance_in_reproject = (t.variance_in_reproject && fused_denoised && t.fuse_wavelet && s.needs_di && s.needs_gi && a.tile_mask) ? 1u : 0u;
        // planes nothing reads again are not stored (st_types.h kLean*). (Fast build and Image mode only — like compose_in_wavelet, but with no output buffer too.)
        if (t.lean_frame && fast && fused_denoised && mode == ST_MODE_IMAGE) {
            s.lean = kLeanPrim | kLeanSamples;
            // (odd tracing frames count on the spatial pass to rewrite the plane: it leaves the last pixel of a row alone when the width is odd and the
            // cell's other pixel, the one it resamples, lies past the edge — as it leaves the dropped tile column alone when the tile count is odd)
            if (t.fuse_gi_reprojection && s.tracing && s.even_tiles && (c.frame % 2u == 0u || a.width % 2u == 0u)) s.lean |= kLeanGiRes2;
            if (s.gi_preview_both) s.lean |= kLeanGiMid;
            if (route.keep_velocity) s.lean |= kLeanKeepVelocity;   // a pack launch reads the velocity map
        }
        // frame composition rides in the last a-trous pass (k_denoise.hip k_denoise_wavelet_far<true>). (Fast build, Image mode and an output buffer.)
        s.compose_in_wavelet = t.fuse_compose && fast && fused_denoised && out != nullptr && mode == ST_MODE_IMAGE;
        // di_spatial's scratch records (di_diff_samples / curr_colors / stash as the reference binds them) are dead stores when the fused launch is
        // followed by resolving, denoise-reproject and the a-trous chain of the same frame. (Either build, any mode with DI; needs the fused spatial launch.)
        s.skip_dead_scratch = (t.skip_scratch_stores && fused_denoised && t.fuse_spatial && s.even_tiles && s.needs_di) ? 1u : 0u;
        // on tracing frames gi_temporal is the only reader of the reprojected reservoirs and does the reprojection itself ... and on validation
        // frames of a whole frame both of its readers — the sampling launch for the half of the pixels it re-traces, then gi_temporal, which
        // stores it — do it for themselves (ST_NO_FUSE_GI_VALIDATION=1: a launch of its own)
        s.fuse_gi_validation_now = t.fuse && t.fuse_gi_reprojection && t.fuse_gi_sampling && t.fuse_gi_validation && !s.tracing && s.whole_graph;
        s.fuse_gi_reprojection_now = (t.fuse && t.fuse_gi_reprojection && s.tracing) || s.fuse_gi_validation_now;
        // per-kernel profiling runs the graph serially on `stream`: a launch's event pair then times that kernel alone, not the kernels of the other stream it would share the chip with
        s.two_streams = t.overlap && !e.profiling && e.launch_filter == ~0ull && s.needs_di && s.needs_gi && s.any_objects;
        a.gi_skip_history_copy = s.gi_skip_history_copy; a.variance_in_reproject = s.variance_in_reproject; a.lean = s.lean; a.skip_dead_scratch = s.skip_dead_scratch;
        c.last_lean = s.lean; c.last_lean_composed = s.compose_in_wavelet && s.lean != 0u;   // which planes the frame leaves unwritten: the last a-trous pass's colour planes too
        return ST_OK;
    }
    // every node that is on gets its argument blocks and steps against where it writes this frame (OutputRoute::target); KArgs is bound by now
    void arm_output() {
        for (int n = 0; n < kHdrNodes; n++) if (route.on(n)) node_arm(n, route.target(n));
    }
    // decoded-surface twins and atmosphere LUTs, on `stream`: ordered before the side stream by ev_setup (two_streams)
    void refresh_inputs() {
        if (c.surface_map_replaced[0] || c.surface_map_replaced[1]) {
            const uint32_t now = c.frame % 2u == 1u ? 1u : 0u;   // this frame's surface map: A or B
            e.L.launch_refresh_internal_planes(a, (c.surface_map_replaced[now] ? 1u : 0u) | (c.surface_map_replaced[now ^ 1u] ? 2u : 0u), stream);
            c.surface_map_replaced[0] = c.surface_map_replaced[1] = false; luts_generated_now = true;
        }
        if (mode == ST_MODE_BVH_HEATMAP) return;   // the rest: AtmospherePass::run (passes/atmosphere.rs:78-110)
        if (!e.atmosphere_initialized) {
            e.L.launch_atmosphere_static(static_cast<float4*>(e.d_transmittance.ptr), static_cast<float4*>(e.d_scattering.ptr), stream);
            e.atmosphere_initialized = true; luts_generated_now = true;
        }
        if (!e.sky_known || e.known_sun_altitude != e.sun_altitude) {
            e.L.launch_atmosphere_sky(static_cast<const float4*>(e.d_transmittance.ptr), static_cast<const float4*>(e.d_scattering.ptr), e.sun_altitude, static_cast<float4*>(e.d_sky.ptr), stream);
            e.sky_known = true; e.known_sun_altitude = e.sun_altitude; luts_generated_now = true;
        }
    }
    // ---- stages
    void observer_modes() {   // the two modes outside the path-traced graph
        if (mode == ST_MODE_BVH_HEATMAP) { run(KS_BVH_HEATMAP, ST_PASS_BVH_HEATMAP, [&] { e.L.launch_bvh_heatmap(a, cur); }); return; }
        for (uint32_t d = 0; d <= c.desc.depth; d++) {
            run(KS_REF_TRACING, ST_PASS_REF_TRACING, [&] { e.L.launch_ref_tracing(a, d, cur); });
            run(KS_REF_SHADING, ST_PASS_REF_SHADING, [&] { e.L.launch_ref_shading(a, seed(SEED_REF_SHADING + d), d, cur); });
        }
        run(KS_REF_SHADING, ST_PASS_REF_SHADING, [&] { e.L.launch_ref_shading(a, seed(SEED_REF_SHADING + 255u), 255u, cur); });
    }
    void prim() {
        // output-chain launches of the frame before last read the G-buffer this launch rewrites, behind that frame's composing launch (the node table's reads_depth)
        (void)c.gbuffer_depth_read[c.frame % 2u].wait(cur, Fence::OtherStreams, Fence::Clear);
        if (e.tuning.fuse && s.any_objects) run(KS_PRIM_VISIBILITY_REPROJECTION, ST_PASS_PRIM_VISIBILITY | ST_PASS_FRAME_REPROJECTION, [&] { e.L.launch_prim_visibility(a, true, e.deform.deform_table(), e.deform.deform_posed(), nm_tri_geo, cur); });
        else run(KS_PRIM_VISIBILITY, ST_PASS_PRIM_VISIBILITY, [&] { e.L.launch_prim_visibility(a, false, e.deform.deform_table(), e.deform.deform_posed(), nm_tri_geo, cur); });
        if (s.any_objects && !e.tuning.fuse) run(KS_FRAME_REPROJECTION, ST_PASS_FRAME_REPROJECTION, [&] { e.L.launch_frame_reprojection(a, cur); });
    }
    // DI up to temporal resampling touches only the DI reservoirs and read-only frame inputs ...
    void di_head() {
        if (e.tuning.fuse && e.tuning.fuse_di_head) run(KS_DI_SAMPLING_TEMPORAL, ST_PASS_DI_SAMPLING | ST_PASS_DI_TEMPORAL, [&] { e.L.launch_di_sampling_temporal(a, seed(SEED_DI_SAMPLING), seed(SEED_DI_TEMPORAL), cur); });
        else {
            run(KS_DI_SAMPLING, ST_PASS_DI_SAMPLING, [&] { e.L.launch_di_sampling(a, seed(SEED_DI_SAMPLING), cur); });
            run(KS_DI_TEMPORAL, ST_PASS_DI_TEMPORAL, [&] { e.L.launch_di_temporal(a, seed(SEED_DI_TEMPORAL), cur); });
        }
    }
    // ... the spatial passes use the denoiser's planes as scratch (passes/di_spatial_resampling.rs binds di_diff_samples / curr_colors / stash),
    // and resolving writes the planes the denoiser reads
    void di_tail() {
        const StTuning& t = e.tuning;
        if (t.fuse && t.fuse_spatial && s.even_tiles) run(KS_DI_SPATIAL_FUSED, ST_PASS_DI_SPATIAL_PICK | ST_PASS_DI_SPATIAL_TRACE | ST_PASS_DI_SPATIAL_SAMPLE, [&] { e.L.launch_di_spatial_fused(a, seed(SEED_DI_SPATIAL_PICK), seed(SEED_DI_SPATIAL_SAMPLE), cur); });
        else {
            run(KS_DI_SPATIAL_PICK, ST_PASS_DI_SPATIAL_PICK, [&] { e.L.launch_di_spatial_pick(a, seed(SEED_DI_SPATIAL_PICK), cur); });
            run(KS_DI_SPATIAL_TRACE, ST_PASS_DI_SPATIAL_TRACE, [&] { e.L.launch_spatial_trace(a, a.di_diff_samples, a.di_diff_curr_colors, a.di_diff_stash, cur); });
            run(KS_DI_SPATIAL_SAMPLE, ST_PASS_DI_SPATIAL_SAMPLE, [&] { e.L.launch_di_spatial_sample(a, seed(SEED_DI_SPATIAL_SAMPLE), cur); });
        }
        if (t.fuse && s.denoise) { run(KS_DI_RESOLVING_REPROJECT, ST_PASS_DI_RESOLVING | ST_PASS_DENOISE_REPROJECT_DI, [&] { e.L.launch_di_resolving(a, true, cur); }); di_reprojected = true; }
        else run(KS_DI_RESOLVING, ST_PASS_DI_RESOLVING, [&] { e.L.launch_di_resolving(a, false, cur); });
    }
    void gi_temporal() {
        if (s.fuse_gi_reprojection_now) run(KS_GI_REPROJECTION_TEMPORAL, ST_PASS_GI_REPROJECTION | ST_PASS_GI_TEMPORAL, [&] { e.L.launch_gi_temporal(a, seed(SEED_GI_TEMPORAL), true, cur); });
        else run(KS_GI_TEMPORAL, ST_PASS_GI_TEMPORAL, [&] { e.L.launch_gi_temporal(a, seed(SEED_GI_TEMPORAL), false, cur); });
    }
    void gi_sampling() {
        if (e.tuning.fuse && e.tuning.fuse_gi_sampling) { run(KS_GI_SAMPLING_AB, ST_PASS_GI_SAMPLING_A | ST_PASS_GI_SAMPLING_B, [&] { e.L.launch_gi_sampling_ab(a, seed(SEED_GI_SAMPLING_A), seed(SEED_GI_SAMPLING_B), s.fuse_gi_validation_now, cur); }); return; }
        run(KS_GI_SAMPLING_A, ST_PASS_GI_SAMPLING_A, [&] { e.L.launch_gi_sampling_a(a, seed(SEED_GI_SAMPLING_A), cur); });
        run(KS_GI_SAMPLING_B, ST_PASS_GI_SAMPLING_B, [&] { e.L.launch_gi_sampling_b(a, seed(SEED_GI_SAMPLING_B), cur); });
    }
    // GI up to the first preview pass: touches only reservoirs, gi_d0..2 and read-only frame inputs
    void gi_head() {
        if (!s.fuse_gi_reprojection_now) run(KS_GI_REPROJECTION, ST_PASS_GI_REPROJECTION, [&] { e.L.launch_gi_reprojection(a, cur); });
        if (s.tracing) {
            if (c.frame % 2u == 0u) gi_sampling();
            gi_temporal();
            if (c.frame % 2u == 1u) {
                if (e.tuning.fuse && e.tuning.fuse_spatial && s.even_tiles)
                    run(KS_GI_SPATIAL_FUSED, ST_PASS_GI_SPATIAL_PICK | ST_PASS_GI_SPATIAL_TRACE | ST_PASS_GI_SPATIAL_SAMPLE, [&] { e.L.launch_gi_spatial_fused(a, seed(SEED_GI_SPATIAL_PICK), seed(SEED_GI_SPATIAL_SAMPLE), cur); });
                else {
                    run(KS_GI_SPATIAL_PICK, ST_PASS_GI_SPATIAL_PICK, [&] { e.L.launch_gi_spatial_pick(a, seed(SEED_GI_SPATIAL_PICK), cur); });
                    run(KS_GI_SPATIAL_TRACE, ST_PASS_GI_SPATIAL_TRACE, [&] { e.L.launch_spatial_trace(a, a.gi_d0, a.gi_d1, a.gi_d2, cur); });
                    run(KS_GI_SPATIAL_SAMPLE, ST_PASS_GI_SPATIAL_SAMPLE, [&] { e.L.launch_gi_spatial_sample(a, seed(SEED_GI_SPATIAL_SAMPLE), cur); });
                }
            }
        } else { gi_sampling(); gi_temporal(); }
        if (!s.gi_preview_both) run(KS_GI_PREVIEW, ST_PASS_GI_PREVIEW_0, [&] { e.L.launch_gi_preview(a, pseed, 0u, gi_preview_src(), a.gi_res[3], cur); });
    }
    // second preview pass + resolving (+ reproject): the first GI stage that writes planes the denoiser/composition read
    void gi_tail() {
        const bool dn = s.denoise; const uint32_t gi_source = s.gi_source;
        if (s.gi_preview_both) {
            // one launch group of two kernels = one set of pass bits
            const uint64_t group = ST_PASS_GI_PREVIEW_0 | ST_PASS_GI_PREVIEW_1 | ST_PASS_GI_RESOLVING | (dn ? (uint64_t)ST_PASS_DENOISE_REPROJECT_GI : 0ull);
            run(dn ? KS_GI_PREVIEW_BOTH : KS_GI_PREVIEW_BOTH_NO_REPROJECT, group, [&] { e.L.launch_gi_preview_both(a, pseed, gi_preview_src(), a.gi_res[3], gi_source, dn, cur); });
            a.gi_preview_late = 1u;
            a.gi_mid_src = (a.lean & kLeanGiMid) ? gi_preview_src() : nullptr;
            run(KS_GI_PREVIEW_LATE, group, [&] { e.L.launch_gi_preview_resolve(a, pseed, 1u, a.gi_res[3], gi_source, dn, cur); });
            a.gi_preview_late = 0u; a.gi_mid_src = nullptr;
            if (dn) gi_reprojected = true;
        } else if (e.tuning.fuse) {
            if (dn) { run(KS_GI_PREVIEW_RESOLVE_REPROJECT, ST_PASS_GI_PREVIEW_1 | ST_PASS_GI_RESOLVING | ST_PASS_DENOISE_REPROJECT_GI, [&] { e.L.launch_gi_preview_resolve(a, pseed, 1u, a.gi_res[3], gi_source, true, cur); }); gi_reprojected = true; }
            else run(KS_GI_PREVIEW_RESOLVE, ST_PASS_GI_PREVIEW_1 | ST_PASS_GI_RESOLVING, [&] { e.L.launch_gi_preview_resolve(a, pseed, 1u, a.gi_res[3], gi_source, false, cur); });
        } else {
            run(KS_GI_PREVIEW, ST_PASS_GI_PREVIEW_1, [&] { e.L.launch_gi_preview(a, pseed, 1u, a.gi_res[3], a.gi_res[0], cur); });
            run(KS_GI_RESOLVING, ST_PASS_GI_RESOLVING, [&] { e.L.launch_gi_resolving(a, gi_source, cur); });
        }
        // the launches above were told not to copy (KArgs::gi_skip_history_copy)
        if (s.swap_gi_history) { std::swap(c.plane[ST_BUF_GI_RESERVOIRS_0], c.plane[ST_BUF_GI_RESERVOIRS_1]); c.gi_aliased = true; }
    }
    void denoise() {
        if (!s.denoise) return;
        // the denoiser can use its own block -> tile mapping (see `tile_map_denoise`)
        struct MapScope { KArgs& a; uint32_t saved; MapScope(KArgs& a_, uint32_t m) : a(a_), saved(a_.tile_map) { a.tile_map = m; } ~MapScope() { a.tile_map = saved; } } map_scope(a, e.tuning.tile_map_denoise);
        if (!di_reprojected) run(KS_DENOISE_REPROJECT, ST_PASS_DENOISE_REPROJECT_DI, [&] { e.L.launch_denoise_reproject(a, a.di_diff_prev_colors, a.di_diff_prev_moments, a.di_diff_samples, a.di_diff_curr_colors, a.di_diff_moments, cur); });
        if (!gi_reprojected) run(KS_DENOISE_REPROJECT, ST_PASS_DENOISE_REPROJECT_GI, [&] { e.L.launch_denoise_reproject(a, a.gi_diff_prev_colors, a.gi_diff_prev_moments, a.gi_diff_samples, a.gi_diff_curr_colors, a.gi_diff_moments, cur); });
        // ping-pong (passes/frame_denoising.rs:87-110): stash -> prev -> stash -> curr -> stash -> curr
        float4* di[3] = {a.di_diff_stash, a.di_diff_prev_colors, a.di_diff_curr_colors};
        float4* gi[3] = {a.gi_diff_stash, a.gi_diff_prev_colors, a.gi_diff_curr_colors};
        const int in_ix[5] = {0, 1, 0, 2, 0}, out_ix[5] = {1, 0, 2, 0, 2};
        uint32_t first = 0;
        // StTuning::side_start: behind which launch of the chain the NEXT frame's primary visibility may start (two_streams). The LDS-staged launches
        // (strides 1+2, stride 4) fill a CU's LDS, so a tracing block beside them waits for a CU instead of sharing one.
        auto side_point = [&](uint32_t point) {
            if (!s.two_streams || first != 2u || e.tuning.side_start != point) return;
            side_rc = c.ev_lds_done.record(stream); c.have_lds_done = side_rc == ST_OK;
        };
        if (e.tuning.fuse && e.tuning.fuse_wavelet) {
            // variance estimation + strides 1 and 2 form one launch group of two kernels: the variance pass hands its output over in an internal pair of planes
            // (k_denoise.hip k_denoise_wavelet_12 says why), so the stash planes receive the stride-2 result directly. One group = one set of pass bits (st_debug_set_pass_mask).
            const uint64_t group = ST_PASS_DENOISE_VARIANCE | ST_PASS_DENOISE_WAVELET_0 | ((uint64_t)ST_PASS_DENOISE_WAVELET_0 << 1);
            // (with KArgs::variance_in_reproject the hand-over planes are the reproject stages' own outputs)
            float4* tmp_di = a.variance_in_reproject ? a.di_diff_curr_colors : c.plane[ST_BUF_COUNT + 2];
            float4* tmp_gi = a.variance_in_reproject ? a.gi_diff_curr_colors : c.plane[ST_BUF_COUNT + 3];
            run(KS_DENOISE_VARIANCE, group, [&] { e.L.launch_denoise_variance(a, tmp_di, tmp_gi, cur); });
            run(KS_DENOISE_WAVELET_12, group, [&] { e.L.launch_denoise_wavelet_12(a, 1.0f, 2.0f, tmp_di, di[1], di[0], tmp_gi, gi[1], gi[0], cur); });
            first = 2;
            side_point(1u);
        } else run(KS_DENOISE_VARIANCE, ST_PASS_DENOISE_VARIANCE, [&] { e.L.launch_denoise_variance(a, a.di_diff_stash, a.gi_diff_stash, cur); });
        for (uint32_t nth = first; nth < 5; nth++) {
            if (nth == 4u && s.compose_in_wavelet) {
                Engine::present_guard(c, out, cur); e.dist_guard(c.handle, out, cur);
                run(KS_DENOISE_WAVELET_COMPOSE, ((uint64_t)ST_PASS_DENOISE_WAVELET_0 << nth) | ST_PASS_COMPOSITION, [&] {
                    e.L.launch_denoise_wavelet_compose(a, 1u << nth, (float)(1u + nth), di[in_ix[nth]], di[out_ix[nth]], gi[in_ix[nth]], gi[out_ix[nth]], mode, route.comp_out, route.comp_format, a.lean == 0u, route.comp_disp, cur); });
                composed = true;
                continue;
            }
            run(KS_DENOISE_WAVELET, (uint64_t)ST_PASS_DENOISE_WAVELET_0 << nth, [&] { e.L.launch_denoise_wavelet(a, 1u << nth, (float)(1u + nth), di[in_ix[nth]], di[out_ix[nth]], gi[in_ix[nth]], gi[out_ix[nth]], cur); });
            side_point(nth);   // 2: behind stride 4, 3: behind stride 8
        }
    }
    // The nodes' early launches (the node table's `early`), in chain order: they read this frame's planes that the NEXT frame's primary
    // visibility overwrites, so they run on `stream` before that may start; what they write is the camera's own.
    void pack_early() {
        for (int n = 0; n < kHdrNodes; n++) if (route.on(n)) run_node(n, 0u, kHdrNode[n].early);
    }
    void compose() {   // every mode's composition, unless the last a-trous pass did it
        if (!out || composed) return;
        Engine::present_guard(c, out, cur); e.dist_guard(c.handle, out, cur);
        const bool dn = s.denoise;
        const float4* di_diff = (dn && (mode == ST_MODE_IMAGE || mode == ST_MODE_DI_DIFFUSE)) ? a.di_diff_curr_colors : a.di_diff_samples;
        const float4* gi_diff = (dn && (mode == ST_MODE_IMAGE || mode == ST_MODE_GI_DIFFUSE)) ? a.gi_diff_curr_colors : a.gi_diff_samples;
        run(KS_COMPOSITION, ST_PASS_COMPOSITION, [&] { e.L.launch_composition(a, mode, di_diff, gi_diff, route.comp_out, route.comp_format, route.comp_disp, cur); });
        composed = true;
    }

    // ---- schedules
    // Two streams, software-pipelined across frames: `side` carries primary visibility and the GI chain; `stream` carries the DI passes (sampling + temporal
    // resampling too, by default: measured 1.2 % on the dungeon, nothing on Cornell, against running them behind primary visibility on `side`), the denoiser
    // and composition. Events express the true data dependencies only, so the reservoir passes of frame N+1 overlap the denoiser of frame N:
    //   prim(N+1)      after DI tail(N)       — it overwrites frame N's "previous" G-buffer + the reprojection map
    //   GI tail(N+1)   after frame N is done  — it writes gi sample/colour/moment planes the denoiser + composition read
    //   DI head(N+1)   after prim(N+1)        (ev_di_head)
    //   DI tail(N+1)   after DI head(N+1)     (and after frame N's composition by stream order: its scratch aliases the denoiser's planes)
    //   denoiser(N+1)  after GI tail(N+1)
    // StTuning::side_start = 1 ... 3 adds one wait in front of prim(N+1): for ev_lds_done(N), recorded on `stream` inside frame N's a-trous chain (denoise()
    // side_point: behind strides 1+2, stride 4 or stride 8). That point is enqueued on `stream` later than ev_prim_ok(N), so the extra wait can only strengthen
    // the order above. No cycle: `stream` waits for ev_di_head(N+1), recorded on `side` behind prim(N+1); `side` waits for ev_lds_done(N), which the previous
    // render call enqueued completely, behind launches that wait for nothing of frame N+1. A frame that records no such point (no denoiser, the unfused
    // a-trous chain, serial()) leaves have_lds_done clear, and the next frame starts behind ev_prim_ok alone, as with side_start = 0.
    int two_streams() {
        const StTuning& t = e.tuning;
        if (!c.side_stream) {
            int least = 0, greatest = 0;
            (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
            const int priority = t.side_priority > 0 ? greatest : (t.side_priority < 0 ? least : 0);
            ST_HIP(hipStreamCreateWithPriority(&c.side_stream.h, hipStreamNonBlocking, priority));
        }
        // LUT generation issued on `stream` in this call must precede the side stream's consumers. (Do NOT do this unconditionally: an event recorded on `stream`
        // here completes only after frame N's denoiser, which would serialise prim(N+1) behind it. Uploads in st_tick are followed by a host-side stream sync.)
        if (luts_generated_now) { if (int rc = c.ev_setup.record(stream)) return rc; if (int rc = c.ev_setup.wait(c.side_stream)) return rc; }
        // copies st_tick queued without joining the stream (staged uploads, dynamic images): they sit behind frame N on the tick's stream, so a frame that
        // follows a scene change gives up the prim(N+1) / denoiser(N) overlap
        if (int rc = e.copies.begin(c.side_stream, kReadsNothing)) return rc;  // the tick's uploads: independent of frame N, the overlap stays
        if (c.have_prev_frame_events) { if (int rc = c.ev_prim_ok.wait(c.side_stream)) return rc; }
        if (c.have_prev_frame_events && c.have_lds_done) { if (int rc = c.ev_lds_done.wait(c.side_stream)) return rc; }
        c.have_lds_done = false;   // this frame's denoise() sets it again
        cur = c.side_stream;
        prim();
        if (!t.di_head_on_main) di_head();
        if (int rc = c.ev_di_head.record(c.side_stream)) return rc;  // primary visibility (+ DI head) of this frame are through
        gi_head();
        if (c.have_prev_frame_events) { if (int rc = c.ev_frame_done.wait(c.side_stream)) return rc; }
        gi_tail();
        if (int rc = c.ev_gi_done.record(c.side_stream)) return rc;
        cur = stream;
        if (int rc = c.ev_di_head.wait(stream)) return rc;
        if (t.di_head_on_main) di_head();
        di_tail();
        pack_early();   // before ev_prim_ok: prim(N+1) rewrites the velocity map
        // stand-alone denoise reprojection kernels (unfused path) still read the reprojection map: prim(N+1) may only start once they are through
        const bool reproject_later = s.denoise && !t.fuse;
        if (!reproject_later) { if (int rc = c.ev_prim_ok.record(stream)) return rc; }
        if (int rc = c.ev_gi_done.wait(stream)) return rc;
        denoise();
        if (side_rc) return side_rc;
        if (reproject_later) { if (int rc = c.ev_prim_ok.record(stream)) return rc; }
        compose();
        if (int rc = c.ev_frame_done.record(stream)) return rc;
        c.have_prev_frame_events = true;
        return ST_OK;
    }
    // everything on `stream`, in the reference's order: the heatmap and reference modes, profiled frames, frames without DI, GI or objects
    int serial() {
        if (mode == ST_MODE_BVH_HEATMAP || mode == ST_MODE_REFERENCE) { observer_modes(); compose(); return ST_OK; }
        prim();
        if (s.any_objects) {
            if (s.needs_di) { di_head(); di_tail(); }
            if (s.needs_gi) { gi_head(); gi_tail(); }
        }
        pack_early();
        denoise();
        compose();
        // (a camera that has run the two-stream schedule: its next such frame waits for these — and for them alone: ev_prim_ok stands behind the whole chain here)
        c.have_lds_done = false;
        if (c.side_stream) { if (int rc = c.ev_prim_ok.record(stream)) return rc; if (int rc = c.ev_frame_done.record(stream)) return rc; }
        return ST_OK;
    }
    // The launches behind the composing launch, which ran on `stream`: the rest of every HDR node that is on, in chain order, then
    // post-processing — one launch group (ST_PASS_POST) —, then the meter's finalize; each stage's fence is recorded behind its launches, and the
    // G-buffer depth's behind the last node that read it here.
    int finish_output() {
        cur = stream;
        int last_depth_reader = -1;
        for (int n = 0; n < kHdrNodes; n++) if (route.on(n) && kHdrNode[n].reads_depth) last_depth_reader = n;
        for (int n = 0; n < kHdrNodes; n++) {
            if (!route.on(n)) continue;
            run_node(n, kHdrNode[n].early, node_steps(n));
            if (int rc = route.planes_read[n]->record(stream)) return rc;   // the planes' fence, behind the node's last launch
            if (n == kNodeGrade && work.grade_lut) if (int rc = work.grade_lut->fence.record(stream)) return rc;   // the table leaves behind its last reader (st_grade.cpp upload_luts)
            if (n == last_depth_reader) if (int rc = c.gbuffer_depth_read[c.frame % 2u].record(stream)) return rc;
        }
        if (route.post) {   // at most two kernels; with the upscale stage (st_upscale.cpp) behind FXAA at most three
            void* const composed = c.post.planes.plane[0].ptr; void* const fxaa_out = c.post.planes.plane[1].ptr;
            const uint32_t w = c.desc.width, h = c.desc.height;
            const bool up = route.up_steps;
            if (route.up_nearest) {   // a heatmap frame under the upscale stage: false colour, brought to the output size and not sharpened
                StPostDesc nearest{}; nearest.output_width = c.upscale.desc.output_width; nearest.output_height = c.upscale.desc.output_height; nearest.filter = ST_RESAMPLE_NEAREST;
                const Engine::PostPlan plan = Engine::post_plan(nearest, false, composed, w, h, nullptr, out, c.out_format);
                run(KS_POST_RESAMPLE, ST_PASS_POST, [&] { e.L.launch_post_resample(plan.rs, cur); }, plan.resample_bytes);
            } else if (route.post_fxaa || !up) {   // under the upscale stage FXAA writes the render-size plane the upscaler reads
                const Engine::PostPlan plan = Engine::post_plan(c.post.desc, route.post_fxaa, composed, w, h, fxaa_out, up ? fxaa_out : out, up ? (uint32_t)ST_FORMAT_RGBA32F : c.out_format);
                if (plan.fxaa) run(KS_POST_FXAA, ST_PASS_POST, [&] { e.L.launch_post_fxaa(plan.fx, cur); }, plan.fxaa_bytes);
                if (plan.resample) run(KS_POST_RESAMPLE, ST_PASS_POST, [&] { e.L.launch_post_resample(plan.rs, cur); }, plan.resample_bytes);
            }
            if (up) {
                const Engine::UpscalePlan plan = Engine::upscale_plan(c.upscale.desc, route.post_fxaa ? fxaa_out : composed, w, h, c.upscale.planes.plane[0].ptr, out, c.out_format, e.upscale_fused);
                if (plan.fused) run(KS_UPSCALE_SHARPEN, ST_PASS_POST, [&] { e.L.launch_upscale_sharpen(plan.fu, plan.fused, cur); }, plan.fused_bytes);
                else if (plan.upscale) run(KS_UPSCALE, ST_PASS_POST, [&] { e.L.launch_upscale(plan.up, cur); }, plan.upscale_bytes);
                if (plan.sharpen && !plan.fused) run(KS_SHARPEN, ST_PASS_POST, [&] { e.L.launch_sharpen(plan.sh, cur); }, plan.sharpen_bytes);
                if (int rc = c.upscale.planes.done(stream)) return rc;
            }
            if (int rc = c.post.planes.done(stream)) return rc;
        }
        if (route.comp_disp.meter && out) if (int rc = e.display_finalize(c, stream)) return rc;
        return ST_OK;
    }
};
}  // namespace

int Engine::render(CameraState& c, void* out, hipStream_t stream) {
    if (!has_device) return fail(ST_ERR_NO_DEVICE, "render_camera on a host-only engine");
    if (!copies.scene.written) return fail(ST_ERR_INVALID_ARGUMENT, "st_tick must precede st_render_camera");
    ST_HIP(hipSetDevice(device));
    if (int rc = copies.begin(stream, kReadsFrame)) return rc;
    Frame f(*this, c, out, stream);
    if (int rc = f.route_output()) return rc;      // display, post-processing, the HDR nodes that are on: where the composing launch and each node write
    if (int rc = f.bind_args()) return rc;         // KArgs: scene, lights, the camera's planes
    f.refresh_inputs();                            // what they name and this call has to make first: decoded-surface twins, atmosphere LUTs
    if (int rc = f.decide_switches()) return rc;   // which fused variants this frame takes, which schedule
    f.arm_output();                                // the HDR nodes' argument blocks and steps
    if (int rc = f.s.two_streams ? f.two_streams() : f.serial()) return rc;
    if (int rc = f.finish_output()) return rc;     // the HDR nodes' launches behind the composing launch, post-processing, the meter's finalize
    if (int rc = copies.end(stream, kReadsFrame)) return rc;   // the end of the last frame that reads these copies of the scene and the lights
    profile_close();
    ST_HIP(hipGetLastError());
    if (f.mask_split) return fail(ST_ERR_INVALID_ARGUMENT, "the pass mask splits a fused launch (st_debug_last_launches lists the launch groups)");
    return ST_OK;
}

}  // namespace st
