// st_tick.cpp — host engine of libstrolle_hip.so: Engine::tick (lib.rs:301-395): refresh of the stores (materials, instances, lights) + uploads (the
// triangle-slot arrays, the scene copy's records and tables, images, lights); the tree's decisions and its half of the upload are
// st_bvh_refresh.cpp's. Behind it SceneCopies (st_copies.h): which copy a tick writes, what its readers wait for and record. See st_engine.h.
#include "st_engine.h"

namespace st {

// Whether copy `t`'s device arrays hold the host's triangle-slot arrays as they are now (otherwise they are sent whole, into a larger allocation).
bool Engine::tri_fits(const SceneSet& t, unsigned arrays) const {
    if ((arrays & TRI_GEO) && (t.tri_geo.capacity < slots.geo().size() * sizeof(float4) || t.tri_bounds.capacity < slots.bounds().size() * sizeof(float4))) return false;
    return !(arrays & TRI_ATTR) || t.tri_attr.capacity >= slots.attr().size() * sizeof(float4);
}
// The triangle slots copy `t` lacks: all when `whole` or an array outgrew its allocation (attribute records then follow the hit-test records), else
// [dirty_lo, dirty_hi). Attribute records go BEFORE a device bake of the copy: an instance the host baked a tick ago and the device moves now ends with the device's.
int Engine::upload_tri_slots(SceneSet& t, unsigned arrays, bool whole, hipStream_t up, bool* pageable) {
    int rc;
    const std::vector<float4>& tri_geo = slots.geo(), & tri_attr = slots.attr(), & tri_bounds = slots.bounds();   // (3, 4 and 2 float4 per slot)
    const size_t lo = t.dirty_lo, n = t.dirty_lo < t.dirty_hi ? t.dirty_hi - t.dirty_lo : 0;
    if (arrays & TRI_GEO) {
        whole = whole || !tri_fits(t, TRI_GEO);
        if (whole) {
            if ((rc = t.tri_geo.upload(tri_geo.data(), tri_geo.size() * sizeof(float4), up, staging, pageable))) return rc;
            if ((rc = t.tri_bounds.upload(tri_bounds.data(), tri_bounds.size() * sizeof(float4), up, staging, pageable))) return rc;
        } else if (n) {
            if ((rc = t.tri_geo.upload_range(tri_geo.data(), 3 * lo * sizeof(float4), 3 * n * sizeof(float4), up, staging, pageable))) return rc;
            if ((rc = t.tri_bounds.upload_range(tri_bounds.data(), 2 * lo * sizeof(float4), 2 * n * sizeof(float4), up, staging, pageable))) return rc;
        }
    }
    if (!(arrays & TRI_ATTR)) return ST_OK;
    if (whole || !tri_fits(t, TRI_ATTR)) return t.tri_attr.upload(tri_attr.data(), tri_attr.size() * sizeof(float4), up, staging, pageable);
    return n ? t.tri_attr.upload_range(tri_attr.data(), 4 * lo * sizeof(float4), 4 * n * sizeof(float4), up, staging, pageable) : ST_OK;
}
// ---- tick (lib.rs:301-395)
int Engine::tick(hipStream_t stream) {
    // skinned meshes: the poses set since the last tick are skinned first — a host bake of this refresh reads their posed triangles back
    const bool skinning = has_device && deform.any();
    deform.begin_tick();   // (deformation motion: a previous pose lasts one tick)
    if (skinning) {
        ST_HIP(hipSetDevice(device));
        staging.begin_tick();
        if (int rc = deform.tick(stream)) return rc;
    }
    const TreePlan plan = refresh_scene();
    apply_environment();   // (before the lights: a map switches the sun, light 0, off)
    if (!has_device) lut_edits.clear();   // (a host-only engine holds no table)
    refresh_sun_and_lights();
    if (has_device) {
        ST_HIP(hipSetDevice(device));
        if (walk_flags_host && (walk_flags_host[0] | walk_flags_host[1]) != 0u) note_walk_overflow();   // a wide walk of an earlier frame dropped a push
        copies.begin_tick();
        if (!skinning) staging.begin_tick();
        TickIo io{stream};
        int rc;
        if ((rc = upload_scene(plan, io)) || (rc = upload_images(io)) || (rc = upload_lights(io)) || (rc = upload_environment(io)) || (rc = upload_luts(io)) || (rc = copies.end_uploads(io))) return rc;
    }
    images.dirty = false;
    for (auto& kv : cameras) kv.second->frame = frame;  // CameraController::flush
    frame += 1;
    if (int rc = take_deferred_status()) return rc;   // a read-back of posed triangles failed: the host baked their bind pose
    return report_deep_bvh();
}
// Materials and instances (baked) on the host, the instances' transform table; then the tree's plan: what upload_scene does with the tree (st_bvh_refresh.h).
TreePlan Engine::refresh_scene() {
    materials_changed_this_tick = materials.dirty || images.rects_dirty || images.dirty;   // a Blend flag may have changed: the tree's topology signature has to be looked at
    if (materials_changed_this_tick) { materials.dirty = images.rects_dirty = false; materials.rebuild(images); }
    const auto t0 = TickClock::now();
    const bool instances_changed = refresh_instances();
    if (instances_changed) instances.fill_xforms();
    // slots, liveness, materials or Blend flags may have changed (a Blend flag under any slot)
    if ((instances_changed && !moved_on_device) || materials_changed_this_tick) tree.slots_changed(materials_changed_this_tick);
    return tree.plan(instances_changed, moved_on_device, materials_changed_this_tick, t0);
}
void Engine::refresh_sun_and_lights() {
    float sa, ca, sz, cz;   // World::sun_dir (world.rs:18-24)
    sincos_(sun_altitude, &sa, &ca); sincos_(sun_azimuth, &sz, &cz);
    sun_dir_ = v3(ca * sz, sa, -ca * cz);
    if (sun_dirty) {
        sun_dirty = false;
        // an environment map replaces the atmosphere, sun included, unless ST_ENV_KEEP_SUN (include/strolle_hip.h "environment lighting")
        const V3 color = env_sun_off ? v3s(0.0f) : sun_transmittance(v3(0.0f, 6.360f + 0.0002f, 0.0f), sun_dir_) * 20.0f * 5.0f;
        GpuLight sun{};
        sun.d0 = f4(sun_dir_ * 1000.0f, 25.0f); sun.d1 = f4(color, INFINITY); sun.d2 = make_float4(b2f(1u), 0, 0, 0);
        lights.set_sun(sun);
    }
    lights.snapshot();
}
// The scene's device copy: its tree as `plan` says (SceneTree::write), then the attribute records still owed, the transforms, tables and materials.
int Engine::upload_scene(TreePlan plan, TickIo& io) {
    if (plan == TreePlan::none && !materials_changed_this_tick && copies.scene.written) return ST_OK;   // (a material or atlas edit changes records, not the tree)
    int rc;
    CopyTarget c;
    if ((rc = copies.pick(io, copies.scene, c))) return rc;
    SceneSet& t = copies.scene.copy[c.index];
    bool attr_sent = false;
    if ((rc = tree.write(t, plan, c.up, c.pageable, &attr_sent))) return rc;
    if (!attr_sent && (rc = upload_tri_slots(t, TRI_ATTR, !t.valid || t.tri_full, c.up, c.pageable))) return rc;
    // Normal mapping reads the hit-test records per slot, and a copy written from a host tree has none (SceneSet::geo_current): while the switch is on and a
    // material has a map they travel with this upload, so that a moving scene pays no host join in its frames (Engine::normal_map_geo sends them only
    // where the switch, or a flagged query, comes after the tick). The host's array is current here: such a copy was just written from it.
    if (normal_mapping && materials.any_normal_map && !t.geo_current && !slots.geo().empty()) {
        if ((rc = t.tri_geo.upload(slots.geo().data(), slots.geo().size() * sizeof(float4), c.up, staging, c.pageable))) return rc;
        t.geo_current = true;
    }
    t.dirty_lo = SIZE_MAX; t.dirty_hi = 0; t.tri_full = false; t.valid = true;
    if ((rc = t.xforms.upload(instances.xforms.data(), instances.xforms.size() * sizeof(float4), c.up, staging, c.pageable))) return rc;
    // the scene queries' handle table follows the slots of this copy (a spawn, a despawn, a re-inserted mesh move triangle ranges)
    fill_instance_table();
    if ((rc = t.instance_table.upload(instance_table_.data(), instance_table_.size() * sizeof(uint32_t), c.up, staging, c.pageable))) return rc;
    if ((rc = t.materials.upload(materials.gpu().data(), materials.gpu().size() * sizeof(GpuMaterial), c.up, staging, c.pageable))) return rc;
    if ((rc = t.base_packed.upload(materials.base_packed().data(), materials.base_packed().size() * sizeof(uint32_t), c.up, staging, c.pageable))) return rc;
    copies.commit(io, copies.scene, c); tree.went_live(plan);
    return ST_OK;
}
// The atlas, the device images and the blue noise: in place, on the caller's stream.
int Engine::upload_images(TickIo& io) {
    if (images.dirty || blue_noise_dirty) io.uploaded = true;
    if (images.dirty) if (int rc = d_atlas.upload(images.texels().data(), images.texels().size(), io.stream, staging, &io.pageable)) return rc;
    const size_t atlas_pitch = (size_t)images.width() * 4;
    for (auto& kv : images.device()) {
        ImageAtlas::DeviceImage& di = kv.second;
        if (!di.pending && !di.dynamic) continue;
        const ImageAtlas::Rect& r = *images.rect_texels(kv.first);
        uint8_t* dst = static_cast<uint8_t*>(d_atlas.ptr) + ((size_t)r.y * images.width() + r.x) * 4;
        ST_HIP(hipMemcpy2DAsync(dst, atlas_pitch, di.pixels, di.pitch, (size_t)r.w * 4, r.h, hipMemcpyDeviceToDevice, io.stream));
        if (!di.dynamic) {  // keep the host copy complete: it is what a later full upload sends
            ST_HIP(hipMemcpy2DAsync(images.texel(r.x, r.y), atlas_pitch, di.pixels, di.pitch, (size_t)r.w * 4, r.h, hipMemcpyDeviceToHost, io.stream));
            io.pageable = true;  // joins the stream below before the host copy is read again
        }
        di.pending = false;
        io.uploaded = true;
    }
    if (blue_noise_dirty) {
        if (int rc = d_blue_noise.upload(blue_noise.data(), blue_noise.size(), io.stream, staging, &io.pageable)) return rc;
        blue_noise_dirty = false;
    }
    return ST_OK;
}
// Lights change rarely; skipping the identical re-upload also skips the stream sync of end_uploads, so the host can run a frame ahead of
// the GPU (the reference re-uploads only dirty buffers too: mapped_storage_buffer.rs:103-121). They alternate like the scene, on their own schedule.
int Engine::upload_lights(TickIo& io) {
    if (!lights.changed()) return ST_OK;
    CopyTarget c;
    if (int rc = copies.pick(io, copies.lights, c)) return rc;
    if (int rc = copies.lights.copy[c.index].buf.upload(lights.table().data(), lights.table().size() * sizeof(GpuLight), c.up, staging, c.pageable)) return rc;
    copies.commit(io, copies.lights, c);
    lights.mark_uploaded();
    return ST_OK;
}
// The tick did everything; these statuses say what the frames rendered so far may have missed, or what the uploaded tree can cost.
int Engine::report_deep_bvh() {
    if (walk_overflow_unreported) {   // later frames walk with the deeper stack
        walk_overflow_unreported = false;
        const std::string msg = "a traversal of the wide BVH stream found its stack full and DROPPED a push: frames rendered so far may have missed geometry behind the dropped subtrees. "
                                "Later frames walk with " + std::to_string(wide_stack_entries_now()) + " pending entries per ray" + (packets_overflowed ? " and primary rays with the per-lane walk instead of the packet walk" : "") +
                                " (st_debug_walk_overflow); StTuning::allow_deep_bvh = 1 turns this status into a warning";
        if (!tuning.allow_deep_bvh) return fail(ST_ERR_BVH_TOO_DEEP, msg);
        fprintf(stderr, "[strolle-hip] warning: %s\n", msg.c_str());
    }
    return tree.report_too_deep();
}
// ---- SceneCopies (st_copies.h)
// Which copy of `pair` this tick writes, on which stream: the first upload and ST_NO_DOUBLE_BUFFER=1 write the live copy in place on the caller's
// stream (behind the frames queued there), and so do mixed streams, behind a join; every later change goes to the other copy on copy_stream.
template <class T> int SceneCopies::pick(TickIo& io, CopyPair<T>& pair, CopyTarget& c) {
    c = CopyTarget{pair.live, io.stream, &io.pageable, false};
    if (!e.tuning.double_buffer || !pair.written || mixed()) return join_mixed();
    if (!copy_stream) ST_HIP(hipStreamCreateWithFlags(&copy_stream.h, hipStreamNonBlocking));
    if (!pair.alternating) {  // frames enqueued so far read the live copy without marking their end: mark it now, behind them
        pair.alternating = true;
        if (int rc = pair.current().fence.record(io.stream)) return rc;
    }
    c = CopyTarget{pair.live ^ 1, copy_stream, &io.pageable_copy, true};
    return pair.other().fence.wait(copy_stream, Fence::AnyStream, Fence::Clear);   // its readers are done first; cleared: the copy is written anew
}
// What was uploaded went through page-locked staging, so the caller may change the scene again at once; the next frame's streams wait for these
// copies' events (begin). Only copies that touch pageable host memory directly (staging full or disabled) make the tick wait for their stream.
int SceneCopies::end_uploads(TickIo& io) {
    if (io.copied) {
        if (int rc = copy_done.record(copy_stream)) return rc;
        if (int rc = copy_done.wait(io.stream, Fence::AnyStream, Fence::Keep)) return rc;  // the caller's stream: the next frame's kernels (and the staging slot's event) come after the copies; kept for begin
    }
    if (int rc = e.staging.end_tick(io.stream)) return rc;
    if (io.uploaded) if (int rc = tick_done.record(io.stream)) return rc;
    if (io.pageable_copy) ST_HIP(hipStreamSynchronize(copy_stream));
    if ((io.uploaded && io.pageable) || e.sync_every_tick) ST_HIP(hipStreamSynchronize(io.stream));
    return ST_OK;
}
// A reader's launches on `stream` come behind the tick's uploads, and a reader of its own (reads != 0) is one of the streams the writer has to know of; end: what it read is in use up to here on `stream`.
int SceneCopies::begin(hipStream_t stream, unsigned reads) {
    if (int rc = tick_done.wait(stream, Fence::AnyStream, Fence::Keep)) return rc;  // a no-op when st_tick ran on this stream. Kept: every stream of every frame waits, until st_tick polls it away
    if (int rc = copy_done.wait(stream, Fence::AnyStream, Fence::Keep)) return rc;  // likewise (st_tick already queued this wait on its own stream)
    if (reads) {
        if (rendered_before && last_render_stream != stream) mixed_render_streams = true;  // the null stream is a stream too
        last_render_stream = stream; rendered_before = true;
    }
    return ST_OK;
}
int SceneCopies::end(hipStream_t stream, unsigned reads) {
    if ((reads & kReadsScene) && scene.alternating) if (int rc = scene.current().fence.record(stream)) return rc;
    if ((reads & kReadsLights) && lights.alternating) if (int rc = lights.current().fence.record(stream)) return rc;
    if ((reads & kReadsEnvironment) && e.env_live) if (int rc = e.env_live->fence.record(stream)) return rc;   // (the map is freed behind its last reader)
    if (reads & kReadsPrevious) if (int rc = e.deform.previous_read_by(stream)) return rc;   // the next skin launch waits for it (st_deform.h deform_read). Chained: readers on several streams, one event
    return ST_OK;
}

}  // namespace st
