// st_stores.h — the scene stores of the host engine: lights, materials, the image atlas, meshes, triangle slots, instances (implementation:
// st_scene.cpp). Part of st_engine.h, which includes it behind the owners of HIP resources.
//
// Each store owns its containers and the policy of its reference module (lights.rs, materials.rs, images.rs, triangles.rs, instances.rs); none
// knows the engine — what a call needs of another store it gets as an argument. The tick's phases that connect them to the tree, the copies and
// the deformer (refresh_instances, bake_stale_on_host, bake_on_device, fill_instance_table) stay Engine's.
#pragma once
namespace st {

// ---- lights (lights.rs:49-172, light.rs:25-79): slot 0 is the sun
struct LightStore {
    LightStore();   // slot 0, dark until the first set_sun
    void insert(uint64_t id, const StLight& l);
    void remove(uint64_t id);   // silent no-op for an unknown id, like the reference
    void set_sun(GpuLight g) { overwrite(0, -1, g); }
    void snapshot();   // lights.rs:128-154: what the device sees this frame (table()), then commit prev_* for the next one
    uint32_t count() const { return count_; }   // lights of the last snapshot, the sun included
    const std::vector<GpuLight>& table() const { return gpu_; }   // the last snapshot
    // which slot of the snapshot's table a handle has (st_shafts.cpp)
    bool uploaded_slot(uint64_t id, uint32_t* slot) const { auto it = slot_uploaded_.find((int64_t)id); if (it == slot_uploaded_.end() || it->second >= gpu_.size()) return false; *slot = it->second; return true; }
    bool changed() const { return gpu_.size() != uploaded_.size() || memcmp(gpu_.data(), uploaded_.data(), gpu_.size() * sizeof(GpuLight)) != 0; }   // since mark_uploaded
    void mark_uploaded() { uploaded_ = gpu_; }
private:
    static void note(std::vector<int64_t>& v, int64_t k) { if (std::find(v.begin(), v.end(), k) == v.end()) v.push_back(k); }
    void overwrite(uint32_t slot, int64_t key, GpuLight g);
    std::vector<GpuLight> buffer_; std::map<int64_t, uint32_t> slot_;
    std::vector<int64_t> created_, updated_; std::map<int64_t, uint32_t> remapped_; std::vector<uint32_t> killed_;
    uint32_t next_id_ = 1, count_ = 0;
    std::vector<GpuLight> gpu_, uploaded_;
    std::map<int64_t, uint32_t> slot_uploaded_;   // slot_ as gpu_ was snapshot
};

// ---- images (images.rs): a single linear RGBA8 atlas of the reference's extent (images.rs:28-29); rectangles from st_atlas.h
struct ImageAtlas {
    static constexpr uint32_t kW = 8192, kMaxH = 8192;
    struct Rect { uint32_t x, y, w, h; };
    // ImageData::Texture (image.rs:46-59): pixels that live in device memory. Static ones are copied into the atlas once
    // (and mirrored into the host copy, which stays the source of every later re-upload); dynamic ones at every tick (images.rs:187-213).
    struct DeviceImage { const void* pixels; size_t pitch; bool dynamic, pending; };
    int insert_rgba8(uint64_t id, uint32_t w, uint32_t h, const uint8_t* rgba);
    int insert_device(uint64_t id, uint32_t w, uint32_t h, const void* pixels, size_t pitch, bool dynamic);
    void remove(uint64_t id);   // images.rs:107-113
    float4 rect_uv(uint64_t id) const;   // in atlas units; zero for handle 0, an unknown image, an empty atlas
    const Rect* rect_texels(uint64_t id) const { auto it = rects_.find(id); return it == rects_.end() ? nullptr : &it->second; }
    // what the tick sends (Engine::upload_images): the host copy when `dirty`; the device images, in handle order (std::map)
    bool dirty = false;         // the host copy changed: cleared by the tick
    bool rects_dirty = false;   // a rectangle appeared, moved or went away: materials that point at images are rebuilt (cleared there)
    uint32_t width() const { return w_; }
    uint32_t height() const { return h_; }
    const std::vector<uint8_t>& texels() const { return texels_; }
    uint8_t* texel(uint32_t x, uint32_t y) { return &texels_[((size_t)y * w_ + x) * 4]; }
    std::map<uint64_t, DeviceImage>& device() { return device_; }
private:
    int place(uint64_t id, uint32_t w, uint32_t h, Rect* out);   // Images::insert (images.rs:54-105)
    bool release(uint64_t id);
    uint32_t w_ = 0, h_ = 0; std::vector<uint8_t> texels_;
    std::unordered_map<uint64_t, Rect> rects_; AtlasShelves shelves_{kW, kMaxH};
    std::map<uint64_t, DeviceImage> device_;
};

// ---- materials (materials.rs:33-96, material.rs:29-50)
struct MaterialStore {
    void insert(uint64_t id, const StMaterial& m);
    bool has(uint64_t id) const { return slot_.count(id) != 0; }
    void remove(uint64_t id);
    bool slot_of(uint64_t id, uint32_t* slot) const { auto it = slot_.find(id); if (it == slot_.end()) return false; *slot = it->second; return true; }
    void rebuild(const ImageAtlas& images);   // gpu(), base_packed(), any_normal_map from the materials and the atlas' rectangles
    bool is_blend(uint32_t slot) const { return slot < materials_.size() && materials_[slot].alpha_mode == 1u; }
    std::vector<uint8_t> blend_flags() const { std::vector<uint8_t> b(materials_.size()); for (size_t i = 0; i < b.size(); i++) b[i] = materials_[i].alpha_mode == 1u; return b; }
    const std::vector<GpuMaterial>& gpu() const { return gpu_; }
    const std::vector<uint32_t>& base_packed() const { return base_packed_; }
    bool dirty = false;            // an insert or a remove since the last rebuild: cleared by the tick
    bool any_normal_map = false;   // some material's normal_map_texture resolved to an atlas rectangle at the last rebuild
private:
    std::vector<StMaterial> materials_; std::unordered_map<uint64_t, uint32_t> slot_; SlotRanges free_;
    std::vector<GpuMaterial> gpu_; std::vector<uint32_t> base_packed_;
};

// ---- meshes, and their object-space copies on the device. Device bake (StTuning::device_bake; k_bvh.hip k_bvh_bake): 24 floats per triangle, appended
// when an instance of the mesh is first moved on the device; a re-inserted mesh is a new version and is appended again.
struct MeshStore {
    void insert(uint64_t id, const StMeshTriangle* t, size_t count);   // a new version: an instance baked from the earlier mesh of this handle is re-baked by the host
    void remove(uint64_t id);
    const std::vector<StMeshTriangle>* find(uint64_t id) const { auto it = meshes_.find(id); return it == meshes_.end() ? nullptr : &it->second; }
    const std::vector<StMeshTriangle>& at(uint64_t id) const { return meshes_.at(id); }   // of a mesh the caller knows to exist
    uint64_t version_of(uint64_t id) const { auto it = version_.find(id); return it == version_.end() ? 0 : it->second; }   // 0: no such mesh
    // (first triangle, count) of `version` of mesh `id` in the device store, appending `tris` to the host image if it is absent (upload then sends it)
    std::pair<size_t, size_t> device_range(uint64_t id, uint64_t version, const std::vector<StMeshTriangle>& tris);
    int upload(hipStream_t up, StagingRing& ring, bool* pageable);   // what device_range appended since the last upload
    const float* device_store() const { return d_store_.as<const float>(); }
private:
    std::unordered_map<uint64_t, std::vector<StMeshTriangle>> meshes_;
    std::unordered_map<uint64_t, uint64_t> version_; uint64_t next_version_ = 1;
    struct DeviceRec { size_t first, count; uint64_t version; };
    std::unordered_map<uint64_t, DeviceRec> device_;
    std::vector<float> store_host_; DeviceArray d_store_; size_t store_uploaded_ = 0;   // floats
};

// ---- instances (instances.rs)
struct InstanceRec {
    uint64_t id, mesh, material; Affine xform, xform_inv, prev_xform; bool dirty; uint32_t xslot;
    // what the triangle slots of this instance were baked from (device bake: a later change of the transform alone can be baked on the device)
    uint64_t baked_mesh = 0, baked_mesh_version = 0; uint32_t baked_material = 0xffffffffu; bool baked = false;
    bool host_stale = false;   // moved on the device since the host's triangle-slot arrays were last baked
};
struct InstanceStore {
    std::vector<InstanceRec> records;
    bool dirty = false;     // some record is: the next refresh looks
    bool removed = false;   // since the last refresh: the set of triangle slots changed, the tree will be rebuilt
    // per-instance transforms for primary visibility's prev_point (the reference's per-draw push constants, passes/prim_raster.rs:196-230):
    // 8 float4 per stable slot — curr_xform_inv (x, y, z axes, translation), then prev_xform. tri_attr[4 t + 3].w holds the slot of the instance that owns triangle t.
    std::vector<float4> xforms;
    InstanceRec* find(uint64_t id) { for (auto& r : records) if (r.id == id) return &r; return nullptr; }
    void insert(uint64_t id, uint64_t mesh, uint64_t material, const Affine& x);   // a known id keeps its transform slot and remembers its previous transform
    void remove(uint64_t id);
    void mark_dirty(InstanceRec* r) { if (r) { r->dirty = true; dirty = true; } }
    void mark_dirty(uint64_t id) { mark_dirty(find(id)); }
    void fill_xforms();
    bool any_host_stale() const { for (const auto& i : records) if (i.host_stale) return true; return false; }
private:
    std::vector<uint32_t> xslot_free_;
};

// ---- world-space triangles in stable slots (triangles.rs; baking: instances.rs:100-139, mesh_triangle.rs:47-86, triangle.rs:16-37): six parallel
// arrays over the slots, the ranges given back, which range an instance holds, and how many slots are live.
struct TriangleSlots {
    const std::vector<HostTriangle>& triangles() const { return triangles_; }
    const std::vector<BuildPrim>& prims() const { return prims_; }
    const std::vector<uint8_t>& alive() const { return alive_; }
    const std::vector<float4>& geo() const { return geo_; }         // 3 per slot: the hit-test record
    const std::vector<float4>& attr() const { return attr_; }       // 4 per slot
    const std::vector<float4>& bounds() const { return bounds_; }   // 2 per slot: (lo, hi) (device refit)
    size_t size() const { return triangles_.size(); }
    size_t capacity() const { return triangles_.capacity(); }
    size_t live() const { return live_; }   // how many of alive() are set (kept by take / drop: device_build_possible asks every tick)
    bool range_of(uint64_t instance, size_t* b, size_t* e) const { auto it = ranges_.find(instance); if (it == ranges_.end()) return false; *b = it->second.first; *e = it->second.second; return true; }
    void reserve(size_t want);   // room for `want` slots in all six arrays
    // the range of `instance`: the one it holds, else `count` slots a drop gave back, else new ones at the end (*appended: the arrays grew)
    void take(uint64_t instance, size_t count, size_t* b, size_t* e, bool* appended);
    bool drop(uint64_t instance, size_t* b, size_t* e);   // gives its range back ([*b, *e): no longer alive); false: it held none
    // The tree lists liveness for the device builder slot by slot and counts as it goes; where it has just listed every slot it hands that count
    // back, so that take / drop's running figure cannot drift from the array the builder is given.
    void set_live(size_t n) { live_ = n; }
    // bakes `t` into `slot`, alive from now on. The device bake repeats these operations in this order (k_bvh.hip k_bvh_bake, which knows this routine by its earlier name, Engine::bake)
    void write(size_t slot, const StMeshTriangle& t, const InstanceRec& inst, uint32_t material);
private:
    void grow_to(size_t end);
    std::vector<HostTriangle> triangles_; std::vector<BuildPrim> prims_; std::vector<uint8_t> alive_;
    std::vector<float4> geo_, attr_, bounds_;
    std::map<uint64_t, std::pair<size_t, size_t>> ranges_; SlotRanges free_;
    size_t live_ = 0;
};

}  // namespace st
