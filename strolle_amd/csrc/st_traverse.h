// st_traverse.h — BVH traversal of the MI355X hot path: the walks over the four device streams (contract, compact, wide, the wide stream's wave
// packet), the triangle and box tests, attribute resolution of the winning triangle, and the choice of stream per ray. Included by st_device.h, in
// the middle of namespace st, after the ray / atlas helpers it uses; never on its own.
#pragma once

// ------------------------------------------------------------------ BVH traversal (ray.rs:114-302, triangle.rs:64-113)
struct TriangleHit { float distance; V3 point, normal; V2 uv; uint32_t material_id; uint32_t xform_slot; };  // xform_slot: owning instance (trace_closest only)
ST_D bool hit_is_some(const TriangleHit& h) { return h.distance < kF32Max; }

// ================================================================== exact island (3/3): traversal
#pragma clang fp contract(off)
ST_D float intersect_box(const Ray& r, V3 bmin, V3 bmax) {
    float tmin = 0.0f, tmax = kF32Max;
    const V3 t1 = xe::mul(xe::sub(bmin, r.origin), r.inv_dir);
    const V3 t2 = xe::mul(xe::sub(bmax, r.origin), r.inv_dir);
    tmin = fmax_(tmin, fmin_(t1.x, t2.x)); tmax = fmin_(tmax, fmax_(t1.x, t2.x));
    tmin = fmax_(tmin, fmin_(t1.y, t2.y)); tmax = fmin_(tmax, fmax_(t1.y, t2.y));
    tmin = fmax_(tmin, fmin_(t1.z, t2.z)); tmax = fmin_(tmax, fmax_(t1.z, t2.z));
    return tmin <= tmax ? tmin : kF32Max;
}
ST_D float intersect_sphere(const Ray& r, float radius) {  // ray.rs:304-321
    const float b = dot(r.origin, r.dir);
    const float c = dot(r.origin, r.origin) - radius * radius;
    if (c > 0.0f && b > 0.0f) return -1.0f;
    const float discr = b * b - c;
    if (discr < 0.0f) return -1.0f;
    if (discr > b * b) return -b + fsqrt(discr);
    return -b - fsqrt(discr);
}

struct Candidate { float t, u, v, inv_det; uint32_t tri, material; };
// the empty candidate every closest-hit walk starts from: nothing closer than max_t found yet
ST_D void candidate_reset(Candidate* c, float max_t) { c->t = max_t; c->tri = 0xffffffffu; c->material = 0u; c->u = 0.0f; c->v = 0.0f; c->inv_det = 1.0f; }
// Entry of the device BVH stream at BYTE offset `at` (traversal pointers are byte offsets: 64 per entry): base + a 32-bit
// offset, which the global-memory form turns into `global_load v, v_offset, s[base]` with immediate offsets for the four
// texels — no per-texel 64-bit address arithmetic (three VALU instructions per texel when indexed as bvh[ptr + k]).
ST_D const float4* bvh_entry(const float4* bvh, uint32_t at) { return reinterpret_cast<const float4*>(reinterpret_cast<const char*>(bvh) + at); }

ST_D V2 tri_uv(const KArgs& a, uint32_t tri, float u, float v) {
    const float4 q0 = a.tri_attr[4u * tri], q1 = a.tri_attr[4u * tri + 1u], q2 = a.tri_attr[4u * tri + 2u], q3 = a.tri_attr[4u * tri + 3u];
    const V2 uv0 = v2(q0.w, q1.w), uv1 = v2(q2.w, q3.x), uv2 = v2(q3.y, q3.z);
    return v2((uv0.x + (uv1.x - uv0.x) * u) + (uv2.x - uv0.x) * v, (uv0.y + (uv1.y - uv0.y) * u) + (uv2.y - uv0.y) * v);
}
// AlphaMode::Blend (Triangle::hit, ray.rs:184-214): a hit at (u, v) of triangle slot `tri` counts only where the base colour is opaque. The texel fetch
// belongs to the contract, so every walk — island or fast — asks here.
ST_D bool alpha_opaque(const KArgs& a, uint32_t tri, uint32_t material, float u, float v) {
    const GpuMaterial m = a.materials[material];
    const float4 bc = sample_atlas(a, tri_uv(a, tri, u, v), m.base_color, m.base_color_texture);
    return !(bc.w < 1.0f);
}
// ANY_HIT: Tracing::ReturnFirst. Returns the reference's `used_memory` byte counter.
// On return `best.t` is the closest accepted distance (or the initial max_t if none).
// (Measured and dropped, round 3: ONE body per step chosen by a vote of the wave — lanes whose fetched entry is of the other kind keep it
// and wait, so that each body runs with more of its lanes: majority vote, triangles-only-when-no-node-is-pending ("while-while")
// and a 16-lane threshold all lost, dungeon 1080p 1.46 -> 1.57 / 1.60 / 1.58 ms per frame, GI sampling a 203 -> 235 / 303 / 268 us.
// The loop below already skips a body no lane wants (s_cbranch_execz); making lanes wait costs more steps than the fuller bodies save.)
template <bool ANY_HIT, class SE>
ST_D uint32_t traverse(const KArgs& a, const Ray& ray, float max_t, SE* stack, Candidate* best, bool* found_any) {
    candidate_reset(best, max_t);
    *found_any = false;
    if (a.bvh_len == 0u) return 0u;
    uint32_t used_memory = 0u;
    uint32_t ptr = 0u;
    int sp = 0;
    for (;;) {
        used_memory += 16u;
        // Every entry of the device stream is four texels (st_types.h "device BVH stream"): an internal node's two child
        // boxes, or a leaf entry with its triangle's hit-test record inline — one round trip per step for either kind
        // (dependent fetches are the traversal's latency chain). The empty asm keeps the four loads together: the compiler
        // otherwise sinks d1..d3 behind the d0.w test, which puts a second, dependent round trip into every step (measured
        // on the dungeon: 1.99 -> 1.87 ms/frame for the internal nodes alone).
        const float4* entry = bvh_entry(a.bvh, ptr);
        const float4 d0 = entry[0], d1 = entry[1], d2 = entry[2], d3 = entry[3];
        asm volatile("" :: "v"(d1.x), "v"(d2.x), "v"(d3.x));
        if (f2b(d0.w) == 0u) {
            used_memory += 48u;
            uint32_t near_ptr = ptr + 64u, far_ptr = f2b(d1.w);
            float near_d = intersect_box(ray, xyz(d0), xyz(d1));
            float far_d = intersect_box(ray, xyz(d2), xyz(d3));
            if (far_d < near_d) { const uint32_t tp = near_ptr; near_ptr = far_ptr; far_ptr = tp; const float td = near_d; near_d = far_d; far_d = td; }
            if (far_d < best->t) { if (sp < (int)a.stack_entries) { stack[sp * 64] = (SE)(far_ptr >> 6); sp++; } }
            if (near_d < best->t) { ptr = near_ptr; continue; }
        } else {
            used_memory += 144u;
            const uint32_t flags = f2b(d0.x), tri = f2b(d0.y), material = f2b(d0.z);
            const V3 p0 = xyz(d1), e1 = xyz(d2), e2 = xyz(d3);
            const V3 pvec = xe::cross(ray.dir, e2);
            const float det = xe::dot(e1, pvec);
            bool found = false;
            if (!(fabsf(det) < kF32Eps)) {
                const float inv_det = 1.0f / det;
                const V3 tvec = xe::sub(ray.origin, p0);
                const float u = xe::dot(tvec, pvec) * inv_det;
                const V3 qvec = xe::cross(tvec, e1);
                const float v = xe::dot(ray.dir, qvec) * inv_det;
                const float t = xe::dot(e2, qvec) * inv_det;
                if (!((u < 0.0f) | (u > 1.0f) | (v < 0.0f) | (u + v > 1.0f) | (t <= 0.0f) | (t >= best->t))) {
                    found = true;
                    if (flags & 2u) {  // AlphaMode::Blend: the hit only counts where the base colour is opaque
                        used_memory += 112u + 16u;
                        if (!alpha_opaque(a, tri, material, u, v)) found = false;
                    }
                    if (found) { best->t = t; best->u = u; best->v = v; best->inv_det = inv_det; best->tri = tri; best->material = material; *found_any = true; }
                }
            }
            if (found && ANY_HIT) break;
            if (flags & 1u) { ptr += 64u; continue; }
        }
        if (sp > 0) { sp--; ptr = (uint32_t)stack[sp * 64] << 6; } else break;
    }
    return used_memory;
}
// Which stream a closest-hit ray walks, decided HERE for every caller. Fast build: the wave's packet over the wide stream where `packets` says so, else the wide
// stream per lane, else the compact stream, else the contract stream (conservative boxes visit a superset of the contract walk's entries, the triangle records are
// the same f32). Exact build: the contract walk. `any`: something was hit; `used`: the contract walk's `used_memory` bytes, 0 for the others. Stack slots: the caller's `SE`.
//   EXACT_LEAF  the wide stream's leaf records are tested in the island's arithmetic (closest_hit_wide says what for); the packet always does.
//   ABLATABLE   -DST_NO_ANYHIT_FAST (the ablation build whose shadow rays walk the contract loop) takes the fast streams away from this caller too.
//   packets     the caller's whole condition, `bvh_w != nullptr` included (the order of its terms is code); never for a scene in LDS or for incoherent rays.
// (A statement macro: a function around traverse() is optimised on its own before it is inlined, and every exact-build caller then differs by an instruction.)
#if defined(ST_NO_ANYHIT_FAST)
constexpr bool kNoAnyhitFast = true;
#else
constexpr bool kNoAnyhitFast = false;
#endif
#if ST_FAST_DEVICE
#define ST_CLOSEST_WALK(EXACT_LEAF, ABLATABLE, a, ray, stack, packets, best, any, used)                                                          \
    do {                                                                                                                                         \
        constexpr bool streams_ = !((ABLATABLE) && kNoAnyhitFast);                                                                               \
        if (streams_ && (packets)) { used = 0u;                         any = closest_hit_packet(a, ray, best); }                                \
        else if (streams_ && (a).bvh_w != nullptr) { used = 0u; any = closest_hit_wide<SE, EXACT_LEAF>(a, ray, stack, best); }                   \
        else if (streams_ && (a).bvh_c != nullptr) { used = 0u; any = closest_hit_compact(a, ray, stack, best); }                                \
        else used = traverse<false>(a, ray, kF32Max, stack, best, &any);                                                                         \
    } while (0)
#else
#define ST_CLOSEST_WALK(EXACT_LEAF, ABLATABLE, a, ray, stack, packets, best, any, used) used = traverse<false>(a, ray, kF32Max, stack, best, &any)
#endif
// Ray::trace (closest hit) with attributes resolved once, for the winning triangle.
template <class SE> ST_D bool closest_hit_compact(const KArgs& a, const Ray& ray, SE* stack, Candidate* best);
template <class SE, bool EXACT_LEAF> ST_D bool closest_hit_wide(const KArgs& a, const Ray& ray, SE* stack, Candidate* best);
ST_D bool closest_hit_packet(const KArgs& a, const Ray& ray, Candidate* best);
ST_D TriangleHit closest_resolve(const KArgs& a, const Ray& ray, const Candidate& c, bool any);
// `won`: the winning candidate (triangle slot, Triangle::hit's barycentrics) — what closest_resolve read, for callers that need it afterwards
template <class SE>
ST_D TriangleHit trace_closest(const KArgs& a, const Ray& ray, SE* stack, uint32_t* used_memory, Candidate* won) {
    Candidate& c = *won; bool any;
    // secondary rays: the fast leaf test, never a packet (a wave's rays are incoherent), the contract walk in the ablation build
    ST_CLOSEST_WALK(false, true, a, ray, stack, false, &c, any, *used_memory);
    return closest_resolve(a, ray, c, any);
}
template <class SE>
ST_D TriangleHit trace_closest(const KArgs& a, const Ray& ray, SE* stack, uint32_t* used_memory) {
    Candidate c;
    return trace_closest(a, ray, stack, used_memory, &c);
}
struct TriAttr { V3 n0, n1, n2; V2 uv0, uv1, uv2; uint32_t xform_slot; };   // the winning triangle's attribute record (four texels): corner normals, uv corners, the owning instance's slot
ST_D TriAttr tri_attr_fetch(const KArgs& a, uint32_t tri) {
    const float4 q0 = a.tri_attr[4u * tri], q1 = a.tri_attr[4u * tri + 1u], q2 = a.tri_attr[4u * tri + 2u], q3 = a.tri_attr[4u * tri + 3u];
    TriAttr t;
    t.n0 = xyz(q0); t.n1 = xyz(q1); t.n2 = xyz(q2);
    t.uv0 = v2(q0.w, q1.w); t.uv1 = v2(q2.w, q3.x); t.uv2 = v2(q3.y, q3.z);
    t.xform_slot = f2b(q3.w);
    return t;
}
// the winning triangle's attributes (normal, uv, instance slot), fetched once
ST_D TriangleHit closest_resolve(const KArgs& a, const Ray& ray, const Candidate& c, bool any) {
    TriangleHit h;
    h.distance = c.t; h.material_id = c.material; h.point = v3s(0.0f); h.normal = v3s(0.0f); h.uv = v2(0.0f, 0.0f); h.xform_slot = 0u;
    if (any) {
        const TriAttr t = tri_attr_fetch(a, c.tri);
        V3 n = c.u * t.n1 + c.v * t.n2 + (1.0f - c.u - c.v) * t.n0;
        h.normal = normalize(n) * copysignf(1.0f, c.inv_det);
        h.uv = t.uv0 + (t.uv1 - t.uv0) * c.u + (t.uv2 - t.uv0) * c.v;
        h.xform_slot = t.xform_slot;
    }
    if (hit_is_some(h)) h.point = ray_at(ray, h.distance);
    return h;
}
// glam Affine3A::transform_point3 with the transform stored as 4 float4 (x, y, z axes, translation)
ST_D V3 affine_point(const float4* m, V3 p) { return ((xyz(m[0]) * p.x) + (xyz(m[1]) * p.y) + (xyz(m[2]) * p.z)) + xyz(m[3]); }
// Deformation motion (include/strolle_hip.h "skinned meshes"): where a primary hit on a skinned instance was before the last tick re-skinned it.
// `slot` is the hit's instance slot, `tri` its triangle slot, (u, v) Triangle::hit's barycentrics (Candidate::u, v; StRayHit::barycentric). Returns
// false — and leaves *prev_point alone — for every instance without a previous pose: the caller then keeps prim_raster.rs:21-27's rigid formula.
// `table` is the scene copy's instance table, `posed` the posed store; called only where the launch got them (deformation motion on). Loads: one table word per hit; for a deforming hit one more word and three positions (36 B).
// The float32 operations and their order, the same in both arithmetic builds (this island: no contraction; tests/deform_ref.py restates them):
//   k  = tri - first triangle slot of the instance            (the triangle's index in its mesh)
//   w  = (1 - u) - v
//   o  = ((q0 * w) + (q1 * u)) + (q2 * v)     per component   (q0..q2: triangle k's positions in the instance's PREVIOUS region of the posed store)
//   prev_point = ((x * o.x + y * o.y) + z * o.z) + t          (x, y, z, t: the instance's prev_xform; affine_point)
ST_D bool deform_prev_point(const KArgs& a, const uint4* table, const float* posed, uint32_t slot, uint32_t tri, float u, float v, V3* prev_point) {
    const uint32_t* rec = reinterpret_cast<const uint32_t*>(table + slot);
    const uint32_t prev = rec[3];
    if (prev == 0u) return false;
    const float* q = posed + 24u * (size_t)((prev - 1u) + (tri - rec[2]));
    const V3 q0 = v3(q[0], q[1], q[2]), q1 = v3(q[3], q[4], q[5]), q2 = v3(q[6], q[7], q[8]);
    const float w = (1.0f - u) - v;
    const V3 o = xe::add(xe::add(xe::scale(q0, w), xe::scale(q1, u)), xe::scale(q2, v));
    *prev_point = affine_point(a.instance_xforms + 8u * slot + 4, o);
    return true;
}
// Triangle::hit's accept / reject and (t, u, v, 1 / det) for a hit-test record (p0, e1, e2), in the island's arithmetic: what traverse() computes for a leaf
// entry, for walks over OTHER streams that owe the contract walk's bits (primary rays over the wide stream: closest_hit_wide<SE, true>, closest_hit_packet)
ST_D bool triangle_hit_exact(const Ray& ray, V3 p0, V3 e1, V3 e2, float limit, float* t_out, float* u_out, float* v_out, float* inv_det_out) {
    const V3 pvec = xe::cross(ray.dir, e2);
    const float det = xe::dot(e1, pvec);
    if (fabsf(det) < kF32Eps) return false;
    const float inv_det = 1.0f / det;
    const V3 tvec = xe::sub(ray.origin, p0);
    const float u = xe::dot(tvec, pvec) * inv_det;
    const V3 qvec = xe::cross(tvec, e1);
    const float v = xe::dot(ray.dir, qvec) * inv_det;
    const float t = xe::dot(e2, qvec) * inv_det;
    *t_out = t; *u_out = u; *v_out = v; *inv_det_out = inv_det;
    return !((u < 0.0f) | (u > 1.0f) | (v < 0.0f) | (u + v > 1.0f) | (t <= 0.0f) | (t >= limit));
}
// closest_resolve() and normal_encode() in the island's arithmetic, for PRIMARY hits (k_trace.hip k_prim_visibility; round 6). glam's
// Vec3::any_orthonormal_pair — behind every hemisphere sample (noise/white.rs:73-81) — branches on the SIGN of normal.z, and a wall whose normal lies in
// the xy-plane decodes to z = +-(an ulp): the fast build's last-bit differences in the G-buffer's encoded normal flipped that sign on 0.2 % of the
// dungeon's pixels, each flip a completely different bounce direction — the largest single consumer of the fast build's tolerance gates
// (profiles/r06_gate_headroom.json). With the primary hit's (u, v) from triangle_hit_exact and these two, the encoded normal is the CPU restatement's bit for bit
// wherever the same triangle wins.
ST_D TriangleHit closest_resolve_exact(const KArgs& a, const Ray& ray, const Candidate& c, bool any) {
    TriangleHit h;
    h.distance = c.t; h.material_id = c.material; h.point = v3s(0.0f); h.normal = v3s(0.0f); h.uv = v2(0.0f, 0.0f); h.xform_slot = 0u;
    if (any) {
        const TriAttr t = tri_attr_fetch(a, c.tri);
        const V3 n = xe::add(xe::add(xe::scale(t.n1, c.u), xe::scale(t.n2, c.v)), xe::scale(t.n0, (1.0f - c.u) - c.v));
        h.normal = xe::scale(xe::normalize(n), copysignf(1.0f, c.inv_det));
        h.uv = v2((t.uv0.x + (t.uv1.x - t.uv0.x) * c.u) + (t.uv2.x - t.uv0.x) * c.v, (t.uv0.y + (t.uv1.y - t.uv0.y) * c.u) + (t.uv2.y - t.uv0.y) * c.v);
        h.xform_slot = t.xform_slot;
    }
    if (hit_is_some(h)) h.point = xe::add(ray.origin, xe::scale(ray.dir, h.distance));
    return h;
}
ST_D V2 normal_encode_exact(V3 n) {  // normal.rs:9-24
    const float s = (fabsf(n.x) + fabsf(n.y)) + fabsf(n.z);
    n = v3(n.x / s, n.y / s, n.z / s);
    V2 r;
    if (n.z >= 0.0f) r = v2(n.x, n.y);
    else r = v2(copysignf(1.0f - fabsf(n.y), n.x), copysignf(1.0f - fabsf(n.x), n.y));
    return v2(r.x * 0.5f + 0.5f, r.y * 0.5f + 0.5f);
}
// Normal mapping (include/strolle_hip.h "normal mapping" has the definition): the resolved normal `n` of the hit on triangle slot `tri`, bent by the
// material's map. `inv_det` is Triangle::hit's (Candidate::inv_det): its sign is the flip closest_resolve applied to face the ray. `geo` is the live scene
// copy's hit-test records (SceneSet::tri_geo: p0, e1, e2 per slot; Engine::normal_map_geo), an argument of the launch and null while the feature is not
// active: callers test it first. Returns `n` itself, bit for bit, for a material without a map and wherever the frame is degenerate. Loads: the material's
// rectangle; for a mapped material two hit-test texels, the four attribute texels again (L1-hot: closest_resolve just read them) and four atlas taps.
// The float32 operations and their order, the same in both arithmetic builds (this island: no contraction; tests/normal_map_ref.py map_f32 restates them):
//   s = copysign(1, inv_det)      nf = n * s                                             per component
//   du1 = uv1.x - uv0.x   dv1 = uv1.y - uv0.y   du2 = uv2.x - uv0.x   dv2 = uv2.y - uv0.y
//   d  = du1 * dv2 - du2 * dv1                                                           unchanged unless kNormalMapTiny <= |d| <= FLT_MAX
//   Pu = (e1 * dv2 - e2 * dv1) / d        Pv = (e2 * du1 - e1 * du2) / d                 per component
//   g  = (nf.x * Pu.x + nf.y * Pu.y) + nf.z * Pu.z          q = Pu - nf * g
//   l2 = (q.x * q.x + q.y * q.y) + q.z * q.z     l = sqrt(l2)                            unchanged unless kNormalMapShort <= l <= kNormalMapLong
//   T  = q * (1 / l)              C = cross(nf, T)   (a.y * b.z - b.y * a.z, ...)
//   h  = ((C.x * Pv.x + C.y * Pv.y) + C.z * Pv.z) <= 0 ? 1 : -1        B = C * h
//   m  = sample_normal_map(uv)    t = (2 * m.x - 1, 2 * m.y - 1, max(2 * m.z - 1, 0))
//   w  = (T * t.x + B * t.y) + nf * t.z                                                  per component
//   k  = sqrt((w.x * w.x + w.y * w.y) + w.z * w.z)                                       unchanged unless kNormalMapShort <= k <= kNormalMapLong
//   n' = (w * (1 / k)) * s
// (the tests are written so that zero, NaN and infinities fail them; a length's bounds keep its SQUARE a normal float32, which a bound at float32's own range would not)
constexpr float kNormalMapTiny = 1e-30f, kNormalMapShort = 1e-18f, kNormalMapLong = 1e18f;
ST_D bool normal_map_det_usable(float d) { return fabsf(d) >= kNormalMapTiny && fabsf(d) <= kF32Max; }
ST_D bool normal_map_length_usable(float l) { return l >= kNormalMapShort && l <= kNormalMapLong; }
ST_D V3 normal_map_apply(const KArgs& a, const float4* geo, uint32_t tri, uint32_t material, float inv_det, V2 uv, V3 n) {
    const float4 rect = a.materials[material].normal_map_texture;
    if (is_zero(rect) || tri >= a.tri_slots) return n;
    const V3 e1 = xyz(geo[3u * tri + 1u]), e2 = xyz(geo[3u * tri + 2u]);
    const TriAttr t = tri_attr_fetch(a, tri);
    const float s = copysignf(1.0f, inv_det);
    const V3 nf = xe::scale(n, s);
    const float du1 = t.uv1.x - t.uv0.x, dv1 = t.uv1.y - t.uv0.y, du2 = t.uv2.x - t.uv0.x, dv2 = t.uv2.y - t.uv0.y;
    const float d = du1 * dv2 - du2 * dv1;
    if (!normal_map_det_usable(d)) return n;
    const V3 pu = v3((e1.x * dv2 - e2.x * dv1) / d, (e1.y * dv2 - e2.y * dv1) / d, (e1.z * dv2 - e2.z * dv1) / d);
    const V3 pv = v3((e2.x * du1 - e1.x * du2) / d, (e2.y * du1 - e1.y * du2) / d, (e2.z * du1 - e1.z * du2) / d);
    const V3 q = xe::sub(pu, xe::scale(nf, xe::dot(nf, pu)));
    const float l = sqrtf(xe::dot(q, q));
    if (!normal_map_length_usable(l)) return n;
    const V3 tangent = xe::scale(q, 1.0f / l);
    const V3 c = xe::cross(nf, tangent);
    const V3 bitangent = xe::scale(c, xe::dot(c, pv) <= 0.0f ? 1.0f : -1.0f);
    const V3 m = sample_normal_map(a, uv, rect);
    const float tx = 2.0f * m.x - 1.0f, ty = 2.0f * m.y - 1.0f, tz = fmax_(2.0f * m.z - 1.0f, 0.0f);
    const V3 w = xe::add(xe::add(xe::scale(tangent, tx), xe::scale(bitangent, ty)), xe::scale(nf, tz));
    const float k = sqrtf(xe::dot(w, w));
    if (!normal_map_length_usable(k)) return n;
    return xe::scale(xe::scale(w, 1.0f / k), s);
}
// Ray::intersect (shadow ray) as the contract states it: the reference's visiting order, arithmetic and `used_memory` count
template <class SE>
ST_D bool trace_any_contract(const KArgs& a, const Ray& ray, SE* stack, uint32_t* used_memory) {
    Candidate c; bool any;
    *used_memory = traverse<true>(a, ray, ray.len, stack, &c, &any);
    return c.t < ray.len;
}
#if defined(ST_FAST_MATH)
#pragma clang fp contract(fast)
#endif
// ================================================================== end of exact island (3/3)

// ------------------------------------------------------------------ any-hit rays of the fast build
// `Ray::intersect` (strolle-gpu/src/ray.rs:84-112) hands back ONE boolean — "some triangle is hit closer than ray.len" — and
// nothing else of the traversal (its `used_memory` is observable only through st_profile_enable(ST_PROFILE_TRAVERSAL_BYTES),
// which switches back to the contract loop above). The fast build therefore walks shadow rays with ordinary fast arithmetic:
//   * the slab test is two FMAs per plane pair against a precomputed -origin * inv_dir (the exact island's (b - o) * inv is a
//     subtraction and a multiplication: 12 VALU instructions fewer per internal node). In position space the difference is
//     half an ulp of the ray ORIGIN's coordinate, however near the plane is: harmless at unit scale, a whole unit of t for a ray grazing a
//     zero-thickness box a thousand units out. any_slab widens each axis' interval by that bound (any_slab_origins), the f16 streams' boxes are
//     never zero-thick (st_half_box.h); tests/test_gpu_geometry_extremes.py holds every walk to brute force from 0.05-unit scenes to
//     coordinates of 1e5. Direction components are floored at 1e-20 in magnitude (slab_safe_dir says why);
//   * Möller–Trumbore is contracted into FMAs and divides by v_rcp_f32 (the island's IEEE division alone is 13 instructions);
//   * near-child-first order is KEPT: tools/packet_sim.py prices "left child first, no near/far sort" at +27 % loop bodies on
//     the dungeon's DI shadow rays (occluded rays find their occluder later) against the ~15 % of an internal step the sort costs;
//     a wave-wide packet walk of the same rays (one node per step for all lanes, scalar fetch) visits 1.8x (DI) to 3x (GI) MORE
//     entries than the per-lane loop executes bodies — rays of one 8x8 tile go to 4-5 different lights — and is not built.
//   * a WORLD-SPACE LAST-OCCLUDER TABLE (key = hash of the ray's origin cell and end-point cell; the leaf entry that ended an earlier
//     ray between the same two cells is tested first) was built on top of this loop and measured NEUTRAL — dungeon 1.4244 vs 1.4212
//     ms/frame without it, DI resolving 138.4 vs 141.6 us, DI spatial 117.6 vs 115.3: packet_sim.py's 0.74 hit rate per ray holds,
//     but a wave only ends when its last lane does, and the waves that end early were not the ones the frame waits for. It is in
//     tools/experiments/occluder_table.inc.
// The boolean can differ from the contract loop's only where a ray grazes a box or a triangle edge within an ulp; the fast
// build's launch-by-launch tolerance tests (tests/test_gpu_fast_*.py) bound how often. The exact build never comes here.
#if ST_FAST_DEVICE
#if defined(ST_ABL_MT_DIV)
#define ST_MT_RCP(det) (1.0f / (det))                  // (ablation build: Moeller-Trumbore divides by an IEEE reciprocal)
#else
#define ST_MT_RCP(det) __builtin_amdgcn_rcpf(det)
#endif
// A direction component of (nearly) zero would make that axis' planes inf - inf = NaN wherever the origin and the plane have the same sign;
// v_min / v_max return the other operand for a NaN, so the axis would either collapse to one plane (a box the ray runs inside gets rejected)
// or constrain nothing (max3 / min3 below: measured — a handful of axis-parallel GI rays per frame walked every box along their other axes
// and turned a 0.3 ms launch into 3 ms). A floor of 1e-20 keeps the products finite: the planes become (bound - origin) * 1e20, which
// rejects a slab the ray runs beside and leaves one it runs inside unconstrained, as it should be.
ST_D float slab_safe_dir(float d) { return fabsf(d) < 1e-20f ? copysignf(1e-20f, d) : d; }
// The planes' error is the rounding of origin * inv — half an ulp of the ORIGIN's coordinate in position space, whatever the distance to the plane — and
// the contract stream's f32 boxes can have zero thickness (a floor at y = 1000.3: both y planes are the same number). A grazing ray that starts near such
// a floor computed both planes up to a unit of t off and outside the x and z intervals, and the floor was skipped: light leaked through it (tests/
// test_gpu_geometry_extremes.py, flat_1000 at 40 triangles). So each axis' interval is widened by that error's bound, 2^-23 |origin * inv|: `oa` goes with
// the lower bounds and `ob` with the upper ones, each -origin * inv moved by the bound towards the outside of the interval for this ray's direction sign.
// Two more ray constants per axis and no instruction per box. A widened interval can only enter a box more.
ST_D void any_slab_origins(V3 inv, V3 origin, V3* oa, V3* ob) {
    const float ox = -origin.x * inv.x, oy = -origin.y * inv.y, oz = -origin.z * inv.z;
    const float ex = copysignf(fabsf(ox) * kF32Eps, inv.x), ey = copysignf(fabsf(oy) * kF32Eps, inv.y), ez = copysignf(fabsf(oz) * kF32Eps, inv.z);   // kF32Eps = 2^-23
    *oa = v3(ox - ex, oy - ey, oz - ez);
    *ob = v3(ox + ex, oy + ey, oz + ez);
}
ST_D float any_slab(V3 lo, V3 hi, V3 inv, V3 oa, V3 ob) {
    const float ax = fmaf(lo.x, inv.x, oa.x), bx = fmaf(hi.x, inv.x, ob.x);
    const float ay = fmaf(lo.y, inv.y, oa.y), by = fmaf(hi.y, inv.y, ob.y);
    const float az = fmaf(lo.z, inv.z, oa.z), bz = fmaf(hi.z, inv.z, ob.z);
    const float tmin = fmax_(fmax_(fmax_(0.0f, fmin_(ax, bx)), fmin_(ay, by)), fmin_(az, bz));
    const float tmax = fmin_(fmin_(fmin_(kF32Max, fmax_(ax, bx)), fmax_(ay, by)), fmax_(az, bz));
    return tmin <= tmax ? tmin : kF32Max;
}
// Triangle::hit's accept / reject for a ray that only asks "closer than limit?" (alpha test excluded)
ST_D bool any_triangle(const Ray& ray, V3 p0, V3 e1, V3 e2, float limit, float* u_out, float* v_out) {
    const V3 pvec = cross(ray.dir, e2);
    const float det = dot(e1, pvec);
    if (fabsf(det) < kF32Eps) return false;
    const float inv_det = ST_MT_RCP(det);
    const V3 tvec = ray.origin - p0;
    const float u = dot(tvec, pvec) * inv_det;
    const V3 qvec = cross(tvec, e1);
    const float v = dot(ray.dir, qvec) * inv_det;
    const float t = dot(e2, qvec) * inv_det;
    *u_out = u; *v_out = v;
    return !((u < 0.0f) | (u > 1.0f) | (v < 0.0f) | (u + v > 1.0f) | (t <= 0.0f) | (t >= limit));
}
template <class SE>
ST_D bool any_hit_fast(const KArgs& a, const Ray& ray, SE* stack) {
    if (a.bvh_len == 0u) return false;
    const float limit = ray.len;
    const V3 inv = v3(__builtin_amdgcn_rcpf(slab_safe_dir(ray.dir.x)), __builtin_amdgcn_rcpf(slab_safe_dir(ray.dir.y)), __builtin_amdgcn_rcpf(slab_safe_dir(ray.dir.z)));
    V3 oa, ob;
    any_slab_origins(inv, ray.origin, &oa, &ob);
    // (Loop shape: ONE loop with `continue`s and a single exit, as traverse() has it. A first version returned from inside the loop;
    // the structurizer turned its exits into an inner and an outer loop, lanes waited for each other at the inner one's end, and the
    // dungeon frame went 1.520 -> 1.604 ms although every body had become cheaper.)
    uint32_t ptr = 0u;
    int sp = 0;
    bool hit = false;
    for (;;) {
        const float4* entry = bvh_entry(a.bvh, ptr);
        const float4 d0 = entry[0], d1 = entry[1], d2 = entry[2], d3 = entry[3];
        asm volatile("" :: "v"(d1.x), "v"(d2.x), "v"(d3.x));   // one round trip for the four texels (see traverse())
        if (f2b(d0.w) == 0u) {
            uint32_t near_ptr = ptr + 64u, far_ptr = f2b(d1.w);
            float near_d = any_slab(xyz(d0), xyz(d1), inv, oa, ob);
            float far_d = any_slab(xyz(d2), xyz(d3), inv, oa, ob);
            if (far_d < near_d) { const uint32_t tp = near_ptr; near_ptr = far_ptr; far_ptr = tp; const float td = near_d; near_d = far_d; far_d = td; }
            if (far_d < limit) { if (sp < (int)a.stack_entries) { stack[sp * 64] = (SE)(far_ptr >> 6); sp++; } }
            if (near_d < limit) { ptr = near_ptr; continue; }
        } else {
            const uint32_t flags = f2b(d0.x);
            float u, v;
            bool found = any_triangle(ray, xyz(d1), xyz(d2), xyz(d3), limit, &u, &v);
            if (found && (flags & 2u)) {  // AlphaMode::Blend: the texel decides (exact-island fetch, as in traverse())
                const uint32_t tri = f2b(d0.y), material = f2b(d0.z);
                if (!alpha_opaque(a, tri, material, u, v)) found = false;
            }
            if (found) { hit = true; break; }
            if (flags & 1u) { ptr += 64u; continue; }
        }
        if (sp > 0) { sp--; ptr = (uint32_t)stack[sp * 64] << 6; } else break;
    }
    return hit;
}
// The same walk over the COMPACT stream (k_bvh.hip k_bvh_compact: 48-B entries, conservative f16 child boxes; KArgs::bvh_c): two texels
// per internal step, three per leaf step instead of four. The slab test reads the f16 planes straight into v_fma_mix_f32
// (f16 x f32 + f32): the narrower boxes cost no conversion. A child's kind travels with its pointer: `cur` and the stack entries are
// (entry << 1 | is a leaf entry).
ST_D float half_lo(uint32_t w) { return (float)__builtin_bit_cast(_Float16, (uint16_t)(w & 0xffffu)); }
ST_D float half_hi(uint32_t w) { return (float)__builtin_bit_cast(_Float16, (uint16_t)(w >> 16)); }
// One child box of a compact internal entry: a word per axis, (lower bound | upper bound << 16). The ray's direction sign per axis says
// which of the two is the entry plane, so the word is rotated by 0 or 16 bits (`rot`, per ray) and its low half is the near plane, its
// high half the far plane: no min / max per axis, max3 / min3 over the axes.
struct RaySlabs { V3 inv, oi; uint32_t rx, ry, rz; };
ST_D RaySlabs ray_slabs(const Ray& ray) {
    RaySlabs r;
    r.inv = v3(__builtin_amdgcn_rcpf(slab_safe_dir(ray.dir.x)), __builtin_amdgcn_rcpf(slab_safe_dir(ray.dir.y)), __builtin_amdgcn_rcpf(slab_safe_dir(ray.dir.z)));
    r.oi = v3(-ray.origin.x * r.inv.x, -ray.origin.y * r.inv.y, -ray.origin.z * r.inv.z);
    r.rx = (f2b(r.inv.x) >> 31) << 4; r.ry = (f2b(r.inv.y) >> 31) << 4; r.rz = (f2b(r.inv.z) >> 31) << 4;
    return r;
}
// the plane arithmetic: the ray's entry and exit distance of the box (a hit where *tmin <= *tmax)
ST_D void compact_planes(uint32_t wx, uint32_t wy, uint32_t wz, const RaySlabs& r, float* tmin, float* tmax) {
    wx = __builtin_amdgcn_alignbit(wx, wx, r.rx); wy = __builtin_amdgcn_alignbit(wy, wy, r.ry); wz = __builtin_amdgcn_alignbit(wz, wz, r.rz);
    const float nx = fmaf(half_lo(wx), r.inv.x, r.oi.x), fx = fmaf(half_hi(wx), r.inv.x, r.oi.x);
    const float ny = fmaf(half_lo(wy), r.inv.y, r.oi.y), fy = fmaf(half_hi(wy), r.inv.y, r.oi.y);
    const float nz = fmaf(half_lo(wz), r.inv.z, r.oi.z), fz = fmaf(half_hi(wz), r.inv.z, r.oi.z);
    *tmin = fmax_(fmax_(fmax_(nx, ny), nz), 0.0f);
    *tmax = fmin_(fmin_(fx, fy), fz);
}
ST_D float compact_slab(uint32_t wx, uint32_t wy, uint32_t wz, const RaySlabs& r) {
    float tmin, tmax;
    compact_planes(wx, wy, wz, r, &tmin, &tmax);
    return tmin <= tmax ? tmin : kF32Max;
}
template <class SE>
ST_D bool any_hit_compact(const KArgs& a, const Ray& ray, SE* stack) {
    if (a.bvh_len == 0u) return false;
    const float limit = ray.len;
    const RaySlabs rs = ray_slabs(ray);
    uint32_t cur = a.bvh_c_root;
    int sp = 0;
    bool hit = false;
    for (;;) {
        const bool leaf = (cur & 1u) != 0u;
        const float4* e = bvh_entry(a.bvh_c, __umul24(cur >> 1, 48u));   // v_mul_u32_u24: full rate, the 32-bit multiply is not
        const float4 t0 = e[0], t1 = e[1];
        float4 t2 = f4z();
        if (leaf) t2 = e[2];
        asm volatile("" :: "v"(t0.x), "v"(t1.x), "v"(t2.x));   // one round trip for the entry
        if (!leaf) {
            const uint32_t link = f2b(t1.z);
            float near_d = compact_slab(f2b(t0.x), f2b(t0.y), f2b(t0.z), rs);
            float far_d = compact_slab(f2b(t0.w), f2b(t1.x), f2b(t1.y), rs);
            uint32_t near_ptr = (((cur >> 1) + 1u) << 1) | (link & 1u), far_ptr = ((link >> 2) << 1) | ((link >> 1) & 1u);
            if (far_d < near_d) { const uint32_t tp = near_ptr; near_ptr = far_ptr; far_ptr = tp; const float td = near_d; near_d = far_d; far_d = td; }
            if (far_d < limit) { if (sp < (int)a.stack_entries) { stack[sp * 64] = (SE)far_ptr; sp++; } }
            if (near_d < limit) { cur = near_ptr; continue; }
        } else {
            const uint32_t head = f2b(t0.w);
            float u, v;
            bool found = any_triangle(ray, xyz(t0), xyz(t1), xyz(t2), limit, &u, &v);
            if (found && (head & 2u)) {  // AlphaMode::Blend: the texel decides (exact-island fetch, as in traverse())
                if (!alpha_opaque(a, head >> 2, f2b(t1.w), u, v)) found = false;
            }
            if (found) { hit = true; break; }
            if (head & 1u) { cur += 2u; continue; }   // the next entry of the run: a leaf entry too
        }
        if (sp > 0) { sp--; cur = (uint32_t)stack[sp * 64]; } else break;
    }
    return hit;
}
// Closest hit over the compact stream: the same loop with the cut-off following the best distance (triangle arithmetic contracted, as in
// any_triangle; Candidate as traverse() fills it, so trace_closest resolves attributes the same way).
template <class SE>
ST_D bool closest_hit_compact(const KArgs& a, const Ray& ray, SE* stack, Candidate* best) {
    candidate_reset(best, kF32Max);
    if (a.bvh_len == 0u) return false;
    const RaySlabs rs = ray_slabs(ray);
    uint32_t cur = a.bvh_c_root;
    int sp = 0;
    bool found_any = false;
    for (;;) {
        const bool leaf = (cur & 1u) != 0u;
        const float4* e = bvh_entry(a.bvh_c, __umul24(cur >> 1, 48u));   // v_mul_u32_u24: full rate, the 32-bit multiply is not
        const float4 t0 = e[0], t1 = e[1];
        float4 t2 = f4z();
        if (leaf) t2 = e[2];
        asm volatile("" :: "v"(t0.x), "v"(t1.x), "v"(t2.x));
        if (!leaf) {
            const uint32_t link = f2b(t1.z);
            float near_d = compact_slab(f2b(t0.x), f2b(t0.y), f2b(t0.z), rs);
            float far_d = compact_slab(f2b(t0.w), f2b(t1.x), f2b(t1.y), rs);
            uint32_t near_ptr = (((cur >> 1) + 1u) << 1) | (link & 1u), far_ptr = ((link >> 2) << 1) | ((link >> 1) & 1u);
            if (far_d < near_d) { const uint32_t tp = near_ptr; near_ptr = far_ptr; far_ptr = tp; const float td = near_d; near_d = far_d; far_d = td; }
            if (far_d < best->t) { if (sp < (int)a.stack_entries) { stack[sp * 64] = (SE)far_ptr; sp++; } }
            if (near_d < best->t) { cur = near_ptr; continue; }
        } else {
            const uint32_t head = f2b(t0.w);
            const V3 p0 = xyz(t0), e1 = xyz(t1), e2 = xyz(t2);
            const V3 pvec = cross(ray.dir, e2);
            const float det = dot(e1, pvec);
            if (!(fabsf(det) < kF32Eps)) {
                const float inv_det = ST_MT_RCP(det);
                const V3 tvec = ray.origin - p0;
                const float u = dot(tvec, pvec) * inv_det;
                const V3 qvec = cross(tvec, e1);
                const float v = dot(ray.dir, qvec) * inv_det;
                const float t = dot(e2, qvec) * inv_det;
                if (!((u < 0.0f) | (u > 1.0f) | (v < 0.0f) | (u + v > 1.0f) | (t <= 0.0f) | (t >= best->t))) {
                    bool found = true;
                    if (head & 2u) {  // alpha_opaque(), written out: called here, every closest-hit kernel's exec-mask bookkeeping grows by 11 scalar instructions (compared in assembly)
                        const GpuMaterial m = a.materials[f2b(t1.w)];
                        const float4 bc = sample_atlas(a, tri_uv(a, head >> 2, u, v), m.base_color, m.base_color_texture);
                        if (bc.w < 1.0f) found = false;
                    }
                    if (found) { best->t = t; best->u = u; best->v = v; best->inv_det = inv_det; best->tri = head >> 2; best->material = f2b(t1.w); found_any = true; }
                }
            }
            if (head & 1u) { cur += 2u; continue; }
        }
        if (sp > 0) { sp--; cur = (uint32_t)stack[sp * 64]; } else break;
    }
    return found_any;
}

// ---- the WIDE stream (round 5; k_bvh.hip k_bvh_wide, StTuning::wide_bvh): the same rays over 4-wide nodes. Round 4's probes priced ONE more 64-B
// line per step at +44 % and tripled box arithmetic at +20 %: the loop is bound by the lines it fetches and by its dependent round trips. The
// compact binary entry spends 32 B (a quarter of them straddling two lines) on TWO child boxes; a wide node holds FOUR conservative f16 child
// boxes (4 x 3 axis words, exactly what compact_slab reads) + four links in ONE aligned 64-B line. Host model (tools/bvh4_sim.py, dungeon):
// 11.6 node steps per GI ray instead of 23.4, the same number of texels, half the lines, 0.55 x the loop iterations per wave, VALU unchanged.
// Round 3's 4-wide nodes lost with 128-B f32 nodes (two lines, seven texels per step) and ~25 instructions of ordering; here ordering is
//   key = (entry distance's high 16 bits | the child's 16-bit link), one v_perm_b32 per child,
// sorted by a 5-comparator network of v_min_u32 / v_max_u32: the link travels inside the key, a push is a 16-bit LDS store of the key itself,
// and children whose distances agree to 7 mantissa bits are visited in link order (order only, never the result).
//   node (64 B, texel 4 n of bvh_w):  texel 0: c0.x c0.y c0.z c1.x   texel 1: c1.y c1.z c2.x c2.y   texel 2: c2.z c3.x c3.y c3.z   (word = lower | upper << 16, f16)
//                                     texel 3: links — 16-bit form (fewer than 32768 nodes and leaf records): l0 | l1 << 16, l2 | l3 << 16, 0, 0
//                                                      32-bit form: l0, l1, l2, l3 (the key then keeps the link in its low 17 ... 24 bits — as many as the tree's
//                                                      largest link needs — and the distance's leading bits above them: one v_and_or_b32 per child).
//                                                      link = index << 1 | is a leaf record; an empty slot has an inverted box
//   leaf record (48 B, bvh_w_leaf_off + 48 k bytes into the same allocation): the compact stream's leaf entry; a run's records are consecutive
// One child's key: its slab test (compact_slab's arithmetic) fused with the cut-off — a miss or a child beyond `lim` is 0xffffffff, which sorts last.
template <class SE> struct WideKeys;
template <> struct WideKeys<uint16_t> {   // links ride in the keys
    static ST_D uint32_t key(float tmin, bool hit, float4 t3, int slot, uint32_t) {
        const uint32_t links = slot < 2 ? f2b(t3.x) : f2b(t3.y);
        return hit ? __builtin_amdgcn_perm(f2b(tmin), links, (slot & 1) ? 0x07060302u : 0x07060100u) : 0xffffffffu;
    }
    static ST_D uint32_t link(uint32_t k, uint32_t) { return k & 0xffffu; }
};
template <> struct WideKeys<uint32_t> {   // the link rides in the key's low KArgs::bvh_w_link_bits bits (17 ... 24), the distance keeps what is left above them
    static ST_D uint32_t key(float tmin, bool hit, float4 t3, int slot, uint32_t mask) {
        const uint32_t link = f2b(slot == 0 ? t3.x : (slot == 1 ? t3.y : (slot == 2 ? t3.z : t3.w)));
        return hit ? ((f2b(tmin) & ~mask) | link) : 0xffffffffu;   // v_and_or_b32
    }
    static ST_D uint32_t link(uint32_t k, uint32_t mask) { return k & mask; }
};
template <class SE>
ST_D uint32_t wide_key(uint32_t wx, uint32_t wy, uint32_t wz, const RaySlabs& r, float lim, float4 t3, int slot, uint32_t mask) {
    float tmin, tmax;
    compact_planes(wx, wy, wz, r, &tmin, &tmax);
    return WideKeys<SE>::key(tmin, (tmin <= tmax) & (tmin < lim), t3, slot, mask);
}
// four keys in ascending order: sort three with v_min3 / v_med3 / v_max3, insert the fourth with two more v_med3 — 7 instructions
// (the compiler finds v_med3_u32 in min / max trees only sometimes and v_min3_u32 never: stated here)
ST_D uint32_t umin3_(uint32_t a, uint32_t b, uint32_t c) { uint32_t r; asm("v_min3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
ST_D uint32_t umax3_(uint32_t a, uint32_t b, uint32_t c) { uint32_t r; asm("v_max3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
ST_D uint32_t umed3_(uint32_t a, uint32_t b, uint32_t c) { uint32_t r; asm("v_med3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
#define ST_WIDE_SORT4(k0, k1, k2, k3)                                                                                   \
    do {                                                                                                                \
        const uint32_t lo_ = umin3_(k0, k1, k2), md_ = umed3_(k0, k1, k2), hi_ = umax3_(k0, k1, k2), d_ = k3;           \
        k0 = min(lo_, d_); k1 = umed3_(lo_, md_, d_); k2 = umed3_(md_, hi_, d_); k3 = max(hi_, d_);                     \
    } while (0)
// (ONE fetch site for both kinds of step, as in the compact loop: with a fetch in each body a wave whose lanes sit on nodes AND on leaf
// records pays two dependent round trips per iteration — measured: the incoherent GI rays lost 10 % that way while coherent rays gained.
// Nodes and leaf records therefore live in one allocation, the records `bvh_w_leaf_off` bytes behind its start.)
// A push the stack has no room for is DROPPED (the subtree behind it is never visited: geometry can be missed) — and reported: the keys are sorted, so
// whenever a node pushes at all its LAST push is k1's, and if any of its pushes found the stack full that one did too. One `else` per node step, never
// taken on any scene measured (deepest stack 11-14 of 24), sets a sticky word of page-locked host memory the engine owns (KArgs::walk_flags:
// a plain store of 1, no atomic — word 0: a per-lane walk, word 1: the primary rays' packet); the next st_tick that sees it re-arms the launches with a
// deeper stack (the packet: hands primary visibility back to the per-lane walk) and returns ST_ERR_BVH_TOO_DEEP once (st_tick.cpp).
constexpr uint32_t kWalkOverflowLane = 0u, kWalkOverflowPacket = 1u;
ST_D void wide_walk_overflowed(const KArgs& a, uint32_t word) { if (a.walk_flags) a.walk_flags[word] = 1u; }
ST_D uint32_t wide_at(const KArgs& a, uint32_t cur) { return (cur & 1u) ? a.bvh_w_leaf_off + __umul24(cur >> 1, 48u) : (cur << 5); }
template <class SE>
ST_D bool any_hit_wide(const KArgs& a, const Ray& ray, SE* stack) {
    if (a.bvh_len == 0u) return false;
    const float limit = ray.len;
    const RaySlabs rs = ray_slabs(ray);
    uint32_t cur = a.bvh_w_root;
    SE* top = stack;                                             // the stack pointer is the LDS address itself: a push / pop is one add, no index -> address step
    const SE* const stack_end = stack + a.stack_entries * 64u;
    bool hit = false;
    for (;;) {
        const bool leaf = (cur & 1u) != 0u;
        const float4* e = bvh_entry(a.bvh_w, wide_at(a, cur));
        const float4 t0 = e[0], t1 = e[1], t2 = e[2];
        float4 t3 = f4z();
        if (!leaf) t3 = e[3];
        asm volatile("" :: "v"(t0.x), "v"(t1.x), "v"(t2.x), "v"(t3.x));   // one round trip for the line
        if (!leaf) {
            uint32_t k0 = wide_key<SE>(f2b(t0.x), f2b(t0.y), f2b(t0.z), rs, limit, t3, 0, a.bvh_w_link_mask);
            uint32_t k1 = wide_key<SE>(f2b(t0.w), f2b(t1.x), f2b(t1.y), rs, limit, t3, 1, a.bvh_w_link_mask);
            uint32_t k2 = wide_key<SE>(f2b(t1.z), f2b(t1.w), f2b(t2.x), rs, limit, t3, 2, a.bvh_w_link_mask);
            uint32_t k3 = wide_key<SE>(f2b(t2.y), f2b(t2.z), f2b(t2.w), rs, limit, t3, 3, a.bvh_w_link_mask);
            ST_WIDE_SORT4(k0, k1, k2, k3);
            if (k3 != 0xffffffffu) { if (top < stack_end) { *top = (SE)WideKeys<SE>::link(k3, a.bvh_w_link_mask); top += 64; } }
            if (k2 != 0xffffffffu) { if (top < stack_end) { *top = (SE)WideKeys<SE>::link(k2, a.bvh_w_link_mask); top += 64; } }
            if (k1 != 0xffffffffu) { if (top < stack_end) { *top = (SE)WideKeys<SE>::link(k1, a.bvh_w_link_mask); top += 64; } else wide_walk_overflowed(a, kWalkOverflowLane); }
            if (k0 != 0xffffffffu) { cur = WideKeys<SE>::link(k0, a.bvh_w_link_mask); continue; }
        } else {
            const uint32_t head = f2b(t0.w);
            float u, v;
            bool found = any_triangle(ray, xyz(t0), xyz(t1), xyz(t2), limit, &u, &v);
            if (found && (head & 2u)) {  // AlphaMode::Blend: the texel decides (exact-island fetch, as in traverse())
                if (!alpha_opaque(a, head >> 2, f2b(t1.w), u, v)) found = false;
            }
            if (found) { hit = true; break; }
            if (head & 1u) { cur += 2u; continue; }   // the next record of the run
        }
        if (top > stack) { top -= 64; cur = (uint32_t)*top; } else break;
    }
    return hit;
}
// EXACT_LEAF (primary rays, round 6): leaf records are tested with the exact island's Triangle::hit — (t, u, v) bit-identical to the contract walk's for the same triangle
// (The node step below is any_hit_wide's, written out again: as one helper — stack pointer by reference or returned — 41 fast-build kernels got other register numbers.)
template <class SE, bool EXACT_LEAF>
ST_D bool closest_hit_wide(const KArgs& a, const Ray& ray, SE* stack, Candidate* best) {
    candidate_reset(best, kF32Max);
    if (a.bvh_len == 0u) return false;
    const RaySlabs rs = ray_slabs(ray);
    uint32_t cur = a.bvh_w_root;
    SE* top = stack;                                             // the stack pointer is the LDS address itself: a push / pop is one add, no index -> address step
    const SE* const stack_end = stack + a.stack_entries * 64u;
    bool found_any = false;
    for (;;) {
        const bool leaf = (cur & 1u) != 0u;
        const float4* e = bvh_entry(a.bvh_w, wide_at(a, cur));
        const float4 t0 = e[0], t1 = e[1], t2 = e[2];
        float4 t3 = f4z();
        if (!leaf) t3 = e[3];
        asm volatile("" :: "v"(t0.x), "v"(t1.x), "v"(t2.x), "v"(t3.x));
        if (!leaf) {
            const float lim = best->t;
            uint32_t k0 = wide_key<SE>(f2b(t0.x), f2b(t0.y), f2b(t0.z), rs, lim, t3, 0, a.bvh_w_link_mask);
            uint32_t k1 = wide_key<SE>(f2b(t0.w), f2b(t1.x), f2b(t1.y), rs, lim, t3, 1, a.bvh_w_link_mask);
            uint32_t k2 = wide_key<SE>(f2b(t1.z), f2b(t1.w), f2b(t2.x), rs, lim, t3, 2, a.bvh_w_link_mask);
            uint32_t k3 = wide_key<SE>(f2b(t2.y), f2b(t2.z), f2b(t2.w), rs, lim, t3, 3, a.bvh_w_link_mask);
            ST_WIDE_SORT4(k0, k1, k2, k3);
            if (k3 != 0xffffffffu) { if (top < stack_end) { *top = (SE)WideKeys<SE>::link(k3, a.bvh_w_link_mask); top += 64; } }
            if (k2 != 0xffffffffu) { if (top < stack_end) { *top = (SE)WideKeys<SE>::link(k2, a.bvh_w_link_mask); top += 64; } }
            if (k1 != 0xffffffffu) { if (top < stack_end) { *top = (SE)WideKeys<SE>::link(k1, a.bvh_w_link_mask); top += 64; } else wide_walk_overflowed(a, kWalkOverflowLane); }
            if (k0 != 0xffffffffu) { cur = WideKeys<SE>::link(k0, a.bvh_w_link_mask); continue; }
        } else {
            const uint32_t head = f2b(t0.w);
            const V3 p0 = xyz(t0), e1 = xyz(t1), e2 = xyz(t2);
            float t, u, v, inv_det;
            bool found;
            if (EXACT_LEAF) found = triangle_hit_exact(ray, p0, e1, e2, best->t, &t, &u, &v, &inv_det);
            else {
                const V3 pvec = cross(ray.dir, e2);
                const float det = dot(e1, pvec);
                inv_det = ST_MT_RCP(det);
                const V3 tvec = ray.origin - p0;
                u = dot(tvec, pvec) * inv_det;
                const V3 qvec = cross(tvec, e1);
                v = dot(ray.dir, qvec) * inv_det;
                t = dot(e2, qvec) * inv_det;
                found = !(fabsf(det) < kF32Eps) & !((u < 0.0f) | (u > 1.0f) | (v < 0.0f) | (u + v > 1.0f) | (t <= 0.0f) | (t >= best->t));
            }
            if (found) {
                if (head & 2u) {  // alpha_opaque(), written out: as in closest_hit_compact
                    const GpuMaterial m = a.materials[f2b(t1.w)];
                    const float4 bc = sample_atlas(a, tri_uv(a, head >> 2, u, v), m.base_color, m.base_color_texture);
                    if (bc.w < 1.0f) found = false;
                }
                if (found) { best->t = t; best->u = u; best->v = v; best->inv_det = inv_det; best->tri = head >> 2; best->material = f2b(t1.w); found_any = true; }
            }
            if (head & 1u) { cur += 2u; continue; }
        }
        if (top > stack) { top -= 64; cur = (uint32_t)*top; } else break;
    }
    return found_any;
}

// ---- A WAVE-WIDE PACKET over the wide stream, for coherent rays (round 5: primary visibility; StTuning::primary_packets). The 64 primary rays of
// an 8 x 8 tile walk nearly the same nodes (host model, dungeon: 13.9 node steps per ray, 15.0 for the tile's longest ray, 15.7 in the UNION of the
// tile's paths), yet in the per-lane loop every lane fetches its own node, sorts its own keys and keeps its own stack: ~89 VALU instructions and
// four vector loads per node step. Here the WAVE walks the union: `cur` and the stack are uniform, a node is fetched ONCE with scalar loads
// (64 B through the scalar cache: no vector memory instruction in the loop), every lane tests the node's four boxes against its own ray — the
// box words arrive as scalar operands —, v_cmp's result IS the ballot, a child is entered when any lane hits it, children are ordered by the
// distances of the first lane that hits each, and the stack is ONE VGPR indexed by lane (v_writelane / v_readlane with a uniform stack pointer:
// 64 entries). A lane that missed a node misses its children too (their boxes lie inside it), so no per-entry lane mask is kept. Leaf records
// are scalar loads as well; the triangle test is each lane's own. Lanes that have left the kernel are simply inactive: ballots skip them.
// Results: each lane's closest hit — the same triangle as the per-lane walk finds, except where two triangles tie.
typedef const __attribute__((address_space(4))) uint32_t* ScalarWords;
ST_D uint32_t wave_uniform(uint32_t x) { return __builtin_amdgcn_readfirstlane(x); }
// lane `lane` of `reg` = `value` (both uniform); v_writelane_b32 ignores EXEC. (This clang has the readlane builtin but no writelane one.)
ST_D uint32_t wave_writelane(uint32_t reg, uint32_t value, uint32_t lane) {
    // (two different SGPR operands would break the one-SGPR constant-bus rule of gfx9 VALU instructions: the lane select goes through M0)
    asm volatile("s_mov_b32 m0, %2\n\tv_writelane_b32 %0, %1, m0" : "+v"(reg) : "s"(wave_uniform(value)), "s"(wave_uniform(lane)) : "m0");
    return reg;
}
// (The same walk over the LDS-resident CONTRACT stream of the Cornell box — uniform pointer, LDS broadcast reads, the exact island's box and
// triangle tests per lane — was built too: prim_visibility 59.3 -> 58.0 us, inside the noise of the frame, and the whole-frame steady-state test
// no longer passed (ties between a quad's two triangles resolve in packet order, not in the per-lane walk's). Not kept: the Cornell box keeps its
// per-lane contract walk.)
// (A software-pipelined form — the nearest child's line fetched before the others are pushed, a leaf step's successor before its triangle is
// tested, keys sorted by a branch-free min / max network with the slot in their low bits — measured SLOWER on the same box: prim_visibility
// 119 -> 132 us on the dungeon, 150 -> 173 at 208 k triangles, 440 -> 485 at 3840 x 2160: sixteen more live SGPRs for the second line spill, and
// scalar loads return out of order, so every wait for an OLD line also waits for the prefetched one. The simple loop below is the one kept.)
ST_D bool closest_hit_packet(const KArgs& a, const Ray& ray, Candidate* best) {
    candidate_reset(best, kF32Max);
    if (a.bvh_len == 0u) return false;
    const RaySlabs rs = ray_slabs(ray);
    const ScalarWords base = (ScalarWords)(a.bvh_w);
    const uint32_t leaf_words = a.bvh_w_leaf_off >> 2;
    uint32_t cur = a.bvh_w_root;          // uniform
    uint32_t stack = 0u;                  // lane k of this VGPR = stack entry k
    uint32_t sp = 0u;                     // uniform
    bool found_any = false;
    for (;;) {
        if (!(cur & 1u)) {
            const ScalarWords n = base + (size_t)cur * 8u;   // node index = cur >> 1, 16 words each
            const uint32_t w0 = n[0], w1 = n[1], w2 = n[2], w3 = n[3], w4 = n[4], w5 = n[5], w6 = n[6], w7 = n[7], w8 = n[8], w9 = n[9], w10 = n[10], w11 = n[11];
            const uint32_t x0 = n[12], x1 = n[13], x2 = n[14], x3 = n[15];
            uint32_t l0, l1, l2, l3;
            if (a.bvh_w_links16) { l0 = x0 & 0xffffu; l1 = x0 >> 16; l2 = x1 & 0xffffu; l3 = x1 >> 16; } else { l0 = x0; l1 = x1; l2 = x2; l3 = x3; }
            const float lim = best->t;
            const float t0 = compact_slab(w0, w1, w2, rs), t1 = compact_slab(w3, w4, w5, rs), t2 = compact_slab(w6, w7, w8, rs), t3 = compact_slab(w9, w10, w11, rs);
            const unsigned long long m0 = __builtin_amdgcn_ballot_w64(t0 < lim), m1 = __builtin_amdgcn_ballot_w64(t1 < lim), m2 = __builtin_amdgcn_ballot_w64(t2 < lim),
                                     m3 = __builtin_amdgcn_ballot_w64(t3 < lim);
            // keys: the entry distance of the first lane that hits the child (bits of a non-negative float order as integers), ~0 when no lane does
            uint32_t k0 = m0 ? (uint32_t)__builtin_amdgcn_readlane((int)f2b(t0), (int)__builtin_ctzll(m0)) : 0xffffffffu;
            uint32_t k1 = m1 ? (uint32_t)__builtin_amdgcn_readlane((int)f2b(t1), (int)__builtin_ctzll(m1)) : 0xffffffffu;
            uint32_t k2 = m2 ? (uint32_t)__builtin_amdgcn_readlane((int)f2b(t2), (int)__builtin_ctzll(m2)) : 0xffffffffu;
            uint32_t k3 = m3 ? (uint32_t)__builtin_amdgcn_readlane((int)f2b(t3), (int)__builtin_ctzll(m3)) : 0xffffffffu;
            // a 5-comparator network on (key, link) pairs: uniform values, scalar unit
#define ST_PKT_CSWAP(ka, la, kb, lb) do { if (kb < ka) { const uint32_t tk_ = ka; ka = kb; kb = tk_; const uint32_t tl_ = la; la = lb; lb = tl_; } } while (0)
            ST_PKT_CSWAP(k0, l0, k1, l1); ST_PKT_CSWAP(k2, l2, k3, l3); ST_PKT_CSWAP(k0, l0, k2, l2); ST_PKT_CSWAP(k1, l1, k3, l3); ST_PKT_CSWAP(k1, l1, k2, l2);
#undef ST_PKT_CSWAP
            if (k3 != 0xffffffffu && sp < 64u) { stack = wave_writelane(stack, l3, sp); sp++; }
            if (k2 != 0xffffffffu && sp < 64u) { stack = wave_writelane(stack, l2, sp); sp++; }
            if (k1 != 0xffffffffu) { if (sp < 64u) { stack = wave_writelane(stack, l1, sp); sp++; } else wide_walk_overflowed(a, kWalkOverflowPacket); }
            if (k0 != 0xffffffffu) { cur = l0; continue; }
        } else {
            const ScalarWords r = base + leaf_words + (size_t)(cur >> 1) * 12u;
            const V3 p0 = v3(b2f(r[0]), b2f(r[1]), b2f(r[2])), e1 = v3(b2f(r[4]), b2f(r[5]), b2f(r[6])), e2 = v3(b2f(r[8]), b2f(r[9]), b2f(r[10]));
            const uint32_t head = r[3], material = r[7];
            // (the island's Triangle::hit: primary hits carry the CPU restatement's (t, u, v) bit for bit — see closest_resolve_exact; 12 more VALU instructions per
            // record than the contracted form with v_rcp_f32, three to five records per ray)
            float t, u, v, inv_det;
            if (triangle_hit_exact(ray, p0, e1, e2, best->t, &t, &u, &v, &inv_det)) {
                bool found = true;
                if (head & 2u) {
                    if (!alpha_opaque(a, head >> 2, material, u, v)) found = false;
                }
                if (found) { best->t = t; best->u = u; best->v = v; best->inv_det = inv_det; best->tri = head >> 2; best->material = material; found_any = true; }
            }
            if (head & 1u) { cur += 2u; continue; }
        }
        if (sp == 0u) break;
        sp--; cur = (uint32_t)__builtin_amdgcn_readlane((int)stack, (int)sp);
    }
    return found_any;
}
#endif
// Ray::intersect (shadow ray)
template <class SE>
ST_D bool trace_any(const KArgs& a, const Ray& ray, SE* stack, uint32_t* used_memory) {
#if ST_FAST_DEVICE && !defined(ST_NO_ANYHIT_FAST)
    if (!a.anyhit_contract) {
        *used_memory = 0u;
        if (a.bvh_w != nullptr) return any_hit_wide(a, ray, stack);
        return a.bvh_c != nullptr ? any_hit_compact(a, ray, stack) : any_hit_fast(a, ray, stack);
    }
#endif
    return trace_any_contract(a, ray, stack, used_memory);
}
