// st_device.h — device-side library of the MI355X hot path: primary-ray generation, BVH traversal with a
// per-wave LDS stack and Möller–Trumbore with deferred attribute fetch (st_traverse.h, included below),
// G-buffer / normal / reservoir codecs, BRDFs, lights, MIS, atmosphere lookup. Behavioural contract: strolle-gpu/src/*.rs (cited per block);
// data layout and control flow are this library's own.
#pragma once
#include "st_types.h"

namespace st {

#define ST_D __device__ __forceinline__

// ------------------------------------------------------------------ launch geometry
// One wavefront == one 8x8 pixel tile (64 lanes); a 256-thread block owns four horizontally adjacent tiles.
// Blocks are dealt to XCDs round-robin by the hardware (block b -> XCD b % 8); the remap below gives every
// XCD one contiguous band of tile rows so that neighbour taps (spatial resampling, à-trous) of a tile stay
// in the same XCD's L2.
struct TileCoord { uint32_t x, y; bool valid; };
// map_mode 0: XCD-banded (each XCD owns a contiguous band of tile rows); 1: hardware order (block b -> XCD b % 8,
// consecutive blocks are horizontal neighbours); 2: XCD-banded in chunks of 4 tile rows (locality for short taps,
// balance for spatially clustered slow paths).
// (`b`: the workgroup's number in the launch that covers the window with one workgroup per four tiles — blockIdx.x, or a number a kernel whose
// workgroups each take several of those derives from it)
ST_D TileCoord tile_for_block(uint32_t b, uint32_t tiles_x, uint32_t tiles_y, uint32_t map_mode) {
    const uint32_t groups_x = (tiles_x + 3u) >> 2;              // blocks per tile row
    const uint32_t n_blocks = groups_x * tiles_y;
    uint32_t lin = b;
    if (map_mode == 0u) {
        const uint32_t q = n_blocks >> 3, r = n_blocks & 7u;    // bijective XCD remap (handles n % 8 != 0)
        const uint32_t xcd = b & 7u, k = b >> 3;
        lin = (xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q) + k;
    } else if (map_mode == 2u) {
        const uint32_t chunk = groups_x * 4u * 8u;              // 8 XCDs x 4 tile rows
        const uint32_t full = (n_blocks / chunk) * chunk;
        if (b < full) {
            const uint32_t c = b / chunk, i = b - c * chunk;
            const uint32_t xcd = i & 7u, k = i >> 3;            // k in [0, groups_x*4)
            lin = c * chunk + xcd * (groups_x * 4u) + k;
        }
    }
    const uint32_t wave = threadIdx.x >> 6;
    TileCoord t;
    t.y = lin / groups_x;
    t.x = (lin - t.y * groups_x) * 4u + wave;
    t.valid = b < n_blocks && t.x < tiles_x && t.y < tiles_y;
    return t;
}
ST_D TileCoord tile_for_thread(uint32_t tiles_x, uint32_t tiles_y, uint32_t map_mode) { return tile_for_block(blockIdx.x, tiles_x, tiles_y, map_mode); }
ST_D U2 pixel_in_tile(TileCoord t) {
    const uint32_t lane = threadIdx.x & 63u;
    return u2(t.x * 8u + (lane & 7u), t.y * 8u + (lane >> 3));
}
// Traversal stack in LDS, [wave][entry][lane] (consecutive lanes -> consecutive banks). Entries are BVH stream indices:
// entry numbers (byte offset / 64): device streams of fewer than 65536 entries (Cornell: 55, dungeon: ~26 k) use 16-bit
// stack slots, which halves the LDS footprint
// (12 KiB per 4-wave block) and lifts the LDS cap on occupancy from 6 to 8 waves per SIMD.
// The stack holds KArgs::stack_entries pending entries per lane: kBvhStackSize (24, strolle-gpu/src/lib.rs:76) or — when the tree's deepest chain of
// internal nodes is longer than that (the 208 k-triangle dungeon: 26) — kBvhStackSizeDeep (32), so that no push is ever dropped. It lives in
// DYNAMIC LDS sized at the launch (k_common.h ST_STACK_LDS / ST_LAUNCH): the 24-entry launches keep their occupancy.
template <class SE>
ST_D SE* lane_stack(const KArgs& a, SE* lds) { return lds + (threadIdx.x >> 6) * (a.stack_entries * 64u) + (threadIdx.x & 63u); }
// Per-kernel counters {rays traced, the reference's `used_memory` bytes}. One returning-free atomic pair per
// wavefront (hipcc's atomic optimizer reduces the uniform-address adds across the wave) lands on one of
// kCounterLines 64-byte lines picked by block id: a single hot word saturates near 88 atomics/us
// (MI355X_MICROARCH.md, row "dequeue"), which alone cost 0.7 ms per full-screen launch at 1080p.

// The byte half is off unless st_profile_enable asked for it (KArgs::count_bytes): summing a per-lane value takes a 64-bit
// cross-lane reduction per call (measured: 12-13 us of primary visibility's 89), counting rays takes a ballot.
ST_D void count_rays_n(const KArgs& a, uint32_t rays /* 0..3 */, unsigned long long used_memory) {
    unsigned long long* line = a.ray_counter + (blockIdx.x & (kCounterLines - 1u)) * 8u;
    if (rays & 1u) atomicAdd(line, 1ull);
    if (rays & 2u) atomicAdd(line, 2ull);
    if (a.count_bytes) atomicAdd(line + 1, used_memory);
}
// any number of rays per lane (the persistent-wave shadow kernel)
ST_D void count_rays_many(const KArgs& a, uint32_t rays, unsigned long long used_memory) {
    unsigned long long* line = a.ray_counter + (blockIdx.x & (kCounterLines - 1u)) * 8u;
    atomicAdd(line, (unsigned long long)rays);
    if (a.count_bytes) atomicAdd(line + 1, used_memory);
}
ST_D void count_rays(const KArgs& a, uint32_t used_memory) {
    unsigned long long* line = a.ray_counter + (blockIdx.x & (kCounterLines - 1u)) * 8u;
    atomicAdd(line, 1ull);
    if (a.count_bytes) atomicAdd(line + 1, (unsigned long long)used_memory);
}

// ------------------------------------------------------------------ small codecs
ST_D uint32_t u32_from_bytes(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return a | (b << 8) | (c << 16) | (d << 24); }
ST_D U2 resolve_checkerboard(U2 gid, uint32_t frame) { return u2(gid.x * 2u + ((frame + gid.y) % 2u), gid.y); }  // utils.rs:33-35
ST_D U2 resolve_checkerboard_alt(U2 gid, uint32_t frame) { return resolve_checkerboard(gid, frame + 1u); }
ST_D bool got_checkerboard_at(U2 p, uint32_t frame) { U2 q = resolve_checkerboard(u2(p.x / 2u, p.y), frame); return q.x == p.x && q.y == p.y; }

ST_D V2 normal_encode(V3 n) {  // normal.rs:9-24
    n = n / (fabsf(n.x) + fabsf(n.y) + fabsf(n.z));  // V3 / float: one reciprocal in the fast build
    V2 r;
    if (n.z >= 0.0f) r = v2(n.x, n.y);
    else { r = v2(copysignf(1.0f - fabsf(n.y), n.x), copysignf(1.0f - fabsf(n.x), n.y)); }
    return r * 0.5f + 0.5f;
}
ST_D V3 normal_decode(V2 e) {  // normal.rs:26-34
    e = e * 2.0f - 1.0f;
    V3 n = v3(e.x, e.y, 1.0f - fabsf(e.x) - fabsf(e.y));
    const float t = fmax_(-n.z, 0.0f);
    n.x -= copysignf(t, n.x);
    n.y -= copysignf(t, n.y);
    return normalize(n);
}

// ------------------------------------------------------------------ noise (noise/white.rs, noise/blue.rs)
struct WhiteNoise {
    uint32_t state;
    ST_D uint32_t sample_int() {
        state = state * 747796405u + 2891336453u;
        const uint32_t word = ((state >> ((state >> 28) + 4u)) ^ state) * 277803737u;
        return (word >> 22) ^ word;
    }
    ST_D float sample() { return (float)sample_int() * 2.3283064365386963e-10f; }  // / 2^32: a power of two, exact either way
    ST_D V2 sample_circle() { const float angle = sample() * kPi * 2.0f; float s, c; sincos_(angle, &s, &c); return v2(c, s); }
    ST_D V2 sample_disk() { const float radius = fsqrt(sample()); return sample_circle() * radius; }
    ST_D V3 sample_sphere() {
        const float phi = sample() * 2.0f * kPi;
        const float cos_theta = sample() * 2.0f - 1.0f;
        const float u = sample();
        const float theta = acos_(cos_theta);
        const float r = fsqrt(u);
        float st_, ct_, sp_, cp_;
        sincos_(theta, &st_, &ct_); sincos_(phi, &sp_, &cp_);
        return v3(r * st_ * cp_, r * st_ * sp_, r * ct_);
    }
    ST_D V3 sample_hemisphere(V3 normal) {
        const float cos_theta = sample();
        const float sin_theta = fsqrt(1.0f - sqr(cos_theta));
        const float phi = 2.0f * kPi * sample();
        V3 t, b;
        any_orthonormal_pair(normal, &t, &b);
        float sp_, cp_;
#if defined(ST_ABL_HEMI_POLY)
        sincos_poly_(phi, &sp_, &cp_);
#else
        sincos_(phi, &sp_, &cp_);
#endif
        return (t * cp_ + b * sp_) * sin_theta + normal * cos_theta;
    }
};
ST_D WhiteNoise white_noise(uint32_t seed, U2 id) { WhiteNoise w; w.state = seed ^ (48619u * id.x) ^ (95461u * id.y); return w; }
ST_D float4 blue_noise_read(const KArgs& a, U2 id) {
    const uint32_t ux = (id.x + 71u * a.frame) % 256u, uy = (id.y + 11u * a.frame) % 256u;
    const uchar4 p = a.blue_noise[uy * 256u + ux];
    return make_float4(fdivc((float)p.x, 255.0f), fdivc((float)p.y, 255.0f), fdivc((float)p.z, 255.0f), fdivc((float)p.w, 255.0f));
}

// ------------------------------------------------------------------ rays & camera (ray.rs:14-53, camera.rs:19-150)
struct Ray { V3 origin, dir, inv_dir; float len; };

// ================================================================== exact island (1/3): ray generation
// Everything between the `contract(off)` pragmas is the same arithmetic in both builds of the kernels: correctly rounded
// + - * / sqrt, never contracted, no hardware approximations. It covers what decides which BVH nodes and triangles a ray
// visits — Camera::ray, the ray's reciprocal direction, intersect_box, Triangle::hit, the alpha test's texture fetch — so
// that the reference's `used_memory` counter (the BVH heatmap's integers) is bit-identical to the CPU restatement whichever
// build runs. Helpers used in here are defined in here (xe::): an inlined helper from outside would bring its own
// contraction setting with it.
#pragma clang fp contract(off)
namespace xe {
ST_D V3 add(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
ST_D V3 sub(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
ST_D V3 mul(V3 a, V3 b) { return v3(a.x * b.x, a.y * b.y, a.z * b.z); }
ST_D V3 scale(V3 a, float s) { return v3(a.x * s, a.y * s, a.z * s); }
ST_D float dot(V3 a, V3 b) { return (a.x * b.x) + (a.y * b.y) + (a.z * b.z); }
ST_D V3 cross(V3 a, V3 b) { return v3(a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y); }
ST_D V3 normalize(V3 a) { return scale(a, 1.0f / sqrtf(dot(a, a))); }
ST_D float4 scale4(float4 a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }
ST_D float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
ST_D float4 sub4(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
ST_D float4 mul4(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
ST_D V3 project_point3(const M4& m, V3 p) {  // glam Mat4::project_point3
    float4 r = scale4(m.c[0], p.x);
    r = add4(scale4(m.c[1], p.y), r);
    r = add4(scale4(m.c[2], p.z), r);
    r = add4(m.c[3], r);
    const float rw = 1.0f / r.w;
    return v3(r.x * rw, r.y * rw, r.z * rw);
}
}  // namespace xe
ST_D Ray make_ray(V3 o, V3 d) { Ray r; r.origin = o; r.dir = d; r.inv_dir = v3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z); r.len = kF32Max; return r; }
ST_D Ray zero_ray() { Ray r; r.origin = v3s(0.0f); r.dir = v3s(0.0f); r.inv_dir = v3s(0.0f); r.len = 0.0f; return r; }  // Ray::default()
ST_D V3 ray_at(const Ray& r, float t) { return r.origin + r.dir * t; }

ST_D Ray camera_ray(const GpuCamera& c, U2 pos) {
    const float spx = (float)pos.x + 0.5f, spy = (float)pos.y + 0.5f;
    const float ndc_x = spx * 2.0f / c.screen.x - 1.0f;
    const float ndc_y = -(spy * 2.0f / c.screen.y - 1.0f);
    const V3 far_plane = xe::project_point3(c.ndc_to_world, v3(ndc_x, ndc_y, kF32Eps));
    const V3 near_plane = xe::project_point3(c.ndc_to_world, v3(ndc_x, ndc_y, 1.0f));
    return make_ray(near_plane, xe::normalize(xe::sub(far_plane, near_plane)));
}
#if defined(ST_FAST_MATH)
#pragma clang fp contract(fast)
#endif
// ================================================================== end of exact island (1/3)
// Camera::ray for SHADING: the ray through a pixel whose G-buffer depth is being turned back into a surface point
// (Hit::from_gbuffer via pixel_hit below) or whose direction a BRDF needs. Nothing traverses the BVH with it, so in the fast
// build it is ordinary fast arithmetic (about a third of the instructions of the exact version above — and pixel_hit runs at
// 17 call sites, once per neighbour tap in the resampling loops); in the exact build it is the same operations as camera_ray.
ST_D Ray camera_ray_shading(const GpuCamera& c, U2 pos) {
    const V2 screen_size = v2(c.screen.x, c.screen.y);
    const V2 sp = as_v2(pos) + v2(0.5f, 0.5f);
    V2 ndc = sp * 2.0f / screen_size - v2(1.0f, 1.0f);
    ndc = v2(ndc.x, -ndc.y);
    const V3 far_plane = project_point3(c.ndc_to_world, v3(ndc.x, ndc.y, kF32Eps));
    const V3 near_plane = project_point3(c.ndc_to_world, v3(ndc.x, ndc.y, 1.0f));
    Ray r; r.origin = near_plane; r.dir = normalize(far_plane - near_plane); r.inv_dir = v3s(0.0f); r.len = kF32Max;  // inv_dir: never traversed
    return r;
}
ST_D float4 world_to_clip(const GpuCamera& c, V3 p) { return mul(c.projection_view, f4(p, 1.0f)); }
ST_D V2 clip_to_screen(const GpuCamera& c, float4 p) {
    V2 ndc = v2(p.x, p.y) / p.w;
    ndc = v2(ndc.x, -ndc.y);
    return (0.5f * ndc + 0.5f) * v2(c.screen.x, c.screen.y);
}
ST_D uint32_t screen_to_idx(const KArgs& a, U2 p) { return p.y * a.width + p.x; }
ST_D U2 camera_contain(const KArgs& a, I2 p) {  // camera.rs:53-75
    const int32_t sx = (int32_t)a.width, sy = (int32_t)a.height;
    if (p.x < 0) p.x = -p.x;
    if (p.y < 0) p.y = -p.y;
    if (p.x >= sx) p.x = sx - p.x + sx - 1;
    if (p.y >= sy) p.y = sy - p.y + sy - 1;
    return u2((uint32_t)p.x, (uint32_t)p.y);
}
ST_D bool contains_u(const KArgs& a, U2 p) { return p.x < a.width && p.y < a.height; }
ST_D bool contains_i(const KArgs& a, I2 p) { return p.x >= 0 && p.y >= 0 && p.x < (int32_t)a.width && p.y < (int32_t)a.height; }
ST_D bool contains_f(const KArgs& a, V2 p) { return p.x >= 0.0f && p.y >= 0.0f && p.x < (float)a.width && p.y < (float)a.height; }
ST_D bool camera_is_eq(const GpuCamera& a, const GpuCamera& b) {  // camera.rs:104-107
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const float4 x = a.projection_view.c[i], y = b.projection_view.c[i];
        ok = ok && fabsf(x.x - y.x) <= 0.0025f && fabsf(x.y - y.y) <= 0.0025f && fabsf(x.z - y.z) <= 0.0025f && fabsf(x.w - y.w) <= 0.0025f;
    }
    return ok;
}
// plane access with storage-image semantics (out-of-range reads are zero, writes are dropped)
ST_D float4 tex_read(const float4* p, const KArgs& a, U2 pos) { return (pos.x < a.width && pos.y < a.height) ? p[pos.y * a.width + pos.x] : f4z(); }
ST_D void tex_write(float4* p, const KArgs& a, U2 pos, float4 v) { if (pos.x < a.width && pos.y < a.height) p[pos.y * a.width + pos.x] = v; }

// ------------------------------------------------------------------ materials & atlas (material.rs:25-104)
// Byte decodes are pure functions of 256 inputs; the engine tabulates them once on the device with these very routines
// (k_trace.hip k_build_byte_luts) so that a texel costs four table reads instead of three pow_() + a division — about
// 250 VALU operations per texel, twelve texels per textured primary hit.
// ================================================================== exact island (2/3): byte tables and atlas sampling
// The tables are built once per engine with the polynomial pow (identical in both builds); the bilinear fetch is what the
// traversal's alpha test reads (Triangle::hit's `base_color.w < 1`, ray.rs:184-214).
#pragma clang fp contract(off)
ST_D float srgb_to_linear_eval(uint32_t v) {
    const float c = (float)v / 255.0f;
    return c <= 0.04045f ? c / 12.92f : pow_poly_((c + 0.055f) / 1.055f, 2.4f);
}
ST_D float unorm8_eval(uint32_t v) { return (float)v / 255.0f; }
constexpr uint32_t kLutSrgb = 0u, kLutUnorm8 = 256u, kLutGamma8 = 512u, kLutGamma6 = 768u, kByteLutFloats = 1024u;  // layout of KArgs::byte_luts
ST_D float gamma8_eval(uint32_t v) { return pow_poly_((float)v / 255.0f, 2.2f); }  // G-buffer base colour RGB (gbuffer.rs:88-97)
ST_D float gamma6_eval(uint32_t v) { return pow_poly_((float)v / 63.0f, 2.2f); }   // ... and its 6-bit alpha
ST_D float srgb_to_linear(const KArgs& a, uint32_t v) { return a.byte_luts[kLutSrgb + v]; }
ST_D float unorm8(const KArgs& a, uint32_t v) { return a.byte_luts[kLutUnorm8 + v]; }
// SRGB: a colour texture's texel (RGB through the sRGB curve). !SRGB: a normal map's (include/strolle_hip.h "normal mapping"): the bytes are a
// direction, not a colour, and all decode as byte / 255. One definition of the clamp, the texel centres and the order of the bilinear blend for both.
template <bool SRGB>
ST_D float4 atlas_texel(const KArgs& a, int32_t x, int32_t y) {
    x = x < 0 ? 0 : (x >= (int32_t)a.atlas_w ? (int32_t)a.atlas_w - 1 : x);
    y = y < 0 ? 0 : (y >= (int32_t)a.atlas_h ? (int32_t)a.atlas_h - 1 : y);
    const uchar4 p = a.atlas[(uint32_t)y * a.atlas_w + (uint32_t)x];
    if (!SRGB) return make_float4(unorm8(a, p.x), unorm8(a, p.y), unorm8(a, p.z), unorm8(a, p.w));
    return make_float4(srgb_to_linear(a, p.x), srgb_to_linear(a, p.y), srgb_to_linear(a, p.z), unorm8(a, p.w));
}
// gfx950 has no texture unit: bilinear, clamp-to-edge, lod 0, sRGB decode before filtering; NaN coordinates -> 0.
template <bool SRGB = true>
ST_D float4 atlas_sample(const KArgs& a, V2 uv) {
    if (a.atlas_w == 0u) return f4z();
    if (uv.x != uv.x) uv.x = 0.0f;
    if (uv.y != uv.y) uv.y = 0.0f;
    const float fx = uv.x * (float)a.atlas_w - 0.5f, fy = uv.y * (float)a.atlas_h - 0.5f;
    const float x0 = floorf(fx), y0 = floorf(fy);
    const float tx = fx - x0, ty = fy - y0;
    const int32_t ix = f2i_sat(x0), iy = f2i_sat(y0);
    const float4 p00 = atlas_texel<SRGB>(a, ix, iy), p10 = atlas_texel<SRGB>(a, ix + 1, iy), p01 = atlas_texel<SRGB>(a, ix, iy + 1), p11 = atlas_texel<SRGB>(a, ix + 1, iy + 1);
    const float4 top = xe::add4(p00, xe::scale4(xe::sub4(p10, p00), tx));
    const float4 bot = xe::add4(p01, xe::scale4(xe::sub4(p11, p01), tx));
    return xe::add4(top, xe::scale4(xe::sub4(bot, top), ty));
}
// fmodf(x, 1) for x >= 0 (material.rs:86-104 `% 1.0`): x - floor(x) is exact in f32 (the fraction of x needs no more
// significant bits than x has), NaN and +inf give NaN either way; libm's fmodf is a 40-instruction loop with two nested
// divergent branches, six times per textured hit.
ST_D float fmod1_nonneg(float x) { return x - floorf(x); }
ST_D float mat_wrap(float t) { return t > 0.0f ? fmod1_nonneg(t) : 1.0f - fmod1_nonneg(-t); }
// where hit_uv falls in the atlas: the wrap, then the texture's rectangle
ST_D V2 atlas_uv(V2 hit_uv, float4 texture) {
    hit_uv.x = mat_wrap(hit_uv.x);
    hit_uv.y = mat_wrap(hit_uv.y);
    return v2(texture.x + hit_uv.x * texture.z, texture.y + hit_uv.y * texture.w);
}
ST_D float4 sample_atlas(const KArgs& a, V2 hit_uv, float4 multiplier, float4 texture) {
    if (is_zero(texture)) return multiplier;
    return xe::mul4(multiplier, atlas_sample(a, atlas_uv(hit_uv, texture)));
}
// the normal map's texel at hit_uv; the caller has tested that `texture` is not zero
ST_D V3 sample_normal_map(const KArgs& a, V2 hit_uv, float4 texture) { return xyz(atlas_sample<false>(a, atlas_uv(hit_uv, texture))); }
#if defined(ST_FAST_MATH)
#pragma clang fp contract(fast)
#endif
// ================================================================== end of exact island (2/3)

#include "st_traverse.h"
ST_D void hit_pack(const TriangleHit& h, float4* d0, float4* d1) {  // hit.rs:112-120
    *d0 = f4(h.point, b2f(h.material_id));
    const V2 n = normal_encode(h.normal);
    *d1 = make_float4(n.x, n.y, h.uv.x, h.uv.y);
}
ST_D TriangleHit hit_unpack(float4 d0, float4 d1) {  // hit.rs:95-110
    TriangleHit h;
    h.xform_slot = 0u;
    if (is_zero(xyz(d0))) { h.distance = kF32Max; h.point = v3s(0.0f); h.normal = v3s(0.0f); h.uv = v2(0.0f, 0.0f); h.material_id = 0u; return h; }
    h.distance = 0.0f; h.point = xyz(d0); h.normal = normal_decode(v2(d1.x, d1.y)); h.uv = v2(d1.z, d1.w); h.material_id = f2b(d0.w);
    return h;
}

// ------------------------------------------------------------------ G-buffer, surface, hit (gbuffer.rs, surface.rs, hit.rs)
struct GBuffer { float4 base_color; V3 normal; float metallic; V3 emissive; float roughness, reflectance, depth; };
ST_D GBuffer gbuffer_zero() { GBuffer g; g.base_color = f4z(); g.normal = v3s(0.0f); g.metallic = 0.0f; g.emissive = v3s(0.0f); g.roughness = 0.0f; g.reflectance = 0.0f; g.depth = 0.0f; return g; }
ST_D GBuffer gbuffer_unpack(const KArgs& a, float4 d0, float4 d1) {
    GBuffer g;
    g.depth = d0.x;
    g.normal = normal_decode(v2(d0.y, d0.z));
    const uint32_t w0 = f2b(d0.w);
    g.metallic = unorm8(a, w0 & 0xffu);
    g.roughness = sqr(unorm8(a, (w0 >> 8) & 0xffu));
    g.reflectance = unorm8(a, (w0 >> 16) & 0xffu);
    g.emissive = xyz(d1);
    const uint32_t w1 = f2b(d1.w);
    const float* lut = a.byte_luts;
    g.base_color = make_float4(lut[kLutGamma8 + (w1 & 0xffu)], lut[kLutGamma8 + ((w1 >> 8) & 0xffu)], lut[kLutGamma8 + ((w1 >> 16) & 0xffu)],
                               lut[kLutGamma6 + ((w1 >> 24) & 0xffu)]);
    return g;
}
// gbuffer.rs:19-50. The base colour's four gamma-encoded bytes (4 pow_ = ~320 VALU operations) depend only on the colour;
// for a material without a base-colour texture that is a per-material constant, which the host packs once with this very
// routine (gbuffer_pack_base_color, st_math.h; KArgs::material_base_packed) and primary visibility / GI sampling pass in
// through `base_bits`.
ST_D void gbuffer_pack_bits(const GBuffer& g, uint32_t base_bits, float4* d0, float4* d1) {
    const V2 n = normal_encode(g.normal);
    const float m = clampf(g.metallic, 0.0f, 1.0f) * 255.0f;
    const float r = clampf(fsqrt(g.roughness), 0.0f, 1.0f) * 255.0f;
    const float rf = clampf(g.reflectance, 0.0f, 1.0f) * 255.0f;
    *d0 = make_float4(g.depth, n.x, n.y, b2f(u32_from_bytes(f2u_sat(m), f2u_sat(r), f2u_sat(rf), 1u)));
    *d1 = make_float4(g.emissive.x, g.emissive.y, g.emissive.z, b2f(base_bits));
}
ST_D void gbuffer_pack(const GBuffer& g, float4* d0, float4* d1) { gbuffer_pack_bits(g, gbuffer_pack_base_color(g.base_color), d0, d1); }
ST_D float clamped_roughness(const GBuffer& g) { return clampf(g.roughness, 0.089f * 0.089f, 1.0f); }

struct Surface { V3 normal; float depth, roughness; };
ST_D Surface surface_from(float4 d) { Surface s; s.normal = normal_decode(v2(d.x, d.y)); s.depth = d.z; s.roughness = d.w; return s; }
ST_D Surface surface_decoded(float4 d) { Surface s; s.normal = v3(d.x, d.y, d.z); s.depth = d.w; s.roughness = 0.0f; return s; }  // from KArgs::sn
ST_D float surface_similarity(const Surface& self, const Surface& other) {  // surface.rs:21-47
    if (self.depth == 0.0f || other.depth == 0.0f) return 0.0f;
    const float d = fmax_(dot(self.normal, other.normal), 0.0f);
    const float normal_score = d <= 0.5f ? 0.0f : 2.0f * d;
    const float t = fabsf(self.depth - other.depth);
    const float depth_score = t >= 0.1f * other.depth ? 0.0f : 1.0f;
    return normal_score * depth_score;
}

struct Hit { V3 origin, dir, point; GBuffer g; };
constexpr float kNudgeOffset = 0.01f;  // hit.rs:19
ST_D Hit hit_make(const Ray& ray, const GBuffer& g) { Hit h; h.origin = ray.origin; h.dir = ray.dir; h.point = ray_at(ray, g.depth - kNudgeOffset); h.g = g; return h; }
ST_D Hit hit_zero() { Hit h; h.origin = v3s(0.0f); h.dir = v3s(0.0f); h.point = v3s(0.0f); h.g = gbuffer_zero(); return h; }
ST_D bool hit_some(const Hit& h) { return h.g.depth != 0.0f; }
ST_D Hit pixel_hit(const KArgs& a, const GpuCamera& cam, const float4* g0, const float4* g1, U2 pos) {
    return hit_make(camera_ray_shading(cam, pos), gbuffer_unpack(a, tex_read(g0, a, pos), tex_read(g1, a, pos)));
}

// ------------------------------------------------------------------ BRDFs (brdf.rs)
ST_D float ggx_distribution(float n_dot_h, float roughness) {
    const float a2 = roughness * roughness;
    const float d = (n_dot_h * a2 - n_dot_h) * n_dot_h + 1.0f;
    return fdiv(a2, kPi * d * d);
}
ST_D float ggx_schlick_masking_term(float n_dot_l, float n_dot_v, float roughness) {
    const float k = roughness * roughness / 2.0f;
    const float g_v = fdiv(n_dot_v, n_dot_v * (1.0f - k) + k);
    const float g_l = fdiv(n_dot_l, n_dot_l * (1.0f - k) + k);
    return g_v * g_l;
}
ST_D V3 ggx_schlick_fresnel(V3 f0, float l_dot_h) {
    const float f90 = saturate(dot(f0, v3s(50.0f * 0.33f)));
    return f0 + (v3s(f90) - f0) * pow5_(fmax_(1.0f - l_dot_h, 0.001f));
}
ST_D V3 diffuse_eval(const GBuffer& g) { return divc3(xyz(g.base_color) * (1.0f - g.metallic), kPi); }
ST_D V3 specular_eval(const GBuffer& g, V3 l, V3 v) {
    if (g.metallic <= 0.0f) return v3s(0.0f);
    const float a = clamped_roughness(g);
    const V3 n = g.normal;
    const V3 h = normalize(l + v);
    const float n_dot_l = saturate(dot(n, l)), n_dot_h = saturate(dot(n, h)), l_dot_h = saturate(dot(l, h)), n_dot_v = saturate(dot(n, v));
    if (n_dot_l <= 0.0f || n_dot_v <= 0.0f) return v3s(0.0f);
    const float d = ggx_distribution(n_dot_h, a);
    const float gg = ggx_schlick_masking_term(n_dot_l, n_dot_v, a);
    const V3 f0 = v3s(0.16f * g.reflectance * g.reflectance * (1.0f - g.metallic)) + xyz(g.base_color) * g.metallic;
    const V3 f = ggx_schlick_fresnel(f0, l_dot_h);
    return d * gg * f / (4.0f * n_dot_l * n_dot_v);
}
struct BrdfSample { V3 dir; float pdf; V3 radiance; };
ST_D BrdfSample layered_brdf_sample(const GBuffer& g, WhiteNoise& wn, V3 v) {
    BrdfSample s;
    if (wn.sample() < g.metallic) {
        const float r0 = wn.sample(), r1 = wn.sample();
        const float a = clamped_roughness(g);
        const V3 n = g.normal;
        const float a2 = sqr(a);
        V3 b, t;
        any_orthonormal_pair(n, &b, &t);  // brdf.rs:91 `(b, t)`
        const float cos_theta = fsqrt(fmax_(0.0f, fdiv(1.0f - r0, (a2 - 1.0f) * r0 + 1.0f)));
        const float sin_theta = fsqrt(fmax_(0.0f, 1.0f - cos_theta * cos_theta));
        const float phi = r1 * kPi * 2.0f;
        float sp_, cp_; sincos_(phi, &sp_, &cp_);
        const V3 h = t * (sin_theta * cp_) + b * (sin_theta * sp_) + n * cos_theta;
        const float n_dot_h = saturate(dot(n, h)), h_dot_v = saturate(dot(h, v));
        s.dir = normalize(2.0f * h_dot_v * h - v);
        s.pdf = fdiv(ggx_distribution(n_dot_h, a) * n_dot_h, 4.0f * h_dot_v);
        s.radiance = specular_eval(g, s.dir, v);
        s.pdf = fdiv(s.pdf, g.metallic);
    } else {
        s.dir = wn.sample_hemisphere(g.normal);
        s.pdf = 1.0f / kPi;
        s.radiance = diffuse_eval(g);
        s.pdf = fdiv(s.pdf, 1.0f - g.metallic);
    }
    return s;
}

// ------------------------------------------------------------------ lights (light.rs)
struct LightRadiance { V3 radiance, diff_brdf, spec_brdf; };
ST_D V3 radiance_sum(const LightRadiance& r) { return r.radiance * (r.diff_brdf + r.spec_brdf); }
ST_D GpuLight light_zero() { GpuLight l; l.d0 = l.d1 = l.d2 = l.d3 = l.prev_d0 = l.prev_d1 = l.prev_d2 = f4z(); return l; }
ST_D GpuLight light_get(const KArgs& a, uint32_t id) {  // unchecked in the reference
    if (id >= a.n_lights_buf) return light_zero();
    if (a.lights_lds != nullptr && id < kLdsLights) return a.lights_lds[id];   // tracing kernels: the head of the table lives in LDS
    return a.lights[id];
}
ST_D GpuLight light_get_prev(const KArgs& a, uint32_t id) { GpuLight l = light_get(a, id); l.d0 = l.prev_d0; l.d1 = l.prev_d1; l.d2 = l.prev_d2; return l; }
ST_D bool light_is_none(const GpuLight& l) { return f2b(l.d2.x) == 0u; }
ST_D bool light_contains(const GpuLight& l, V3 p) { return distance(xyz(l.d0), p) <= l.d0.w; }

ST_D LightRadiance light_radiance(const GpuLight& l, const Hit& hit) {  // light.rs:143-207
    const V3 center = xyz(l.d0);
    const float radius = l.d0.w, range = l.d1.w;
    const V3 lv = center - hit.point;
    float f_angle;
    if (f2b(l.d2.x) == 1u) f_angle = 1.0f;
    else {
        const float angle = angle_between(normal_decode(v2(l.d2.y, l.d2.z)), hit.point - center);
        f_angle = saturate(1.0f - pow3_(fdiv(angle, l.d2.w)));
    }
    float f_dist;
    if (range == INFINITY) f_dist = 1.0f;
    else {
        const float l2 = length_squared(lv);
        const float inv_r2 = frcp(sqr(range));
        const float factor = l2 * inv_r2;
        const float smooth_factor = saturate(1.0f - factor * factor);
        const float attenuation = smooth_factor * smooth_factor;
        f_dist = fdiv(attenuation, fmax_(l2, 0.0001f));
    }
    const float f_cosine = saturate(dot(hit.g.normal, normalize(lv)));
    LightRadiance out;
    out.diff_brdf = diffuse_eval(hit.g);
    {
        const V3 v = -hit.dir;
        const V3 n = hit.g.normal;
        const V3 r = reflect(-v, n);
        const V3 center_to_ray = dot(lv, r) * r - lv;
        const float t = radius * inverse_sqrt(dot(center_to_ray, center_to_ray));
        const V3 closest_point = lv + center_to_ray * saturate(t);
        const float l_spec_length_inverse = inverse_sqrt(dot(closest_point, closest_point));
        const float tt = clamped_roughness(hit.g) + radius * 0.5f * l_spec_length_inverse;
        const float i_roughness = fdiv(clamped_roughness(hit.g), saturate(tt));
        const float intensity = sqr(i_roughness);
        const V3 ls = closest_point * l_spec_length_inverse;
        out.spec_brdf = intensity * specular_eval(hit.g, ls, v);
    }
    out.radiance = xyz(l.d1) * f_angle * f_dist * f_cosine;
    return out;
}
ST_D Ray light_ray_wnoise(const GpuLight& l, WhiteNoise& wn, V3 hit_point) {  // light.rs:209-215
    const V3 light_pos = xyz(l.d0) + l.d0.w * wn.sample_sphere();
    const V3 light_to_hit = hit_point - light_pos;
    Ray r = make_ray(light_pos, normalize(light_to_hit));
    r.len = length(light_to_hit);
    return r;
}
ST_D Ray light_ray_bnoise(const GpuLight& l, V2 sample, V3 hit_point) {  // light.rs:217-239
    const V3 to_light = xyz(l.d0) - hit_point;
    const V3 light_dir = normalize(to_light);
    const float light_distance = length(to_light);
    const float light_radius = fdiv(l.d0.w, light_distance);
    V3 lt, lb;
    any_orthonormal_pair(light_dir, &lt, &lb);
    const float angle = 2.0f * kPi * sample.x;
    const float rad = fsqrt(sample.y);
    float s_, c_; sincos_(angle, &s_, &c_);
    const V2 disk_point = v2(s_, c_) * rad * light_radius;
    V3 ray_dir = light_dir + disk_point.x * lt + disk_point.y * lb;
    ray_dir = normalize(ray_dir);
    Ray r = make_ray(hit_point + ray_dir * light_distance, -ray_dir);
    r.len = light_distance;
    return r;
}

// ------------------------------------------------------------------ atmosphere lookup (atmosphere.rs:86-205)
constexpr float kGroundRadiusMm = 6.360f, kAtmosphereRadiusMm = 6.460f, kExposure = 20.0f;
ST_D float4 lut_texel(const float4* lut, int32_t w, int32_t h, int32_t x, int32_t y) {
    x = x < 0 ? 0 : (x >= w ? w - 1 : x);
    y = y < 0 ? 0 : (y >= h ? h - 1 : y);
    return lut[y * w + x];
}
ST_D float4 lut_sample(const float4* lut, int32_t w, int32_t h, V2 uv) {
    if (uv.x != uv.x) uv.x = 0.0f;
    if (uv.y != uv.y) uv.y = 0.0f;
    const float fx = uv.x * (float)w - 0.5f, fy = uv.y * (float)h - 0.5f;
    const float x0 = floorf(fx), y0 = floorf(fy);
    const float tx = fx - x0, ty = fy - y0;
    const int32_t ix = f2i_sat(x0), iy = f2i_sat(y0);
    const float4 p00 = lut_texel(lut, w, h, ix, iy), p10 = lut_texel(lut, w, h, ix + 1, iy), p01 = lut_texel(lut, w, h, ix, iy + 1), p11 = lut_texel(lut, w, h, ix + 1, iy + 1);
    const float4 top = p00 + (p10 - p00) * tx;
    const float4 bot = p01 + (p11 - p01) * tx;
    return top + (bot - top) * ty;
}
ST_D V3 atmosphere_sample(const KArgs& a, V3 ray_dir) {
    const V3 sun_dir = v3(a.sun_dir[0], a.sun_dir[1], a.sun_dir[2]);
    const V3 view_pos = v3(0.0f, kGroundRadiusMm + 0.0002f, 0.0f);
    // sample_sky_lut
    V3 lum;
    {
        const float height = length(view_pos);
        const V3 up = view_pos / height;
        float th = sqr(height) - sqr(kGroundRadiusMm);
        th = fdiv(fsqrt(th), height);
        const float horizon = acos_(clampf(th, -1.0f, 1.0f));
        const float altitude = horizon - acos_(dot(ray_dir, up));
        float azimuth;
        if (fabsf(altitude) > (0.5f * kPi - 0.0001f)) azimuth = 0.0f;
        else {
            const V3 right = cross(sun_dir, up);
            const V3 forward = cross(up, right);
            const V3 projected_dir = normalize(ray_dir - up * dot(ray_dir, up));
            const float sin_theta = dot(projected_dir, right);
            const float cos_theta = dot(projected_dir, forward);
            azimuth = atan2_(sin_theta, cos_theta) + kPi;
        }
        const float u = fdivc(azimuth, 2.0f * kPi);
        const float v = 0.5f + 0.5f * copysignf(fsqrt(fdivc(fabsf(altitude) * 2.0f, kPi)), altitude);
        lum = xyz(lut_sample(a.sky_lut, 256, 256, v2(u, v)));
    }
    // evaluate_bloom + interpolate_bloom
    V3 sun_lum;
    {
        const float sun_solid_angle = 0.53f * kPi / 180.0f;
        const float min_sun_cos_theta = cos_(sun_solid_angle);
        const float cos_theta = dot(ray_dir, sun_dir);
        if (cos_theta >= min_sun_cos_theta) sun_lum = v3s(1.0f);
        else {
            const float offset = min_sun_cos_theta - cos_theta;
            const float gaussian_bloom = exp_(-offset * 50000.0f) * 0.5f;
            const float inv_bloom = frcp(0.02f + offset * 300.0f) * 0.01f;
            sun_lum = v3s(gaussian_bloom + inv_bloom);
        }
        const V3 t = vclamp((sun_lum - v3s(0.002f)) / (v3s(1.0f) - v3s(0.002f)), v3s(0.0f), v3s(1.0f));
        sun_lum = t * t * (v3s(3.0f) - 2.0f * t);
    }
    if (length_squared(sun_lum) > 0.0f) {
        const Ray ray = make_ray(view_pos, ray_dir);
        if (intersect_sphere(ray, kGroundRadiusMm) >= 0.0f) sun_lum = v3s(0.0f);
        else {
            const float height = length(view_pos);
            const V3 up = view_pos / height;
            const float sun_cos_zenith_angle = dot(sun_dir, up);
            const float u = saturate(0.5f + 0.5f * sun_cos_zenith_angle);
            const float v = saturate(fdivc(height - kGroundRadiusMm, kAtmosphereRadiusMm - kGroundRadiusMm));
            sun_lum = sun_lum * xyz(lut_sample(a.transmittance_lut, 256, 64, v2(u, v)));
        }
    }
    lum = lum + sun_lum;
    lum = lum * kExposure;
    return lum;
}

// ------------------------------------------------------------------ environment map (include/strolle_hip.h "environment lighting")
// An equirectangular map replaces the atmosphere while KArgs::env_map is set. The world direction is rotated by -yaw about +Y (d);
// u = 0.5 + atan2(d.x, -d.z) / 2 pi, v = acos(d.y) / pi: row 0 is the zenith, the image centre looks down -Z. Bilinear at texel
// centres, wrapping in u and clamping in v, times the intensity.
constexpr float kEnvAlpha = 0.5f;  // one-sample MIS: the probability that GI's two sky sites draw from the map's importance table
ST_D V3 env_local(const KArgs& a, V3 w) { return v3(a.env_cos_yaw * w.x - a.env_sin_yaw * w.z, w.y, a.env_sin_yaw * w.x + a.env_cos_yaw * w.z); }
ST_D V3 env_world(const KArgs& a, V3 d) { return v3(a.env_cos_yaw * d.x + a.env_sin_yaw * d.z, d.y, a.env_cos_yaw * d.z - a.env_sin_yaw * d.x); }
ST_D V2 env_uv(V3 d) {
    V2 uv = v2(0.5f + atan2_(d.x, -d.z) * (0.5f / kPi), acos_(clampf(d.y, -1.0f, 1.0f)) * (1.0f / kPi));
    if (uv.x != uv.x) uv.x = 0.0f;
    if (uv.y != uv.y) uv.y = 0.0f;
    return uv;
}
ST_D V3 env_texel(const KArgs& a, int32_t x, int32_t y) {
    const int32_t w = (int32_t)a.env_w, h = (int32_t)a.env_h;
    x %= w; if (x < 0) x += w;
    y = y < 0 ? 0 : (y >= h ? h - 1 : y);
    return xyz(a.env_map[(uint32_t)y * a.env_w + (uint32_t)x]);
}
ST_D V3 env_eval(const KArgs& a, V3 dir) {
    const V2 uv = env_uv(env_local(a, dir));
    const float fx = uv.x * (float)a.env_w - 0.5f, fy = uv.y * (float)a.env_h - 0.5f;
    const float x0 = floorf(fx), y0 = floorf(fy);
    const float tx = fx - x0, ty = fy - y0;
    const int32_t ix = f2i_sat(x0), iy = f2i_sat(y0);
    const V3 p00 = env_texel(a, ix, iy), p10 = env_texel(a, ix + 1, iy), p01 = env_texel(a, ix, iy + 1), p11 = env_texel(a, ix + 1, iy + 1);
    const V3 top = p00 + (p10 - p00) * tx;
    const V3 bot = p01 + (p11 - p01) * tx;
    return (top + (bot - top) * ty) * a.env_intensity;
}
// what every ray that leaves the scene sees: the map, or the atmosphere when none is set
ST_D V3 sky_radiance(const KArgs& a, V3 dir) { return a.env_map ? env_eval(a, dir) : atmosphere_sample(a, dir); }
// Solid-angle density of env_sample: the cell's probability spread uniformly over its (u, v) rectangle, p * cells / (2 pi^2 sin theta).
// sin theta comes from d.y, which the rotation about +Y leaves as it is: env_sample and env_pdf of its direction agree.
ST_D float env_pdf_of(const KArgs& a, float p, float cos_theta) {
    const float sin_theta = fsqrt(fmax_(0.0f, 1.0f - cos_theta * cos_theta));
    if (!(sin_theta > 0.0f) || !(p > 0.0f)) return 0.0f;
    return fdiv(p * (float)(a.env_gw * a.env_gh), (2.0f * kPi * kPi) * sin_theta);
}
ST_D float env_pdf(const KArgs& a, V3 dir) {
    const V3 d = env_local(a, dir);
    const V2 uv = env_uv(d);
    const uint32_t cx = min(f2u_sat(uv.x * (float)a.env_gw), a.env_gw - 1u), cy = min(f2u_sat(uv.y * (float)a.env_gh), a.env_gh - 1u);
    return env_pdf_of(a, a.env_table[cy * a.env_gw + cx].p, d.y);
}
struct EnvSample { V3 dir; float pdf; };
// Three uniforms: u0 picks a cell of the alias table (its remainder decides against the alias), u1 and u2 place the sample across and down
// the cell, each at its full resolution. At most two dependent loads.
ST_D EnvSample env_sample(const KArgs& a, float u0, float u1, float u2) {
    const uint32_t cells = a.env_gw * a.env_gh;
    const float x = u0 * (float)cells;
    uint32_t i = min(f2u_sat(x), cells - 1u);
    const EnvCell c = a.env_table[i];
    float p = c.p;
    if (!(x - (float)i < c.q)) { i = c.alias; p = a.env_table[i].p; }
    const uint32_t cy = i / a.env_gw, cx = i - cy * a.env_gw;
    const float u = fdiv((float)cx + u1, (float)a.env_gw), v = fdiv((float)cy + u2, (float)a.env_gh);
    float st_, ct_, sp_, cp_;
    sincos_(v * kPi, &st_, &ct_);
    sincos_((u - 0.5f) * (2.0f * kPi), &sp_, &cp_);
    st_ = fsqrt(fmax_(0.0f, 1.0f - ct_ * ct_));
    EnvSample s;
    s.dir = env_world(a, v3(st_ * sp_, ct_, -st_ * cp_));
    s.pdf = env_pdf_of(a, p, ct_);
    return s;
}

// ------------------------------------------------------------------ reprojection (reprojection.rs, utils/bilinear_filter.rs)
struct Reprojection { float prev_x, prev_y, confidence; uint32_t validity; };
ST_D Reprojection reprojection_read(float4 d) { Reprojection r; r.prev_x = d.x; r.prev_y = d.y; r.confidence = d.z; r.validity = f2b(d.w); return r; }
ST_D U2 reprojection_prev_round(const Reprojection& r) { return as_u2(round2(v2(r.prev_x, r.prev_y))); }
ST_D bool reprojection_is_exact(const Reprojection& r) {
    const float fx = r.prev_x - floorf(r.prev_x), fy = r.prev_y - floorf(r.prev_y);  // glam Vec2::fract
    return (fx * fx + fy * fy) == 0.0f;
}
ST_D float4 bilinear_reproject(const KArgs& a, const Reprojection& r, const float4* plane) {
    if (reprojection_is_exact(r)) return tex_read(plane, a, reprojection_prev_round(r));
    const float fl_x = floorf(r.prev_x), fl_y = floorf(r.prev_y), ce_x = ceilf(r.prev_x), ce_y = ceilf(r.prev_y);
    const I2 p[4] = {i2(f2i_sat(fl_x), f2i_sat(fl_y)), i2(f2i_sat(ce_x), f2i_sat(fl_y)), i2(f2i_sat(fl_x), f2i_sat(ce_y)), i2(f2i_sat(ce_x), f2i_sat(ce_y))};
    float4 s[4]; float w[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        s[i] = f4z(); w[i] = 0.0f;
        if ((r.validity & (1u << i)) > 0u && p[i].x >= 0 && p[i].y >= 0) { s[i] = tex_read(plane, a, u2((uint32_t)p[i].x, (uint32_t)p[i].y)); w[i] = 1.0f; }
    }
    const float ux = r.prev_x - truncf(r.prev_x), uy = r.prev_y - truncf(r.prev_y);  // f32::fract
    const float4 weights = make_float4(w[0], w[1], w[2], w[3]) * make_float4((1.0f - ux) * (1.0f - uy), ux * (1.0f - uy), (1.0f - ux) * uy, ux * uy);
    const float w_sum = (weights.x * 1.0f) + (weights.y * 1.0f) + (weights.z * 1.0f) + (weights.w * 1.0f);
    if (w_sum == 0.0f) return f4z();
    return div4(s[0] * weights.x + s[1] * weights.y + s[2] * weights.z + s[3] * weights.w, w_sum);
}
// Two planes at once (the denoiser's colour and moment history share the reprojection): the taps of both are in flight together — one
// round trip instead of two — and each plane's arithmetic is bilinear_reproject's, operation for operation.
ST_D void bilinear_reproject2(const KArgs& a, const Reprojection& r, const float4* plane_a, const float4* plane_b, float4* out_a, float4* out_b) {
    if (reprojection_is_exact(r)) { const U2 q = reprojection_prev_round(r); *out_a = tex_read(plane_a, a, q); *out_b = tex_read(plane_b, a, q); return; }
    const float fl_x = floorf(r.prev_x), fl_y = floorf(r.prev_y), ce_x = ceilf(r.prev_x), ce_y = ceilf(r.prev_y);
    const I2 p[4] = {i2(f2i_sat(fl_x), f2i_sat(fl_y)), i2(f2i_sat(ce_x), f2i_sat(fl_y)), i2(f2i_sat(fl_x), f2i_sat(ce_y)), i2(f2i_sat(ce_x), f2i_sat(ce_y))};
    float4 sa[4], sb[4]; float w[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        sa[i] = f4z(); sb[i] = f4z(); w[i] = 0.0f;
        if ((r.validity & (1u << i)) > 0u && p[i].x >= 0 && p[i].y >= 0) {
            const U2 q = u2((uint32_t)p[i].x, (uint32_t)p[i].y);
            sa[i] = tex_read(plane_a, a, q); sb[i] = tex_read(plane_b, a, q); w[i] = 1.0f;
        }
    }
    const float ux = r.prev_x - truncf(r.prev_x), uy = r.prev_y - truncf(r.prev_y);  // f32::fract
    const float4 weights = make_float4(w[0], w[1], w[2], w[3]) * make_float4((1.0f - ux) * (1.0f - uy), ux * (1.0f - uy), (1.0f - ux) * uy, ux * uy);
    const float w_sum = (weights.x * 1.0f) + (weights.y * 1.0f) + (weights.z * 1.0f) + (weights.w * 1.0f);
    if (w_sum == 0.0f) { *out_a = f4z(); *out_b = f4z(); return; }
    *out_a = div4(sa[0] * weights.x + sa[1] * weights.y + sa[2] * weights.z + sa[3] * weights.w, w_sum);
    *out_b = div4(sb[0] * weights.x + sb[1] * weights.y + sb[2] * weights.z + sb[3] * weights.w, w_sum);
}

// ------------------------------------------------------------------ reservoirs (reservoir.rs, reservoir/*.rs)
struct DiSample { float pdf, confidence; uint32_t light_id; V3 light_point; bool is_occluded; };
struct DiReservoir { DiSample s; float m, w; };
ST_D DiReservoir di_empty() { DiReservoir r; r.s.pdf = 0.0f; r.s.confidence = 0.0f; r.s.light_id = 0u; r.s.light_point = v3s(0.0f); r.s.is_occluded = false; r.m = 0.0f; r.w = 0.0f; return r; }
// reservoir/di.rs:17-59: two texels per pixel
ST_D DiReservoir di_unpack(float4 d0, float4 d1) {
    const uint32_t w = f2b(d0.w);
    DiReservoir r;
    r.s.pdf = d0.z; r.s.confidence = (float)((w >> 8) & 0xffu); r.s.light_id = f2b(d1.w); r.s.light_point = xyz(d1); r.s.is_occluded = (w & 0xffu) > 0u;
    r.m = d0.x; r.w = d0.y;
    return r;
}
ST_D void di_pack(const DiReservoir& r, float4* d0, float4* d1) {
    *d0 = make_float4(r.m, r.w, r.s.pdf, b2f(u32_from_bytes(r.s.is_occluded ? 1u : 0u, f2u_sat(r.s.confidence), 0u, 0u)));
    *d1 = f4(r.s.light_point, b2f(r.s.light_id));
}
ST_D DiReservoir di_read(const float4* buf, uint32_t id, uint32_t count) {
    if (id >= count) return di_empty();
    return di_unpack(buf[2u * id], buf[2u * id + 1u]);
}
ST_D void di_write(float4* buf, uint32_t id, const DiReservoir& r) { di_pack(r, &buf[2u * id], &buf[2u * id + 1u]); }
// what di_read() returns for a reservoir di_write() just stored (the confidence passes through a byte)
ST_D DiReservoir di_after_store(const DiReservoir& r) { float4 d0, d1; di_pack(r, &d0, &d1); return di_unpack(d0, d1); }
ST_D float di_pdf_ex(const DiSample& s, const GpuLight& l, Hit hit) {  // reservoir/di.rs:105-116
    hit.g.base_color = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
    if (!light_is_none(l) && light_contains(l, s.light_point)) return luma(radiance_sum(light_radiance(l, hit)));
    return 0.0f;
}
ST_D Ray di_sample_ray(const DiSample& s, V3 hit_point) {
    const V3 dir = hit_point - s.light_point;
    Ray r = make_ray(s.light_point, normalize(dir));
    r.len = length(dir);
    return r;
}

struct GiSample { float pdf; uint32_t rng; V3 radiance, v1_point, v2_point, v2_normal; };
struct GiReservoir { GiSample s; float m, w, confidence; };
ST_D GiReservoir gi_empty() { GiReservoir r; r.s.pdf = 0.0f; r.s.rng = 0u; r.s.radiance = r.s.v1_point = r.s.v2_point = r.s.v2_normal = v3s(0.0f); r.m = 0.0f; r.w = 0.0f; r.confidence = 0.0f; return r; }
ST_D GiReservoir gi_from_texels(float4 d0, float4 d1, float4 d2, float4 d3) {
    GiReservoir r;
    r.s.pdf = d2.w; r.s.rng = f2b(d3.w); r.s.radiance = xyz(d0); r.s.v1_point = xyz(d1); r.s.v2_point = xyz(d2); r.s.v2_normal = normal_decode(v2(d3.x, d3.y));
    r.m = d0.w; r.w = d1.w; r.confidence = d3.z;
    return r;
}
ST_D GiReservoir gi_read(const float4* buf, uint32_t id, uint32_t count) {
    if (id >= count) return gi_empty();
    return gi_from_texels(buf[4u * id], buf[4u * id + 1u], buf[4u * id + 2u], buf[4u * id + 3u]);
}
ST_D void gi_write(float4* buf, uint32_t id, const GiReservoir& r) {
    buf[4u * id] = f4(r.s.radiance, r.m);
    buf[4u * id + 1u] = f4(r.s.v1_point, r.w);
    buf[4u * id + 2u] = f4(r.s.v2_point, r.s.pdf);
    const V2 n = normal_encode(r.s.v2_normal);
    buf[4u * id + 3u] = make_float4(n.x, n.y, r.confidence, b2f(r.s.rng));
}
// what gi_read() returns for a reservoir gi_write() just stored: every field is kept bit for bit except the normal, which
// passes through the octahedral code
ST_D GiReservoir gi_after_store(GiReservoir r) { r.s.v2_normal = normal_decode(normal_encode(r.s.v2_normal)); return r; }
// ---- quad-transposed reservoir I/O
// A GI reservoir is a 64-B record (four float4). gi_read / gi_write move it with four instructions whose lanes are 64 B
// apart: every instruction touches a quarter of every cache line the wave covers. Measured (tools/fetch_calib.hip,
// calib_aos64_*): a 1080p plane of such records copies at 4.1 TB/s that way and at 5.5 TB/s when the four lanes of a quad
// move one whole record per instruction (64 contiguous bytes per quad) — the same bytes, 25 % less time. So where a kernel
// streams its OWN pixel's reservoir (consecutive lanes of a quad = consecutive pixels of a row = consecutive records), the
// quad loads record k with instruction k and a 4x4 transpose across the quad (two rounds of quad_perm DPP moves — no LDS)
// hands every lane its own record; stores do the inverse. All four lanes must take part: the helpers check with a ballot
// that the whole quad is executing the call with a real pixel (`valid`) and fall back to the per-lane form otherwise
// (image edges, divergent callers), so they are safe anywhere and fast where the quad is convergent.
ST_D bool quad_all(bool p) { const unsigned long long b = __ballot(p); return ((b >> (threadIdx.x & 60u)) & 0xFull) == 0xFull; }
ST_D bool quad_any(bool p) { const unsigned long long b = __ballot(p); return ((b >> (threadIdx.x & 60u)) & 0xFull) != 0ull; }
// component-wise select (`c ? a : b` on the vector class can be lowered as a select of two stack addresses -> scratch)
ST_D float4 sel4(bool c, float4 a, float4 b) { return make_float4(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z, c ? a.w : b.w); }
template <int CTRL>
ST_D float4 quad_dpp(float4 v) {
    float4 r;
    r.x = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v.x), CTRL, 0xf, 0xf, true));
    r.y = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v.y), CTRL, 0xf, 0xf, true));
    r.z = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v.z), CTRL, 0xf, 0xf, true));
    r.w = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v.w), CTRL, 0xf, 0xf, true));
    return r;
}
// v[k] in quad lane j holds M[k][j]; afterwards it holds M[j][k]
ST_D void quad_transpose(float4& v0, float4& v1, float4& v2, float4& v3) {
    const bool b0 = (threadIdx.x & 1u) != 0u, b1 = (threadIdx.x & 2u) != 0u;
    {   // lanes j and j ^ 1 (quad_perm [1,0,3,2] = 0xB1): 2x2 blocks of rows (0,1) and (2,3)
        const float4 ra = quad_dpp<0xB1>(sel4(b0, v0, v1)), rb = quad_dpp<0xB1>(sel4(b0, v2, v3));
        if (b0) { v0 = ra; v2 = rb; } else { v1 = ra; v3 = rb; }
    }
    {   // lanes j and j ^ 2 (quad_perm [2,3,0,1] = 0x4E): rows (0,2) and (1,3)
        const float4 ra = quad_dpp<0x4E>(sel4(b1, v0, v2)), rb = quad_dpp<0x4E>(sel4(b1, v1, v3));
        if (b1) { v0 = ra; v1 = rb; } else { v2 = ra; v3 = rb; }
    }
}
// The reservoir of this lane's own pixel. `valid`: `id` is a pixel of this launch (lanes of a quad then hold consecutive
// ids); `want`: this lane needs the record (a lane that does not still helps move its neighbours').
ST_D GiReservoir gi_read_own(const float4* buf, uint32_t id, bool valid, bool want) {
    want = want && valid;
    if (quad_all(valid)) {
        if (!quad_any(want)) return gi_empty();
        const uint32_t j = threadIdx.x & 3u, first = id - j;
        float4 v0 = buf[4u * first + j], v1 = buf[4u * (first + 1u) + j], v2 = buf[4u * (first + 2u) + j], v3 = buf[4u * (first + 3u) + j];
        quad_transpose(v0, v1, v2, v3);
        return want ? gi_from_texels(v0, v1, v2, v3) : gi_empty();
    }
    if (!want) return gi_empty();
    return gi_from_texels(buf[4u * id], buf[4u * id + 1u], buf[4u * id + 2u], buf[4u * id + 3u]);
}
ST_D void gi_write_own(float4* buf, uint32_t id, const GiReservoir& r, bool valid, bool want) {
    want = want && valid;
    const V2 n = normal_encode(r.s.v2_normal);
    float4 v0 = f4(r.s.radiance, r.m), v1 = f4(r.s.v1_point, r.w), v2 = f4(r.s.v2_point, r.s.pdf), v3 = make_float4(n.x, n.y, r.confidence, b2f(r.s.rng));
    if (quad_all(want)) {
        const uint32_t j = threadIdx.x & 3u, first = id - j;
        quad_transpose(v0, v1, v2, v3);
        buf[4u * first + j] = v0; buf[4u * (first + 1u) + j] = v1; buf[4u * (first + 2u) + j] = v2; buf[4u * (first + 3u) + j] = v3;
        return;
    }
    if (!want) return;
    buf[4u * id] = v0; buf[4u * id + 1u] = v1; buf[4u * id + 2u] = v2; buf[4u * id + 3u] = v3;
}
// ---- quad-cooperative gathers: ANY record per lane (spatial-neighbour reservoirs)
// A lane that fetches a neighbour's 64-B reservoir with gi_read issues four 16-B loads, and across the wave every one of them
// lands on 64 different 64-B segments: the texture-address unit serialises them (tools/tap_probe.hip: 64-B records read per
// lane 127-158 us, a whole record per quad and instruction 99 us; k_gi_spatial_fused shows the far a-trous kernel's
// signature in the SQ counters — 42 % of its waves' life stalled at issue). Here the four lanes of a quad fetch ONE lane's
// record per instruction — 64 contiguous bytes, one segment — for each lane of the quad that wants one (the record index is
// broadcast with a DPP move; quads in which no lane wants that round skip it), and the 4x4 transpose of quad_transpose
// hands every lane its own record. Pure data movement: same bytes, same values. The call must be made by all four lanes
// of a quad together (`want` says who needs a record); where the quad is not whole — divergent callers, image edges —
// the helper falls back to gi_read, so it is safe anywhere.
template <int CTRL>
ST_D uint32_t quad_dpp_u(uint32_t v) { return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xf, 0xf, true); }
#ifdef ST_NO_COOP_GATHER  // A/B (tools/ab_bench.sh): every gather takes the per-lane fallback
ST_D bool quad_whole() { return false; }
#else
ST_D bool quad_whole() { const unsigned long long b = __ballot(true); return ((b >> (threadIdx.x & 60u)) & 0xFull) == 0xFull; }
#endif
ST_D GiReservoir gi_read_coop(const float4* buf, uint32_t id, uint32_t count, bool want) {
    want = want && id < count;
    if (!quad_whole()) return want ? gi_read(buf, id, count) : gi_empty();
    const uint32_t j = threadIdx.x & 3u;
    const uint32_t w = want ? 1u : 0u;
    float4 v0 = f4z(), v1 = f4z(), v2 = f4z(), v3 = f4z();
    if (quad_dpp_u<0x00>(w)) v0 = buf[4u * quad_dpp_u<0x00>(id) + j];   // lane 0's record: the quad's lanes take its four texels
    if (quad_dpp_u<0x55>(w)) v1 = buf[4u * quad_dpp_u<0x55>(id) + j];
    if (quad_dpp_u<0xAA>(w)) v2 = buf[4u * quad_dpp_u<0xAA>(id) + j];
    if (quad_dpp_u<0xFF>(w)) v3 = buf[4u * quad_dpp_u<0xFF>(id) + j];
    quad_transpose(v0, v1, v2, v3);
    return want ? gi_from_texels(v0, v1, v2, v3) : gi_empty();
}
// the inverse: every lane with `want` stores its record at its own index, one whole record per quad and instruction
ST_D void gi_write_coop(float4* buf, uint32_t id, const GiReservoir& r, bool want) {
    if (!quad_whole()) { if (want) gi_write(buf, id, r); return; }
    const V2 n = normal_encode(r.s.v2_normal);
    float4 v0 = f4(r.s.radiance, r.m), v1 = f4(r.s.v1_point, r.w), v2 = f4(r.s.v2_point, r.s.pdf), v3 = make_float4(n.x, n.y, r.confidence, b2f(r.s.rng));
    quad_transpose(v0, v1, v2, v3);   // lane j now holds texel j of lane k's record in v<k>
    const uint32_t j = threadIdx.x & 3u;
    const uint32_t w = want ? 1u : 0u;
    if (quad_dpp_u<0x00>(w)) buf[4u * quad_dpp_u<0x00>(id) + j] = v0;
    if (quad_dpp_u<0x55>(w)) buf[4u * quad_dpp_u<0x55>(id) + j] = v1;
    if (quad_dpp_u<0xAA>(w)) buf[4u * quad_dpp_u<0xAA>(id) + j] = v2;
    if (quad_dpp_u<0xFF>(w)) buf[4u * quad_dpp_u<0xFF>(id) + j] = v3;
}
// The same for 32-B records (two float4: a DI reservoir, a path tracer hit): the quad's four records are eight consecutive
// texels; instruction k moves texels 4k..4k+3 (64 contiguous bytes per quad), and lane j wants texels 2j and 2j+1 = lanes
// (2j mod 4), (2j+1 mod 4) of instruction j / 2 — two quad_perm moves per register and a select. `ok` is false (and the
// texels zero) for a lane that does not want its record. (Returned by value: output pointers ended up in scratch memory.)
struct Rec2 { float4 d0, d1; bool ok; };
ST_D Rec2 rec2_read_own(const float4* buf, uint32_t id, bool valid, bool want) {
    want = want && valid;
    Rec2 r; r.d0 = f4z(); r.d1 = f4z(); r.ok = false;
    if (quad_all(valid)) {
        if (!quad_any(want)) return r;
        const uint32_t j = threadIdx.x & 3u, first = id - j;
        const float4 v0 = buf[2u * first + j], v1 = buf[2u * first + 4u + j];
        const bool hi = j >= 2u;
        const float4 e0 = quad_dpp<0x88>(v0), e1 = quad_dpp<0x88>(v1);  // quad_perm [0,2,0,2]
        const float4 o0 = quad_dpp<0xDD>(v0), o1 = quad_dpp<0xDD>(v1);  // quad_perm [1,3,1,3]
        if (want) { r.d0 = sel4(hi, e1, e0); r.d1 = sel4(hi, o1, o0); r.ok = true; }
        return r;
    }
    if (!want) return r;
    r.d0 = buf[2u * id]; r.d1 = buf[2u * id + 1u]; r.ok = true;
    return r;
}
ST_D void rec2_write_own(float4* buf, uint32_t id, float4 d0, float4 d1, bool valid, bool want) {
    want = want && valid;
    if (quad_all(want)) {
        // lane j holds texels 2j, 2j+1 of the quad's eight; instruction k stores texel 4k + j: texel t lives in lane t / 2,
        // register t % 2, so instruction 0 takes lanes [0,0,1,1] and instruction 1 lanes [2,2,3,3], even lanes d0, odd lanes d1
        const uint32_t j = threadIdx.x & 3u, first = id - j;
        const bool odd = (j & 1u) != 0u;
        const float4 a0 = quad_dpp<0x50>(d0), a1 = quad_dpp<0x50>(d1);  // quad_perm [0,0,1,1]
        const float4 b0 = quad_dpp<0xFA>(d0), b1 = quad_dpp<0xFA>(d1);  // quad_perm [2,2,3,3]
        buf[2u * first + j] = sel4(odd, a1, a0);
        buf[2u * first + 4u + j] = sel4(odd, b1, b0);
        return;
    }
    if (!want) return;
    buf[2u * id] = d0; buf[2u * id + 1u] = d1;
}
// (Measured and not used for the DI reservoirs: same-box A/B of the Cornell frame 1.062 ms with these accessors in DI
// resolving and DI sampling + temporal against 1.053 ms without — 32-B records are half-line accesses already, and both
// kernels are bound by VALU issue, to which the ballots and DPP moves add. The 64-B GI reservoirs gain 25 %.)
ST_D bool gi_exists(const GiSample& s) { return !is_zero(s.v2_point); }
ST_D V3 gi_dir(const GiSample& s, V3 p) { return normalize(s.v2_point - p); }
ST_D float gi_cosine(const GiSample& s, const Hit& hit) { return fmax_(dot(gi_dir(s, hit.point), hit.g.normal), 0.0f); }
ST_D V3 gi_spec_brdf(const GiSample& s, const Hit& hit) { return specular_eval(hit.g, gi_dir(s, hit.point), -hit.dir); }
ST_D float gi_pdf(const GiSample& s, Hit hit) {  // reservoir/gi.rs:98-112
    if (!gi_exists(s)) return 0.0f;
    hit.g.base_color = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
    const float d = luma(diffuse_eval(hit.g));
    const float sp = luma(gi_spec_brdf(s, hit));
    return luma(s.radiance) * gi_cosine(s, hit) * (d + sp);
}
ST_D Ray gi_sample_ray(const GiSample& s, V3 hit_point) {
    Ray r = make_ray(hit_point, gi_dir(s, hit_point));
    r.len = distance(s.v2_point, hit_point) - 0.01f;
    return r;
}
ST_D void gi_partial_jacobian(const GiSample& s, V3 hit_point, float* dist, float* cosv) {
    const V3 vec = hit_point - s.v2_point;
    *dist = length(vec);
    *cosv = saturate(dot(s.v2_normal, vec / *dist));
}
ST_D float gi_jacobian(const GiSample& s, V3 new_hit_point) {
    if (!gi_exists(s)) return 1.0f;
    float nd, nc, od, oc;
    gi_partial_jacobian(s, new_hit_point, &nd, &nc);
    gi_partial_jacobian(s, s.v1_point, &od, &oc);
    const float x = nc * od * od, y = oc * nd * nd;
    return y == 0.0f ? 0.0f : fdiv(x, y);
}

// Reservoir<T>::update / merge / norm as free templates (reservoir.rs:24-79)
template <class R, class S>
ST_D bool res_update(R& r, WhiteNoise& wn, const S& sample, float weight) {
    r.m += 1.0f; r.w += weight;
    if (wn.sample() * r.w < weight) { r.s = sample; return true; }
    return false;
}
template <class R>
ST_D bool res_merge(R& r, WhiteNoise& wn, const R& other, float pdf) {
    if (other.m <= 0.0f) return false;
    r.m += other.m - 1.0f;
    return res_update(r, wn, other.s, other.w * other.m * pdf);
}
template <class R>
ST_D void res_norm(R& r, float pdf, float num, float denom_) { const float denom = pdf * denom_; r.w = denom == 0.0f ? 0.0f : fdiv(r.w * num, denom); }

// EphemeralReservoir::build (reservoir/ephemeral.rs:14-55): RIS over min(16, light_count) uniformly picked lights
struct EphemeralResult { uint32_t light_id; LightRadiance light_rad; float m, w; };
ST_D EphemeralResult ephemeral_build(const KArgs& a, WhiteNoise& wn, const Hit& hit) {
    EphemeralResult res; res.light_id = 0u; res.light_rad.radiance = res.light_rad.diff_brdf = res.light_rad.spec_brdf = v3s(0.0f); res.m = 0.0f; res.w = 0.0f;
    float res_pdf = 0.0f;
    const uint32_t max_samples = a.light_count < 16u ? a.light_count : 16u;
    const float sample_ipdf = (float)a.light_count;
    for (uint32_t nth = 0; nth < max_samples; nth++) {
        const uint32_t light_id = wn.sample_int() % a.light_count;
        const LightRadiance rad = light_radiance(light_get(a, light_id), hit);
        const float sample_pdf = fsqrt(luma(rad.radiance));  // perc_luma
        const float weight = sample_pdf * sample_ipdf;
        res.m += 1.0f; res.w += weight;
        if (wn.sample() * res.w < weight) { res.light_id = light_id; res.light_rad = rad; res_pdf = sample_pdf; }
    }
    { const float denom = res_pdf * res.m; res.w = denom == 0.0f ? 0.0f : fdiv(res.w * 1.0f, denom); }  // norm_avg
    return res;
}

// defensive pairwise MIS (reservoir/mis.rs:96-144)
struct Mis { float lhs_m, rhs_m, rhs_jacobian, lhs_lhs_pdf, lhs_rhs_pdf, rhs_lhs_pdf, rhs_rhs_pdf; };
struct MisResult { float m, lhs_pdf, lhs_mis, rhs_pdf, rhs_mis; };
ST_D float mis2(float x, float y) { const float sum = x + y; return sum == 0.0f ? 0.0f : fdiv(x, sum); }
ST_D float mis_mfac(float q0, float q1) { return q0 <= 0.0f ? 1.0f : saturate(pow8_(fmin_(fdiv(q1, q0), 1.0f))); }
ST_D MisResult mis_eval(const Mis& s) {
    MisResult r;
    r.m = s.rhs_m * fmin_(mis_mfac(s.rhs_rhs_pdf, s.rhs_lhs_pdf), mis_mfac(s.lhs_rhs_pdf, s.lhs_lhs_pdf));
    const float t = mis2(s.lhs_m, s.rhs_m);
    r.lhs_mis = t + (1.0f - t) * mis2(s.lhs_m * s.lhs_lhs_pdf, s.rhs_m * s.lhs_rhs_pdf);
    r.rhs_mis = (1.0f - t) * mis2(s.rhs_m * s.rhs_rhs_pdf * s.rhs_jacobian, s.lhs_m * s.rhs_lhs_pdf);
    r.lhs_pdf = s.lhs_lhs_pdf; r.rhs_pdf = s.rhs_lhs_pdf;
    return r;
}

}  // namespace st
