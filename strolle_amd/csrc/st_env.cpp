// st_env.cpp — host engine of libstrolle_hip.so: environment lighting (include/strolle_hip.h "environment lighting"; k_env.hip). An edit is
// validated and stored by the call, applied by the next st_tick: on the host (the sun switch of light 0) and on the device (a fresh map,
// its luminance grid, and the alias table built here from it). Frames read the map of the tick before them through KArgs::env_*.
#include <cmath>

#include "st_engine.h"
#include "st_hdr.h"

namespace st {

// Vose's alias method over the grid's weights, in index order (the same weights give the same table). A grid with no positive finite
// weight (a black map) falls back to sin theta: the table then samples the sphere uniformly and the look-ups return 0 anyway.
static void build_alias_table(const std::vector<float>& weight, uint32_t gw, uint32_t gh, std::vector<EnvCell>& table) {
    const size_t n = weight.size();
    std::vector<double> w(n);
    double sum = 0.0;
    for (size_t i = 0; i < n; i++) { const float v = weight[i]; w[i] = (std::isfinite(v) && v > 0.0f) ? (double)v : 0.0; sum += w[i]; }
    if (!(sum > 0.0) || !std::isfinite(sum)) {
        sum = 0.0;
        for (size_t i = 0; i < n; i++) { w[i] = std::sin(M_PI * ((double)(i / gw) + 0.5) / (double)gh); sum += w[i]; }
    }
    table.assign(n, EnvCell{1.0f, 0u, 0.0f});
    std::vector<double> scaled(n);
    std::vector<uint32_t> small, large;
    for (size_t i = 0; i < n; i++) {
        table[i].p = (float)(w[i] / sum); table[i].alias = (uint32_t)i;
        scaled[i] = w[i] / sum * (double)n;
        (scaled[i] < 1.0 ? small : large).push_back((uint32_t)i);
    }
    while (!small.empty() && !large.empty()) {
        const uint32_t l = small.back(); small.pop_back();
        const uint32_t g = large.back(); large.pop_back();
        table[l].q = (float)scaled[l]; table[l].alias = g;
        scaled[g] = (scaled[g] + scaled[l]) - 1.0;
        (scaled[g] < 1.0 ? small : large).push_back(g);
    }
    for (uint32_t i : large) table[i].q = 1.0f;
    for (uint32_t i : small) table[i].q = 1.0f;   // (round-off leftovers)
}

// host part of the tick: which sky the frames after it see, and light 0's colour
void Engine::apply_environment() {
    if (env_edit.kind == ENV_EDIT_CLEAR) env_set = false;
    else if (env_edit.kind != ENV_EDIT_NONE) env_set = true;
    env_desc = env_desc_next;
    const bool sun_off = env_set && !(env_desc.flags & ST_ENV_KEEP_SUN);
    if (sun_off != env_sun_off) { env_sun_off = sun_off; sun_dirty = true; }
    if (!has_device) env_edit = EnvEdit();
}

// device part: the new map in an allocation of its own, on the tick's stream; the old one is retired behind the frames that read it
int Engine::upload_environment(TickIo& io) {
    env_retired.release();
    const EnvEditKind kind = env_edit.kind;
    if (kind == ENV_EDIT_NONE) return ST_OK;
    std::unique_ptr<EnvMap> m;
    if (kind != ENV_EDIT_CLEAR) {
        m.reset(new EnvMap());
        const uint32_t w = env_edit.w, h = env_edit.h;
        m->w = w; m->h = h; m->gw = std::min(w, 512u); m->gh = std::min(h, 256u);
        const size_t bytes = (size_t)w * h * sizeof(float4), cells = (size_t)m->gw * m->gh;
        if (int rc = m->texels.reserve(bytes, bytes)) return rc;
        if (kind == ENV_EDIT_HOST) {
            if (int rc = m->texels.upload_range(env_edit.texels.data(), 0, bytes, io.stream, staging, &io.pageable)) return rc;
        } else {
            if (!d_env_bad.ptr) { if (int rc = d_env_bad.reserve(sizeof(uint32_t), sizeof(uint32_t))) return rc; ST_HIP(hipMemset(d_env_bad.ptr, 0, sizeof(uint32_t))); }
            L.launch_env_upload(env_edit.src, env_edit.pitch, w, h, env_edit.channels, static_cast<float4*>(m->texels.ptr), d_env_bad.as<uint32_t>(), io.stream);
        }
        if (int rc = d_env_grid.reserve(cells * sizeof(float), cells * sizeof(float))) return rc;
        L.launch_env_grid(static_cast<const float4*>(m->texels.ptr), w, h, m->gw, m->gh, static_cast<float*>(d_env_grid.ptr), io.stream);
        ST_HIP(hipGetLastError());
        env_grid_host.resize(cells);
        ST_HIP(hipMemcpyAsync(env_grid_host.data(), d_env_grid.ptr, cells * sizeof(float), hipMemcpyDeviceToHost, io.stream));
        uint32_t bad = 0;
        if (kind == ENV_EDIT_DEVICE) {
            ST_HIP(hipMemcpyAsync(&bad, d_env_bad.ptr, sizeof(uint32_t), hipMemcpyDeviceToHost, io.stream));
            ST_HIP(hipMemsetAsync(d_env_bad.ptr, 0, sizeof(uint32_t), io.stream));
        }
        ST_HIP(hipStreamSynchronize(io.stream));   // maps change rarely: the table is built on the host from the device's grid
        env_sanitized += bad;
        build_alias_table(env_grid_host, m->gw, m->gh, env_table_host);
        if (int rc = m->table.reserve(cells * sizeof(EnvCell), cells * sizeof(EnvCell))) return rc;
        if (int rc = m->table.upload_range(env_table_host.data(), 0, cells * sizeof(EnvCell), io.stream, staging, &io.pageable)) return rc;
    }
    if (env_live) if (int rc = env_retired.retire(std::move(env_live))) return rc;
    env_live = std::move(m);
    env_edit = EnvEdit();   // (the host texels went to the device before the synchronisation above)
    io.uploaded = true;
    return ST_OK;
}

void Engine::environment_args(KArgs& a) const {
    if (!env_live) return;
    a.env_map = static_cast<const float4*>(env_live->texels.ptr); a.env_table = static_cast<const EnvCell*>(env_live->table.ptr);
    a.env_w = env_live->w; a.env_h = env_live->h; a.env_gw = env_live->gw; a.env_gh = env_live->gh;
    a.env_intensity = env_desc.intensity;
    a.env_cos_yaw = std::cos(env_desc.yaw); a.env_sin_yaw = std::sin(env_desc.yaw);
    a.env_uniform = (env_desc.flags & ST_ENV_UNIFORM_SAMPLING) ? 1u : 0u;
}

int Engine::environment_debug(uint32_t what, const float* in, uint32_t n, float* out, hipStream_t stream) {
    if (!has_device) return fail(ST_ERR_NO_DEVICE, "environment debug seam on a host-only engine");
    if (!env_live) return fail(ST_ERR_INVALID_ARGUMENT, "no environment map is live (st_environment_set, then st_tick)");
    if (n == 0) return ST_OK;
    if (!in || !out) return fail(ST_ERR_INVALID_ARGUMENT, "null argument");
    ST_HIP(hipSetDevice(device));
    if (int rc = copies.begin(stream, kReadsEnvironment)) return rc;   // (a reader like a frame: a seam on another stream makes the streams mixed)
    KArgs a{};
    environment_args(a);
    L.launch_env_debug(a, what, in, n, out, stream);
    ST_HIP(hipGetLastError());
    return copies.end(stream, kReadsEnvironment);
}

}  // namespace st

using namespace st;
static Engine* EE(StEngine* e) { return reinterpret_cast<Engine*>(e); }

static int check_env_desc(const StEnvironmentDesc* d) {
    if (!d) return fail(ST_ERR_INVALID_ARGUMENT, "null environment desc");
    if (d->struct_size != sizeof(StEnvironmentDesc)) return fail(ST_ERR_INVALID_ARGUMENT, "StEnvironmentDesc: wrong struct_size");
    if (d->flags & ~(uint32_t)(ST_ENV_KEEP_SUN | ST_ENV_UNIFORM_SAMPLING)) return fail(ST_ERR_INVALID_ARGUMENT, "StEnvironmentDesc: unknown flag bits");
    if (!std::isfinite(d->intensity) || d->intensity < 0.0f) return fail(ST_ERR_INVALID_ARGUMENT, "StEnvironmentDesc: intensity must be finite and >= 0");
    if (!std::isfinite(d->yaw)) return fail(ST_ERR_INVALID_ARGUMENT, "StEnvironmentDesc: yaw must be finite");
    return ST_OK;
}
static int check_env_size(uint32_t w, uint32_t h, uint32_t channels) {
    if (w < 1 || h < 1 || w > 16384 || h > 16384 || (uint64_t)w * h > (1ull << 25)) return fail(ST_ERR_INVALID_ARGUMENT, "environment map: a side outside 1..16384 or more than 2^25 texels");
    if (channels != 3 && channels != 4) return fail(ST_ERR_INVALID_ARGUMENT, "environment map: channels must be 3 or 4");
    return ST_OK;
}

extern "C" {

int st_environment_set(StEngine* e, const float* texels, uint32_t width, uint32_t height, uint32_t channels, const StEnvironmentDesc* desc) {
    if (!e || !texels) return fail(ST_ERR_INVALID_ARGUMENT, "null argument");
    if (int rc = check_env_size(width, height, channels)) return rc;
    if (int rc = check_env_desc(desc)) return rc;
    const size_t n = (size_t)width * height;
    std::vector<float4> t(n);
    for (size_t i = 0; i < n; i++) {
        const float* p = texels + i * channels;
        for (int k = 0; k < 3; k++)
            if (!std::isfinite(p[k]) || p[k] < 0.0f) return fail(ST_ERR_INVALID_ARGUMENT, "environment map: texel " + std::to_string(i) + " has a negative or non-finite channel");
        t[i] = make_float4(p[0], p[1], p[2], 0.0f);
    }
    Engine* en = EE(e);
    en->env_edit = Engine::EnvEdit();
    en->env_edit.kind = Engine::ENV_EDIT_HOST; en->env_edit.texels = std::move(t);
    en->env_edit.w = width; en->env_edit.h = height; en->env_edit.channels = channels;
    en->env_desc_next = *desc;
    return ST_OK;
}

int st_environment_set_device(StEngine* e, const void* texels, uint32_t width, uint32_t height, uint32_t channels, size_t row_pitch_bytes, const StEnvironmentDesc* desc) {
    if (!e || !texels) return fail(ST_ERR_INVALID_ARGUMENT, "null argument");
    if (int rc = check_env_size(width, height, channels)) return rc;
    if (int rc = check_env_desc(desc)) return rc;
    const size_t row = (size_t)width * channels * sizeof(float);
    const size_t pitch = row_pitch_bytes ? row_pitch_bytes : row;
    if (pitch < row || pitch % sizeof(float) != 0) return fail(ST_ERR_INVALID_ARGUMENT, "environment map: the row pitch is shorter than a row or not a multiple of 4");
    Engine* en = EE(e);
    if (!en->has_device) return fail(ST_ERR_NO_DEVICE, "st_environment_set_device on a host-only engine");
    en->env_edit = Engine::EnvEdit();
    en->env_edit.kind = Engine::ENV_EDIT_DEVICE; en->env_edit.src = texels; en->env_edit.pitch = pitch;
    en->env_edit.w = width; en->env_edit.h = height; en->env_edit.channels = channels;
    en->env_desc_next = *desc;
    return ST_OK;
}

int st_environment_update(StEngine* e, const StEnvironmentDesc* desc) {
    if (!e) return fail(ST_ERR_INVALID_ARGUMENT, "null engine");
    if (int rc = check_env_desc(desc)) return rc;
    EE(e)->env_desc_next = *desc;
    return ST_OK;
}

int st_environment_clear(StEngine* e) {
    if (!e) return fail(ST_ERR_INVALID_ARGUMENT, "null engine");
    Engine* en = EE(e);
    en->env_edit = Engine::EnvEdit();
    en->env_edit.kind = Engine::ENV_EDIT_CLEAR;
    return ST_OK;
}

int st_debug_environment_eval(StEngine* e, const float* dirs, uint32_t n, float* rgb, void* stream) {
    if (!e) return fail(ST_ERR_INVALID_ARGUMENT, "null engine");
    return EE(e)->environment_debug(0u, dirs, n, rgb, static_cast<hipStream_t>(stream));
}
int st_debug_environment_sample(StEngine* e, const float* u, uint32_t n, float* dir_pdf, void* stream) {
    if (!e) return fail(ST_ERR_INVALID_ARGUMENT, "null engine");
    return EE(e)->environment_debug(1u, u, n, dir_pdf, static_cast<hipStream_t>(stream));
}
int st_debug_environment_pdf(StEngine* e, const float* dirs, uint32_t n, float* pdf, void* stream) {
    if (!e) return fail(ST_ERR_INVALID_ARGUMENT, "null engine");
    return EE(e)->environment_debug(2u, dirs, n, pdf, static_cast<hipStream_t>(stream));
}
int st_debug_environment_sanitized(StEngine* e, uint64_t* texels) {
    if (!e || !texels) return fail(ST_ERR_INVALID_ARGUMENT, "null argument");
    if (!EE(e)->has_device) return fail(ST_ERR_NO_DEVICE, "environment debug seam on a host-only engine");
    *texels = EE(e)->env_sanitized;
    return ST_OK;
}
int st_debug_environment_table(StEngine* e, void* table, size_t capacity_bytes, uint32_t* cells_x, uint32_t* cells_y) {
    if (!e || !cells_x || !cells_y) return fail(ST_ERR_INVALID_ARGUMENT, "null argument");
    Engine* en = EE(e);
    if (!en->has_device) return fail(ST_ERR_NO_DEVICE, "environment debug seam on a host-only engine");
    if (!en->env_live) return fail(ST_ERR_INVALID_ARGUMENT, "no environment map is live (st_environment_set, then st_tick)");
    *cells_x = en->env_live->gw; *cells_y = en->env_live->gh;
    if (!table) return ST_OK;
    const size_t bytes = (size_t)en->env_live->gw * en->env_live->gh * sizeof(EnvCell);
    if (capacity_bytes < bytes) return fail(ST_ERR_INVALID_ARGUMENT, "output buffer too small");
    ST_HIP(hipSetDevice(en->device));
    ST_HIP(hipDeviceSynchronize());
    ST_HIP(hipMemcpy(table, en->env_live->table.ptr, bytes, hipMemcpyDeviceToHost));
    return ST_OK;
}

int st_decode_hdr(const void* bytes, size_t size, float* out_rgb, size_t capacity_floats, uint32_t* width, uint32_t* height) {
    if (!bytes || !width || !height) return fail(ST_ERR_INVALID_ARGUMENT, "null argument");
    HdrImage img;
    try {
        const HdrResult r = decode_hdr(static_cast<const uint8_t*>(bytes), size, &img, out_rgb == nullptr, ST_OK, ST_ERR_PARSE, ST_ERR_UNSUPPORTED);
        if (r.status != ST_OK) return fail(r.status, r.message);
    } catch (const std::bad_alloc&) {
        return fail(ST_ERR_PARSE, "hdr: out of memory while decoding");
    }
    *width = img.width; *height = img.height;
    if (!out_rgb) return ST_OK;
    if (capacity_floats < img.rgb.size()) return fail(ST_ERR_INVALID_ARGUMENT, "output buffer too small");
    memcpy(out_rgb, img.rgb.data(), img.rgb.size() * sizeof(float));
    return ST_OK;
}

}  // extern "C"
