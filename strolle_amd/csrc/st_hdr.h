// st_hdr.h — Radiance .hdr (RGBE) decoder of the ingest layer (include/strolle_hip.h st_decode_hdr); own code, no dependency.
// Header "#?RADIANCE" / "#?RGBE", FORMAT=32-bit_rle_rgbe, resolution "-Y H +X W"; scanlines flat or new-style run-length encoded
// ("2 2 hi lo", then each of the four channels as runs / literals). Texel = m * 2^(e - 136), e == 0 -> 0 (Ward's rgbe.c, no +0.5).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace st {

struct HdrImage { uint32_t width = 0, height = 0; std::vector<float> rgb; };
struct HdrResult { int status = 0; std::string message; };   // status: ST_OK, ST_ERR_PARSE or ST_ERR_UNSUPPORTED

inline HdrResult decode_hdr(const uint8_t* p, size_t size, HdrImage* out, bool header_only, int ok, int err_parse, int err_unsupported) {
    size_t at = 0;
    auto line = [&](std::string* s) {   // one header line without its '\n'; false at the end of the data
        s->clear();
        while (at < size && p[at] != '\n') s->push_back((char)p[at++]);
        if (at >= size) return false;
        at++;
        return true;
    };
    std::string s;
    if (!line(&s) || (s != "#?RADIANCE" && s != "#?RGBE")) return {err_parse, "hdr: the file does not start with #?RADIANCE or #?RGBE"};
    bool rgbe = false;
    for (;;) {
        if (!line(&s)) return {err_parse, "hdr: the header does not end"};
        if (s.empty()) break;
        if (s.compare(0, 7, "FORMAT=") == 0) {
            if (s == "FORMAT=32-bit_rle_rgbe") rgbe = true;
            else return {err_unsupported, "hdr: unsupported " + s + " (only 32-bit_rle_rgbe is read)"};
        }   // EXPOSURE, GAMMA, PRIMARIES, comments: ignored
    }
    if (!rgbe) return {err_unsupported, "hdr: the header names no FORMAT=32-bit_rle_rgbe"};
    if (!line(&s)) return {err_parse, "hdr: no resolution line"};
    char ay[3] = {}, ax[3] = {};
    long h = 0, w = 0;
    int used = 0;
    if (sscanf(s.c_str(), "%2s %ld %2s %ld%n", ay, &h, ax, &w, &used) != 4 || used != (int)s.size() || (ay[1] != 'Y' && ay[1] != 'X') || (ax[1] != 'X' && ax[1] != 'Y'))
        return {err_parse, "hdr: malformed resolution line \"" + s + "\""};
    if (strcmp(ay, "-Y") != 0 || strcmp(ax, "+X") != 0) return {err_unsupported, "hdr: orientation \"" + s + "\" (only -Y H +X W is read)"};
    if (w < 1 || h < 1) return {err_parse, "hdr: empty image"};
    if (w > 32768 || h > 32768 || (uint64_t)w * (uint64_t)h > (1ull << 26)) return {err_unsupported, "hdr: more than 2^26 texels or a side above 32768"};
    // the cheapest scanline: a flat one takes 4 bytes per texel, a run-length one its 4-byte header and at least one 2-byte run per channel
    // (runs hold up to 127 bytes): no allocation for pixels the file cannot hold
    const uint64_t min_line = w >= 8 ? std::min<uint64_t>(4u * (uint64_t)w, 4u + 8u * (((uint64_t)w + 126u) / 127u)) : 4u * (uint64_t)w;
    if (min_line * (uint64_t)h > (uint64_t)(size - at)) return {err_parse, "hdr: the pixel data is truncated (the resolution needs more bytes than the file has)"};
    out->width = (uint32_t)w; out->height = (uint32_t)h;
    if (header_only) return {ok, ""};
    out->rgb.assign((size_t)w * (size_t)h * 3u, 0.0f);
    std::vector<uint8_t> row((size_t)w * 4u);
    auto texel = [&](size_t i, const uint8_t* q) {
        float* d = out->rgb.data() + 3u * i;
        if (q[3] == 0) { d[0] = d[1] = d[2] = 0.0f; return; }
        const float f = std::ldexp(1.0f, (int)q[3] - 136);
        d[0] = (float)q[0] * f; d[1] = (float)q[1] * f; d[2] = (float)q[2] * f;
    };
    const char* truncated = "hdr: the pixel data is truncated";
    for (long y = 0; y < h; y++) {
        const bool rle = w >= 8 && w < 32768 && at + 4 <= size && p[at] == 2 && p[at + 1] == 2 && !(p[at + 2] & 0x80);
        if (!rle) {   // flat: four bytes per pixel; (1, 1, 1, n) would be an old-style run
            if (at + (size_t)w * 4u > size) return {err_parse, truncated};
            for (long x = 0; x < w; x++) {
                const uint8_t* q = p + at + 4u * (size_t)x;
                if (q[0] == 1 && q[1] == 1 && q[2] == 1) return {err_unsupported, "hdr: old-style run-length encoding"};
                texel((size_t)y * w + x, q);
            }
            at += (size_t)w * 4u;
            continue;
        }
        if ((((long)p[at + 2] << 8) | p[at + 3]) != w) return {err_parse, "hdr: a scanline's width disagrees with the resolution line"};
        at += 4;
        for (int c = 0; c < 4; c++) {
            long x = 0;
            while (x < w) {
                if (at >= size) return {err_parse, truncated};
                uint32_t n = p[at++];
                if (n > 128) {
                    n -= 128;
                    if (at >= size) return {err_parse, truncated};
                    if (n > (uint32_t)(w - x)) return {err_parse, "hdr: a run overruns its scanline"};
                    const uint8_t v = p[at++];
                    for (uint32_t k = 0; k < n; k++) row[4u * (size_t)(x++) + c] = v;
                } else {
                    if (n == 0 || n > (uint32_t)(w - x)) return {err_parse, "hdr: a literal overruns its scanline"};
                    if (at + n > size) return {err_parse, truncated};
                    for (uint32_t k = 0; k < n; k++) row[4u * (size_t)(x++) + c] = p[at++];
                }
            }
        }
        for (long x = 0; x < w; x++) texel((size_t)y * w + x, &row[4u * (size_t)x]);
    }
    return {ok, ""};
}

}  // namespace st
