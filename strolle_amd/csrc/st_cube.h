// st_cube.h — .cube 3-D look-up table decoder of the ingest layer (include/strolle_hip.h st_decode_cube); own code, no dependency.
// Lines end in LF or CR LF; blanks and tabs separate tokens. In front of the table: TITLE "...", # comments, blank lines, LUT_3D_SIZE N
// (2..65), DOMAIN_MIN 0 0 0, DOMAIN_MAX 1 1 1. Then exactly N^3 rows of three numbers, red fastest. LUT_1D_SIZE, another domain and any
// other keyword are "unsupported"; everything malformed is a parse error. The input need not end in a newline and is never read past `size`.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

namespace st {

struct CubeLut { uint32_t size = 0; std::vector<float> rgb; };
struct CubeResult { int status = 0; std::string message; };   // status: ST_OK, ST_ERR_PARSE or ST_ERR_UNSUPPORTED
constexpr uint32_t kLutMinSide = 2u, kLutMaxSide = 65u;

namespace cube_detail {
inline bool blank(char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\v' || c == '\f'; }
// the tokens of one line (at most `most` + 1 are kept: one more than a caller accepts tells it "too many")
inline void split(const std::string& s, size_t most, std::vector<std::string>* out) {
    out->clear();
    size_t i = 0;
    while (i < s.size() && out->size() <= most) {
        while (i < s.size() && blank(s[i])) i++;
        size_t j = i;
        while (j < s.size() && !blank(s[j])) j++;
        if (j > i) out->push_back(s.substr(i, j - i));
        i = j;
    }
}
// a whole token as a finite number
inline bool number(const std::string& t, double* v) {
    if (t.empty() || t.size() > 64u) return false;
    for (char c : t) if (!((c >= '0' && c <= '9') || c == '+' || c == '-' || c == '.' || c == 'e' || c == 'E')) return false;   // no inf, nan, hex floats
    char* end = nullptr;
    *v = std::strtod(t.c_str(), &end);
    return end == t.c_str() + t.size() && std::isfinite(*v);
}
}  // namespace cube_detail

inline CubeResult decode_cube(const uint8_t* p, size_t size, CubeLut* out, bool size_only, int ok, int err_parse, int err_unsupported) {
    using namespace cube_detail;
    size_t at = 0, rows = 0, want = 0, line_no = 0;
    std::string s;
    std::vector<std::string> tok;
    out->size = 0; out->rgb.clear();
    auto where = [&] { return " (line " + std::to_string(line_no) + ")"; };
    while (at < size) {
        s.clear();
        while (at < size && p[at] != '\n') s.push_back((char)p[at++]);
        if (at < size) at++;
        line_no++;
        split(s, 4u, &tok);
        if (tok.empty() || tok[0][0] == '#') continue;
        const std::string& k = tok[0];
        std::string low;
        for (char c : k.substr(0, 9)) low.push_back((c >= 'A' && c <= 'Z') ? (char)(c - 'A' + 'a') : c);
        const bool not_a_number = low == "nan" || low == "inf" || low == "infinity";   // a row's non-finite value, not a keyword
        const bool keyword = !not_a_number && ((k[0] >= 'A' && k[0] <= 'Z') || (k[0] >= 'a' && k[0] <= 'z') || k[0] == '_');
        if (keyword) {
            if (rows != 0) return {err_parse, "cube: a keyword inside the table" + where()};
            if (k == "TITLE") continue;
            if (k == "LUT_1D_SIZE") return {err_unsupported, "cube: a 1-D table (only LUT_3D_SIZE is read)"};
            if (k == "LUT_3D_SIZE") {
                double n = 0.0;
                if (out->size != 0 || tok.size() != 2u || !number(tok[1], &n) || n != std::floor(n)) return {err_parse, "cube: malformed or repeated LUT_3D_SIZE" + where()};
                if (n < (double)kLutMinSide || n > (double)kLutMaxSide) return {err_parse, "cube: LUT_3D_SIZE outside 2..65" + where()};
                out->size = (uint32_t)n; want = (size_t)out->size * out->size * out->size;
                continue;
            }
            if (k == "DOMAIN_MIN" || k == "DOMAIN_MAX") {
                double v[3];
                if (tok.size() != 4u || !number(tok[1], &v[0]) || !number(tok[2], &v[1]) || !number(tok[3], &v[2])) return {err_parse, "cube: malformed " + k + where()};
                const double d = k == "DOMAIN_MIN" ? 0.0 : 1.0;
                if (v[0] != d || v[1] != d || v[2] != d) return {err_unsupported, "cube: only the domain 0 0 0 .. 1 1 1 is read"};
                continue;
            }
            return {err_unsupported, "cube: unknown keyword " + k.substr(0, 32) + where()};
        }
        if (out->size == 0) return {err_parse, "cube: a table row in front of LUT_3D_SIZE" + where()};
        if (size_only) return {ok, ""};
        double v[3];
        if (tok.size() != 3u || !number(tok[0], &v[0]) || !number(tok[1], &v[1]) || !number(tok[2], &v[2])) return {err_parse, "cube: a row that is not three finite numbers" + where()};
        if (rows == want) return {err_parse, "cube: more rows than LUT_3D_SIZE^3" + where()};
        if (rows == 0) out->rgb.reserve(want * 3u);
        for (int i = 0; i < 3; i++) {
            const float f = (float)v[i];
            if (!std::isfinite(f)) return {err_parse, "cube: a value beyond float" + where()};
            out->rgb.push_back(f);
        }
        rows++;
    }
    if (out->size == 0) return {err_parse, "cube: no LUT_3D_SIZE"};
    if (size_only) return {ok, ""};
    if (rows != want) return {err_parse, "cube: " + std::to_string(rows) + " rows, LUT_3D_SIZE^3 is " + std::to_string(want)};
    return {ok, ""};
}

}  // namespace st
