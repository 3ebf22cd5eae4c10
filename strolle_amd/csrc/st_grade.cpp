// st_grade.cpp — colour grading (include/strolle_hip.h "colour grading"): the setter's checks, the host constants (the white-balance matrix,
// the LOG2 domain's reciprocal range, which steps run), the one launch (k_grade.hip) that st_render_camera and st_color_grading_process
// share, the look-up-table store (edits wait for the tick; a table leaves behind the frames that read it) and st_decode_cube. The
// camera's HDR plane: st_engine.h CameraState::grade. The node needs no scratch: the stateless call allocates nothing.
#include <cmath>

#include "st_cube.h"
#include "st_engine.h"

namespace st {

static_assert(KS_COUNT <= ST_PROFILE_MAX_KERNELS, "st_profile_read's callers size their arrays with ST_PROFILE_MAX_KERNELS");
static_assert(sizeof(StColorGradingDesc) == 96, "StColorGradingDesc is 96 B");
static_assert(offsetof(StColorGradingDesc, temperature) == 8 && offsetof(StColorGradingDesc, contrast) == 16 && offsetof(StColorGradingDesc, slope) == 24 &&
              offsetof(StColorGradingDesc, offset) == 36 && offsetof(StColorGradingDesc, power) == 48 && offsetof(StColorGradingDesc, cdl_saturation) == 60 &&
              offsetof(StColorGradingDesc, lut) == 64 && offsetof(StColorGradingDesc, lut_domain) == 72 && offsetof(StColorGradingDesc, lut_ev_min) == 76 &&
              offsetof(StColorGradingDesc, lut_strength) == 84 && offsetof(StColorGradingDesc, _pad) == 88,
              "StColorGradingDesc's fields are sixteen 4-B words, the 8-B handle at 64, six more words: no implicit padding");
static_assert(sizeof(StColorGradingPlan) == 48 && offsetof(StColorGradingPlan, white_balance) == 4 && offsetof(StColorGradingPlan, lut_inv_range) == 40, "StColorGradingPlan is 48 B");
static_assert(kGradeWhiteBalance == ST_GRADE_STEP_WHITE_BALANCE && kGradeContrast == ST_GRADE_STEP_CONTRAST && kGradeSaturation == ST_GRADE_STEP_SATURATION &&
              kGradeCdl == ST_GRADE_STEP_CDL && kGradeLut == ST_GRADE_STEP_LUT && kGradeDither == ST_GRADE_STEP_DITHER, "st_types.h restates ST_GRADE_STEP_*");

static bool within(float x, float lo, float hi) { return x >= lo && x <= hi; }   // (NaN: false)

static int check_grade(const StColorGradingDesc& d) {
    if (d.struct_size != sizeof(StColorGradingDesc)) return fail(ST_ERR_INVALID_ARGUMENT, "StColorGradingDesc.struct_size is not sizeof(StColorGradingDesc)");
    if ((d.flags & ~(uint32_t)ST_GRADE_DITHER) != 0u) return fail(ST_ERR_INVALID_ARGUMENT, "unknown colour grading flag bits");
    if (d.lut_domain > (uint32_t)ST_LUT_DOMAIN_LOG2) return fail(ST_ERR_INVALID_ARGUMENT, "unknown LUT domain");
    if (!within(d.temperature, -1.0f, 1.0f) || !within(d.tint, -1.0f, 1.0f)) return fail(ST_ERR_INVALID_ARGUMENT, "temperature and tint must be in [-1, 1]");
    if (!(d.contrast > 0.0f && d.contrast <= 4.0f)) return fail(ST_ERR_INVALID_ARGUMENT, "contrast must be in (0, 4]");
    if (!within(d.saturation, 0.0f, 4.0f) || !within(d.cdl_saturation, 0.0f, 4.0f)) return fail(ST_ERR_INVALID_ARGUMENT, "saturation and cdl_saturation must be in [0, 4]");
    for (int i = 0; i < 3; i++) {
        if (!within(d.slope[i], 0.0f, 16.0f)) return fail(ST_ERR_INVALID_ARGUMENT, "a CDL slope must be in [0, 16]");
        if (!within(d.offset[i], -1.0f, 1.0f)) return fail(ST_ERR_INVALID_ARGUMENT, "a CDL offset must be in [-1, 1]");
        if (!(d.power[i] > 0.0f && d.power[i] <= 8.0f)) return fail(ST_ERR_INVALID_ARGUMENT, "a CDL power must be in (0, 8]");
    }
    if (!within(d.lut_strength, 0.0f, 1.0f)) return fail(ST_ERR_INVALID_ARGUMENT, "lut_strength must be in [0, 1]");
    if (!finite(d.lut_ev_min) || !finite(d.lut_ev_max)) return fail(ST_ERR_INVALID_ARGUMENT, "lut_ev_min and lut_ev_max must be finite");
    if (d.lut_domain == ST_LUT_DOMAIN_LOG2) {
        if (!(d.lut_ev_min < d.lut_ev_max)) return fail(ST_ERR_INVALID_ARGUMENT, "the LOG2 domain needs lut_ev_min < lut_ev_max");
        if (d.lut_strength != 1.0f) return fail(ST_ERR_INVALID_ARGUMENT, "the LOG2 domain takes lut_strength 1: the table maps scene-referred values");
    }
    return ST_OK;
}

// The host constants, in double, each rounded to float once (the header's stage A): M = LMS2LIN diag(w1 / w2) LIN2LMS
int Engine::grade_plan(const StColorGradingDesc& d, GradePlan& out) {
    if (int rc = check_grade(d)) return rc;
    out = GradePlan{};
    if (d.temperature != 0.0f || d.tint != 0.0f) {
        static const double lin2lms[3][3] = {{0.390405, 0.549941, 0.00892632}, {0.0708416, 0.963172, 0.00135775}, {0.0231082, 0.128021, 0.936245}};
        static const double lms2lin[3][3] = {{2.85847, -1.62879, -0.0248910}, {-0.210182, 1.15820, 0.000324281}, {-0.0418120, -0.118169, 1.06867}};
        const double t = (double)d.temperature, u = (double)d.tint;
        const double x = 0.31271 - t * (t < 0.0 ? 0.1 : 0.05);
        const double y = 2.87 * x - 3.0 * x * x - 0.27509507 + 0.05 * u;
        const double X = x / y, Y = 1.0, Z = (1.0 - x - y) / y;
        const double w2[3] = {0.7328 * X + 0.4296 * Y - 0.1624 * Z, -0.7036 * X + 1.6975 * Y + 0.0061 * Z, 0.0030 * X + 0.0136 * Y + 0.9834 * Z};
        const double w1[3] = {0.949237, 1.03542, 1.08728};
        double a[3][3];   // LMS2LIN diag(k)
        for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) a[r][c] = lms2lin[r][c] * (w1[c] / w2[c]);
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) out.M[3 * r + c] = (float)((a[r][0] * lin2lms[0][c] + a[r][1] * lin2lms[1][c]) + a[r][2] * lin2lms[2][c]);
        out.steps |= kGradeWhiteBalance;
    }
    if (d.contrast != 1.0f) out.steps |= kGradeContrast;
    if (d.saturation != 1.0f) out.steps |= kGradeSaturation;
    bool cdl = d.cdl_saturation != 1.0f;
    for (int i = 0; i < 3; i++) cdl |= d.slope[i] != 1.0f || d.offset[i] != 0.0f || d.power[i] != 1.0f;
    if (cdl) out.steps |= kGradeCdl;
    if (d.lut != 0u) out.steps |= kGradeLut;
    if (d.flags & ST_GRADE_DITHER) out.steps |= kGradeDither;
    if (d.lut_domain == ST_LUT_DOMAIN_LOG2) out.inv_range = (float)(1.0 / ((double)d.lut_ev_max - (double)d.lut_ev_min));
    return ST_OK;
}

int Engine::set_grade(CameraState& c, const StColorGradingDesc* desc) {
    if (int rc = set_node(c.windowed(), c.grade, desc, check_grade)) return rc;
    c.grade.desc._pad[0] = c.grade.desc._pad[1] = 0u;
    return ST_OK;
}

// The launch's arguments over the window [row0, row1) x [col0, col1). Compulsory bytes per pixel of the window: 16 B of colour in, the
// format's bytes out (the table is shared by all pixels and stays in L2: not counted).
void Engine::grade_step(const StColorGradingDesc& d, const GradePlan& plan, const float4* lut, uint32_t lut_size, const NodeSource& src, uint32_t row0, uint32_t row1,
                        uint32_t col0, uint32_t col1, const NodeTarget& target, GradeStep& out) {
    GradeArgs& a = out.args;
    a = GradeArgs{};
    a.color = static_cast<const float4*>(src.color);
    a.width = src.w; a.height = src.h; a.row0 = row0; a.row1 = row1; a.col0 = col0; a.col1 = col1;
    apply_target(target, a);
    const bool table = lut != nullptr && lut_size >= kLutMinSide && lut_size <= kLutMaxSide;
    a.steps = table ? (plan.steps | kGradeLut) : (plan.steps & ~kGradeLut);
    a.lut = table ? lut : nullptr; a.lut_n = table ? lut_size : 0u;
    a.lut_log2 = d.lut_domain == ST_LUT_DOMAIN_LOG2 ? 1u : 0u; a.lut_blend = d.lut_strength != 1.0f ? 1u : 0u;
    for (int i = 0; i < 9; i++) a.M[i] = plan.M[i];
    a.contrast = d.contrast; a.saturation = d.saturation; a.cdl_saturation = d.cdl_saturation; a.cdl_sat_on = d.cdl_saturation != 1.0f ? 1u : 0u;
    for (int i = 0; i < 3; i++) { a.slope[i] = d.slope[i]; a.offset[i] = d.offset[i]; a.power[i] = d.power[i]; if (d.power[i] != 1.0f) a.cdl_pow |= 1u << i; }
    a.ev_min = d.lut_ev_min; a.inv_range = plan.inv_range; a.lut_strength = d.lut_strength;
    out.step = {KS_GRADE, (double)(row1 - row0) * (double)(col1 - col0) * (16.0 + format_bytes(a.format))};
}

int Engine::grade_process(const StColorGradingDesc* desc, const StDisplayDesc* display, const void* lut, uint32_t lut_size, const void* src, uint32_t w, uint32_t h, void* dst,
                          int format, hipStream_t stream) {
    if (!desc || !src || !dst) return fail(ST_ERR_INVALID_ARGUMENT, "null argument");
    if (w == 0u || h == 0u || w > kMaxImageSide || h > kMaxImageSide) return fail(ST_ERR_INVALID_ARGUMENT, "the image's sides must be in 1..16384");
    if (lut && (lut_size < kLutMinSide || lut_size > kLutMaxSide)) return fail(ST_ERR_INVALID_ARGUMENT, "the LUT's side must be in 2..65");
    GradePlan plan;
    if (int rc = grade_plan(*desc, plan)) return rc;
    NodeTarget target;
    if (int rc = process_target("st_color_grading_process", display, dst, format, target)) return rc;
    if (!has_device) return fail(ST_ERR_NO_DEVICE, "st_color_grading_process on a host-only engine");
    ST_HIP(hipSetDevice(device));
    GradeStep step;
    grade_step(*desc, plan, static_cast<const float4*>(lut), lut_size, {src, nullptr, nullptr, false, w, h}, 0u, h, 0u, w, target, step);
    L.launch_grade(step.args, stream);
    ST_HIP(hipGetLastError());
    return ST_OK;
}

// ---- the look-up-table store
int Engine::lut_insert(StHandle id, uint32_t size, const float* rgb) {
    if (!rgb) return fail(ST_ERR_INVALID_ARGUMENT, "null argument");
    if (id == 0u) return fail(ST_ERR_INVALID_ARGUMENT, "LUT id 0 means none");
    if (size < kLutMinSide || size > kLutMaxSide) return fail(ST_ERR_INVALID_ARGUMENT, "the LUT's side must be in 2..65");
    const size_t n = (size_t)size * size * size;
    LutEdit edit;
    edit.size = size; edit.texels.resize(n);
    for (size_t i = 0; i < n; i++) {
        const float* p = rgb + 3u * i;
        if (!finite(p[0]) || !finite(p[1]) || !finite(p[2])) return fail(ST_ERR_INVALID_ARGUMENT, "LUT texel " + std::to_string(i) + " is not finite");
        edit.texels[i] = make_float4(p[0], p[1], p[2], 1.0f);
    }
    lut_edits[id] = std::move(edit);
    return ST_OK;
}
int Engine::lut_remove(StHandle id) {
    lut_edits[id] = LutEdit{};
    return ST_OK;
}

// The tick's device part: each edit becomes a fresh allocation filled on the tick's stream (frames rendered behind the tick on another stream
// are ordered behind it as behind every upload); the table it replaces, or the one removed, is retired behind the frames that read it
int Engine::upload_luts(TickIo& io) {
    luts_retired.release();
    if (lut_edits.empty()) return ST_OK;
    for (auto& kv : lut_edits) {
        std::unique_ptr<Lut> fresh;
        if (kv.second.size != 0u) {
            fresh.reset(new Lut());
            fresh->size = kv.second.size;
            const size_t bytes = kv.second.texels.size() * sizeof(float4);
            if (int rc = fresh->texels.reserve(bytes, bytes)) return rc;
            if (int rc = fresh->texels.upload_range(kv.second.texels.data(), 0, bytes, io.stream, staging, &io.pageable)) return rc;
            io.uploaded = true;
        }
        auto it = luts_live.find(kv.first);
        if (it != luts_live.end()) {
            if (int rc = luts_retired.retire(std::move(it->second))) return rc;
            luts_live.erase(it);
        }
        if (fresh) luts_live[kv.first] = std::move(fresh);
    }
    if (io.pageable) { ST_HIP(hipStreamSynchronize(io.stream)); }   // (a copy straight from an edit's memory ends before the edit goes)
    lut_edits.clear();
    return ST_OK;
}

}  // namespace st

using namespace st;

extern "C" {

int st_decode_cube(const void* bytes, size_t size, float* out_rgb, size_t capacity_floats, uint32_t* lut_size) {
    if (!bytes || !lut_size) return fail(ST_ERR_INVALID_ARGUMENT, "null argument");
    CubeLut lut;
    try {
        const CubeResult r = decode_cube(static_cast<const uint8_t*>(bytes), size, &lut, out_rgb == nullptr, ST_OK, ST_ERR_PARSE, ST_ERR_UNSUPPORTED);
        if (r.status != ST_OK) return fail(r.status, r.message);
    } catch (const std::bad_alloc&) {
        return fail(ST_ERR_PARSE, "cube: out of memory while decoding");
    }
    *lut_size = lut.size;
    if (!out_rgb) return ST_OK;
    if (capacity_floats < lut.rgb.size()) return fail(ST_ERR_INVALID_ARGUMENT, "output buffer too small");
    memcpy(out_rgb, lut.rgb.data(), lut.rgb.size() * sizeof(float));
    return ST_OK;
}

}  // extern "C"
