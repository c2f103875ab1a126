// The input-layout table (layouts.hpp) and the frame plan (frame_plan.cpp): host only, no GPU and
// no HIP library.  Built plain and under AddressSanitizer + UBSan; tests/test_frame_plan_cpu.py
// runs both and reads the "ok"/"FAIL" lines.
//
// What a layout is (bytes per pixel, planes, least row, where each sample lies) is written out here
// by hand from jpge.h's wording; nothing expected is computed from the table.
#include <cstdio>
#include <cstring>
#include <vector>

#include "frame_plan.hpp"

using namespace jpge;

static int g_fail = 0;
static void report(const char* name, bool ok) {
    std::printf("%s %s\n", ok ? "ok" : "FAIL", name);
    if (!ok) ++g_fail;
}
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            if (ok) std::printf("  line %d: %s\n", __LINE__, #cond);      \
            ok = false;                                                   \
        }                                                                 \
    } while (0)

// ---- the 23 layouts, by hand ----
static uint64_t even(uint64_t w) { return (w + 1) / 2 * 2; }
struct Want {
    int fmt, bpp, planes, shape;
    uint64_t (*row)(uint64_t w);  // least bytes of a row of the first plane
    int sample_bytes;             // 1, 2, or 0 for v210's 10-bit fields
    int cx, cy;                   // chroma subsampling
};
static const Want kWant[] = {
    {0, 3, 1, 0, [](uint64_t w) { return 3 * w; }, 1, 1, 1},                 // RGB8
    {1, 3, 1, 1, [](uint64_t w) { return 3 * w; }, 1, 1, 1},                 // BGR8
    {2, 4, 1, 2, [](uint64_t w) { return 4 * w; }, 1, 1, 1},                 // RGBA8
    {3, 4, 1, 2, [](uint64_t w) { return 4 * w; }, 1, 1, 1},                 // BGRA8
    {4, 1, 3, 3, [](uint64_t w) { return w; }, 1, 1, 1},                     // RGB8_PLANAR
    {8, 1, 1, 7, [](uint64_t w) { return w; }, 1, 1, 1},                     // GRAY8
    {10, 1, 1, 17, [](uint64_t w) { return w; }, 1, 1, 1},                   // BAYER_RGGB8
    {11, 1, 1, 17, [](uint64_t w) { return w; }, 1, 1, 1},                   // BAYER_GRBG8
    {12, 1, 1, 17, [](uint64_t w) { return w; }, 1, 1, 1},                   // BAYER_GBRG8
    {13, 1, 1, 17, [](uint64_t w) { return w; }, 1, 1, 1},                   // BAYER_BGGR8
    {16, 1, 2, 4, [](uint64_t w) { return even(w); }, 1, 2, 2},              // NV12
    {17, 1, 3, 5, [](uint64_t w) { return w; }, 1, 2, 2},                    // I420
    {18, 1, 3, 6, [](uint64_t w) { return w; }, 1, 1, 1},                    // YUV444_PLANAR
    {20, 2, 1, 8, [](uint64_t w) { return 4 * ((w + 1) / 2); }, 1, 2, 1},    // YUYV
    {21, 2, 1, 8, [](uint64_t w) { return 4 * ((w + 1) / 2); }, 1, 2, 1},    // UYVY
    {22, 1, 2, 9, [](uint64_t w) { return even(w); }, 1, 2, 1},              // NV16
    {23, 1, 3, 10, [](uint64_t w) { return w; }, 1, 2, 1},                   // I422
    {32, 2, 2, 11, [](uint64_t w) { return 2 * even(w); }, 2, 2, 2},         // P010
    {33, 2, 3, 12, [](uint64_t w) { return 2 * w; }, 2, 2, 2},               // I010
    {40, 2, 1, 13, [](uint64_t w) { return 8 * ((w + 1) / 2); }, 2, 2, 1},   // Y210
    {41, 2, 2, 14, [](uint64_t w) { return 2 * even(w); }, 2, 2, 1},         // P210
    {42, 2, 3, 15, [](uint64_t w) { return 2 * w; }, 2, 2, 1},               // I210
    {48, 0, 1, 16, [](uint64_t w) { return 16 * ((w + 5) / 6); }, 0, 2, 1},  // V210
};
static const Want* want_of(int fmt) {
    for (const Want& w : kWant)
        if (w.fmt == fmt) return &w;
    return nullptr;
}
static bool one_of(int fmt, std::initializer_list<int> set) {
    for (int f : set)
        if (f == fmt) return true;
    return false;
}
// I420, I422, I010, I210: Y, Cb and Cr planes, the chroma planes at a pitch of their own
static bool three_sub(int fmt) { return one_of(fmt, {17, 23, 33, 42}); }
static bool two_plane(int fmt) { return one_of(fmt, {16, 22, 32, 41}); }
static uint64_t want_chroma_pitch(int fmt, uint64_t stride) {
    return one_of(fmt, {33, 42}) ? 2 * ((stride + 3) / 4) : one_of(fmt, {17, 23}) ? (stride + 1) / 2 : stride;
}

static void test_table() {
    bool ok = true;
    CHECK(sizeof(kWant) / sizeof(kWant[0]) == 23 && kLayoutCount == 23);
    for (int f = -2; f <= 63; ++f) CHECK(fmt_valid(f) == (want_of(f) != nullptr));
    report("table_valid_codes", ok);
    ok = true;
    for (const Want& w : kWant) {
        CHECK((int)fmt_bpp(w.fmt) == w.bpp);
        CHECK((int)fmt_planes(w.fmt) == w.planes);
        CHECK(fmt_shape(w.fmt) == w.shape);
        for (uint32_t width : {1u, 2u, 5u, 6u, 7u, 47u, 48u, 49u, 65535u}) CHECK(fmt_row_bytes(w.fmt, width) == w.row(width));
        for (uint64_t s = 0; s <= 64; ++s) CHECK(fmt_chroma_pitch(w.fmt, s) == want_chroma_pitch(w.fmt, s));
        CHECK(fmt_yuv420(w.fmt) == (w.cx == 2 && w.cy == 2));
        CHECK(fmt_yuv422(w.fmt) == (w.cx == 2 && w.cy == 1));
        CHECK(layout(w.fmt).cx == w.cx && layout(w.fmt).cy == w.cy && layout(w.fmt).fmt == w.fmt);
    }
    CHECK(v210_row_bytes(0xFFFFFFFFu) == 16ull * 715827883ull);  // (no 32-bit overflow)
    report("table_rows", ok);
    ok = true;
    for (int f = -2; f <= 63; ++f) {
        const bool rgb4 = f >= 0 && f <= 3, bayer = f >= 10 && f <= 13;
        CHECK(ds_fmt(f) == (rgb4 || f == 16));
        CHECK(orient_fmt(f) == rgb4 && fmt_rgb4(f) == rgb4 && stripe_fmt(f) == rgb4);
        CHECK(lut_fmt(f) == (rgb4 || bayer) && ((layout(f).is & kLayLut) != 0) == (rgb4 || bayer));
        CHECK(fmt_bayer(f) == bayer && ((layout(f).is & kLayBayer) != 0) == bayer);
        CHECK(fmt_gray(f) == (f == 8));
        CHECK(fmt_yuv10(f) == one_of(f, {32, 33, 40, 41, 42, 48}));
        CHECK(fmt_yuv422p10(f) == one_of(f, {40, 41, 42, 48}));
        CHECK(fmt_packed422(f) == one_of(f, {20, 21}));
        if (fmt_valid(f)) CHECK(fmt_yuv(f) == (f >= 16));
        if (fmt_valid(f)) CHECK(layout(f).align == (f == 48 ? 4 : fmt_yuv10(f) ? 2 : 1));
    }
    report("table_capabilities", ok);
}

// ---- refusals ----
alignas(16) static uint8_t g_base[64];  // (a frame's pointer: the plan never reads through it)
struct Case {
    FrameDesc f;
    PlanSettings set;
    uint32_t flags = 0;
};
static Case frame(int fmt, uint32_t w, uint32_t h) {
    Case c;
    c.f.rgb = g_base;
    c.f.fmt = fmt;
    c.f.width = w;
    c.f.height = h;
    return c;
}
static int run(const Case& c) {
    FramePlan p;
    return plan_frame(c.f, c.set, c.flags, p);
}
// `bad` is refused with `want`; `good`, its nearest accepted frame, is planned
static void refusal(const char* name, int want, const Case& bad, const Case& good) {
    const int b = run(bad), g = run(good);
    if (b != want || g != kOk) std::printf("  %s: refused frame %d (want %d), accepted frame %d\n", name, b, want, g);
    report(name, b == want && g == kOk);
}
template <class F>
static Case with(Case c, F change) {
    change(c);
    return c;
}

static void test_refusals() {
    const Case rgb = frame(kFmtRgb8, 16, 16);
    refusal("refuse_null_pointer", kErrArg, with(rgb, [](Case& c) { c.f.rgb = nullptr; }), rgb);
    refusal("refuse_zero_width", kErrArg, frame(kFmtRgb8, 0, 1), frame(kFmtRgb8, 1, 1));
    refusal("refuse_zero_height", kErrArg, frame(kFmtRgb8, 1, 0), frame(kFmtRgb8, 1, 1));
    refusal("refuse_width_65536", kErrArg, frame(kFmtRgb8, 65536, 1), frame(kFmtRgb8, 65535, 1));
    refusal("refuse_height_65536", kErrArg, frame(kFmtRgb8, 1, 65536), frame(kFmtRgb8, 1, 65535));
    refusal("refuse_maxval_0", kErrRange, with(rgb, [](Case& c) { c.f.maxval = 0; }), with(rgb, [](Case& c) { c.f.maxval = 1; }));
    refusal("refuse_maxval_256", kErrRange, with(rgb, [](Case& c) { c.f.maxval = 256; }), with(rgb, [](Case& c) { c.f.maxval = 255; }));
    refusal("refuse_maxval_0_null_pointer", kErrArg, with(rgb, [](Case& c) { c.f.maxval = 0; c.f.rgb = nullptr; }), rgb);
    refusal("refuse_unknown_layout", kErrArg, frame(19, 16, 16), frame(18, 16, 16));
    refusal("refuse_plane_stride_one_plane", kErrArg, with(rgb, [](Case& c) { c.f.plane_stride = 4096; }),
            with(frame(kFmtRgb8Planar, 16, 16), [](Case& c) { c.f.plane_stride = 4096; }));
    refusal("refuse_stride_below_row", kErrArg, with(rgb, [](Case& c) { c.f.stride = 47; }), with(rgb, [](Case& c) { c.f.stride = 48; }));
    for (int fmt : {kFmtI420, kFmtGray8, kFmtBayerGrbg8}) {
        char name[64];
        std::snprintf(name, sizeof name, "refuse_maxval_254_layout_%d", fmt);
        refusal(name, kErrArg, with(frame(fmt, 16, 16), [](Case& c) { c.f.maxval = 254; }), frame(fmt, 16, 16));
    }
    for (int fmt : {kFmtNv12, kFmtI420, kFmtP010, kFmtI010})
        for (int mode : {444, 422, 411, 4200, 4201}) {
            char name[64];
            std::snprintf(name, sizeof name, "refuse_420_layout_%d_mode_%d", fmt, mode);
            refusal(name, kErrArg, with(frame(fmt, 16, 16), [mode](Case& c) { c.set.mode = mode; }), frame(fmt, 16, 16));
        }
    refusal("refuse_bayer_1x2", kErrArg, frame(kFmtBayerRggb8, 1, 2), frame(kFmtBayerRggb8, 2, 2));
    refusal("refuse_bayer_2x1", kErrArg, frame(kFmtBayerBggr8, 2, 1), frame(kFmtBayerBggr8, 2, 2));
    const auto ds2 = [](Case& c) { c.set.ds = 2; };
    const auto flip = [](Case& c) { c.set.orient = kOrientFlipH; };
    const auto lut = [](Case& c) { c.set.lut = true; };
    refusal("refuse_downscale_layout", kErrArg, with(frame(kFmtI420, 16, 16), ds2), with(frame(kFmtNv12, 16, 16), ds2));
    refusal("refuse_orientation_layout", kErrArg, with(frame(kFmtNv12, 16, 16), flip), with(frame(kFmtBgra8, 16, 16), flip));
    refusal("refuse_orientation_with_downscale", kErrArg, with(with(rgb, flip), ds2), with(rgb, flip));
    for (int mode : {444, 422, 411}) {
        char name[64];
        std::snprintf(name, sizeof name, "refuse_transposed_mode_%d", mode);
        // (beside it: the same orientation in 4:2:0, and a flip in this mode)
        refusal(name, kErrArg, with(rgb, [mode](Case& c) { c.set.orient = kOrientRot90; c.set.mode = mode; }),
                with(rgb, [](Case& c) { c.set.orient = kOrientRot90; }));
        std::snprintf(name, sizeof name, "refuse_transposed_mode_%d_beside_flip", mode);
        refusal(name, kErrArg, with(rgb, [mode](Case& c) { c.set.orient = kOrientTranspose; c.set.mode = mode; }),
                with(rgb, [mode](Case& c) { c.set.orient = kOrientFlipV; c.set.mode = mode; }));
    }
    refusal("refuse_lut_layout", kErrArg, with(frame(kFmtNv12, 16, 16), lut), with(frame(kFmtBayerGbrg8, 16, 16), lut));
    refusal("refuse_lut_planar", kErrArg, with(frame(kFmtRgb8Planar, 16, 16), lut), with(frame(kFmtRgba8, 16, 16), lut));
    refusal("refuse_lut_maxval_254", kErrArg, with(with(rgb, lut), [](Case& c) { c.f.maxval = 254; }), with(rgb, lut));
    refusal("refuse_lut_downscale", kErrArg, with(with(rgb, lut), ds2), with(rgb, lut));
    refusal("refuse_lut_orientation", kErrArg, with(with(rgb, lut), flip), with(rgb, lut));
    for (int fmt : {kFmtP010, kFmtI010, kFmtY210, kFmtP210, kFmtI210, kFmtV210}) {
        char name[64];
        const size_t row = want_of(fmt)->row(16), step = fmt == kFmtV210 ? 4 : 2;
        const Case good = with(frame(fmt, 16, 16), [=](Case& c) { c.f.stride = row + step; });
        std::snprintf(name, sizeof name, "refuse_odd_base_layout_%d", fmt);
        refusal(name, kErrArg, with(good, [](Case& c) { c.f.rgb = g_base + 1; }), good);
        std::snprintf(name, sizeof name, "refuse_odd_stride_layout_%d", fmt);
        refusal(name, kErrArg, with(good, [=](Case& c) { c.f.stride = row + 1; }), good);
        if (want_of(fmt)->planes == 1) continue;
        std::snprintf(name, sizeof name, "refuse_odd_plane_stride_layout_%d", fmt);
        refusal(name, kErrArg, with(good, [=](Case& c) { c.f.plane_stride = (row + step) * 16 + 1; }),
                with(good, [=](Case& c) { c.f.plane_stride = (row + step) * 16 + 2; }));
    }
    {
        const size_t row = want_of(kFmtV210)->row(16);
        const Case good = with(frame(kFmtV210, 16, 16), [=](Case& c) { c.f.stride = row + 4; });
        refusal("refuse_v210_base_2", kErrArg, with(good, [](Case& c) { c.f.rgb = g_base + 2; }), with(good, [](Case& c) { c.f.rgb = g_base + 4; }));
        refusal("refuse_v210_stride_2", kErrArg, with(good, [=](Case& c) { c.f.stride = row + 2; }), good);
    }
    {
        // a device frame read in place: stride * height reaches K1's offset bound, 0xFFFFFF00 = 256 * 16777215
        const Case at = with(frame(kFmtRgb8, 16, 256), [](Case& c) { c.f.stride = 16777215; c.flags = kFlagDeviceInput; });
        bool ok = true;
        CHECK(at.f.stride * at.f.height == kK1OffsetBound);
        report("offset_bound_is_256_rows", ok);
        refusal("refuse_device_frame_at_offset_bound", kErrArg, at, with(at, [](Case& c) { c.f.stride = 16777214; }));
    }
    report("stripe_settings", stripe_settings_ok(kFmtBgra8, PlanSettings{}, false) && !stripe_settings_ok(kFmtBgra8, PlanSettings{}, true) &&
                                  !stripe_settings_ok(kFmtBgra8, PlanSettings{444, 1, 0, false}, false) &&
                                  !stripe_settings_ok(kFmtBgra8, PlanSettings{420, 2, 0, false}, false) &&
                                  !stripe_settings_ok(kFmtBgra8, PlanSettings{420, 1, 3, false}, false) &&
                                  !stripe_settings_ok(kFmtBgra8, PlanSettings{420, 1, 0, true}, false) &&
                                  !stripe_settings_ok(kFmtRgb8Planar, PlanSettings{}, false) && !stripe_settings_ok(kFmtGray8, PlanSettings{}, false) &&
                                  !stripe_settings_ok(kFmtYuyv, PlanSettings{}, false) && !stripe_settings_ok(kFmtBayerRggb8, PlanSettings{}, false));
}

// ---- the upload plan, by simulation ----
// Where a frame's samples lie, by the layouts' definitions: sample k of the list is the same sample
// of the frame whatever the pitches.  kind: 1 or 2 bytes at off; 0: v210's 10-bit field `shift`
// bits up in the little-endian 32-bit word at off.
struct Sample {
    size_t off;
    int kind, shift;
};
static void samples(int fmt, uint32_t w, uint32_t h, size_t stride, size_t plane_stride, std::vector<Sample>& out) {
    const Want& wt = *want_of(fmt);
    const uint32_t cw = (w + 1) / 2, crows = wt.cy == 2 ? (h + 1) / 2 : h;
    const size_t cp = (size_t)fmt_chroma_pitch(fmt, stride);
    const size_t sb = (size_t)wt.sample_bytes;
    out.clear();
    if (fmt == kFmtV210) {
        const auto field = [&](uint32_t y, uint32_t i) { out.push_back({y * stride + 4 * (size_t)(i / 3), 0, (int)(10 * (i % 3))}); };
        for (uint32_t y = 0; y < h; ++y) {
            for (uint32_t x = 0; x < w; ++x) field(y, 2 * x + 1);
            for (uint32_t c = 0; c < cw; ++c) field(y, 4 * c), field(y, 4 * c + 2);
        }
    } else if (wt.planes == 1) {  // interleaved pixels, gray, a mosaic, or groups Y0 Cb Y1 Cr in some order
        const size_t px = wt.cx == 2 ? 2 * sb : (size_t)wt.bpp;  // bytes a pixel adds to a row
        for (uint32_t y = 0; y < h; ++y)
            for (size_t b = 0; b < px * (wt.cx == 2 ? 2 * cw : w); b += sb) {
                // (a packed 4:2:2 row of odd width: the last group's second Y is no sample)
                if (wt.cx == 2 && (w & 1) && b / sb == 4 * (size_t)(cw - 1) + (fmt == kFmtUyvy ? 3 : 2)) continue;
                out.push_back({y * stride + b, (int)sb, 0});
            }
    } else if (wt.cx == 1) {  // three equal planes
        for (size_t c = 0; c < 3; ++c)
            for (uint32_t y = 0; y < h; ++y)
                for (uint32_t x = 0; x < w; ++x) out.push_back({c * plane_stride + y * stride + x, 1, 0});
    } else {
        for (uint32_t y = 0; y < h; ++y)
            for (uint32_t x = 0; x < w; ++x) out.push_back({y * stride + sb * x, (int)sb, 0});
        for (uint32_t y = 0; y < crows; ++y)
            for (uint32_t x = 0; x < cw; ++x)
                for (size_t k = 0; k < 2; ++k)  // Cb, Cr
                    out.push_back({two_plane(fmt) ? plane_stride + y * stride + sb * (2 * x + k)
                                                  : plane_stride + k * cp * crows + y * cp + sb * x,
                                   (int)sb, 0});
    }
}
static uint32_t value(size_t k, int kind) {
    return kind == 1 ? (uint32_t)(k * 73 + 19) & 0xFFu : kind == 2 ? (uint32_t)(k * 40503 + 977) & 0xFFFFu : (uint32_t)(k * 569 + 3) & 0x3FFu;
}
static void put(std::vector<uint8_t>& buf, const Sample& s, uint32_t v) {
    if (s.kind) {
        std::memcpy(&buf[s.off], &v, (size_t)s.kind);  // (little-endian words)
    } else {
        uint32_t word;
        std::memcpy(&word, &buf[s.off], 4);
        word = (word & ~(0x3FFu << s.shift)) | (v << s.shift);
        std::memcpy(&buf[s.off], &word, 4);
    }
}
static uint32_t get(const std::vector<uint8_t>& buf, const Sample& s) {
    uint32_t word = 0;
    std::memcpy(&word, &buf[s.off], s.kind ? (size_t)s.kind : 4);
    return s.kind ? word : (word >> s.shift) & 0x3FFu;
}
// a frame's planes: `rows` rows of `pitch` bytes from `start`, the first `row` bytes of each its
// samples.  A copy may read a plane's rows whole (jpge.h: rows of `stride` bytes), but of a v210
// frame's last row only the groups: a capture row's padding need not be there.
struct Plane {
    size_t start, pitch, rows, row;
    size_t bytes(int fmt) const { return fmt == kFmtV210 ? pitch * (rows - 1) + row : pitch * rows; }
};
static int planes_of(int fmt, uint32_t w, uint32_t h, size_t stride, size_t plane_stride, Plane out[3]) {
    const Want& wt = *want_of(fmt);
    const size_t row = (size_t)wt.row(w), crows = wt.cy == 2 ? (h + 1) / 2 : h, cp = (size_t)want_chroma_pitch(fmt, stride);
    out[0] = {0, stride, h, row};
    if (wt.planes == 1) return 1;
    if (two_plane(fmt)) {
        out[1] = {plane_stride, stride, crows, row};
        return 2;
    }
    for (size_t c = 1; c < 3; ++c)
        out[c] = three_sub(fmt) ? Plane{plane_stride + (c - 1) * cp * crows, cp, crows, (size_t)wt.sample_bytes * ((w + 1) / 2)}
                                : Plane{c * plane_stride, stride, h, row};
    return 3;
}

static bool simulate(int fmt, uint32_t w, uint32_t h, size_t stride, size_t plane_stride_arg) {
    bool ok = true;
    const size_t plane_stride = plane_stride_arg ? plane_stride_arg : stride * h;
    Plane pl[3];
    const int np = planes_of(fmt, w, h, stride, plane_stride, pl);
    size_t extent = 0;
    for (int i = 0; i < np; ++i) extent = std::max(extent, pl[i].start + pl[i].bytes(fmt));
    std::vector<uint8_t> src(extent), may_read(extent, 0);
    for (size_t i = 0; i < extent; ++i) src[i] = (uint8_t)(0xA5 ^ (i * 7));
    for (int i = 0; i < np; ++i) std::memset(&may_read[pl[i].start], 1, pl[i].bytes(fmt));
    std::vector<Sample> at;
    samples(fmt, w, h, stride, plane_stride, at);
    for (size_t k = 0; k < at.size(); ++k) {
        CHECK(at[k].off + (at[k].kind ? (size_t)at[k].kind : 4) <= extent);
        if (!ok) return false;
        put(src, at[k], value(k, at[k].kind));
    }
    FrameDesc f;
    f.rgb = src.data();
    f.width = w;
    f.height = h;
    f.fmt = fmt;
    f.stride = stride;
    f.plane_stride = plane_stride_arg;
    FramePlan p;
    CHECK(plan_frame(f, PlanSettings{}, 0, p) == kOk);
    if (!ok) return false;
    CHECK(p.in.ptr == nullptr && p.in.fmt == fmt && p.in_bytes > 0 && (p.linear != 0) != (p.ncopy != 0) && p.ncopy <= 3);
    CHECK(p.g.width == w && p.g.height == h && p.in.ds == 1 && p.in.orient == 0 && p.in.src_w == 0 && p.in.src_h == 0);
    CHECK(p.out_cap == max_jpeg_bytes(w, h));
    // the device pitch: aligned (v210: 128 bytes per 48 pixels), the chroma's too
    CHECK(p.in.stride >= want_of(fmt)->row(w) && p.in.stride % (fmt == kFmtV210 ? 128 : three_sub(fmt) ? 32 : 16) == 0);
    CHECK((p.in.plane_stride == 0) == (want_of(fmt)->planes == 1));
    if (!ok) return false;
    // the copies, as the encoder issues them
    std::vector<uint8_t> dev(p.in_bytes, 0x5A);
    const auto copy = [&](size_t so, size_t d_o, size_t n) {
        CHECK(so + n <= extent && d_o + n <= dev.size());
        if (!ok) return;
        for (size_t i = 0; i < n; ++i) CHECK(may_read[so + i]);
        std::memcpy(&dev[d_o], f.rgb + so, n);
    };
    if (p.linear) copy(0, 0, p.linear);
    for (int c = 0; c < p.ncopy && ok; ++c)
        for (size_t r = 0; r < p.copy[c].rows && ok; ++r)
            copy(p.copy[c].src_off + r * p.copy[c].src_pitch, p.copy[c].dst_off + r * p.copy[c].dst_pitch, p.copy[c].row_bytes);
    if (!ok) return false;
    // every sample, at the address the device pitches give it
    std::vector<Sample> dat;
    samples(fmt, w, h, p.in.stride, p.in.plane_stride, dat);
    CHECK(dat.size() == at.size());
    for (size_t k = 0; k < dat.size() && ok; ++k) {
        CHECK(dat[k].off + (dat[k].kind ? (size_t)dat[k].kind : 4) <= dev.size());
        if (ok) CHECK(get(dev, dat[k]) == value(k, dat[k].kind));
    }
    return ok;
}

static void test_upload() {
    size_t frames = 0;
    for (const Want& wt : kWant) {
        bool ok = true;
        const size_t align = wt.fmt == kFmtV210 ? 4 : wt.sample_bytes == 2 ? 2 : 1;
        for (uint32_t w : {1u, 2u, 5u, 6u, 7u, 17u, 49u})
            for (uint32_t h : {1u, 2u, 3u}) {
                if (fmt_bayer(wt.fmt) && (w < 2 || h < 2)) continue;  // (refused: no 2x2 cell)
                const size_t row = (size_t)wt.row(w);
                // the least stride, one 3 bytes above it (raised to the layout's alignment), and the
                // device copy's own pitch (one linear copy)
                for (size_t stride : {row, align_up(row + 3, align), align_up(row, wt.fmt == kFmtV210 ? 128 : three_sub(wt.fmt) ? 32 : 16)})
                    for (size_t plane_stride : {(size_t)0, align_up(stride * h + 5, align)}) {
                        if (plane_stride && wt.planes == 1) continue;
                        if (!simulate(wt.fmt, w, h, stride, plane_stride)) {
                            if (ok) std::printf("  layout %d, %u x %u, stride %zu, plane stride %zu\n", wt.fmt, w, h, stride, plane_stride);
                            ok = false;
                        }
                        ++frames;
                    }
            }
        char name[64];
        std::snprintf(name, sizeof name, "upload_layout_%d", wt.fmt);
        report(name, ok);
    }
    std::printf("  (%zu frames uploaded)\n", frames);
}

static void test_coded_size() {
    bool ok = true;
    const uint32_t sizes[3][2] = {{1, 1}, {5, 3}, {65535, 1}};
    for (const auto& s : sizes) {
        const uint32_t w = s[0], h = s[1];
        uint32_t ow = 0, oh = 0;
        for (int o = 0; o <= 7; ++o) {
            coded_size(w, h, PlanSettings{420, 1, o, false}, &ow, &oh);
            CHECK(ow == (o >= 4 ? h : w) && oh == (o >= 4 ? w : h));
        }
        for (int ds : {1, 2, 4}) {
            coded_size(w, h, PlanSettings{420, ds, 0, false}, &ow, &oh);
            CHECK(ow == (w + ds - 1) / ds && oh == (h + ds - 1) / ds);
        }
    }
    uint32_t ow = 0, oh = 0;
    coded_size(5, 3, PlanSettings{420, 2, 0, false}, &ow, &oh);
    CHECK(ow == 3 && oh == 2);
    coded_size(65535, 1, PlanSettings{420, 4, 0, false}, &ow, &oh);
    CHECK(ow == 16384 && oh == 1);
    // the plan's geometry and source size follow it
    Case c = frame(kFmtRgb8, 5, 3);
    c.set.orient = kOrientRot270;
    FramePlan p;
    CHECK(plan_frame(c.f, c.set, 0, p) == kOk && p.g.width == 3 && p.g.height == 5 && p.in.src_w == 5 && p.in.src_h == 3 && p.in.orient == kOrientRot270);
    c.set = PlanSettings{444, 4, 0, false};
    CHECK(plan_frame(c.f, c.set, kFlagDeviceInput | kFlagDeviceOutput, p) == kOk && p.g.width == 2 && p.g.height == 1 && p.g.bpm == 3 &&
          p.in.src_w == 5 && p.in.src_h == 3 && p.in.ds == 4 && p.in.ptr == g_base && p.in.stride == 15 && p.in_bytes == 0 && p.out_cap == 0 &&
          p.linear == 0 && p.ncopy == 0);
    report("coded_size", ok);
}

int main() {
    test_table();
    test_refusals();
    test_upload();
    test_coded_size();
    std::printf(g_fail ? "%d FAILED\n" : "all ok\n", g_fail);
    return g_fail ? 1 : 0;
}
