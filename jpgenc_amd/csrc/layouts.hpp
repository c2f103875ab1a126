// The input layouts as data: one row per layout (kernels.hpp kFmt*, whose comments define each
// layout's byte order), and the host's questions about a layout as lookups in its row.  Host code
// only: the few questions device code asks (fmt_bayer, lut_fmt, ...) keep their bodies in
// kernels.hpp.
#pragma once
#include "kernels.hpp"

namespace jpge {

// how a chroma plane's row pitch follows from the frame's `stride` (the 4:2:0 layouts: ceil(height
// / 2) chroma rows of ceil(width / 2) samples, starting plane_stride bytes after the Y plane; the
// 4:2:2 ones: `height` such rows)
enum : uint8_t {
    kChromaPitchSame,      // stride (the two-plane layouts' Cb,Cr rows; no chroma plane at all)
    kChromaPitchHalf,      // (stride + 1) / 2 (I420, I422, whose Cr plane follows the Cb plane's rows)
    kChromaPitchHalfWords  // 2 * ceil(stride / 4), whole 16-bit words (I010, I210, likewise)
};
// families and capabilities
enum : uint16_t {
    kLayYuv = 1,       // Y, Cb, Cr samples: no colour conversion
    kLay10 = 2,        // 10-bit samples (in 16-bit words; v210: three to a 32-bit word)
    kLayGray = 4,      // one component
    kLayBayer = 8,     // a mosaic, coded as its demosaic
    kLayRgb4 = 16,     // the four interleaved RGB layouts: the ones K1 reads oriented
    kLayDs = 32,       // has downscaling kernels (jpge_set_downscale)
    kLayLut = 64,      // has channel-table kernels (jpge_set_channel_lut)
    kLayStripes = 128  // the stripe phases take it (one row of interleaved colour pixels)
};

struct Layout {
    int8_t fmt;         // kFmt*
    int8_t shape;       // K1's load shape (kShape*)
    uint8_t bpp;        // bytes per pixel within a row (planar: of one plane; v210: 0, no whole number)
    uint8_t planes;
    uint8_t gpx, gbytes;  // a row's least byte count: ceil(width / gpx) groups of gbytes
    uint8_t cx, cy;     // chroma subsampling across and down (1, 2)
    uint8_t cpitch;     // kChromaPitch*
    uint8_t align;      // of base, stride and plane stride (bytes)
    uint8_t dev_align;  // of the pitch of a host frame's device copy (v210: 128 bytes per 48 pixels)
    uint16_t is;        // kLay*
};

constexpr uint16_t kLayRgbAll = kLayRgb4 | kLayDs | kLayLut | kLayStripes, kLayYuv10 = kLayYuv | kLay10;
inline constexpr Layout kLayouts[] = {
    // fmt              shape            bpp pl gpx gb cx cy chroma pitch         align dev  is
    {kFmtRgb8,          kShapeRgb8,      3, 1, 1, 3,  1, 1, kChromaPitchSame,      1, 16,  kLayRgbAll},
    {kFmtBgr8,          kShapeBgr8,      3, 1, 1, 3,  1, 1, kChromaPitchSame,      1, 16,  kLayRgbAll},
    {kFmtRgba8,         kShapeX4,        4, 1, 1, 4,  1, 1, kChromaPitchSame,      1, 16,  kLayRgbAll},
    {kFmtBgra8,         kShapeX4,        4, 1, 1, 4,  1, 1, kChromaPitchSame,      1, 16,  kLayRgbAll},
    {kFmtRgb8Planar,    kShapePlanar,    1, 3, 1, 1,  1, 1, kChromaPitchSame,      1, 16,  0},
    {kFmtGray8,         kShapeGray,      1, 1, 1, 1,  1, 1, kChromaPitchSame,      1, 16,  kLayGray},
    {kFmtBayerRggb8,    kShapeBayer8,    1, 1, 1, 1,  1, 1, kChromaPitchSame,      1, 16,  kLayBayer | kLayLut},
    {kFmtBayerGrbg8,    kShapeBayer8,    1, 1, 1, 1,  1, 1, kChromaPitchSame,      1, 16,  kLayBayer | kLayLut},
    {kFmtBayerGbrg8,    kShapeBayer8,    1, 1, 1, 1,  1, 1, kChromaPitchSame,      1, 16,  kLayBayer | kLayLut},
    {kFmtBayerBggr8,    kShapeBayer8,    1, 1, 1, 1,  1, 1, kChromaPitchSame,      1, 16,  kLayBayer | kLayLut},
    {kFmtNv12,          kShapeNv12,      1, 2, 2, 2,  2, 2, kChromaPitchSame,      1, 16,  kLayYuv | kLayDs},
    {kFmtI420,          kShapeI420,      1, 3, 1, 1,  2, 2, kChromaPitchHalf,      1, 32,  kLayYuv},
    {kFmtYuv444Planar,  kShapeYuv444,    1, 3, 1, 1,  1, 1, kChromaPitchSame,      1, 16,  kLayYuv},
    {kFmtYuyv,          kShapePacked422, 2, 1, 2, 4,  2, 1, kChromaPitchSame,      1, 16,  kLayYuv},
    {kFmtUyvy,          kShapePacked422, 2, 1, 2, 4,  2, 1, kChromaPitchSame,      1, 16,  kLayYuv},
    {kFmtNv16,          kShapeNv16,      1, 2, 2, 2,  2, 1, kChromaPitchSame,      1, 16,  kLayYuv},
    {kFmtI422,          kShapeI422,      1, 3, 1, 1,  2, 1, kChromaPitchHalf,      1, 32,  kLayYuv},
    {kFmtP010,          kShapeP010,      2, 2, 2, 4,  2, 2, kChromaPitchSame,      2, 16,  kLayYuv10},
    {kFmtI010,          kShapeI010,      2, 3, 1, 2,  2, 2, kChromaPitchHalfWords, 2, 32,  kLayYuv10},
    {kFmtY210,          kShapeY210,      2, 1, 2, 8,  2, 1, kChromaPitchSame,      2, 16,  kLayYuv10},
    {kFmtP210,          kShapeP210,      2, 2, 2, 4,  2, 1, kChromaPitchSame,      2, 16,  kLayYuv10},
    {kFmtI210,          kShapeI210,      2, 3, 1, 2,  2, 1, kChromaPitchHalfWords, 2, 32,  kLayYuv10},
    {kFmtV210,          kShapeV210,      0, 1, 6, 16, 2, 1, kChromaPitchSame,      4, 128, kLayYuv10},
};
constexpr int kLayoutCount = (int)(sizeof(kLayouts) / sizeof(kLayouts[0]));

// A code that is no layout has no row.  The questions below still answer for one as the range
// tests they replace did (three bytes per pixel below 0, four up to 15, and a three-plane Y, Cb,
// Cr layout of one above): fmt_valid is the only answer a caller may rely on.
inline constexpr Layout kNoLayout[3] = {{-1, kShapeX4, 3, 1, 1, 3, 1, 1, kChromaPitchSame, 1, 16, 0},
                                 {-1, kShapeX4, 4, 1, 1, 4, 1, 1, kChromaPitchSame, 1, 16, 0},
                                 {-1, kShapeX4, 1, 3, 1, 1, 1, 1, kChromaPitchSame, 1, 16, kLayYuv}};

// the row of each code 0..63 (-1: none)
struct LayoutIndex {
    int8_t row[64];
};
constexpr LayoutIndex layout_index() {
    LayoutIndex x{};
    for (int8_t& r : x.row) r = -1;
    for (int i = 0; i < kLayoutCount; ++i) x.row[kLayouts[i].fmt] = (int8_t)i;
    return x;
}
inline constexpr LayoutIndex kLayoutIndex = layout_index();

constexpr bool fmt_valid(int fmt) { return fmt >= 0 && fmt < 64 && kLayoutIndex.row[fmt] >= 0; }
constexpr const Layout& layout(int fmt) {
    return fmt_valid(fmt) ? kLayouts[kLayoutIndex.row[fmt]] : kNoLayout[fmt < 0 ? 0 : fmt < kFmtNv12 ? 1 : 2];
}

constexpr int fmt_shape(int fmt) { return layout(fmt).shape; }
constexpr uint32_t fmt_bpp(int fmt) { return layout(fmt).bpp; }
constexpr uint32_t fmt_planes(int fmt) { return layout(fmt).planes; }
constexpr bool fmt_gray(int fmt) { return (layout(fmt).is & kLayGray) != 0; }
constexpr bool fmt_yuv(int fmt) { return (layout(fmt).is & kLayYuv) != 0; }
constexpr bool fmt_yuv10(int fmt) { return (layout(fmt).is & kLay10) != 0; }
constexpr bool fmt_yuv420(int fmt) { return layout(fmt).cy == 2; }                           // chroma planes at half size
constexpr bool fmt_yuv422(int fmt) { return layout(fmt).cx == 2 && layout(fmt).cy == 1; }    // chroma at half width, every row
constexpr bool fmt_yuv422p10(int fmt) { return fmt_yuv422(fmt) && fmt_yuv10(fmt); }
constexpr bool fmt_packed422(int fmt) { return layout(fmt).shape == kShapePacked422; }       // (8-bit: 4-byte groups)
constexpr bool ds_fmt(int fmt) { return (layout(fmt).is & kLayDs) != 0; }
constexpr bool orient_fmt(int fmt) { return (layout(fmt).is & kLayRgb4) != 0; }
constexpr bool fmt_rgb4(int fmt) { return orient_fmt(fmt); }  // asked for its own sake: interleaved R, G, B bytes
constexpr bool stripe_fmt(int fmt) { return (layout(fmt).is & kLayStripes) != 0; }

// The least row pitch of a frame's first plane (NV12, NV16: the width rounded up to even, so that
// the Cb,Cr rows of the same pitch hold ceil(width / 2) pairs; the packed 4:2:2 layouts, Y210 and
// v210: whole groups)
constexpr uint64_t layout_row_bytes(const Layout& l, uint32_t width) { return l.gbytes * (((uint64_t)width + l.gpx - 1) / l.gpx); }
constexpr uint64_t fmt_row_bytes(int fmt, uint32_t width) { return layout_row_bytes(layout(fmt), width); }
constexpr uint64_t v210_row_bytes(uint32_t width) { return fmt_row_bytes(kFmtV210, width); }
constexpr uint64_t layout_chroma_pitch(const Layout& l, uint64_t stride) {
    return l.cpitch == kChromaPitchHalfWords ? 2 * ((stride + 3) / 4) : l.cpitch == kChromaPitchHalf ? (stride + 1) / 2 : stride;
}
constexpr uint64_t fmt_chroma_pitch(int fmt, uint64_t stride) { return layout_chroma_pitch(layout(fmt), stride); }

// The transform kernel reaches a frame's pixels and its coefficients through 32-bit buffer
// offsets: stride * height (planar layouts: of one plane; each plane has a descriptor of its
// own, the chroma planes' extents are no larger) and nblocks * 128 must stay below
// kK1OffsetBound.  The frame entries refuse a frame that does not fit with the argument error,
// before anything is queued (jpge.h, jpge_frame.stride).
inline bool k1_offsets_fit(int fmt, const Geometry& g, uint64_t stride) {
    const uint64_t row = fmt_row_bytes(fmt, g.width);
    if (g.height == 0 || stride < row || stride >= kK1OffsetBound) return false;
    const uint64_t extent = stride * (g.height - 1) + row;  // the descriptor's range
    return extent < kK1OffsetBound && stride * g.height < kK1OffsetBound && (uint64_t)g.nblocks() * 128 < kK1OffsetBound;
}

}  // namespace jpge
