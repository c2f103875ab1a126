#include "frame_plan.hpp"

#include <algorithm>

namespace jpge {

bool mode_shape(int mode, uint32_t& yh, uint32_t& bpm, uint32_t& cfilt) {
    cfilt = kFiltS420m;
    switch (mode) {
        case 420: yh = 2; bpm = 6; return true;
        case 4201: yh = 2; bpm = 6; cfilt = kFiltS420lm; return true;
        case 4200: yh = 2; bpm = 6; cfilt = kFiltS420; return true;
        case 444: yh = 1; bpm = 3; return true;
        case 422: yh = 2; bpm = 4; return true;
        case 411: yh = 4; bpm = 6; return true;
        default: return false;
    }
}

Geometry geometry(uint32_t w, uint32_t h, int mode) {
    Geometry g;
    g.width = w;
    g.height = h;
    mode_shape(mode, g.yh, g.bpm, g.cfilt);
    g.mw = (w + g.mcu_w() - 1) / g.mcu_w();
    g.mh = (h + g.mcu_h() - 1) / g.mcu_h();
    return g;
}

Geometry gray_geometry(uint32_t w, uint32_t h) {
    Geometry g;
    g.width = w;
    g.height = h;
    g.yh = 1;
    g.bpm = 1;
    g.mw = (w + 7) / 8;
    g.mh = (h + 7) / 8;
    return g;
}

size_t max_jpeg_bytes(uint32_t w, uint32_t h) {
    // header <= 20 + 2*69 + 19 + 4*(4+17+256) + 14 ; entropy <= 1665 bits/block,
    // doubled for worst-case 0xFF stuffing; + EOI.
    // Restart intervals add per MCU at most an RST marker, a fill byte and its stuffing.
    // (The largest bound over the MCU shapes: one capacity serves every mode.)
    size_t cap = 0;
    for (int mode : {420, 444, 422, 411}) {
        const Geometry g = geometry(w, h, mode);
        cap = std::max(cap, 2048 + (size_t)g.nblocks() * 2 * 209 + 16 + (size_t)g.nmcu() * 4);
    }
    return cap;
}

void coded_size(uint32_t w, uint32_t h, const PlanSettings& set, uint32_t* out_w, uint32_t* out_h) {
    *out_w = set.orient ? orient_w(w, h, set.orient) : ds_dim(w, set.ds);
    *out_h = set.orient ? orient_h(w, h, set.orient) : ds_dim(h, set.ds);
}

int plan_frame(const FrameDesc& f, const PlanSettings& set, uint32_t flags, FramePlan& p) {
    if (!f.rgb || f.width == 0 || f.height == 0 || f.width > 65535 || f.height > 65535) return kErrArg;
    if (f.maxval < 1 || f.maxval > 255) return kErrRange;
    if (!fmt_valid(f.fmt)) return kErrArg;
    const Layout& l = layout(f.fmt);
    const auto is = [&l](uint16_t what) { return (l.is & what) != 0; };
    if (f.plane_stride && l.planes == 1) return kErrArg;
    // a downscaled or oriented frame: f is the source (its limits, pitches and upload are the
    // source's), and the geometry of everything K1 writes is the coded frame's.  The layouts with
    // such kernels; not both settings together; the transposed kernels are the 16x16-MCU ones.
    if (set.ds > 1 && !is(kLayDs)) return kErrArg;
    if (set.orient && (!is(kLayRgb4) || set.ds > 1)) return kErrArg;
    uint32_t out_w, out_h;
    coded_size(f.width, f.height, set, &out_w, &out_h);
    // (one component: no chroma, so the subsampling mode does not enter)
    p.g = is(kLayGray) ? gray_geometry(out_w, out_h) : geometry(out_w, out_h, set.mode);
    if (orient_transposed(set.orient) && p.g.row8()) return kErrArg;
    // Y, Cb, Cr, gray and raw samples are 8-bit values as they are; half-size chroma planes are the
    // S420_m mode's planes; a mosaic has a 2x2 cell at least (a reflected neighbour exists)
    if ((is(kLayYuv) || is(kLayGray) || is(kLayBayer)) && f.maxval != 255) return kErrArg;
    if (l.cy == 2 && set.mode != 420) return kErrArg;
    if (is(kLayBayer) && (f.width < 2 || f.height < 2)) return kErrArg;
    // channel tables: the layouts that stage R, G, B bytes, as they are, at full size and as they lie
    if (set.lut && (!is(kLayLut) || f.maxval != 255 || set.ds > 1 || set.orient)) return kErrArg;
    // (16-bit words: an even base and even pitches; v210's 32-bit words: multiples of 4)
    if (((uintptr_t)f.rgb | f.stride | f.plane_stride) & (size_t)(l.align - 1)) return kErrArg;
    const size_t row = (size_t)layout_row_bytes(l, f.width);
    const size_t stride = f.stride ? f.stride : row;
    if (stride < row) return kErrArg;
    const size_t planes = l.planes;
    const size_t plane_stride = f.plane_stride ? f.plane_stride : stride * f.height;  // (planar)
    const bool dev_in = (flags & kFlagDeviceInput) != 0;
    const size_t dev_pitch = align_up(row, l.dev_align), dev_plane = dev_pitch * f.height;
    // the kernel's 32-bit offsets must span the frame it reads (a device frame in place at its
    // own pitch, a host frame's copy)
    Geometry src = p.g;
    src.width = f.width;
    src.height = f.height;
    if (!k1_offsets_fit(f.fmt, src, dev_in ? stride : dev_pitch)) return kErrArg;

    p.in.ptr = dev_in ? f.rgb : nullptr;
    p.in.stride = dev_in ? stride : dev_pitch;
    p.in.fmt = f.fmt;
    p.in.plane_stride = planes > 1 ? (dev_in ? plane_stride : dev_plane) : 0;
    p.in.ds = set.ds;
    p.in.orient = set.orient;
    const bool resampled = set.ds > 1 || set.orient;
    p.in.src_w = resampled ? f.width : 0;
    p.in.src_h = resampled ? f.height : 0;
    p.out_cap = (flags & kFlagDeviceOutput) ? 0 : max_jpeg_bytes(out_w, out_h);
    p.in_bytes = p.linear = 0;
    p.ncopy = 0;
    if (dev_in) return kOk;

    // The device copy.  Chroma planes of their own size (the 4:2:0 layouts; I422 and I210, whose
    // chroma pitch is half the luma's) follow the Y plane and each other at their own pitch:
    // chroma_rows rows of chroma_row bytes (a Cb,Cr plane's rows are as long as the Y plane's).
    // The other planar layouts are `planes` equal planes.
    const bool own_chroma = l.cy == 2 || l.cpitch != kChromaPitchSame;
    const size_t chroma_rows = (f.height + l.cy - 1) / l.cy, chroma_row = planes == 2 ? row : (size_t)l.bpp * chroma_dim(f.width);
    const size_t cpitch = (size_t)layout_chroma_pitch(l, stride), dev_cpitch = (size_t)layout_chroma_pitch(l, dev_pitch);
    p.in_bytes = own_chroma ? dev_plane + (planes - 1) * dev_cpitch * chroma_rows : planes * dev_plane;
    if (stride == dev_pitch && (planes == 1 || plane_stride == dev_plane)) {
        // (v210: up to the last row's last group; a capture row's padding need not be there)
        p.linear = l.shape == kShapeV210 ? p.in_bytes - dev_pitch + row : p.in_bytes;
    } else if (own_chroma) {
        p.copy[p.ncopy++] = {0, stride, 0, dev_pitch, (size_t)l.bpp * f.width, f.height};
        for (size_t c = 0; c + 1 < planes; ++c)
            p.copy[p.ncopy++] = {plane_stride + c * cpitch * chroma_rows, cpitch, dev_plane + c * dev_cpitch * chroma_rows,
                                 dev_cpitch, chroma_row, chroma_rows};
    } else {
        for (size_t c = 0; c < planes; ++c) p.copy[p.ncopy++] = {c * plane_stride, stride, c * dev_plane, dev_pitch, row, f.height};
    }
    return kOk;
}

bool stripe_settings_ok(int fmt, const PlanSettings& set, bool fixed_huffman) {
    return set.mode == 420 && !fixed_huffman && set.ds <= 1 && !set.orient && !set.lut && stripe_fmt(fmt);
}

}  // namespace jpge
