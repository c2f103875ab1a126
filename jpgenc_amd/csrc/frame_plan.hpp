// The host's plan for one frame, before anything touches the device: which frames are refused
// and with which error, the geometry the kernels run on, what K1 is given as its input, and where
// every byte of a host frame goes in its device copy.  Pure arithmetic: no HIP runtime call, no
// allocation, so the rules and the upload layout are tested without a GPU
// (tests/cpp/test_frame_plan.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

#include "host_io.hpp"
#include "layouts.hpp"

namespace jpge {

constexpr uint32_t kFlagDeviceInput = 1u;
constexpr uint32_t kFlagDeviceOutput = 2u;
constexpr uint32_t kFlagCoefficients = 1u << 30;  // (internal) the frame's coefficients are read back
constexpr uint32_t kFlagFixedTables = 1u << 29;   // (internal) the frame is coded with the context's fixed Huffman tables

struct FrameDesc {
    const uint8_t* rgb = nullptr;
    uint32_t width = 0, height = 0;
    size_t stride = 0;  // bytes per input row (0 = width * the layout's bytes per pixel)
    int maxval = 255;
    // input layout (kernels.hpp kFmt*); planar: plane c at rgb + c * plane_stride
    // (0 = stride * height).  The C ABI's pixel entries fill these from the context's
    // setting; the PPM entries leave the default.
    int fmt = kFmtRgb8;
    size_t plane_stride = 0;
    uint8_t* out = nullptr;
    size_t cap = 0;
    size_t len = 0;
    int status = 0;
};

// MCU shape of a subsampling mode (jpge.h JPGE_S*): Y blocks across, blocks per MCU
// and the 4:2:0 chroma filter; false for an unknown mode.
bool mode_shape(int mode, uint32_t& yh, uint32_t& bpm, uint32_t& cfilt);
// The frame in whole MCUs (4:2:0: 16x16 px, the reference's padding, Image.cpp:480-531;
// the other modes pad to their own MCU size: edge replication either way)
Geometry geometry(uint32_t w, uint32_t h, int mode = 420);
// One component (kFmtGray8): the frame in single 8x8 blocks, no chroma (kernels.hpp Geometry)
Geometry gray_geometry(uint32_t w, uint32_t h);
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
// an upper bound of a w x h frame's .jpg, in every subsampling mode (Encoder::max_jpeg_bytes)
size_t max_jpeg_bytes(uint32_t w, uint32_t h);

// The context's settings that decide how a frame is read.
struct PlanSettings {
    int mode = 420;    // subsampling (jpge_set_subsampling)
    int ds = 1;        // box downscale factor (jpge_set_downscale)
    int orient = 0;    // orientation (jpge_set_orientation)
    bool lut = false;  // channel tables on (jpge_set_channel_lut)
};

// The size of the frame that is coded from a w x h source: the oriented frame's, else that of
// ceil(w / ds) x ceil(h / ds) pixels.  Everything after K1 goes by it.
void coded_size(uint32_t w, uint32_t h, const PlanSettings& set, uint32_t* out_w, uint32_t* out_h);

// What K1 reads (FdctArgs's input side).  ds > 1 or orient != 0: the frame at ptr is the src_w x
// src_h source, and the geometry and everything after K1 are the coded frame's; else src_w and
// src_h are 0.
struct FrameInput {
    const uint8_t* ptr = nullptr;
    size_t stride = 0;
    int fmt = kFmtRgb8;
    size_t plane_stride = 0;  // (one plane: 0)
    int ds = 1, orient = 0;
    uint32_t src_w = 0, src_h = 0;
};

// rows x row_bytes from src_off at src_pitch (in the caller's frame) to dst_off at dst_pitch (in
// the device copy)
struct CopyRect {
    size_t src_off, src_pitch, dst_off, dst_pitch, row_bytes, rows;
};

struct FramePlan {
    Geometry g;     // the coded frame's (g.width x g.height: coded_size)
    // K1's input.  A device frame is read in place, at its own pitches.  A host frame (ptr null: the
    // slot's buffer) is read from its device copy: the same layout at an aligned pitch, the planes
    // one after the other.
    FrameInput in;
    size_t in_bytes = 0;  // the device copy's size (0: none)
    // the copies that make it: one linear copy of `linear` bytes (a 2D copy can fall back to a
    // slower engine path), else ncopy rectangles
    size_t linear = 0;
    int ncopy = 0;
    CopyRect copy[3];
    size_t out_cap = 0;  // of the slot's output buffer (0: the caller's device buffer takes the .jpg)
};

// kOk and the plan, or the frame's refusal: kErrArg; kErrRange for a maxval outside 1..255 in a
// frame with a pointer and dimensions within 1..65535.  (The quantisers are the caller's to
// check: tables_nonzero.)
int plan_frame(const FrameDesc& f, const PlanSettings& set, uint32_t flags, FramePlan& p);

// The stripe phases take a layout and settings at all: S420_m, per-image Huffman tables (the
// histogram all-reduce), full size, as the rows lie and with their own values, of one row of
// interleaved colour pixels (a mosaic's stripe would need its neighbours' rows).
bool stripe_settings_ok(int fmt, const PlanSettings& set, bool fixed_huffman);

}  // namespace jpge
