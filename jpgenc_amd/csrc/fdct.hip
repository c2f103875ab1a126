// K1 fdct_kernel (gfx950): RGB8 (or another input layout, Y, Cb, Cr samples included, see "input layouts" below) -> YCbCr -> 4:2:0 (S420_m) -> Arai FDCT (fp64)
// -> quantise -> int16 coefficients (natural order, MCU-interleaved blocks).
//
// One wavefront owns a tile of 4 MCUs (64x16 px) staged in LDS for the column
// pass, the transpose and the row pass; each lane stores one 16-byte row of a
// block straight from registers.  Persistent workgroups (8 waves, two per CU, alone) own a
// contiguous run of tiles; its waves take tiles from an LDS counter (the SIMD
// favours its oldest wave, so static shares finish unevenly) and prefetch the next
// tile's RGB run during the transform.  Three rounds per tile (chroma, Y MCUs 0-1,
// Y MCUs 2-3), each round's LDS reads issued in one batch during the previous
// round's row pass.  Pixels and coefficients go through buffer descriptors so that
// every tile issues the same loads and stores (no branches around them) and the
// in-order wait for the prefetch never drains a just-issued store; the stores are
// write-through (sc1), so the kernel ends without dirty L2 lines to flush.
// Reference: Image.cpp:112-147, 198-235, 540-636; Dct.hpp:47-215; Coding.hpp:84-97.
//
// Bit-exactness: every fp64 operation of the reference is reproduced in order with
// no contraction (-ffp-contract=off plus the pragma in device_common.hpp); the
// colour conversion of 8-bit input uses FMA chains only where every partial result
// is exact (all terms are multiples of 2^-27 far inside 53 bits).
#include <cstring>

#include "arai.hpp"
#include "device_common.hpp"
#include "layouts.hpp"  // (the host launcher's questions about a layout)

namespace jpge {
namespace {
using namespace dev;

// ---- colour constants, Image.cpp:131-134 (float literals widened) ----
constexpr double kYr = (double).299f, kYg = (double).587f, kYb = (double).114f;
constexpr double kCbR = (double)-.1687f, kCbG = (double)-.3312f, kCbB = (double).5f;
constexpr double kCrR = (double).5f, kCrG = (double)-.4186f, kCrB = (double)-.0813f;

// quantize, Coding.hpp:92-94, of the row pass's output o = w * s_u (Dct.hpp:124-131):
// (int)std::round(o / q) — two correctly rounded fp64 operations, then round half
// away from zero.  Fast path in one fp64 instruction per coefficient: the exact
// product x = w * c, c = fl(s_u / q), is within 2^-40 of the reference's quotient
// fl(fl(w s_u) / q) (|x| < 2^11: 8-bit samples, q >= 1), and
// y = fma(w, c, 1.5 * 2^36 + 0x8001 * 2^-16) rounds it once onto the 2^-16 grid (the
// addend lies on the grid, and y stays in [2^36, 2^37)), so the low word of y is
// t = n + 0x8001 with n = round(x * 2^16) (two's complement, mod 2^32):
//   - t >> 16 (its high half) is floor(x + 1/2), the reference's integer unless x
//     lies within 2^-15 of a half-integer — where the reference's quotient could sit
//     on the other side of it;
//   - those are exactly the t whose low half is 0, 1 or 2: one 16-bit min over the
//     row's 8 values finds them, and such a row is redone the reference's way
//     (quant_exact; rare, one wave-uniform branch per row).
// Integer boundaries are harmless (a quotient on either side of k rounds to k).
constexpr double kQuantMagic = 103079215104.50002;  // 1.5 * 2^36 + 0x8001 * 2^-16 (bits 0x4238000000008001)
static_assert(kQuantMagic - 103079215104.0 == 0x8001 * 0x1p-16, "the magic addend is exact");
__device__ __forceinline__ uint32_t quant_fix16(double w, double c) {
    return (uint32_t)__builtin_bit_cast(uint64_t, __builtin_fma(w, c, kQuantMagic));
}

__device__ __forceinline__ int quant_exact(double w, double s, double q) { return (int)round((w * s) / q); }

// One row of 8 quantised coefficients as int16 x 8 (natural order): the fast path,
// or the reference's two divisions when any lane of the wave has a near-half row.
// qrow: this lane's 8 quantisers (LDS).
__device__ __forceinline__ u32x4 quant_row(const double o[8], const double c[8], const double* qrow) {
    uint32_t t[8];
    uint16_t m = 0xFFFF;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        t[u] = quant_fix16(o[u], c[u]);
        m = __builtin_elementwise_min(m, (uint16_t)t[u]);  // v_min_u16 on the low half
    }
    if (__builtin_amdgcn_ballot_w64(m <= 2)) {  // wave-uniform: a real branch, not predication
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = (uint32_t)quant_exact(o[u], kS[u], qrow[u]) << 16;
    }
    u32x4 pk;  // the high halves, two per word
    pk.x = __builtin_amdgcn_perm(t[1], t[0], 0x07060302u);
    pk.y = __builtin_amdgcn_perm(t[3], t[2], 0x07060302u);
    pk.z = __builtin_amdgcn_perm(t[5], t[4], 0x07060302u);
    pk.w = __builtin_amdgcn_perm(t[7], t[6], 0x07060302u);
    return pk;
}

constexpr uint32_t kOob = 0xFFFFFF00u;  // buffer offset past every descriptor's range
constexpr int kK1StoreAux = 16;  // sc1: write-through coefficient stores (no dirty L2 lines at the kernel's end)
constexpr uint32_t kK1SharedCap = 512;  // shared-shape workgroups per launch, at most (2 per CU: measured
                                        // +1.5% in the pipeline over 1024, which filled every CU)

// Workgroup shapes: whole-CU, one 16-wave workgroup per CU (4 waves per SIMD), whose
// waves balance their tiles among themselves — for large frames with the GPU to
// itself (two 8-wave workgroups per CU: equal at 4K, 4% slower at 16384^2); 4 waves,
// four per CU alone (smaller frames, launch_fdct) or at most two per CU beside other
// lanes' kernels (a whole-CU workgroup waits for a whole CU to drain).
constexpr int kK1WavesSolo = 16;
constexpr int kK1WavesShared = 4;  // (pipeline: 8 waves x 256 -1.4%, 8 x 512 -3.3%, 2 x 1024 -2.3%)
constexpr int kRgbPitch = 66;    // u32 per staged pixel row: Y column reads conflict-free
constexpr int kTmpBlock = 72;    // doubles per transpose block (rows of 9 doubles)
constexpr int kTmpRow = 9;

struct K1WaveLds {
    uint32_t rgbx[16 * kRgbPitch];  // packed R | G<<8 | B<<16
    double tmp[8 * kTmpBlock];      // pass-1 output, transposed
};
constexpr int kQRow = 9;  // padded q-table rows: lanes reading rows j=0..7 hit distinct banks

// (JPGE_K1_LUT: the builds that map every staged word through the context's channel tables, see
// "channel tables" below)
#ifndef JPGE_K1_LUT
#define JPGE_K1_LUT 0
#endif
constexpr int kLutWords = kLutBytes / 4;

template <int kWaves>
struct K1Lds {
    K1WaveLds w[kWaves];
    uint32_t next;  // next tile of the workgroup's run to hand out
#if JPGE_K1_LUT
    uint32_t lut[kLutWords];  // the frame's channel tables: bytes T_R[0..255], T_G[0..255], T_B[0..255]
#endif
    double q[2][8 * kQRow];     // luma, chroma
    double invq[2][8 * kQRow];  // s_u / q (correctly rounded), u = column
};

__device__ __forceinline__ double ycc_exact_y(uint32_t p) {
    const double r = (double)(p & 0xFF), g = (double)((p >> 8) & 0xFF), b = (double)(p >> 16);
    // (0 + ((.299 r + .587 g) + .114 b)) - 128 : every partial result is exact
    return __builtin_fma(kYb, b, __builtin_fma(kYg, g, __builtin_fma(kYr, r, -128.0)));
}

__device__ __forceinline__ double ycc_ref_y(uint32_t p, double scale) {
    const double r = (double)(p & 0xFF) * scale, g = (double)((p >> 8) & 0xFF) * scale,
                 b = (double)(p >> 16) * scale;
    return (0.0 + ((kYr * r + kYg * g) + kYb * b)) - 128;
}

__device__ __forceinline__ double ycc_ref_c(uint32_t p, double scale, double kr, double kg, double kb) {
    const double r = (double)(p & 0xFF) * scale, g = (double)((p >> 8) & 0xFF) * scale,
                 b = (double)(p >> 16) * scale;
    return (128.0 + ((kr * r + kg * g) + kb * b)) - 128;
}

// exact chroma of one 8-bit pixel: (128 + v) - 128 == v, v exact
__device__ __forceinline__ double ycc_exact_c(uint32_t p, double kr, double kg, double kb) {
    const double r = (double)(p & 0xFF), g = (double)((p >> 8) & 0xFF), b = (double)(p >> 16);
    return __builtin_fma(kb, b, __builtin_fma(kg, g, kr * r));
}

// The prologue reads its constants without vector loads: a vector load issued after
// the first tile's pixel loads waits for them (the vector memory counter retires in
// order), which held every workgroup's prologue for the start-up burst (~3.5 us).
// kS[u] as a select over the constants (no load from the constant table):
__device__ __forceinline__ double arai_scale(int u) {
    double r = kS[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) r = u == i ? kS[i] : r;
    return r;
}
// quantiser entry tid (< 128) of the kernel arguments, through scalar loads (the
// array is 16-byte aligned in FdctArgs):
__device__ __forceinline__ uint32_t q_entry(const FdctArgs& a, int tid) {
    const uint32_t* qw = reinterpret_cast<const uint32_t*>(a.q);
    uint32_t w = 0;
#pragma unroll
    for (int i = 0; i < 32; ++i) w = (tid >> 2) == i ? qw[i] : w;
    return (w >> (8 * (tid & 3))) & 0xFF;
}

// v_permlane32_swap on a double pair: lanes 32-63 of a trade places with lanes 0-31
// of b (a keeps its low half, b its high half).
__device__ __forceinline__ void swap_halves(double& a, double& b) {
    const uint64_t ua = __builtin_bit_cast(uint64_t, a), ub = __builtin_bit_cast(uint64_t, b);
    const auto lo = __builtin_amdgcn_permlane32_swap((uint32_t)ua, (uint32_t)ub, false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap((uint32_t)(ua >> 32), (uint32_t)(ub >> 32), false, false);
    a = __builtin_bit_cast(double, ((uint64_t)hi[0] << 32) | lo[0]);
    b = __builtin_bit_cast(double, ((uint64_t)hi[1] << 32) | lo[1]);
}

// ---- input layouts ----
// This file is built once per load shape (kernels.hpp kShape*; JPGE_K1_SHAPE, default
// the RGB8 shape): the shape decides what a lane loads for its 16-pixel run and how the
// run becomes 16 staged words R | G<<8 | B<<16.  Everything after the staging is the
// same code in every build.  The kernels have internal linkage, so each build has its
// own; the RGB8 build also holds the launch entry points, which dispatch by shape.
#ifndef JPGE_K1_SHAPE
#define JPGE_K1_SHAPE 0
#endif
constexpr int kShape = JPGE_K1_SHAPE;
static_assert(kShape >= kShapeRgb8 && kShape <= kShapeBayer8, "JPGE_K1_SHAPE");
// The Y, Cb, Cr shapes (NV12, I420, planar 4:4:4) stage words Y | Cb<<8 | Cr<<16, a 4:2:0
// layout's chroma sample in each pixel of its 2x2 cell, and read them back without a colour
// conversion: a sample v is v - 128.  NV12 and I420 run the kFiltS420 instance, which
// takes each cell's top-left word: no chroma filter.  maxval is 255.  Their !kExact instances
// (FdctArgs::xf_on) convert each staged word by the context's sample transform (XfK below)
// on its way to a double; nothing else differs.
// The gray shape stages words that hold Y alone and has the row-8 kernel's one-component
// instance only: 16 one-block MCUs per tile, the two Y rounds, no chroma rounds.
// The Bayer shape stages the RGB shapes' words R | G<<8 | B<<16, each the bilinear demosaic of a raw
// byte and its 3x3 neighbourhood ("Bayer loads" below), and has the kExact instances only (maxval is
// 255), in 4-wave workgroups and frame sets, as the downscaling and the oriented builds.
constexpr bool kBayer = kShape == kShapeBayer8;
constexpr bool kYuv = kShape >= kShapeNv12 && !kBayer;
constexpr bool kGray = kShape == kShapeGray;
// The 10-bit 4:2:0 shapes (P010, I010) stage words s_y | s_cb<<10 | s_cr<<20 of 10-bit samples s,
// each the exact fp64 value s / 4 in 8-bit units, and have the !kExact instances only: the
// sample transform always runs (FULL_601: with the identity), because its clamps are what
// keeps 1023 / 4 = 255.75 inside an 8-bit sample's interval.
// The 10-bit 4:2:2 shapes (Y210, P210, I210) stage the same ten-bit words, a cell's chroma pair in
// both of its pixels (cell x >> 1 of the pixel's own row), and have the !kExact instance of every
// kernel the planar 4:4:4 shape has: each mode's filter runs on the chroma-repeated frame.
// The v210 shape stages the same words from 32-bit words of three samples: ten-bit 4:2:2 with no
// chroma descriptors and no plane_stride, like Y210, its samples neither the top nor the low 10
// bits of a 16-bit word (kTenHi does not apply); its loads and its unpack depend on the lane's
// phase ("v210" below).
constexpr bool kV210 = kShape == kShapeV210;
constexpr bool kTen422 = kShape == kShapeY210 || kShape == kShapeP210 || kShape == kShapeI210 || kV210;
constexpr bool kTen = kShape == kShapeP010 || kShape == kShapeI010 || kTen422;
constexpr bool kTenHi = kShape == kShapeP010 || kShape == kShapeP210;  // planes of words that hold a sample in their top 10 bits
constexpr bool kYuv420 = kShape == kShapeNv12 || kShape == kShapeI420 || (kTen && !kTen422);
// The 4:2:2 shapes (YUYV / UYVY, NV16, I422) stage the same words, a cell's chroma sample in
// both of its pixels (cell x >> 1 of the pixel's own row), and have every instance the planar
// 4:4:4 shape has: each mode's filter then runs on the chroma-repeated frame.  In 4:2:2 the
// row-8 kernel keeps the first word of each pair: the cell's sample, no arithmetic.
constexpr bool kPacked422 = kShape == kShapePacked422;
constexpr bool kPlanes422 = kShape == kShapeNv16 || kShape == kShapeI422;  // chroma loads of their own, row = pixel row
constexpr bool kPairs = kShape == kShapeNv12 || kShape == kShapeNv16;      // Cb,Cr byte pairs
constexpr bool kHalfPitch = kShape == kShapeI420 || kShape == kShapeI422;  // chroma pitch (stride + 1) / 2
constexpr uint32_t kBpp = kShape == kShapeX4 || kShape == kShapeY210 ? 4u : kPacked422 || kTen ? 2u : kShape == kShapePlanar || kYuv || kBayer ? 1u : 3u;  // bytes per pixel along a row
constexpr uint32_t kRun = 16 * kBpp;  // bytes of a lane's 16-pixel run (of one plane)
// The downscaling builds (JPGE_K1_DS 2 or 4; FdctArgs::ds) of the RGB8, BGR8, 4-byte and NV12
// shapes: a staged word holds the rounded means of kDs x kDs source samples, so the lane's run
// comes from 16 * kDs source pixels on kDs rows ("downscaling loads" below).  The tile, the
// staged words and everything after the staging are those of the frame of ceil(src / kDs) pixels.
#ifndef JPGE_K1_DS
#define JPGE_K1_DS 1
#endif
constexpr int kDs = JPGE_K1_DS;
static_assert(kDs == 1 || ((kDs == 2 || kDs == 4) && (kShape <= kShapeX4 || kShape == kShapeNv12)), "JPGE_K1_DS");
constexpr uint32_t kDsBits = kDs == 4 ? 4u : kDs == 2 ? 2u : 0u;  // log2 of the samples of a mean
constexpr uint32_t kDsHalf = (1u << kDsBits) >> 1;                // round half up
constexpr uint32_t kSelRgbx = 0x0C020100u, kSelBgrx = 0x0C000102u;  // perm selectors of a 4-byte pixel (0x0c: zero)
// The oriented builds (JPGE_K1_ORIENT 1..4, kernels.hpp orient_class; FdctArgs::orient) of the RGB8,
// BGR8 and 4-byte shapes: g is the oriented frame O, read from the src_w x src_h source.  A lane
// loads the same kRun bytes of one source row; what changes is which row and start column, the
// order its 16 words are staged in (mirrored: reversed, a renaming of registers) and, transposed,
// where they go: down a column of the staged tile ("oriented loads" in fdct_kernel).  Whether the
// source's rows run backwards is a wave-uniform scalar of the frame (orient_rows_back).  The tile,
// the staged words and everything after the staging are O's.  4-wave workgroups and frame sets only.
#ifndef JPGE_K1_ORIENT
#define JPGE_K1_ORIENT 0
#endif
constexpr int kOrient = JPGE_K1_ORIENT;
static_assert(kOrient == 0 || (kOrient >= 1 && kOrient <= 4 && kDs == 1 && kShape <= kShapeX4), "JPGE_K1_ORIENT");
constexpr bool kOrMirror = kOrient == 2 || kOrient == 4;  // the source's columns run backwards
constexpr bool kOrTrans = kOrient >= 3;                   // O's rows are the source's columns (fdct_kernel only)
// ---- channel tables (JPGE_K1_LUT 1; kernels.hpp fdct_lut) ----
// The builds of the RGB8, BGR8, 4-byte and Bayer shapes for a context with per-channel lookup
// tables (jpge_set_channel_lut): every staged word R | G<<8 | B<<16 becomes
// T_R[R] | T_G[G]<<8 | T_B[B]<<16 before it is written to the staged tile, on the fast path and on
// the byte paths alike (the clamped path fills the same 16 registers; the Bayer shape's rolled byte
// loop, which writes its words itself, maps each as it writes it).  Everything after the staging
// reads the mapped frame.  kExact instances, 4-wave workgroups and frame sets only, as the Bayer build.
// The tables are 768 bytes of LDS, one copy per workgroup, loaded in the prologue from the frame's
// own pointer.  A channel's 256 bytes are 64 consecutive words, two to each of the 32 banks a 32-bit
// read sees: lanes that read the same word are served together, so a read of random samples is a
// 2-way conflict at the worst, whatever the pixels are.  (256 packed words T_R | T_G<<8 | T_B<<16,
// one b32 read per channel and a byte select, would put eight words in each bank, up to 8-way, and
// need a scaled address per channel.)  A pixel costs three byte reads at the immediate offsets 0,
// 256, 512, three field extractions and two v_lshl_or_b32.
constexpr bool kLut = JPGE_K1_LUT != 0;
static_assert(!kLut || (kDs == 1 && kOrient == 0 && (kShape == kShapeRgb8 || kShape == kShapeBgr8 || kShape == kShapeX4 || kShape == kShapeBayer8)),
              "JPGE_K1_LUT");
// the mapped word of a staged word p (byte 3 of p is zero); t: the workgroup's tables in LDS
__device__ __forceinline__ uint32_t lut_map(const uint8_t* t, uint32_t p) {
    const uint32_t r = t[p & 0xFF], g = t[256 + ((p >> 8) & 0xFF)], b = t[512 + (p >> 16)];
    return r | (g << 8) | (b << 16);
}

// perm selector of a 3-byte pixel starting at byte o8 of a word pair
__device__ __forceinline__ constexpr uint32_t sel3(uint32_t o8) {
    return kShape == kShapeBgr8 ? 0x0C000000u | (o8 << 16) | ((o8 + 1) << 8) | (o8 + 2)
                                : 0x0C000000u | ((o8 + 2) << 16) | ((o8 + 1) << 8) | o8;
}
// The prefetched run of a lane as 16 staged words, 4-byte and planar shapes: v0..v3 are
// the four loads, or v0, v1, v2 the R, G, B planes' 16 bytes.  (The 3-byte shapes unpack
// in the kernels.)
__device__ __forceinline__ void unpack_run(const uint4& v0, const uint4& v1, const uint4& v2, const uint4& v3,
                                           uint32_t sel4, uint32_t px[16]) {
    if constexpr (kShape == kShapeX4) {
        // the loaded word, alpha cleared (RGBA) or bytes 2,1,0 (BGRA): one perm either way
        const uint32_t wd[16] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w,
                                 v2.x, v2.y, v2.z, v2.w, v3.x, v3.y, v3.z, v3.w};
#pragma unroll
        for (int i = 0; i < 16; ++i) px[i] = __builtin_amdgcn_perm(0u, wd[i], sel4);
    } else if constexpr (kShape == kShapePlanar || kShape == kShapeYuv444) {
        const uint32_t r[4] = {v0.x, v0.y, v0.z, v0.w}, g[4] = {v1.x, v1.y, v1.z, v1.w}, b[4] = {v2.x, v2.y, v2.z, v2.w};
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t o8 = (uint32_t)(i & 3);
            const uint32_t rg = __builtin_amdgcn_perm(g[i >> 2], r[i >> 2], 0x0C0C0000u | ((4 + o8) << 8) | o8);
            px[i] = __builtin_amdgcn_perm(b[i >> 2], rg, 0x0C000100u | ((4 + o8) << 16));
        }
    }
}
// The packed 4:2:2 shape's run: v0, v1 its 8 groups of 4 bytes, Y0 Cb Y1 Cr or Cb Y0 Cr Y1.
// sel4 selects Y0, Cb, Cr of a group (the even pixel); the odd pixel's Y1 lies two bytes on.
constexpr uint32_t kSelYuyv = 0x0C030100u, kSelUyvy = 0x0C020001u;
__device__ __forceinline__ void unpack_packed422(const uint4& v0, const uint4& v1, uint32_t sel4, uint32_t px[16]) {
    const uint32_t wd[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
    for (int i = 0; i < 16; ++i) px[i] = __builtin_amdgcn_perm(0u, wd[i >> 1], sel4 + 2u * (uint32_t)(i & 1));
}
// The 4:2:0 layouts' run: v0 the 16 Y bytes; NV12: v1 the 8 Cb,Cr pairs of the run's cells;
// I420: v1, v2 16 Cb and 16 Cr bytes, of which the run's cells are the low (half = 0) or
// high 8.  Pixel i takes the chroma of cell i / 2.  (NV16 and I422: the same bytes, of the
// pixels' own chroma row.)
__device__ __forceinline__ void unpack_yuv420(const uint4& v0, const uint4& v1, const uint4& v2, uint32_t half,
                                              uint32_t px[16]) {
    const uint32_t y[4] = {v0.x, v0.y, v0.z, v0.w};
    if constexpr (kPairs) {
        const uint32_t c[4] = {v1.x, v1.y, v1.z, v1.w};
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t o8 = (uint32_t)(i & 3), c8 = 4 + 2 * (uint32_t)((i >> 1) & 1);  // the pair's bytes of c[i / 4]
            px[i] = __builtin_amdgcn_perm(c[i >> 2], y[i >> 2], 0x0C000000u | ((c8 + 1) << 16) | (c8 << 8) | o8);
        }
    } else {
        const uint32_t cb[2] = {half ? v1.z : v1.x, half ? v1.w : v1.y}, cr[2] = {half ? v2.z : v2.x, half ? v2.w : v2.y};
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t o8 = (uint32_t)(i & 3), c8 = 4 + (uint32_t)((i >> 1) & 3);
            const uint32_t yb = __builtin_amdgcn_perm(cb[i >> 3], y[i >> 2], 0x0C0C0000u | (c8 << 8) | o8);
            px[i] = __builtin_amdgcn_perm(cr[i >> 3], yb, 0x0C000100u | (c8 << 16));
        }
    }
}
// The 10-bit layouts' run: v0, v1 the 16 Y words, two per register.  P010 (a sample is its
// word's top 10 bits): v2, v3 the 8 Cb,Cr word pairs of the run's cells, one per register.
// I010 (the low 10 bits): v2 the cells' 8 Cb words, v3 their 8 Cr words.  (P210 and I210: the
// same words, of the pixels' own chroma row.)  Y210 (the top 10 bits): v0..v3 the run's 8 groups
// Y0 Cb Y1 Cr, a group per register pair, Y0 | Cb << 16 and Y1 | Cr << 16.
__device__ __forceinline__ void unpack_yuv10(const uint4& v0, const uint4& v1, const uint4& v2, const uint4& v3,
                                             uint32_t px[16]) {
    if constexpr (kShape == kShapeY210) {
        const uint32_t g[16] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w, v3.x, v3.y, v3.z, v3.w};
#pragma unroll
        for (int cell = 0; cell < 8; ++cell) {
            const uint32_t a = g[2 * cell], b = g[2 * cell + 1];
            const uint32_t cc = ((a >> 12) & 0x000FFC00u) | ((b >> 2) & 0x3FF00000u);  // s_cb << 10 | s_cr << 20
            px[2 * cell] = __builtin_amdgcn_ubfe(a, 6u, 10u) | cc;
            px[2 * cell + 1] = __builtin_amdgcn_ubfe(b, 6u, 10u) | cc;
        }
        return;
    }
    const uint32_t y[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    const uint32_t c[8] = {v2.x, v2.y, v2.z, v2.w, v3.x, v3.y, v3.z, v3.w};
    constexpr uint32_t lo = kTenHi ? 6u : 0u;  // the sample's first bit in its word
#pragma unroll
    for (int cell = 0; cell < 8; ++cell) {
        uint32_t cc;  // s_cb << 10 | s_cr << 20
        if constexpr (kTenHi) {
            cc = ((c[cell] << 4) & 0x000FFC00u) | ((c[cell] >> 2) & 0x3FF00000u);
        } else {
            const uint32_t sh = 16u * (uint32_t)(cell & 1);
            cc = (__builtin_amdgcn_ubfe(c[cell >> 1], sh, 10u) << 10) | (__builtin_amdgcn_ubfe(c[4 + (cell >> 1)], sh, 10u) << 20);
        }
        px[2 * cell] = __builtin_amdgcn_ubfe(y[cell], lo, 10u) | cc;
        px[2 * cell + 1] = __builtin_amdgcn_ubfe(y[cell], 16u + lo, 10u) | cc;
    }
}
// v210: a row is groups of four 32-bit words (16 bytes) that hold six pixels, three samples to
// a word at bits 0-9, 10-19, 20-29:
//   w0 = Cb0 Y0 Cr0,  w1 = Y1 Cb1 Y2,  w2 = Cr1 Y3 Cb2,  w3 = Y4 Cr2 Y5
// A lane's run n = xs / 16 (16 pixels = 2 2/3 groups) starts p = 16 n - 6 g0 pixels into group
// g0 = floor(8 n / 3): with n = 3 q + r, g0 = 8 q + {0, 2, 5}[r] and p = {0, 4, 2}[r], always even,
// so that a cell never straddles two runs.  The run lies in groups g0 .. g0 + 2 (r = 1: g0 + 3,
// whose first cell holds its last two pixels).  r differs between the lanes of a wave.
// The unpack is branch-free: v0..v3 are the four groups; their first 20 pixels become staged
// words c[0..19] with compile-time words and fields, and pixel i of the run is c[i + p], chosen
// by two selects on the lane's r.  (A lane with r != 1 has zeros in v3 and never selects them.)
__device__ __forceinline__ void unpack_v210(const uint4& v0, const uint4& v1, const uint4& v2, const uint4& v3,
                                            uint32_t r, uint32_t px[16]) {
    const uint32_t w[16] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w, v3.x, v3.y, v3.z, v3.w};
    uint32_t c[24];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const uint32_t w0 = w[4 * g], w1 = w[4 * g + 1], w2 = w[4 * g + 2], w3 = w[4 * g + 3];
        // s_cb << 10 | s_cr << 20 of the group's three cells
        const uint32_t cc0 = ((w0 << 10) & 0x000FFC00u) | (w0 & 0x3FF00000u);
        const uint32_t cc1 = (w1 & 0x000FFC00u) | ((w2 << 20) & 0x3FF00000u);
        const uint32_t cc2 = ((w2 >> 10) & 0x000FFC00u) | ((w3 << 10) & 0x3FF00000u);
        c[6 * g] = __builtin_amdgcn_ubfe(w0, 10u, 10u) | cc0;
        c[6 * g + 1] = (w1 & 0x3FFu) | cc0;
        c[6 * g + 2] = __builtin_amdgcn_ubfe(w1, 20u, 10u) | cc1;
        c[6 * g + 3] = __builtin_amdgcn_ubfe(w2, 10u, 10u) | cc1;
        c[6 * g + 4] = (w3 & 0x3FFu) | cc2;
        c[6 * g + 5] = __builtin_amdgcn_ubfe(w3, 20u, 10u) | cc2;
    }
    // the selects as bit masks (all ones or zero per lane), opaque to the compiler, which
    // otherwise turns each ternary into a divergent branch: two v_bfi_b32 per pixel
    uint32_t m1 = r == 1 ? ~0u : 0u, m2 = r == 2 ? ~0u : 0u;
    asm("" : "+v"(m1), "+v"(m2));
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        // (z ^ (m & (y ^ z)): the form the back end matches to v_bfi_b32 m, y, z)
        const uint32_t a = c[i] ^ (m2 & (c[i + 2] ^ c[i]));
        px[i] = a ^ (m1 & (c[i + 4] ^ a));  // (c[20..23] are never read)
    }
}
// The gray shape's run: the load's 16 bytes, one per staged word.
__device__ __forceinline__ void unpack_gray(const uint4& v0, uint32_t px[16]) {
    const uint32_t y[4] = {v0.x, v0.y, v0.z, v0.w};
#pragma unroll
    for (int i = 0; i < 16; ++i) px[i] = __builtin_amdgcn_perm(0u, y[i >> 2], 0x0C0C0C00u | (uint32_t)(i & 3));
}
// a staged word's samples (exact: integers)
__device__ __forceinline__ double yuv_y(uint32_t p) { return (double)(p & 0xFF) - 128.0; }
__device__ __forceinline__ double yuv_c(uint32_t p, int comp) {
    // (10-bit fields: s / 4, exact)
    if constexpr (kTen) return (double)((p >> (10 * comp)) & 0x3FF) * 0.25 - 128.0;
    return (double)((p >> (8 * comp)) & 0xFF) - 128.0;
}

// The sample transform of the Y, Cb, Cr shapes' !kExact instances (host_io.hpp YuvXf: limited
// range, BT.709 or the caller's coefficients): wave-uniform, held in scalar registers.  Every
// product and sum is rounded on its own, in the order written (no contraction: the bytes
// are defined by it, as ycc_ref_y's are).  The clamps keep a converted sample inside the
// interval of an 8-bit one, [-128, 127], whatever the input: the coefficient bounds of the
// entropy stage (DC category <= 11, AC size <= 10) rest on it.
struct XfK {
    double y_off, m0, m1, m2, m3, m4, m5, m6;
};
__device__ __forceinline__ double xf_clamp_y(double s) { return __builtin_fmin(__builtin_fmax(s, 0.0), 255.0) - 128.0; }
// Y' of a word's Y byte, given the products t1 = m1 u, t2 = m2 v of its chroma
__device__ __forceinline__ double xf_y(const XfK& k, uint32_t p, double t1, double t2) {
    const double yc = kTen ? (double)(p & 0x3FF) * 0.25 - k.y_off : (double)(p & 0xFF) - k.y_off;  // (10-bit: s / 4, exact)
    if constexpr (kGray) return xf_clamp_y(k.m0 * yc);  // (one component: y_off and m0 only)
    return xf_clamp_y((k.m0 * yc + t1) + t2);
}
__device__ __forceinline__ double xf_y(const XfK& k, uint32_t p) {
    return xf_y(k, p, k.m1 * yuv_c(p, 1), k.m2 * yuv_c(p, 2));
}
// Cb' (ku = m3, kv = m4) or Cr' (m5, m6) of a word
__device__ __forceinline__ double xf_c(uint32_t p, double ku, double kv) {
    const double s = ku * yuv_c(p, 1) + kv * yuv_c(p, 2);
    return __builtin_fmin(__builtin_fmax(s, -128.0), 127.0);
}
// the coefficients of a's transform, by scalar loads (the prologue issues no vector load,
// see above), pinned: the tile loop would otherwise reload them
__device__ __forceinline__ XfK xf_load(const FdctArgs& a) {
    XfK k{a.xf[0], a.xf[1], a.xf[2], a.xf[3], a.xf[4], a.xf[5], a.xf[6], a.xf[7]};
    asm volatile("" : "+s"(k.y_off), "+s"(k.m0), "+s"(k.m1), "+s"(k.m2), "+s"(k.m3), "+s"(k.m4), "+s"(k.m5), "+s"(k.m6));
    return k;
}

// One pixel of the Y, Cb, Cr shapes' clamped edge path: row sy, column sx (inside the
// frame); a 4:2:0 layout's chroma of the pixel's cell (inside the chroma plane: the
// clamped pixel's cell is the clamped cell).
__device__ __forceinline__ uint32_t edge_yuv(const uint8_t* base, uint64_t stride, uint64_t plane_stride, uint32_t gh,
                                             uint32_t sel4, uint32_t sy, uint32_t sx) {
    if constexpr (kPacked422) {
        // the pixel's group, by byte loads (it may be unaligned); the odd pixel's Y two bytes on
        const uint8_t* p = base + (uint64_t)sy * stride + 4 * (uint64_t)(sx >> 1);
        const uint32_t w = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
        return __builtin_amdgcn_perm(0u, w, sel4 + 2u * (sx & 1));
    }
    if constexpr (kV210) {
        // the pixel's group of four 32-bit words; sample s of the group's stream is field s % 3 of
        // word s / 3, each word by four byte loads (any base and pitch that are multiples of 4)
        const uint32_t g = sx / 6, k = sx - 6 * g, c = k >> 1;
        const uint8_t* p = base + (uint64_t)sy * stride + 16 * (uint64_t)g;
        auto sample = [p](uint32_t s) {
            const uint8_t* q = p + 4 * (s / 3);
            const uint32_t w = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
            return (w >> (10 * (s % 3))) & 0x3FFu;
        };
        return sample(2 * k + 1) | (sample(4 * c) << 10) | (sample(4 * c + 2) << 20);
    } else if constexpr (kTen) {
        // 16-bit little-endian words, by byte loads: P010 the word's top 10 bits, Cb,Cr word
        // pairs in rows of pitch stride; I010 the low 10 bits, planes of pitch 2 * ceil(stride / 4)
        auto word = [](const uint8_t* q) { return (uint32_t)q[0] | ((uint32_t)q[1] << 8); };
        // (the 4:2:2 ones: the pixel's own chroma row; Y210: the pixel's group of four words)
        if constexpr (kShape == kShapeY210) {
            const uint8_t* p = base + (uint64_t)sy * stride + 8 * (uint64_t)(sx >> 1);
            return (word(p + 4 * (sx & 1)) >> 6) | ((word(p + 2) >> 6) << 10) | ((word(p + 6) >> 6) << 20);
        }
        const uint8_t* c = base + plane_stride;
        if constexpr (kShape == kShapeP210) {
            c += (uint64_t)sy * stride + 4 * (uint64_t)(sx >> 1);
            return (word(base + (uint64_t)sy * stride + 2 * (uint64_t)sx) >> 6) | ((word(c) >> 6) << 10) | ((word(c + 2) >> 6) << 20);
        } else if constexpr (kShape == kShapeI210) {
            const uint64_t cs = 2 * ((stride + 3) / 4);
            c += (uint64_t)sy * cs + 2 * (uint64_t)(sx >> 1);
            return (word(base + (uint64_t)sy * stride + 2 * (uint64_t)sx) & 0x3FF) | ((word(c) & 0x3FF) << 10) |
                   ((word(c + cs * gh) & 0x3FF) << 20);
        } else if constexpr (kShape == kShapeP010) {
            c += (uint64_t)(sy >> 1) * stride + 4 * (uint64_t)(sx >> 1);
            return (word(base + (uint64_t)sy * stride + 2 * (uint64_t)sx) >> 6) | ((word(c) >> 6) << 10) | ((word(c + 2) >> 6) << 20);
        } else {
            const uint64_t cs = 2 * ((stride + 3) / 4);
            c += (uint64_t)(sy >> 1) * cs + 2 * (uint64_t)(sx >> 1);
            return (word(base + (uint64_t)sy * stride + 2 * (uint64_t)sx) & 0x3FF) | ((word(c) & 0x3FF) << 10) |
                   ((word(c + cs * ((gh + 1) / 2)) & 0x3FF) << 20);
        }
    }
    const uint32_t yv = base[(uint64_t)sy * stride + sx];
    const uint8_t* c = base + plane_stride;
    if constexpr (kGray) {
        return yv;
    } else if constexpr (kShape == kShapeNv16) {
        c += (uint64_t)sy * stride + 2 * (uint64_t)(sx >> 1);
        return yv | ((uint32_t)c[0] << 8) | ((uint32_t)c[1] << 16);
    } else if constexpr (kShape == kShapeI422) {
        const uint64_t cs = (stride + 1) / 2;
        c += (uint64_t)sy * cs + (sx >> 1);
        return yv | ((uint32_t)c[0] << 8) | ((uint32_t)c[cs * gh] << 16);
    } else if constexpr (kShape == kShapeNv12) {
        c += (uint64_t)(sy >> 1) * stride + 2 * (uint64_t)(sx >> 1);
        return yv | ((uint32_t)c[0] << 8) | ((uint32_t)c[1] << 16);
    } else if constexpr (kShape == kShapeI420) {
        const uint64_t cs = (stride + 1) / 2;
        c += (uint64_t)(sy >> 1) * cs + (sx >> 1);
        return yv | ((uint32_t)c[0] << 8) | ((uint32_t)c[cs * ((gh + 1) / 2)] << 16);
    } else {
        c += (uint64_t)sy * stride + sx;
        return yv | ((uint32_t)c[0] << 8) | ((uint32_t)c[plane_stride] << 16);
    }
}

// One pixel of the clamped edge path: row sy, column sx (inside the frame).
__device__ __forceinline__ uint32_t edge_pixel(const uint8_t* rgb, uint64_t stride, uint64_t plane_stride,
                                               uint32_t sel4, uint32_t sy, uint32_t sx) {
    const uint8_t* p = rgb + (uint64_t)sy * stride + (uint64_t)sx * kBpp;
    if constexpr (kShape == kShapePlanar)
        return (uint32_t)p[0] | ((uint32_t)p[plane_stride] << 8) | ((uint32_t)p[2 * plane_stride] << 16);
    else if constexpr (kShape == kShapeBgr8)
        return (uint32_t)p[2] | ((uint32_t)p[1] << 8) | ((uint32_t)p[0] << 16);
    else if constexpr (kShape == kShapeX4)  // (byte loads: the pixel may be unaligned)
        return __builtin_amdgcn_perm(0u, (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16), sel4);
    else
        return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
}

// Descriptors of the pixel loads: the frame's rows (planar: one per plane; the others
// repeat the first and are unused).  A lane's loads of a tile on the fast path end
// inside their row, so the range is the last row's end.
struct RgbRsrc {
    __amdgpu_buffer_rsrc_t p0;
#if JPGE_K1_SHAPE >= 3 && JPGE_K1_SHAPE != 7 && JPGE_K1_SHAPE != 8 && JPGE_K1_SHAPE != 13 && JPGE_K1_SHAPE != 16 && JPGE_K1_SHAPE != 17
    __amdgpu_buffer_rsrc_t p1, p2;  // (NV12, NV16: p2 repeats p1, unused)
#endif
};
__device__ __forceinline__ RgbRsrc rgb_rsrc(const uint8_t* rgb, uint64_t stride, uint64_t plane_stride, uint32_t gw,
                                            uint32_t gh) {
    // (packed 4:2:2: a row is ceil(gw / 2) whole groups, of 4 bytes or, Y210, 8)
    // (v210: ceil(gw / 6) whole 16-byte groups)
    const int range = kV210 ? (int)(uint32_t)((uint64_t)stride * (gh - 1) + 16 * (((uint64_t)gw + 5) / 6)) :
        (int)(uint32_t)((uint64_t)stride * (gh - 1) + (kPacked422 || kShape == kShapeY210 ? kBpp * 2 * (uint64_t)((gw + 1) / 2) : (uint64_t)kBpp * gw));
    uint8_t* b = const_cast<uint8_t*>(rgb);
    RgbRsrc r;
    r.p0 = __builtin_amdgcn_make_buffer_rsrc(b, 0, range, 0x00020000);
#if JPGE_K1_SHAPE == 3 || JPGE_K1_SHAPE == 6
    r.p1 = __builtin_amdgcn_make_buffer_rsrc(b + plane_stride, 0, range, 0x00020000);
    r.p2 = __builtin_amdgcn_make_buffer_rsrc(b + 2 * plane_stride, 0, range, 0x00020000);
#elif JPGE_K1_SHAPE == 4
    // the Cb,Cr plane: ch rows of pitch stride, 2 * cw bytes each
    const uint32_t cw = (gw + 1) / 2, ch = (gh + 1) / 2;
    r.p1 = __builtin_amdgcn_make_buffer_rsrc(b + plane_stride, 0, (int)(uint32_t)(stride * (ch - 1) + 2 * (uint64_t)cw),
                                             0x00020000);
    r.p2 = r.p1;
#elif JPGE_K1_SHAPE == 5
    // the Cb plane, then the Cr plane: ch rows of pitch cs, cw bytes each
    const uint32_t cw = (gw + 1) / 2, ch = (gh + 1) / 2;
    const uint64_t cs = (stride + 1) / 2;
    const int crange = (int)(uint32_t)(cs * (ch - 1) + cw);
    r.p1 = __builtin_amdgcn_make_buffer_rsrc(b + plane_stride, 0, crange, 0x00020000);
    r.p2 = __builtin_amdgcn_make_buffer_rsrc(b + plane_stride + cs * ch, 0, crange, 0x00020000);
#elif JPGE_K1_SHAPE == 9
    // the Cb,Cr plane: gh rows of pitch stride, 2 * cw bytes each
    const uint32_t cw = (gw + 1) / 2;
    r.p1 = __builtin_amdgcn_make_buffer_rsrc(b + plane_stride, 0, (int)(uint32_t)(stride * (gh - 1) + 2 * (uint64_t)cw),
                                             0x00020000);
    r.p2 = r.p1;
#elif JPGE_K1_SHAPE == 11
    // the Cb,Cr plane: ch rows of pitch stride, cw pairs of 16-bit words each
    const uint32_t cw = (gw + 1) / 2, ch = (gh + 1) / 2;
    r.p1 = __builtin_amdgcn_make_buffer_rsrc(b + plane_stride, 0, (int)(uint32_t)(stride * (ch - 1) + 4 * (uint64_t)cw),
                                             0x00020000);
    r.p2 = r.p1;
#elif JPGE_K1_SHAPE == 12
    // the Cb plane, then the Cr plane: ch rows of pitch cs, cw 16-bit words each
    const uint32_t cw = (gw + 1) / 2, ch = (gh + 1) / 2;
    const uint64_t cs = 2 * ((stride + 3) / 4);
    const int crange = (int)(uint32_t)(cs * (ch - 1) + 2 * (uint64_t)cw);
    r.p1 = __builtin_amdgcn_make_buffer_rsrc(b + plane_stride, 0, crange, 0x00020000);
    r.p2 = __builtin_amdgcn_make_buffer_rsrc(b + plane_stride + cs * ch, 0, crange, 0x00020000);
#elif JPGE_K1_SHAPE == 14
    // the Cb,Cr plane: gh rows of pitch stride, cw pairs of 16-bit words each
    const uint32_t cw = (gw + 1) / 2;
    r.p1 = __builtin_amdgcn_make_buffer_rsrc(b + plane_stride, 0, (int)(uint32_t)(stride * (gh - 1) + 4 * (uint64_t)cw),
                                             0x00020000);
    r.p2 = r.p1;
#elif JPGE_K1_SHAPE == 15
    // the Cb plane, then the Cr plane: gh rows of pitch cs, cw 16-bit words each
    const uint32_t cw = (gw + 1) / 2;
    const uint64_t cs = 2 * ((stride + 3) / 4);
    const int crange = (int)(uint32_t)(cs * (gh - 1) + 2 * (uint64_t)cw);
    r.p1 = __builtin_amdgcn_make_buffer_rsrc(b + plane_stride, 0, crange, 0x00020000);
    r.p2 = __builtin_amdgcn_make_buffer_rsrc(b + plane_stride + cs * gh, 0, crange, 0x00020000);
#elif JPGE_K1_SHAPE == 10
    // the Cb plane, then the Cr plane: gh rows of pitch cs, cw bytes each
    const uint32_t cw = (gw + 1) / 2;
    const uint64_t cs = (stride + 1) / 2;
    const int crange = (int)(uint32_t)(cs * (gh - 1) + cw);
    r.p1 = __builtin_amdgcn_make_buffer_rsrc(b + plane_stride, 0, crange, 0x00020000);
    r.p2 = __builtin_amdgcn_make_buffer_rsrc(b + plane_stride + cs * gh, 0, crange, 0x00020000);
#endif
    return r;
}
// the lane's run at buffer offset off (kOob: zeros); the 4:2:0, NV16 and I422 layouts' chroma at coff
__device__ __forceinline__ void load_run(const RgbRsrc& rs, uint32_t off, uint32_t coff, uint4& v0, uint4& v1, uint4& v2,
                                         uint4& v3) {
#if JPGE_K1_SHAPE == 3 || JPGE_K1_SHAPE == 6
    v0 = as_u4(__builtin_amdgcn_raw_buffer_load_b128(rs.p0, off, 0, 0));
    v1 = as_u4(__builtin_amdgcn_raw_buffer_load_b128(rs.p1, off, 0, 0));
    v2 = as_u4(__builtin_amdgcn_raw_buffer_load_b128(rs.p2, off, 0, 0));
#elif JPGE_K1_SHAPE == 4 || JPGE_K1_SHAPE == 9
    v0 = as_u4(__builtin_amdgcn_raw_buffer_load_b128(rs.p0, off, 0, 0));
    v1 = as_u4(__builtin_amdgcn_raw_buffer_load_b128(rs.p1, coff, 0, 0));
#elif JPGE_K1_SHAPE == 8
    v0 = as_u4(__builtin_amdgcn_raw_buffer_load_b128(rs.p0, off, 0, 0));
    v1 = as_u4(__builtin_amdgcn_raw_buffer_load_b128(rs.p0, off + 16, 0, 0));
#elif JPGE_K1_SHAPE == 5 || JPGE_K1_SHAPE == 10
    v0 = as_u4(__builtin_amdgcn_raw_buffer_load_b128(rs.p0, off, 0, 0));
    v1 = as_u4(__builtin_amdgcn_raw_buffer_load_b128(rs.p1, coff, 0, 0));
    v2 = as_u4(__builtin_amdgcn_raw_buffer_load_b128(rs.p2, coff, 0, 0));
#elif JPGE_K1_SHAPE == 7
    v0 = as_u4(__builtin_amdgcn_raw_buffer_load_b128(rs.p0, off, 0, 0));
#elif JPGE_K1_SHAPE == 13
    // the run's 8 groups
    v0 = as_u4(__builtin_amdgcn_raw_buffer_load_b128(rs.p0, off, 0, 0));
    v1 = as_u4(__builtin_amdgcn_raw_buffer_load_b128(rs.p0, off + 16, 0, 0));
    v2 = as_u4(__builtin_amdgcn_raw_buffer_load_b128(rs.p0, off + 32, 0, 0));
    v3 = as_u4(__builtin_amdgcn_raw_buffer_load_b128(rs.p0, off + 48, 0, 0));
#elif JPGE_K1_SHAPE == 16
    // groups g0, g0 + 1, g0 + 2 at off, and at coff group g0 + 3 (a lane that does not need it: kOob)
    v0 = as_u4(__builtin_amdgcn_raw_buffer_load_b128(rs.p0, off, 0, 0));
    v1 = as_u4(__builtin_amdgcn_raw_buffer_load_b128(rs.p0, off + 16, 0, 0));
    v2 = as_u4(__builtin_amdgcn_raw_buffer_load_b128(rs.p0, off + 32, 0, 0));
    v3 = as_u4(__builtin_amdgcn_raw_buffer_load_b128(rs.p0, coff, 0, 0));
#elif JPGE_K1_SHAPE == 11 || JPGE_K1_SHAPE == 12 || JPGE_K1_SHAPE == 14 || JPGE_K1_SHAPE == 15
    // 32 bytes of Y; P010, P210: the 32 bytes of Cb,Cr pairs under them; I010, I210: 16 bytes of each plane
    v0 = as_u4(__builtin_amdgcn_raw_buffer_load_b128(rs.p0, off, 0, 0));
    v1 = as_u4(__builtin_amdgcn_raw_buffer_load_b128(rs.p0, off + 16, 0, 0));
    v2 = as_u4(__builtin_amdgcn_raw_buffer_load_b128(rs.p1, coff, 0, 0));
    v3 = kTenHi ? as_u4(__builtin_amdgcn_raw_buffer_load_b128(rs.p1, coff + 16, 0, 0))
                              : as_u4(__builtin_amdgcn_raw_buffer_load_b128(rs.p2, coff, 0, 0));
#else
    v0 = as_u4(__builtin_amdgcn_raw_buffer_load_b128(rs.p0, off, 0, 0));
    v1 = as_u4(__builtin_amdgcn_raw_buffer_load_b128(rs.p0, off + 16, 0, 0));
    v2 = as_u4(__builtin_amdgcn_raw_buffer_load_b128(rs.p0, off + 32, 0, 0));
    if constexpr (kShape == kShapeX4) v3 = as_u4(__builtin_amdgcn_raw_buffer_load_b128(rs.p0, off + 48, 0, 0));
#endif
}

// ---- Bayer loads (kBayer) ----
// A lane's run of 16 output pixels on row y, columns xs .. xs + 15, needs raw rows y - 1, y, y + 1 and
// columns xs - 1 .. xs + 16.  The reflection of jpge.h (row -1 is row 1, row gh is row gh - 2, the
// columns likewise) is applied to the addresses: the lane loads 16 bytes of each of the three rows
// and the byte on either side of each, six narrow loads, every one inside the frame's rows.  So the
// fast path's conditions are the RGB shapes': an aligned source, and the run inside the frame.  The
// rows above and below are the neighbouring lanes' own rows, from the L1.
// (ya, ym, yb: the rows' byte offsets; xl, xr: the columns left and right of the run)
__device__ __forceinline__ void load_bayer(const RgbRsrc& rs, bool ok, uint32_t ya, uint32_t ym, uint32_t yb, uint32_t xs,
                                           uint32_t xl, uint32_t xr, uint4& v0, uint4& v1, uint4& v2, uint32_t (&h)[6]) {
    const uint32_t row[3] = {ya, ym, yb};
    uint4* const v[3] = {&v0, &v1, &v2};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        *v[r] = as_u4(__builtin_amdgcn_raw_buffer_load_b128(rs.p0, ok ? row[r] + xs : kOob, 0, 0));
        h[2 * r] = __builtin_amdgcn_raw_buffer_load_b8(rs.p0, ok ? row[r] + xl : kOob, 0, 0);
        h[2 * r + 1] = __builtin_amdgcn_raw_buffer_load_b8(rs.p0, ok ? row[r] + xr : kOob, 0, 0);
    }
}
// z where the mask is 0, y where it is all ones: one v_bfi_b32 (a ternary on a per-lane condition
// becomes a divergent branch, see unpack_v210)
__device__ __forceinline__ uint32_t bit_select(uint32_t m, uint32_t y, uint32_t z) { return z ^ (m & (y ^ z)); }
// The run as 16 staged words.  va, vm, vb: the three rows' 16 bytes; h: the bytes left and right of
// each.  dy: the row is a B row (bayer_rgb); q: the run's even pixels are G sites (dy ^ the column
// parity of the R sites), both per lane.  Four pixels at a time, a word of each row:
//   - the R or B sites are bytes q and 2 + q.  v_perm lifts those two bytes of a word, or of its
//     left or right neighbours (from the word pair), into 16-bit fields; four such values are
//     summed with plain 32-bit adds (no carry between the fields: at most 1022) for G and for the
//     other colour, and the site's own byte is the third.
//   - the G sites, the other two bytes: v_lerp_u8 is the rounded mean of two words' bytes, all four
//     at once, of the words shifted a byte either way (the row's colour) and of the rows above and
//     below (the column's).
// A word R | G<<8 | B<<16 is then two v_perm; on a B row the sources of the low and the high byte
// trade places first.  The selectors are per-lane registers, so nothing branches.
__device__ __forceinline__ void unpack_bayer(const uint4& va, const uint4& vm, const uint4& vb, const uint32_t (&h)[6],
                                             uint32_t dy, uint32_t q, uint32_t px[16]) {
    // words -1 .. 4 of each row: the byte on the left is the top byte of word -1, the one on the right the low byte of word 4
    const uint32_t a[6] = {h[0] << 24, va.x, va.y, va.z, va.w, h[1]};
    const uint32_t m[6] = {h[2] << 24, vm.x, vm.y, vm.z, vm.w, h[3]};
    const uint32_t b[6] = {h[4] << 24, vb.x, vb.y, vb.z, vb.w, h[5]};
    uint32_t mdy = dy ? ~0u : 0u, mq = q ? ~0u : 0u;
    asm("" : "+v"(mdy), "+v"(mq));
    const uint32_t q2 = q * 0x00010001u;
    // bytes q, 2 + q of a word; the bytes left of them (3 + q, 5 + q of the pair previous, word);
    // the bytes right of them (1 + q, 3 + q of the pair word, next)
    const uint32_t sel_c = 0x0C020C00u + q2, sel_l = 0x0C050C03u + q2, sel_r = 0x0C030C01u + q2;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint32_t aw = a[w + 1], mw = m[w + 1], bw = b[w + 1];
        const uint32_t c2 = __builtin_amdgcn_perm(0u, mw, sel_c);
        const uint32_t g2 = ((__builtin_amdgcn_perm(0u, aw, sel_c) + __builtin_amdgcn_perm(0u, bw, sel_c) +
                              __builtin_amdgcn_perm(mw, m[w], sel_l) + __builtin_amdgcn_perm(m[w + 2], mw, sel_r) + 0x00020002u) >> 2) & 0x00FF00FFu;
        const uint32_t d2 = ((__builtin_amdgcn_perm(aw, a[w], sel_l) + __builtin_amdgcn_perm(a[w + 2], aw, sel_r) +
                              __builtin_amdgcn_perm(bw, b[w], sel_l) + __builtin_amdgcn_perm(b[w + 2], bw, sel_r) + 0x00020002u) >> 2) & 0x00FF00FFu;
        const uint32_t hh = __builtin_amdgcn_lerp(__builtin_amdgcn_alignbyte(mw, m[w], 3u), __builtin_amdgcn_alignbyte(m[w + 2], mw, 1u), 0x01010101u);
        const uint32_t vv = __builtin_amdgcn_lerp(aw, bw, 0x01010101u);
        // the low and the high byte's sources (an R row: own colour, diagonals; row mean, column mean)
        const uint32_t rlo = bit_select(mdy, d2, c2), rhi = bit_select(mdy, c2, d2);
        const uint32_t glo = bit_select(mdy, vv, hh), ghi = bit_select(mdy, hh, vv);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            // the R or B site: field k of rlo, g2, rhi
            const uint32_t t = __builtin_amdgcn_perm(g2, rlo, 0x0C0C0000u | ((4u + 2u * k) << 8) | (2u * k));
            const uint32_t rb = __builtin_amdgcn_perm(rhi, t, 0x0C000100u | ((4u + 2u * k) << 16));
            // the G site: byte 2k + 1 - q of glo, the word, ghi
            const uint32_t bg = 2u * k + 1u - q;
            const uint32_t u = __builtin_amdgcn_perm(mw, glo, 0x0C0C0000u | ((4u + bg) << 8) | bg);
            const uint32_t g = __builtin_amdgcn_perm(ghi, u, 0x0C000100u | ((4u + bg) << 16));
            px[4 * w + 2 * k] = bit_select(mq, g, rb);
            px[4 * w + 2 * k + 1] = bit_select(mq, rb, g);
        }
    }
}
// The clamped path of a lane: the run's 16 words written to dst one by one, in a loop that stays
// rolled.  A coordinate is clamped in the demosaiced frame first (row min(y, gh - 1), column
// min(xs + i, gw - 1)), and that pixel's neighbours are the reflected ones.  The 3x3 window slides:
// three byte loads a pixel (a column), by plain pointers, any base and pitch.
// (lut: the workgroup's channel tables, read by the kLut builds only)
__device__ __forceinline__ void edge_bayer(const uint8_t* base, uint64_t stride, uint32_t gw, uint32_t gh, uint32_t phase,
                                           uint32_t y, uint32_t xs, uint32_t* dst, const uint8_t* lut) {
    const uint32_t sy = min(y, gh - 1);
    const uint8_t* ra = base + (uint64_t)bayer_before(sy) * stride;
    const uint8_t* rm = base + (uint64_t)sy * stride;
    const uint8_t* rb = base + (uint64_t)bayer_after(sy, gh) * stride;
    auto column = [&](uint32_t x) { return (uint32_t)ra[x] | ((uint32_t)rm[x] << 8) | ((uint32_t)rb[x] << 16); };
    uint32_t cx = min(xs, gw - 1);
    uint32_t l = column(bayer_before(cx)), m = column(cx), r = 0;
#pragma unroll 1
    for (uint32_t i = 0; i < 16; ++i) {
        const uint32_t x = min(xs + i, gw - 1);
        if (x != cx) {  // one column on (r was column cx + 1, inside the frame)
            l = m;
            m = r;
            cx = x;
        }
        r = column(bayer_after(cx, gw));
        if constexpr (kLut) dst[i] = lut_map(lut, bayer_rgb(phase, sy, cx, l, m, r));  // (the channel tables: this path writes its words itself)
        else dst[i] = bayer_rgb(phase, sy, cx, l, m, r);
    }
}

// ---- downscaling loads (kDs > 1) ----
// A lane's run is 16 output pixels of one output row: kDs units of 16 / kDs pixels, each unit
// the kRun source bytes under it on kDs source rows, loaded as the shape's b128 loads of one
// row at a time and reduced as they arrive, so that a few unit rows of raw bytes (ds_pipeline)
// and one unit's sums are live at once.  A sum is at most 16 * 255: each is a 32-bit accumulator of
// v_dot4_u32_u8 with a constant byte mask, one per word the sample's bytes of that row touch.
//
// acc + the n bytes first, first + step, ... of a unit row's words w (all compile-time
// after unrolling: the masks are constants, and a word without a byte costs nothing)
template <int kW>
__device__ __forceinline__ uint32_t add_bytes(const uint32_t (&w)[kW], int first, int step, int n, uint32_t acc) {
#pragma unroll
    for (int d = 0; d < kW; ++d) {
        uint32_t m = 0;
#pragma unroll
        for (int t = 0; t < n; ++t)
            if (((first + t * step) >> 2) == d) m |= 1u << (8 * ((first + t * step) & 3));
        if (m) acc = __builtin_amdgcn_udot4(w[d], m, acc, false);
    }
    return acc;
}
// kN b128 loads at off, off + 16, ... as words (kOob + 48 is still past every range)
template <int kN>
__device__ __forceinline__ void load_words(__amdgpu_buffer_rsrc_t rs, uint32_t off, uint32_t (&w)[4 * kN]) {
#pragma unroll
    for (int q = 0; q < kN; ++q) {
        const uint4 v = as_u4(__builtin_amdgcn_raw_buffer_load_b128(rs, off + 16u * (uint32_t)q, 0, 0));
        w[4 * q] = v.x;
        w[4 * q + 1] = v.y;
        w[4 * q + 2] = v.z;
        w[4 * q + 3] = v.w;
    }
}
__device__ __forceinline__ uint32_t ds_mean(uint32_t sum) { return (sum + kDsHalf) >> kDsBits; }
// A step's sums are pinned where they are computed: they are pure arithmetic whose results the
// next tile's staging uses, and the compiler otherwise sinks all of it below the loads, which
// then hold every raw byte of the run in registers.
__device__ __forceinline__ void ds_pin(uint32_t& v) { asm volatile("" : "+v"(v)); }
// kSteps unit rows (kN b128 loads each, step s at off_of(s)) through a ring of kDepth buffers:
// kDepth - 1 loads ahead of the one use(s, words) reduces.  The scheduling barriers keep the
// compiler from issuing every load first, which is what bounds the registers: at most kDepth
// unit rows of raw bytes are live.
template <int kN, int kSteps, int kDepth, class Off, class Use>
__device__ __forceinline__ void ds_pipeline(__amdgpu_buffer_rsrc_t rs, Off&& off_of, Use&& use) {
    uint32_t w[kDepth][4 * kN];
#pragma unroll
    for (int s = 0; s < kDepth - 1 && s < kSteps; ++s) load_words<kN>(rs, off_of(s), w[s % kDepth]);
#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
        if (s + kDepth - 1 < kSteps) load_words<kN>(rs, off_of(s + kDepth - 1), w[(s + kDepth - 1) % kDepth]);
        __builtin_amdgcn_sched_barrier(0);
        use(s, w[s % kDepth]);
        __builtin_amdgcn_sched_barrier(0);
    }
}
// The lane's run as 16 staged words.  ok: the fast path (else every load is out of range and
// the words are discarded); off: the run's first source byte, in source rows of pitch stride;
// NV12: coff the first Cb,Cr byte of the run's 8 cells, in chroma rows of pitch cpitch.
// Step s = (unit s / kDs, source row s % kDs): a unit's sums are complete after its last row.
__device__ __forceinline__ void ds_load_run(const RgbRsrc& rs, bool ok, uint32_t off, uint32_t stride, uint32_t coff,
                                            uint32_t cpitch, uint32_t sel4, uint32_t px[16]) {
    constexpr int kU = 16 / kDs;  // output pixels of a unit
    constexpr int kSteps = kDs * kDs;
    if constexpr (kShape == kShapeNv12) {
#if JPGE_K1_SHAPE == 4
        constexpr int kDepth = kDs == 2 ? 4 : 8;
        uint32_t acc[kU];
        ds_pipeline<1, kSteps, kDepth>(
            rs.p0, [&](int s) __attribute__((always_inline)) { return ok ? off + (uint32_t)(s % kDs) * stride + 16u * (uint32_t)(s / kDs) : kOob; },
            [&](int s, const uint32_t(&w)[4]) __attribute__((always_inline)) {
#pragma unroll
                for (int i = 0; i < kU; ++i) {
                    acc[i] = add_bytes(w, i * kDs, 1, kDs, s % kDs ? acc[i] : 0u);
                    ds_pin(acc[i]);
                }
                if (s % kDs == kDs - 1) {
#pragma unroll
                    for (int i = 0; i < kU; ++i) px[(s / kDs) * kU + i] = ds_mean(acc[i]);
                }
            });
        // the run's 8 cells: kDs units of 8 / kDs cells, 16 bytes of Cb,Cr pairs on each of kDs chroma rows
        constexpr int kC = 8 / kDs;
        uint32_t cb[kC], cr[kC];
        ds_pipeline<1, kSteps, kDepth>(
            rs.p1, [&](int s) __attribute__((always_inline)) { return ok ? coff + (uint32_t)(s % kDs) * cpitch + 16u * (uint32_t)(s / kDs) : kOob; },
            [&](int s, const uint32_t(&w)[4]) __attribute__((always_inline)) {
#pragma unroll
                for (int i = 0; i < kC; ++i) {
                    cb[i] = add_bytes(w, i * kDs * 2, 2, kDs, s % kDs ? cb[i] : 0u);
                    cr[i] = add_bytes(w, i * kDs * 2 + 1, 2, kDs, s % kDs ? cr[i] : 0u);
                    ds_pin(cb[i]);
                    ds_pin(cr[i]);
                }
                if (s % kDs == kDs - 1) {
#pragma unroll
                    for (int i = 0; i < kC; ++i) {
                        const uint32_t c = (ds_mean(cb[i]) << 8) | (ds_mean(cr[i]) << 16);
                        px[2 * ((s / kDs) * kC + i)] |= c;
                        px[2 * ((s / kDs) * kC + i) + 1] |= c;
                    }
                }
            });
#endif
    } else {
        constexpr int kN = (int)kRun / 16;  // b128 loads of a unit row (3, or 4 of 4-byte pixels)
        constexpr int kDepth = kDs == 2 ? 3 : kN == 3 ? 4 : 3;
        uint32_t acc[kU][3];
        ds_pipeline<kN, kSteps, kDepth>(
            rs.p0, [&](int s) __attribute__((always_inline)) { return ok ? off + (uint32_t)(s % kDs) * stride + kRun * (uint32_t)(s / kDs) : kOob; },
            [&](int s, const uint32_t(&w)[4 * kN]) __attribute__((always_inline)) {
#pragma unroll
                for (int i = 0; i < kU; ++i)
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        acc[i][c] = add_bytes(w, i * kDs * (int)kBpp + c, (int)kBpp, kDs, s % kDs ? acc[i][c] : 0u);
                        ds_pin(acc[i][c]);
                    }
                if (s % kDs == kDs - 1) {
#pragma unroll
                    for (int i = 0; i < kU; ++i) {
                        const uint32_t b0 = ds_mean(acc[i][0]), b1 = ds_mean(acc[i][1]), b2 = ds_mean(acc[i][2]);
                        uint32_t& o = px[(s / kDs) * kU + i];
                        if constexpr (kShape == kShapeBgr8) o = b2 | (b1 << 8) | (b0 << 16);
                        else if constexpr (kShape == kShapeX4) o = __builtin_amdgcn_perm(0u, b0 | (b1 << 8) | (b2 << 16), sel4);
                        else o = b0 | (b1 << 8) | (b2 << 16);
                    }
                }
            });
    }
}
// One output pixel of the downscaling builds' clamped edge path: row oy, column ox of the
// output frame (inside it), the mean of its kDs x kDs source pixels, their coordinates clamped
// to the sw x sh source frame (NV12: the cell's chroma of its kDs x kDs source cells, clamped
// to the chroma plane), by byte loads.  The sums fit 16-bit fields.
__device__ __forceinline__ uint32_t edge_ds(const uint8_t* base, uint64_t stride, uint64_t plane_stride, uint32_t sw,
                                            uint32_t sh, uint32_t sel4, uint32_t oy, uint32_t ox) {
    if constexpr (kShape == kShapeNv12) {
        const uint32_t scw = (sw + 1) / 2, sch = (sh + 1) / 2;
        const uint8_t* cp = base + plane_stride;
        uint32_t ys = 0, cs = 0;  // cs: Cb | Cr << 16
#pragma unroll 1  // (rolled: the 16 pixels' loads would otherwise all be issued first, at hundreds of registers)
        for (uint32_t r = 0; r < (uint32_t)kDs; ++r) {
            const uint8_t* yrow = base + (uint64_t)min(kDs * oy + r, sh - 1) * stride;
            const uint8_t* crow = cp + (uint64_t)min(kDs * (oy >> 1) + r, sch - 1) * stride;
            for (uint32_t i = 0; i < (uint32_t)kDs; ++i) {
                ys += yrow[min(kDs * ox + i, sw - 1)];
                const uint8_t* c = crow + 2 * (uint64_t)min(kDs * (ox >> 1) + i, scw - 1);
                cs += (uint32_t)c[0] | ((uint32_t)c[1] << 16);
            }
        }
        return ds_mean(ys) | (ds_mean(cs & 0xFFFF) << 8) | (ds_mean(cs >> 16) << 16);
    } else {
        uint32_t rb = 0, gs = 0;  // rb: R | B << 16 of the staged order
#pragma unroll 1  // (rolled, as above)
        for (uint32_t r = 0; r < (uint32_t)kDs; ++r)
            for (uint32_t i = 0; i < (uint32_t)kDs; ++i) {
                const uint32_t p = edge_pixel(base, stride, plane_stride, sel4, min(kDs * oy + r, sh - 1), min(kDs * ox + i, sw - 1));
                rb += p & 0x00FF00FFu;
                gs += (p >> 8) & 0xFF;
            }
        return ds_mean(rb & 0xFFFF) | (ds_mean(gs) << 8) | (ds_mean(rb >> 16) << 16);
    }
}

#if JPGE_K1_SHAPE >= 11
#define JPGE_K1_OCC __attribute__((amdgpu_waves_per_eu(4, 4)))
#else
#define JPGE_K1_OCC
#endif
template <bool kExact, int kWaves, int kFilt, int kN>
__global__ __launch_bounds__(kWaves * 64) JPGE_K1_OCC void fdct_kernel(FrameSet<FdctArgs, kN> fs) {
    const uint32_t set_f = set_member<kN>(fs.wg0, fs.n, blockIdx.x);  // (frame sets: kernels.hpp)
    const FdctArgs& a = fs.a[set_f];
    const uint32_t bid = blockIdx.x - fs.wg0[set_f], nbk = fs.wg0[set_f + 1] - fs.wg0[set_f];
    // the arguments the tile loop reads, loaded once into scalar registers: a set
    // member's arguments sit at a computed kernarg offset, and the compiler otherwise
    // reloads them per tile (scalar loads whose lgkmcnt waits also wait for LDS traffic)
    const uint8_t* rgb_ = a.rgb;
    uint64_t stride_ = a.stride;
    uint32_t gw_ = a.g.width, gh_ = a.g.height;
    asm volatile("" : "+s"(rgb_), "+s"(stride_), "+s"(gw_), "+s"(gh_));
    uint32_t sw_ = gw_, sh_ = gh_;   // the frame the loads read: the downscaling builds' source
    if constexpr (kDs > 1) {
        sw_ = a.src_w;
        sh_ = a.src_h;
        asm volatile("" : "+s"(sw_), "+s"(sh_));
    }
    uint32_t rows_back_ = 0;         // the oriented builds: the source's rows run backwards
    if constexpr (kOrient != 0) {
        sw_ = a.src_w;
        sh_ = a.src_h;
        rows_back_ = orient_rows_back((int)a.orient) ? 1u : 0u;
        asm volatile("" : "+s"(sw_), "+s"(sh_), "+s"(rows_back_));
    }
    uint64_t ps_ = 0;                // planar: the plane pitch
    uint32_t sel4_ = kSelRgbx;       // 4-byte pixels: the byte selector of the channel order
    if constexpr (kShape == kShapePlanar || (kYuv && !kGray && !kPacked422 && kShape != kShapeY210 && !kV210)) {
        ps_ = a.plane_stride;
        asm volatile("" : "+s"(ps_));
    }
    if constexpr (kShape == kShapeX4) {
        sel4_ = a.fmt == kFmtBgra8 ? kSelBgrx : kSelRgbx;
        asm volatile("" : "+s"(sel4_));
    }
    if constexpr (kPacked422) {
        sel4_ = a.fmt == kFmtUyvy ? kSelUyvy : kSelYuyv;
        asm volatile("" : "+s"(sel4_));
    }
    uint32_t phase_ = 0;             // Bayer: the CFA phase of the frame's layout (kernels.hpp bayer_phase)
    if constexpr (kBayer) {
        phase_ = bayer_phase(a.fmt);
        asm volatile("" : "+s"(phase_));
    }
    XfK xf{};  // (the Y, Cb, Cr shapes' !kExact instances)
    if constexpr (kYuv && !kExact) xf = xf_load(a);
    constexpr int kK1Threads = kWaves * 64;
    __shared__ K1Lds<kWaves> lds;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;  // wv: 0..15
    K1WaveLds& W = lds.w[wv];
    // (the channel tables' builds: the workgroup's copy, and this thread's word of the frame's tables,
    // loaded ahead of the first tile's pixel loads below: the vector memory counter retires in order,
    // so the wait for this word before its LDS write leaves the pixel loads in flight)
    const uint8_t* lut_ = nullptr;
    uint32_t lut_w_ = 0;
    if constexpr (kLut) {
        static_assert(kWaves * 64 >= kLutWords, "a thread loads one word of the tables");
        lut_ = reinterpret_cast<const uint8_t*>(lds.lut);
        // (through a descriptor of the 768 bytes, as the pixels: a thread past the tables loads nothing)
        const __amdgpu_buffer_rsrc_t lut_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(fdct_lut_raw(a)), 0, kLutBytes, 0x00020000);
        lut_w_ = __builtin_amdgcn_raw_buffer_load_b32(lut_rs, (uint32_t)tid * 4u, 0, 0);
    }
    JPGE_STAMP(1);
    const uint32_t mw = a.g.mw;
    const uint32_t tiles_per_row = (mw + 3) / 4;
    const uint32_t ntiles = tiles_per_row * a.g.mh;
    const double scale = 255.0 / (double)a.maxval;  // Image.cpp:465
    // (I420, I422, I010, I210: the chroma pitch, half the stride, is 16-byte aligned too)
    const bool aligned = (((uintptr_t)rgb_ | stride_ | ps_) & 15) == 0 && (!(kHalfPitch || kShape == kShapeI010 || kShape == kShapeI210) || (stride_ & 31) == 0);
    const int r16 = lane >> 2, c16 = lane & 3;  // staging: lane -> (pixel row, 16-px chunk)
    const int b8 = lane >> 3, j = lane & 7;     // DCT: lane -> (block of the round, column)
    // ---- oriented loads (kOrient != 0) ----
    // Not transposed: the lane map stays, (r16, c16) is O's row y and columns xs .. xs + 15; the
    // source row is y or sh - 1 - y, the run starts at source column xs, or sw - 16 - xs mirrored.
    // Transposed: the 64x16 tile of O is a source block 16 pixels wide and 64 rows tall; lane l
    // loads the run of the source row under O's column mcol0 * 16 + l (or sh - 1 - that), from
    // source column mrow * 16 (mirrored: sw - 16 - mrow * 16), and stages it down column l.
    // A mirrored run's bytes start 16-byte aligned only when the row's bytes are a multiple of 16.
    const bool or_aligned = aligned && (!kOrMirror || ((kBpp * sw_) & 15u) == 0);
    // pixel (oy, ox) of O, both inside it, by the clamped path's byte loads
    auto or_pixel = [&](uint32_t oy, uint32_t ox) -> uint32_t {
        const uint32_t r = kOrTrans ? ox : oy, c = kOrTrans ? oy : ox;
        return edge_pixel(rgb_, stride_, ps_, sel4_, rows_back_ ? sh_ - 1 - r : r, kOrMirror ? sw_ - 1 - c : c);
    };

    // Pixels and coefficients move through buffer descriptors: an out-of-range
    // offset (kOob) makes a load return zeros and drops a store, so every tile
    // issues the same 3 loads (4-byte pixels: 4) and 3 stores with no branch around them, and the
    // wait for the prefetched pixels leaves the previous tile's stores in flight.
    const RgbRsrc rgb_rs = rgb_rsrc(rgb_, stride_, ps_, sw_, sh_);
    const __amdgpu_buffer_rsrc_t coef_rs =
        __builtin_amdgcn_make_buffer_rsrc(a.coef, 0, (int)(uint32_t)((uint64_t)a.g.nblocks() * 128), 0x00020000);

    // Dynamic tiles.  One workgroup per CU owns a contiguous run of n_p tiles; each
    // of its 16 waves takes its first tile by rank, then grabs more from an LDS
    // counter until the run is exhausted.  The SIMD issues the oldest ready wave
    // first, so waves progress unequally: grabbing lets the faster ones take more
    // tiles, and all waves of a CU finish within about a tile of each other.
    const uint32_t tb_p = (uint32_t)((uint64_t)ntiles * bid / nbk);
    const uint32_t n_p = (uint32_t)((uint64_t)ntiles * (bid + 1) / nbk) - tb_p;
    auto grab = [&]() -> uint32_t {
        uint32_t v = 0;
        if (lane == 0) v = atomicAdd(&lds.next, 1u);
        return __builtin_amdgcn_readfirstlane(v);
    };

    // the pixel run of this lane (48 bytes of RGB8) for partition tile k, if the tile is on the
    // aligned fast path (else zeros, and the staging takes the clamped edge path)
    // (tile numbers are wave-uniform: the tile's row and column come from scalar
    // arithmetic, and only this lane's fixed offset within the tile is per lane)
    const uint32_t lane_off = (uint32_t)r16 * (uint32_t)stride_ + (uint32_t)c16 * kRun;
    // 4:2:0 layouts: the chroma of the run's 8 cells, in chroma row (tile row * 8 + r16 / 2) of
    // pitch cpitch: NV12 the 16 bytes under the run, I420 the 16 bytes that hold its 8
    uint32_t cpitch = 0, lane_coff = 0;
    if constexpr (kYuv420 && !kTen) {
        cpitch = kShape == kShapeNv12 ? (uint32_t)stride_ : (uint32_t)((stride_ + 1) / 2);
        lane_coff = (uint32_t)(r16 >> 1) * cpitch + (kShape == kShapeNv12 ? (uint32_t)c16 : (uint32_t)(c16 >> 1)) * 16;
    }
    // 10-bit: P010 the 32 bytes of pairs under the run, I010 the 16 bytes of each plane that are its 8 cells
    // (P210, I210: the same bytes of chroma row (tile row * 16 + r16), the pixels' own; Y210: no chroma loads)
    constexpr uint32_t kCellRun = kTenHi ? 32u : 16u;  // chroma bytes (of one plane) of 8 cells
    constexpr uint32_t kCRows = kTen422 ? 16u : 8u;    // chroma rows of a tile
    if constexpr (kTen) {
        cpitch = kTenHi ? (uint32_t)stride_ : (uint32_t)(2 * ((stride_ + 3) / 4));
        lane_coff = (uint32_t)(kTen422 ? r16 : r16 >> 1) * cpitch + (uint32_t)c16 * kCellRun;
    }
    // NV16, I422: the same bytes of chroma row (tile row * 16 + r16), the pixels' own
    if constexpr (kPlanes422) {
        cpitch = kPairs ? (uint32_t)stride_ : (uint32_t)((stride_ + 1) / 2);
        lane_coff = (uint32_t)r16 * cpitch + (kPairs ? (uint32_t)c16 : (uint32_t)(c16 >> 1)) * 16;
    }
    uint32_t hb[6];  // (Bayer: the prefetched bytes left and right of the run's three rows)
    auto fast_load = [&](uint32_t k, uint4& v0, uint4& v1, uint4& v2, uint4& v3) -> bool {
        const uint32_t t = tb_p + k;
        const uint32_t mrow = t / tiles_per_row, mcol0 = (t % tiles_per_row) * 4;
        const uint32_t y = mrow * 16 + r16, xs = mcol0 * 16 + c16 * 16;
        if constexpr (kOrient != 0) {
            // r: the source row before rows_back; c0: the run's first source column before the mirror.
            // Fast: the run's 16 pixels of O and the lane's row (transposed: column) lie inside O.
            const uint32_t ox = mcol0 * 16 + (uint32_t)lane;
            const uint32_t r = kOrTrans ? ox : y, c0 = kOrTrans ? mrow * 16 : xs;
            const bool in = kOrTrans ? ox < gw_ && mrow * 16 + 16 <= gh_ : y < gh_ && xs + 16 <= gw_;
            const bool ok = k < n_p && or_aligned && in;
            // (ok: r < sh and c0 + 16 <= sw, so the offset is inside the descriptor's range, below 2^32)
            const uint32_t sr = rows_back_ ? sh_ - 1 - r : r, sc = kOrMirror ? sw_ - 16 - c0 : c0;
            load_run(rgb_rs, ok ? sr * (uint32_t)stride_ + sc * kBpp : kOob, kOob, v0, v1, v2, v3);
            return ok;
        }
        if constexpr (kBayer) {
            // ("Bayer loads" above; ok: every row and column is inside the frame, the offsets below 2^32)
            const bool ok = k < n_p && aligned && y < gh_ && xs + 16 <= gw_;
            const uint32_t st = (uint32_t)stride_;
            load_bayer(rgb_rs, ok, bayer_before(y) * st, y * st, bayer_after(y, gh_) * st, xs, bayer_before(xs),
                       bayer_after(xs + 15, gw_), v0, v1, v2, hb);
            return ok;
        }
        bool ok = k < n_p && aligned && y < gh_ && xs + 16 <= gw_;
        // (I420: and the 16 chroma bytes lie inside their row)
        if constexpr (kShape == kShapeI420) ok = ok && ((xs >> 5) + 1) * 16 <= (gw_ + 1) / 2;
        if constexpr (kShape == kShapeI422) ok = ok && ((xs >> 5) + 1) * 16 <= (gw_ + 1) / 2;
        const uint32_t base = (uint32_t)((uint64_t)(mrow * 16) * stride_ + (uint64_t)mcol0 * kRun);  // (uniform)
        const uint32_t off = ok ? base + lane_off : kOob;
        uint32_t coff = kOob;
        if constexpr (kYuv420 && !kTen) {
            const uint32_t cbase = (uint32_t)((uint64_t)(mrow * 8) * cpitch + (uint64_t)mcol0 * (kShape == kShapeNv12 ? 16 : 8));
            coff = ok ? cbase + lane_coff : kOob;
        }
        if constexpr (kTen && !kV210) {
            // (I010: the run's 8 cells are the 16 bytes themselves, inside their row whenever the run is)
            const uint32_t cbase = (uint32_t)((uint64_t)(mrow * kCRows) * cpitch + (uint64_t)mcol0 * kCellRun);
            coff = ok ? cbase + lane_coff : kOob;
        }
        if constexpr (kV210) {
            // the run's groups ("v210" above).  Its last pixel xs + 15 <= gw - 1 lies in group
            // (xs + 15) / 6 <= (gw - 1) / 6, the row's last, so every group a lane needs is inside
            // the row whenever the run is; the fourth load of a lane that needs three moves nothing.
            const uint32_t n = xs >> 4, g0 = (8 * n) / 3;
            const uint32_t o = (uint32_t)((uint64_t)(mrow * 16) * stride_) + (uint32_t)r16 * (uint32_t)stride_ + 16 * g0;
            load_run(rgb_rs, ok ? o : kOob, ok && n % 3 == 1 ? o + 48 : kOob, v0, v1, v2, v3);
            return ok;
        }
        if constexpr (kPlanes422) {
            const uint32_t cbase = (uint32_t)((uint64_t)(mrow * 16) * cpitch + (uint64_t)mcol0 * (kPairs ? 16 : 8));
            coff = ok ? cbase + lane_coff : kOob;
        }
        load_run(rgb_rs, off, coff, v0, v1, v2, v3);
        return ok;
    };
    // The downscaling builds: the lane's run of partition tile k, loaded and reduced to its 16
    // staged words (ds_load_run).  The fast path's conditions are on the source: its kDs rows
    // and 16 * kDs pixels (NV12: and the kDs chroma rows of the run's cells) lie inside the frame.
    auto fast_load_ds = [&](uint32_t k, uint32_t nx[16]) -> bool {
        const uint32_t t = tb_p + k;
        const uint32_t mrow = t / tiles_per_row, mcol0 = (t % tiles_per_row) * 4;
        const uint32_t y = mrow * 16 + r16, xs = mcol0 * 16 + c16 * 16;
        bool ok = k < n_p && aligned && kDs * y + kDs <= sh_ && kDs * (xs + 16) <= sw_;
        if constexpr (kShape == kShapeNv12) ok = ok && kDs * (y >> 1) + kDs <= (sh_ + 1) / 2;
        const uint32_t off = (uint32_t)((uint64_t)(mrow * 16 * kDs) * stride_ + (uint64_t)mcol0 * (kRun * kDs)) +
                             (uint32_t)(r16 * kDs) * (uint32_t)stride_ + (uint32_t)c16 * (kRun * kDs);
        uint32_t coff = 0;
        if constexpr (kShape == kShapeNv12)
            coff = (uint32_t)((uint64_t)(mrow * 8 * kDs) * stride_ + (uint64_t)mcol0 * (16 * kDs)) +
                   (uint32_t)((r16 >> 1) * kDs) * (uint32_t)stride_ + (uint32_t)c16 * (16 * kDs);
        ds_load_run(rgb_rs, ok, off, (uint32_t)stride_, coff, (uint32_t)stride_, sel4_, nx);
        return ok;
    };
    // The last round's 16-byte coefficient row (kOob: none) is stored during the
    // next tile, after its staging: the staging's wait for the prefetched pixels
    // then finds only long-issued stores ahead of them in the in-order counter.
    u32x4 pend;
    uint32_t poff = kOob;
    auto store_pending = [&] { __builtin_amdgcn_raw_buffer_store_b128(pend, coef_rs, poff, 0, kK1StoreAux); };
    uint32_t k = __builtin_amdgcn_readfirstlane((uint32_t)wv);  // this wave's current tile of the run
    uint4 c0, c1, c2, c3;
    uint32_t nx[16];  // (the downscaling builds' prefetch: the next tile's run as staged words)
    bool cfast;
    if constexpr (kDs > 1) cfast = fast_load_ds(k, nx);
    else cfast = fast_load(k, c0, c1, c2, c3);  // issued before the prologue's own memory traffic
    // (the channel tables' word, loaded before the pixels: written here, ahead of the loop below, so
    // that the wait is a count the compiler knows, "all but the pixel loads", not zero)
    if constexpr (kLut)
        if (tid < kLutWords) lds.lut[tid] = lut_w_;

    for (uint32_t i = bid * kK1Threads + tid; i < a.zero_words; i += nbk * kK1Threads) a.zero[i] = 0;
    if (bid == 0)  // carried: another frame's tables + headers, host -> device
        for (uint32_t i = tid; i < a.imp_n16; i += kK1Threads) a.imp_dst[i] = a.imp_src[i];
    if (tid == 0) lds.next = kWaves;
    if (tid < 128) {
        const int c = tid >> 6, e = tid & 63, o = (e >> 3) * kQRow + (e & 7);
        const double q = (double)q_entry(a, tid);  // Image.cpp:611-636 divides by the entry as double
        lds.q[c][o] = q;
        lds.invq[c][o] = arai_scale(e & 7) / q;
    }
    // LDS-only barrier: the prologue's shared state is in LDS (a full __syncthreads
    // would also wait for the first tile's pixels, issued above)
    lds_barrier();
    JPGE_STAMP(0);
    uint32_t kn = k < n_p ? grab() : n_p;  // the next tile (its pixels are prefetched a tile ahead)

    // Round inputs, read from LDS in one batch per round (issued during the previous
    // round's row pass): 8 pixel words of a Y column, or the 2x2 pixel pairs of 8
    // chroma samples, and the lane's 8 reciprocal quantisers.
    const int ycolbase = (b8 >> 2) * 16 + (b8 & 1) * 8 + j;  // Y round: column of the lane's block
    const int yrow0 = ((b8 >> 1) & 1) * 8;
    const int ccomp = b8 >> 2, cm = b8 & 3;
    const int ccol = cm * 16 + 2 * j;
    double* tb = &W.tmp[b8 * kTmpBlock];
    auto load_y = [&](int round, uint32_t p[8]) {
        const int col = round * 32 + ycolbase;
#pragma unroll
        for (int i = 0; i < 8; ++i) p[i] = W.rgbx[(yrow0 + i) * kRgbPitch + col];
    };
    // Exact colour (8-bit input): a Cb lane and its Cr partner 32 lanes up read the same
    // pixels, so each reads half of them (rows 8h..8h+7, its 4 samples), converts them for
    // both components, and the pair trades the other component's values (swap_halves).
    const int crow0 = kExact ? 8 * ccomp : 0;
    auto load_c = [&](uint2 c[16]) {
        constexpr int n = kExact ? 8 : 16;
#pragma unroll
        for (int i = 0; i < n; ++i)
            c[i] = *reinterpret_cast<const uint2*>(&W.rgbx[(crow0 + i) * kRgbPitch + ccol]);
    };
    auto load_iq = [&](int qb, double iq[8]) {
#pragma unroll
        for (int u = 0; u < 8; ++u) iq[u] = lds.invq[qb][j * kQRow + u];
    };
    auto y_inputs = [&](const uint32_t p[8], double x[8]) {
        if constexpr (kYuv && !kExact) {
            // the sample transform; a 4:2:0 layout's rows 2r, 2r + 1 lie in one cell (yrow0 is
            // even), so the chroma bytes are converted and scaled once per pair (the 4:2:2
            // layouts, 8-bit and 10-bit: per pixel, the two rows hold different chroma)
            constexpr int n = kYuv420 ? 2 : 1;
#pragma unroll
            for (int i = 0; i < 8; i += n) {
                const double t1 = xf.m1 * yuv_c(p[i], 1), t2 = xf.m2 * yuv_c(p[i], 2);
#pragma unroll
                for (int r = 0; r < n; ++r) x[i + r] = xf_y(xf, p[i + r], t1, t2);
            }
            return;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] = kYuv ? yuv_y(p[i]) : kExact ? ycc_exact_y(p[i]) : ycc_ref_y(p[i], scale);
    };
    auto c_inputs = [&](const uint2 c[16], double x[8]) {
        if constexpr (kExact) {
            // channel sums of this lane's 4 samples (exact integers), then both components:
            // the chroma of 8-bit input is exact, and each filter's
            // 1/4, 1/2 or 1 is folded into the constants (every product stays exact):
            //   S420_m  ((a+b)+(c+d))/4 of the 2x2 pixels, Image.cpp:207-224;
            //   S420_lm (a+c)/2 of the two rows' left pixels, Image.cpp:218-224, 297-306;
            //   S420    the top-left pixel (the masks' zero terms add zeros), Image.cpp:279-286
            constexpr double f = kFilt == kFiltS420 ? 1.0 : kFilt == kFiltS420lm ? 0.5 : 0.25;
            double vb[4], vr[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint2 t0 = c[2 * i], t1 = c[2 * i + 1];
                uint32_t sr = t0.x & 0xFF, sg = (t0.x >> 8) & 0xFF, sb = t0.x >> 16;
                if (kFilt != kFiltS420) {
                    sr += t1.x & 0xFF;
                    sg += (t1.x >> 8) & 0xFF;
                    sb += t1.x >> 16;
                }
                if (kFilt == kFiltS420m) {
                    sr += (t0.y & 0xFF) + (t1.y & 0xFF);
                    sg += ((t0.y >> 8) & 0xFF) + ((t1.y >> 8) & 0xFF);
                    sb += (t0.y >> 16) + (t1.y >> 16);
                }
                const double dr = (double)sr, dg = (double)sg, db = (double)sb;
                if constexpr (kYuv) {
                    // Y, Cb, Cr words: the sums are of Cb (bits 8-15) and Cr (16-23) samples, and
                    // the filter of the samples v - 128 is f * sum - 128, exact (sums below 2^10)
                    vb[i] = dg * f - 128.0;
                    vr[i] = db * f - 128.0;
                } else {
                    vb[i] = __builtin_fma(kCbB * f, db, __builtin_fma(kCbG * f, dg, (kCbR * f) * dr));
                    vr[i] = __builtin_fma(kCrB * f, db, __builtin_fma(kCrG * f, dg, (kCrR * f) * dr));
                }
            }
            // lanes < 32 (Cb) keep Cb of samples 0-3 and receive Cb of 4-7; lanes >= 32 (Cr)
            // receive Cr of 0-3 and keep Cr of 4-7
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                swap_halves(vb[i], vr[i]);
                x[i] = vb[i];
                x[4 + i] = vr[i];
            }
            return;
        }
        const double kr = ccomp ? kCrR : kCbR, kg = ccomp ? kCrG : kCbG, kb = ccomp ? kCrB : kCbB;
        const double ku = ccomp ? xf.m5 : xf.m3, kv = ccomp ? xf.m6 : xf.m4;  // (Y, Cb, Cr words)
        // a pixel's chroma: the colour conversion, or the sample transform of a Y, Cb, Cr word
        auto ref_c = [&](uint32_t w) {
            if constexpr (kYuv) return xf_c(w, ku, kv);
            else return ycc_ref_c(w, scale, kr, kg, kb);
        };
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint2 t0 = c[2 * i], t1 = c[2 * i + 1];
            // other maxvals: the reference's per-pixel op order
            if (kFilt == kFiltS420) {
                // subsample(S420), Image.cpp:279-286: mask {1, 0} on even rows only, the
                // top-left sample (the mask's 0 * b adds a zero)
                x[i] = ref_c(t0.x);
            } else if (kFilt == kFiltS420lm) {
                // subsample(S420_lm), Image.cpp:297-306, 218-224: (a + c) / 2 of the left
                // samples of both rows
                double v = ref_c(t0.x);
                v += ref_c(t1.x);
                x[i] = v / 2;
            } else {
                // subsample(S420_m), Image.cpp:207-224: ((0+a+b) + (0+c+d)) / 4
                double top = 0.0, bot = 0.0;
                top += ref_c(t0.x);
                top += ref_c(t0.y);
                bot += ref_c(t1.x);
                bot += ref_c(t1.y);
                x[i] = (top + bot) / 4;
            }
        }
    };

    uint32_t ndone = 0;
    for (; k < n_p; ++ndone) {
        const uint32_t t = tb_p + k;
        const uint32_t mrow = t / tiles_per_row;
        const uint32_t mcol0 = (t % tiles_per_row) * 4;
        const int nvalid = (int)min(4u, mw - mcol0);
        const uint32_t y = mrow * 16 + r16, xs = mcol0 * 16 + c16 * 16;

        JPGE_STAMP(2 + min(ndone, 4u));
        // ---- stage 16 px per lane as packed u32 ----
        // (the prefetched registers are consumed on every path, so no later wait on
        // them can also drain the previous tile's coefficient stores)
        uint32_t px[16];
        if constexpr (kDs > 1) {
#pragma unroll
            for (int i = 0; i < 16; ++i) px[i] = nx[i];
        } else if constexpr (kBayer) {
            // (y's parity is r16's: a tile starts on an even row; xs is even)
            const uint32_t dy = ((uint32_t)r16 ^ (phase_ >> 1)) & 1u;
            unpack_bayer(c0, c1, c2, hb, dy, (dy ^ phase_) & 1u, px);
        } else if constexpr (kV210) {
            unpack_v210(c0, c1, c2, c3, (xs >> 4) % 3, px);
        } else if constexpr (kTen) {
            unpack_yuv10(c0, c1, c2, c3, px);
        } else if constexpr (kYuv420 || kPlanes422) {
            unpack_yuv420(c0, c1, c2, (uint32_t)(c16 & 1), px);
        } else if constexpr (kPacked422) {
            unpack_packed422(c0, c1, sel4_, px);
        } else if constexpr (kShape == kShapeX4 || kShape == kShapePlanar || kShape == kShapeYuv444) {
            unpack_run(c0, c1, c2, c3, sel4_, px);
        } else {
            const uint4 v0 = c0, v1 = c1, v2 = c2;
            const uint32_t wd[13] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w, 0u};
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int b0 = 3 * i, d = b0 >> 2;
                // bytes b0..b0+2 of the run, zero-extended (perm selector 0x0c = 0x00); BGR8: 2, 1, 0
                const uint32_t o8 = (uint32_t)(b0 & 3);
                px[i] = __builtin_amdgcn_perm(wd[d + 1], wd[d], sel3(o8));
            }
        }
        if constexpr (kOrMirror) {  // the run in O's order: a renaming of registers
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const uint32_t t = px[i];
                px[i] = px[15 - i];
                px[15 - i] = t;
            }
        }
        if (!kBayer && !cfast) {  // right/bottom edge replication (Image.cpp:498-531) as clamped addressing
            const uint32_t sy = min(y, gh_ - 1);
            if constexpr (kOrTrans)  // (O's coordinates clamped first, then mapped to the source)
                for (int i = 0; i < 16; ++i) px[i] = or_pixel(min(mrow * 16 + i, gh_ - 1), min(mcol0 * 16 + (uint32_t)lane, gw_ - 1));
            else if constexpr (kOrient != 0)
                for (int i = 0; i < 16; ++i) px[i] = or_pixel(sy, min(xs + i, gw_ - 1));
            else if constexpr (kDs > 1)  // (of the downscaled frame, each pixel from its clamped source pixels)
                for (int i = 0; i < 16; ++i) px[i] = edge_ds(rgb_, stride_, ps_, sw_, sh_, sel4_, sy, min(xs + i, gw_ - 1));
            else if constexpr (kYuv)
                for (int i = 0; i < 16; ++i) px[i] = edge_yuv(rgb_, stride_, ps_, gh_, sel4_, sy, min(xs + i, gw_ - 1));
            else
                for (int i = 0; i < 16; ++i) px[i] = edge_pixel(rgb_, stride_, ps_, sel4_, sy, min(xs + i, gw_ - 1));
        }
        if constexpr (kLut) {  // the channel tables: fast path and clamped path alike
#pragma unroll
            for (int i = 0; i < 16; ++i) px[i] = lut_map(lut_, px[i]);
        }
        if constexpr (kOrTrans) {
            // down column `lane` of the staged tile: the lanes' addresses are consecutive words
#pragma unroll
            for (int i = 0; i < 16; ++i) W.rgbx[i * kRgbPitch + lane] = px[i];
        } else {
            uint32_t* dst = &W.rgbx[r16 * kRgbPitch + c16 * 16];
#pragma unroll
            for (int i = 0; i < 16; i += 2) *reinterpret_cast<uint2*>(dst + i) = make_uint2(px[i], px[i + 1]);
            // (Bayer: a lane on the clamped path writes its words over the ones just staged, in a rolled loop)
            if constexpr (kBayer)
                if (!cfast) edge_bayer(rgb_, stride_, gw_, gh_, phase_, y, xs, dst, lut_);
        }
        wave_order();
        // prefetch the next tile of this wave (into the registers just staged) while
        // this one is transformed
        if constexpr (kDs > 1) {
            // (the reduction waits for its loads: before the store, so that the wait finds only
            // the previous tile's long-issued stores ahead of them)
            cfast = fast_load_ds(kn, nx);
            store_pending();
        } else {
            store_pending();
            cfast = fast_load(kn, c0, c1, c2, c3);
        }
        const uint32_t kn2 = kn < n_p ? grab() : n_p;

        // ---- rounds: Cb x4 + Cr x4, Y blocks 0-7 (MCUs 0, 1), Y blocks 8-15 (MCUs 2, 3) ----
        // A round: inputs -> column pass -> transposed LDS write (Dct.hpp:124-131) ->
        // row pass -> quantise -> one 16-byte row store.  A wave's LDS operations run
        // in issue order, so only the compiler needs fencing between them.
        // The chroma round's inputs are read now; each later round's during the
        // previous round's row pass.
        uint32_t p[8];
        uint2 cc[16];
        double iq[8];
        load_c(cc);
        load_iq(1, iq);
        wave_order();
        auto finish = [&](double x[8], int m, int slot, int qb, u32x4& pk, uint32_t& off, auto&& prefetch_next) {
            double o[8];
            arai8(x, o);
#pragma unroll
            for (int k = 0; k < 8; ++k) tb[j * kTmpRow + k] = o[k];
            wave_order();
#pragma unroll
            for (int i = 0; i < 8; ++i) x[i] = tb[i * kTmpRow + j];
            double iqc[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) iqc[u] = iq[u];
            wave_order();
            prefetch_next();  // next round's inputs: after this round's LDS reads
            arai8_unscaled(x, o);  // y(j, u) = o[u] * s_u
            pk = quant_row(o, iqc, &lds.q[qb][j * kQRow]);
            const uint32_t blk = (mrow * mw + mcol0 + m) * 6 + slot;
            off = m < nvalid ? blk * 128 + j * 16 : kOob;
        };
        {
            double x[8];
            c_inputs(cc, x);
            u32x4 pk;
            uint32_t off;
            finish(x, cm, 4 + ccomp, 1, pk, off, [&] {
                load_y(0, p);
                load_iq(0, iq);
            });
            __builtin_amdgcn_raw_buffer_store_b128(pk, coef_rs, off, 0, kK1StoreAux);
        }
        {
            double x[8];
            y_inputs(p, x);
            u32x4 pk;
            uint32_t off;
            finish(x, b8 >> 2, b8 & 3, 0, pk, off, [&] { load_y(1, p); });
            __builtin_amdgcn_raw_buffer_store_b128(pk, coef_rs, off, 0, kK1StoreAux);
        }
        {
            double x[8];
            y_inputs(p, x);
            finish(x, 2 + (b8 >> 2), b8 & 3, 0, pend, poff, [] {});
        }
        wave_order();  // the next tile's staging overwrites the transpose buffer
        k = kn;
        kn = kn2;
    }
    store_pending();
    __syncthreads();
    JPGE_STAMP(7);
}

// ---- MCUs one block row high: 4:4:4, 4:2:2, 4:1:1 (applySubsampling S444, S422,
// S411, Image.cpp:257-278; the MCU is kYh Y blocks across + Cb + Cr) ----
// Same machinery as fdct_kernel: a wave owns a tile of 128x8 px (16 Y blocks,
// 16 / kYh MCUs; a lane stages one 16-px run of one row), in rounds of 8 blocks
// (lane = (block of the round, column)): Y blocks 0-7, Y blocks 8-15, then the
// chroma blocks — 4:4:4: Cb 0-7, Cb 8-15, Cr 0-7, Cr 8-15; 4:2:2: Cb 0-7, Cr 0-7;
// 4:1:1: Cb 0-3 + Cr 0-3 in one round.  S422 / S411 keep the first sample of each
// 2 / 4 along a row (mask {1,0} / {1,0,0,0}, every scanline; the mask's zero terms
// add zeros).  Chroma is converted per pixel: for 8-bit input (128 + v) - 128 == v
// exactly, and v = fma(kb, b, fma(kg, g, kr r)) is exact.
constexpr int kRgbPitch444 = 130;  // u32 per staged row of 128 px (+2: even, for uint2 stores)
static_assert(8 * kRgbPitch444 <= 16 * kRgbPitch, "the 4:4:4 tile fits the 4:2:0 staging area");

template <bool kExact, int kWaves, int kYh, int kN>
__global__ __launch_bounds__(kWaves * 64) JPGE_K1_OCC void fdct_row8_kernel(FrameSet<FdctArgs, kN> fs) {
    const uint32_t set_f = set_member<kN>(fs.wg0, fs.n, blockIdx.x);  // (frame sets: kernels.hpp)
    const FdctArgs& a = fs.a[set_f];
    const uint32_t bid = blockIdx.x - fs.wg0[set_f], nbk = fs.wg0[set_f + 1] - fs.wg0[set_f];
    // the arguments the tile loop reads, loaded once into scalar registers: a set
    // member's arguments sit at a computed kernarg offset, and the compiler otherwise
    // reloads them per tile (scalar loads whose lgkmcnt waits also wait for LDS traffic)
    const uint8_t* rgb_ = a.rgb;
    uint64_t stride_ = a.stride;
    uint32_t gw_ = a.g.width, gh_ = a.g.height;
    asm volatile("" : "+s"(rgb_), "+s"(stride_), "+s"(gw_), "+s"(gh_));
    uint32_t sw_ = gw_, sh_ = gh_;   // the frame the loads read: the downscaling builds' source
    if constexpr (kDs > 1) {
        sw_ = a.src_w;
        sh_ = a.src_h;
        asm volatile("" : "+s"(sw_), "+s"(sh_));
    }
    uint32_t rows_back_ = 0;         // the oriented builds: the source's rows run backwards
    if constexpr (kOrient != 0) {
        sw_ = a.src_w;
        sh_ = a.src_h;
        rows_back_ = orient_rows_back((int)a.orient) ? 1u : 0u;
        asm volatile("" : "+s"(sw_), "+s"(sh_), "+s"(rows_back_));
    }
    uint64_t ps_ = 0;                // planar: the plane pitch
    uint32_t sel4_ = kSelRgbx;       // 4-byte pixels: the byte selector of the channel order
    if constexpr (kShape == kShapePlanar || (kYuv && !kGray && !kPacked422 && kShape != kShapeY210 && !kV210)) {
        ps_ = a.plane_stride;
        asm volatile("" : "+s"(ps_));
    }
    if constexpr (kShape == kShapeX4) {
        sel4_ = a.fmt == kFmtBgra8 ? kSelBgrx : kSelRgbx;
        asm volatile("" : "+s"(sel4_));
    }
    if constexpr (kPacked422) {
        sel4_ = a.fmt == kFmtUyvy ? kSelUyvy : kSelYuyv;
        asm volatile("" : "+s"(sel4_));
    }
    uint32_t phase_ = 0;             // Bayer: the CFA phase of the frame's layout (kernels.hpp bayer_phase)
    if constexpr (kBayer) {
        phase_ = bayer_phase(a.fmt);
        asm volatile("" : "+s"(phase_));
    }
    XfK xf{};  // (the Y, Cb, Cr shapes' !kExact instances)
    if constexpr (kYuv && !kExact) xf = xf_load(a);
    constexpr int kK1Threads = kWaves * 64;
    constexpr uint32_t kMcus = 16 / kYh;            // MCUs per tile
    static_assert(!kGray || kYh == 1, "one component: one-block MCUs");
    constexpr int kBpm = kGray ? 1 : kYh + 2;         // blocks per MCU
    constexpr int kRounds = kGray ? 2 : 2 + 4 / kYh;  // 2 Y rounds + the chroma rounds (one component: none)
    __shared__ K1Lds<kWaves> lds;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    K1WaveLds& W = lds.w[wv];
    // (the channel tables' builds: the workgroup's copy, and this thread's word of the frame's tables,
    // loaded ahead of the first tile's pixel loads below: the vector memory counter retires in order,
    // so the wait for this word before its LDS write leaves the pixel loads in flight)
    const uint8_t* lut_ = nullptr;
    uint32_t lut_w_ = 0;
    if constexpr (kLut) {
        static_assert(kWaves * 64 >= kLutWords, "a thread loads one word of the tables");
        lut_ = reinterpret_cast<const uint8_t*>(lds.lut);
        // (through a descriptor of the 768 bytes, as the pixels: a thread past the tables loads nothing)
        const __amdgpu_buffer_rsrc_t lut_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(fdct_lut_raw(a)), 0, kLutBytes, 0x00020000);
        lut_w_ = __builtin_amdgcn_raw_buffer_load_b32(lut_rs, (uint32_t)tid * 4u, 0, 0);
    }
    JPGE_STAMP(1);
    const uint32_t mw = a.g.mw;
    const uint32_t tiles_per_row = (mw + kMcus - 1) / kMcus;
    const uint32_t ntiles = tiles_per_row * a.g.mh;
    const double scale = 255.0 / (double)a.maxval;  // Image.cpp:465
    // (I420, I422, I010, I210: the chroma pitch, half the stride, is 16-byte aligned too)
    const bool aligned = (((uintptr_t)rgb_ | stride_ | ps_) & 15) == 0 && (!(kHalfPitch || kShape == kShapeI010 || kShape == kShapeI210) || (stride_ & 31) == 0);
    const int r8 = lane >> 3, c8 = lane & 7;  // staging: lane -> (pixel row, 16-px chunk)
    const int b8 = lane >> 3, j = lane & 7;   // DCT: lane -> (block of the round, column)
    // (the oriented builds that are not transposed, as in fdct_kernel)
    const bool or_aligned = aligned && (!kOrMirror || ((kBpp * sw_) & 15u) == 0);
    auto or_pixel = [&](uint32_t oy, uint32_t ox) -> uint32_t {
        return edge_pixel(rgb_, stride_, ps_, sel4_, rows_back_ ? sh_ - 1 - oy : oy, kOrMirror ? sw_ - 1 - ox : ox);
    };

    const RgbRsrc rgb_rs = rgb_rsrc(rgb_, stride_, ps_, sw_, sh_);
    const __amdgpu_buffer_rsrc_t coef_rs =
        __builtin_amdgcn_make_buffer_rsrc(a.coef, 0, (int)(uint32_t)((uint64_t)a.g.nblocks() * 128), 0x00020000);

    // dynamic tiles over the workgroup's contiguous run, as in fdct_kernel
    const uint32_t tb_p = (uint32_t)((uint64_t)ntiles * bid / nbk);
    const uint32_t n_p = (uint32_t)((uint64_t)ntiles * (bid + 1) / nbk) - tb_p;
    auto grab = [&]() -> uint32_t {
        uint32_t v = 0;
        if (lane == 0) v = atomicAdd(&lds.next, 1u);
        return __builtin_amdgcn_readfirstlane(v);
    };
    const uint32_t lane_off = (uint32_t)r8 * (uint32_t)stride_ + (uint32_t)c8 * kRun;  // (as in fdct_kernel)
    // NV16, I422: the chroma of the run's 8 cells, in the pixels' own chroma row of pitch cpitch:
    // NV16 the 16 bytes under the run, I422 the 16 bytes that hold its 8
    uint32_t cpitch = 0, lane_coff = 0;
    if constexpr (kPlanes422) {
        cpitch = kPairs ? (uint32_t)stride_ : (uint32_t)((stride_ + 1) / 2);
        lane_coff = (uint32_t)r8 * cpitch + (kPairs ? (uint32_t)c8 : (uint32_t)(c8 >> 1)) * 16;
    }
    // P210, I210: the 32 bytes of pairs under the run, or the 16 bytes of each plane that are its 8 cells
    constexpr uint32_t kCellRun = kTenHi ? 32u : 16u;  // chroma bytes (of one plane) of 8 cells
    if constexpr (kTen) {
        cpitch = kTenHi ? (uint32_t)stride_ : (uint32_t)(2 * ((stride_ + 3) / 4));
        lane_coff = (uint32_t)r8 * cpitch + (uint32_t)c8 * kCellRun;
    }
    uint32_t hb[6];  // (Bayer: the prefetched bytes left and right of the run's three rows)
    auto fast_load = [&](uint32_t k, uint4& v0, uint4& v1, uint4& v2, uint4& v3) -> bool {
        const uint32_t t = tb_p + k;
        const uint32_t mrow = t / tiles_per_row, mcol0 = (t % tiles_per_row) * kMcus;
        const uint32_t y = mrow * 8 + r8, xs = mcol0 * 8 * kYh + c8 * 16;
        if constexpr (kOrient != 0) {
            const bool ok = k < n_p && or_aligned && y < gh_ && xs + 16 <= gw_;
            const uint32_t sr = rows_back_ ? sh_ - 1 - y : y, sc = kOrMirror ? sw_ - 16 - xs : xs;
            load_run(rgb_rs, ok ? sr * (uint32_t)stride_ + sc * kBpp : kOob, kOob, v0, v1, v2, v3);
            return ok;
        }
        if constexpr (kBayer) {  // (as in fdct_kernel)
            const bool ok = k < n_p && aligned && y < gh_ && xs + 16 <= gw_;
            const uint32_t st = (uint32_t)stride_;
            load_bayer(rgb_rs, ok, bayer_before(y) * st, y * st, bayer_after(y, gh_) * st, xs, bayer_before(xs),
                       bayer_after(xs + 15, gw_), v0, v1, v2, hb);
            return ok;
        }
        bool ok = k < n_p && aligned && y < gh_ && xs + 16 <= gw_;
        // (I422: and the 16 chroma bytes lie inside their row)
        if constexpr (kShape == kShapeI422) ok = ok && ((xs >> 5) + 1) * 16 <= (gw_ + 1) / 2;
        const uint32_t base = (uint32_t)((uint64_t)(mrow * 8) * stride_ + (uint64_t)mcol0 * (kRun / 2) * kYh);  // (uniform)
        const uint32_t off = ok ? base + lane_off : kOob;
        uint32_t coff = kOob;
        if constexpr (kPlanes422) {
            // the tile's 128 px: 128 bytes of Cb,Cr pairs (NV16), or 64 of each plane (I422)
            const uint32_t cbase = (uint32_t)((uint64_t)(mrow * 8) * cpitch + (uint64_t)mcol0 * (kPairs ? 8 : 4) * kYh);
            coff = ok ? cbase + lane_coff : kOob;
        }
        if constexpr (kTen && !kV210) {
            // (I210: the run's 8 cells are the 16 bytes themselves, inside their row whenever the run is)
            const uint32_t cbase = (uint32_t)((uint64_t)(mrow * 8) * cpitch + (uint64_t)mcol0 * (kCellRun / 2) * kYh);
            coff = ok ? cbase + lane_coff : kOob;
        }
        if constexpr (kV210) {
            // (as in fdct_kernel: xs = 16 n with n = 8 * tile column + c8)
            const uint32_t n = xs >> 4, g0 = (8 * n) / 3;
            const uint32_t o = (uint32_t)((uint64_t)(mrow * 8) * stride_) + (uint32_t)r8 * (uint32_t)stride_ + 16 * g0;
            load_run(rgb_rs, ok ? o : kOob, ok && n % 3 == 1 ? o + 48 : kOob, v0, v1, v2, v3);
            return ok;
        }
        load_run(rgb_rs, off, coff, v0, v1, v2, v3);
        return ok;
    };
    u32x4 pend;
    uint32_t poff = kOob;
    auto store_pending = [&] { __builtin_amdgcn_raw_buffer_store_b128(pend, coef_rs, poff, 0, kK1StoreAux); };
    // (the downscaling builds, as in fdct_kernel)
    auto fast_load_ds = [&](uint32_t k, uint32_t nx[16]) -> bool {
        const uint32_t t = tb_p + k;
        const uint32_t mrow = t / tiles_per_row, mcol0 = (t % tiles_per_row) * kMcus;
        const uint32_t y = mrow * 8 + r8, xs = mcol0 * 8 * kYh + c8 * 16;
        const bool ok = k < n_p && aligned && kDs * y + kDs <= sh_ && kDs * (xs + 16) <= sw_;
        const uint32_t off = (uint32_t)((uint64_t)(mrow * 8 * kDs) * stride_ + (uint64_t)mcol0 * (kRun / 2 * kDs) * kYh) +
                             (uint32_t)(r8 * kDs) * (uint32_t)stride_ + (uint32_t)c8 * (kRun * kDs);
        ds_load_run(rgb_rs, ok, off, (uint32_t)stride_, 0u, 0u, sel4_, nx);
        return ok;
    };
    uint32_t k = __builtin_amdgcn_readfirstlane((uint32_t)wv);
    uint4 c0, c1, c2, c3;
    uint32_t nx[16];
    bool cfast;
    if constexpr (kDs > 1) cfast = fast_load_ds(k, nx);
    else cfast = fast_load(k, c0, c1, c2, c3);
    // (the channel tables' word, loaded before the pixels: written here, ahead of the loop below, so
    // that the wait is a count the compiler knows, "all but the pixel loads", not zero)
    if constexpr (kLut)
        if (tid < kLutWords) lds.lut[tid] = lut_w_;

    for (uint32_t i = bid * kK1Threads + tid; i < a.zero_words; i += nbk * kK1Threads) a.zero[i] = 0;
    if (bid == 0)
        for (uint32_t i = tid; i < a.imp_n16; i += kK1Threads) a.imp_dst[i] = a.imp_src[i];
    if (tid == 0) lds.next = kWaves;
    if (tid < 128) {
        const int c = tid >> 6, e = tid & 63, o = (e >> 3) * kQRow + (e & 7);
        const double q = (double)q_entry(a, tid);
        lds.q[c][o] = q;
        lds.invq[c][o] = arai_scale(e & 7) / q;
    }
    // LDS-only barrier: the prologue's shared state is in LDS (a full __syncthreads
    // would also wait for the first tile's pixels, issued above)
    lds_barrier();
    JPGE_STAMP(0);
    uint32_t kn = k < n_p ? grab() : n_p;

    double* tb = &W.tmp[b8 * kTmpBlock];
    auto load_px = [&](int round, uint32_t p[8]) {  // column j of the round's block b8
        int col;
        if (round < 2 || kYh == 1) col = ((round & 1) * 8 + b8) * 8 + j;  // full resolution
        else if (kYh == 2) col = b8 * 16 + 2 * j;                          // S422: left of each pair
        else col = (b8 & 3) * 32 + 4 * j;                                  // S411: first of each 4
#pragma unroll
        for (int i = 0; i < 8; ++i) p[i] = W.rgbx[i * kRgbPitch444 + col];
    };
    auto load_iq = [&](int qb, double iq[8]) {
#pragma unroll
        for (int u = 0; u < 8; ++u) iq[u] = lds.invq[qb][j * kQRow + u];
    };

    for (; k < n_p;) {
        const uint32_t t = tb_p + k;
        const uint32_t mrow = t / tiles_per_row;
        const uint32_t mcol0 = (t % tiles_per_row) * kMcus;
        const int nvalid = (int)min(kMcus, mw - mcol0);
        const uint32_t y = mrow * 8 + r8, xs = mcol0 * 8 * kYh + c8 * 16;

        uint32_t px[16];
        if constexpr (kDs > 1) {
#pragma unroll
            for (int i = 0; i < 16; ++i) px[i] = nx[i];
        } else if constexpr (kGray) {
            unpack_gray(c0, px);
        } else if constexpr (kBayer) {
            const uint32_t dy = ((uint32_t)r8 ^ (phase_ >> 1)) & 1u;  // (as in fdct_kernel)
            unpack_bayer(c0, c1, c2, hb, dy, (dy ^ phase_) & 1u, px);
        } else if constexpr (kV210) {
            unpack_v210(c0, c1, c2, c3, (xs >> 4) % 3, px);
        } else if constexpr (kTen) {
            unpack_yuv10(c0, c1, c2, c3, px);
        } else if constexpr (kPlanes422) {
            unpack_yuv420(c0, c1, c2, (uint32_t)(c8 & 1), px);
        } else if constexpr (kPacked422) {
            unpack_packed422(c0, c1, sel4_, px);
        } else if constexpr (kShape == kShapeX4 || kShape == kShapePlanar || kShape == kShapeYuv444) {
            unpack_run(c0, c1, c2, c3, sel4_, px);
        } else {
            const uint4 v0 = c0, v1 = c1, v2 = c2;
            const uint32_t wd[13] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w, 0u};
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int b0 = 3 * i, d = b0 >> 2;
                // bytes b0..b0+2 of the run, zero-extended (perm selector 0x0c = 0x00); BGR8: 2, 1, 0
                const uint32_t o8 = (uint32_t)(b0 & 3);
                px[i] = __builtin_amdgcn_perm(wd[d + 1], wd[d], sel3(o8));
            }
        }
        if constexpr (kOrMirror) {  // the run in O's order: a renaming of registers
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const uint32_t t = px[i];
                px[i] = px[15 - i];
                px[15 - i] = t;
            }
        }
        if (!kBayer && !cfast) {  // edge replication (Image.cpp:498-531) as clamped addressing
            const uint32_t sy = min(y, gh_ - 1);
            if constexpr (kOrient != 0)  // (O's coordinates clamped first, then mapped to the source)
                for (int i = 0; i < 16; ++i) px[i] = or_pixel(sy, min(xs + i, gw_ - 1));
            else if constexpr (kDs > 1)
                for (int i = 0; i < 16; ++i) px[i] = edge_ds(rgb_, stride_, ps_, sw_, sh_, sel4_, sy, min(xs + i, gw_ - 1));
            else if constexpr (kYuv)
                for (int i = 0; i < 16; ++i) px[i] = edge_yuv(rgb_, stride_, ps_, gh_, sel4_, sy, min(xs + i, gw_ - 1));
            else
                for (int i = 0; i < 16; ++i) px[i] = edge_pixel(rgb_, stride_, ps_, sel4_, sy, min(xs + i, gw_ - 1));
        }
        if constexpr (kLut) {  // the channel tables: fast path and clamped path alike
#pragma unroll
            for (int i = 0; i < 16; ++i) px[i] = lut_map(lut_, px[i]);
        }
        uint32_t* dst = &W.rgbx[r8 * kRgbPitch444 + c8 * 16];
#pragma unroll
        for (int i = 0; i < 16; i += 2) *reinterpret_cast<uint2*>(dst + i) = make_uint2(px[i], px[i + 1]);
        if constexpr (kBayer)  // (as in fdct_kernel)
            if (!cfast) edge_bayer(rgb_, stride_, gw_, gh_, phase_, y, xs, dst, lut_);
        wave_order();
        if constexpr (kDs > 1) {
            cfast = fast_load_ds(kn, nx);
            store_pending();
        } else {
            store_pending();
            cfast = fast_load(kn, c0, c1, c2, c3);
        }
        const uint32_t kn2 = kn < n_p ? grab() : n_p;

        uint32_t p[8];
        double iq[8];
        load_px(0, p);
        load_iq(0, iq);
        wave_order();
#pragma unroll
        for (int round = 0; round < kRounds; ++round) {
            // the lane's block: component, MCU of the tile, slot in the MCU
            int comp, m, slot;
            if (round < 2) {
                const int bx = round * 8 + b8;  // Y block of the tile
                comp = 0; m = bx / kYh; slot = bx % kYh;
            } else {
                comp = kYh == 1 ? 1 + ((round - 2) >> 1) : kYh == 2 ? round - 1 : 1 + (b8 >> 2);
                m = kYh == 1 ? (round & 1) * 8 + b8 : kYh == 2 ? b8 : (b8 & 3);
                slot = kYh + comp - 1;
            }
            const int qb = comp ? 1 : 0;
            double x[8];
            if (comp == 0) {
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    x[i] = kYuv ? (kExact ? yuv_y(p[i]) : xf_y(xf, p[i])) : kExact ? ycc_exact_y(p[i]) : ycc_ref_y(p[i], scale);
            } else if constexpr (kYuv) {  // the kept sample itself, or its transform
                const double ku = comp == 2 ? xf.m5 : xf.m3, kv = comp == 2 ? xf.m6 : xf.m4;
#pragma unroll
                for (int i = 0; i < 8; ++i) x[i] = kExact ? yuv_c(p[i], comp) : xf_c(p[i], ku, kv);
            } else {
                const double kr = comp == 2 ? kCrR : kCbR, kg = comp == 2 ? kCrG : kCbG, kb = comp == 2 ? kCrB : kCbB;
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    x[i] = kExact ? ycc_exact_c(p[i], kr, kg, kb) : ycc_ref_c(p[i], scale, kr, kg, kb);
            }
            double o[8];
            arai8(x, o);
#pragma unroll
            for (int u = 0; u < 8; ++u) tb[j * kTmpRow + u] = o[u];
            wave_order();
#pragma unroll
            for (int i = 0; i < 8; ++i) x[i] = tb[i * kTmpRow + j];
            double iqc[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) iqc[u] = iq[u];
            wave_order();
            if (round + 1 < kRounds) {  // the next round's inputs, after this round's LDS reads
                load_px(round + 1, p);
                if (round == 1) load_iq(1, iq);
            }
            arai8_unscaled(x, o);
            const u32x4 pk = quant_row(o, iqc, &lds.q[qb][j * kQRow]);
            const uint32_t blk = (mrow * mw + mcol0 + m) * kBpm + slot;
            const uint32_t off = m < nvalid ? blk * 128 + j * 16 : kOob;
            if (round < kRounds - 1) {
                __builtin_amdgcn_raw_buffer_store_b128(pk, coef_rs, off, 0, kK1StoreAux);
            } else {
                pend = pk;
                poff = off;
            }
        }
        wave_order();  // the next tile's staging overwrites the transpose buffer
        k = kn;
        kn = kn2;
    }
    store_pending();
    __syncthreads();
    JPGE_STAMP(7);
}

}  // namespace

// Alone on the GPU, frames with fewer than kK1WholeCuTiles tiles (a 4K frame has
// 8 100) run the 4-wave shape at 4 workgroups per CU, larger ones the whole-CU shape:
// measured 15.5-15.6 vs 16.2-16.3 us at 4K, but 340-349 vs 317-326 us at 16384^2
// (262 144 tiles), where the whole-CU workgroups' shared tile counter balances ~64
// tiles per wave.
constexpr uint32_t kK1WholeCuTiles = 65536;
uint32_t k1_tiles(const Geometry& g);
bool k1_whole_cu(const Geometry& g, bool solo, uint32_t ds = 1, uint32_t orient = 0);
#if JPGE_K1_SHAPE == 0 && JPGE_K1_DS == 1 && JPGE_K1_ORIENT == 0 && JPGE_K1_LUT == 0
uint32_t k1_tiles(const Geometry& g) {
    const uint32_t per = g.row8() ? 16 / g.yh : 4;  // MCUs per tile
    return ((g.mw + per - 1) / per) * g.mh;
}
// (a downscaled frame, ds > 1: always the 4-wave shape, whose registers hold the reduction without spilling;
// an oriented frame, orient != 0: likewise, its builds have no other)
bool k1_whole_cu(const Geometry& g, bool solo, uint32_t ds, uint32_t orient) {
    return solo && ds <= 1 && orient == 0 && k1_tiles(g) >= kK1WholeCuTiles;
}
#endif

// (static, like the kernels: every load shape's build has its own)
template <int kYh, int kN>
static hipError_t launch_row8(const FrameSet<FdctArgs, kN>& fs, uint32_t grid, hipStream_t s, const KTimer* t) {
    const FdctArgs& a = fs.a[0];
    // (Y, Cb, Cr samples are 8-bit, maxval 255: their !kExact instances are the sample transform's)
    const bool ex = kYuv ? a.xf_on == 0 : a.maxval == 255;
    if constexpr (kTen) {
        // 10-bit samples always go through the sample transform: no kExact instance
        if (ex) return hipErrorInvalidValue;
        if (k1_whole_cu(a.g, a.solo)) return launch_timed(t, fdct_row8_kernel<false, kK1WavesSolo, kYh, kN>, dim3(grid), dim3(kK1WavesSolo * 64), s, fs);
        return launch_timed(t, fdct_row8_kernel<false, kK1WavesShared, kYh, kN>, dim3(grid), dim3(kK1WavesShared * 64), s, fs);
    } else if constexpr (kBayer || kLut) {
        // (the Bayer build and the channel tables' builds have the exact colour path's 4-wave workgroup only: maxval is 255)
        return !ex ? hipErrorInvalidValue : launch_timed(t, fdct_row8_kernel<true, kK1WavesShared, kYh, kN>, dim3(grid), dim3(kK1WavesShared * 64), s, fs);
    } else {
        // (the downscaling and the oriented builds have the 4-wave workgroup only: k1_whole_cu is false for them)
        if constexpr (kDs == 1 && kOrient == 0) {
            if (k1_whole_cu(a.g, a.solo)) {
                if (ex) return launch_timed(t, fdct_row8_kernel<true, kK1WavesSolo, kYh, kN>, dim3(grid), dim3(kK1WavesSolo * 64), s, fs);
                else return launch_timed(t, fdct_row8_kernel<false, kK1WavesSolo, kYh, kN>, dim3(grid), dim3(kK1WavesSolo * 64), s, fs);
            }
        }
        if (ex) return launch_timed(t, fdct_row8_kernel<true, kK1WavesShared, kYh, kN>, dim3(grid), dim3(kK1WavesShared * 64), s, fs);
        else return launch_timed(t, fdct_row8_kernel<false, kK1WavesShared, kYh, kN>, dim3(grid), dim3(kK1WavesShared * 64), s, fs);
    }
}

template <int kFilt, int kN>
static hipError_t launch_420(const FrameSet<FdctArgs, kN>& fs, uint32_t grid, hipStream_t s, const KTimer* t) {
    const FdctArgs& a = fs.a[0];
    // (Y, Cb, Cr samples are 8-bit, maxval 255: their !kExact instances are the sample transform's)
    const bool ex = kYuv ? a.xf_on == 0 : a.maxval == 255;
    if constexpr (kTen) {
        // 10-bit samples always go through the sample transform: no kExact instance
        if (ex) return hipErrorInvalidValue;
        if (k1_whole_cu(a.g, a.solo)) return launch_timed(t, fdct_kernel<false, kK1WavesSolo, kFilt, kN>, dim3(grid), dim3(kK1WavesSolo * 64), s, fs);
        return launch_timed(t, fdct_kernel<false, kK1WavesShared, kFilt, kN>, dim3(grid), dim3(kK1WavesShared * 64), s, fs);
    } else if constexpr (kBayer || kLut) {
        // (the Bayer build and the channel tables' builds have the exact colour path's 4-wave workgroup only: maxval is 255)
        return !ex ? hipErrorInvalidValue : launch_timed(t, fdct_kernel<true, kK1WavesShared, kFilt, kN>, dim3(grid), dim3(kK1WavesShared * 64), s, fs);
    } else {
        // (the downscaling and the oriented builds have the 4-wave workgroup only: k1_whole_cu is false for them)
        if constexpr (kDs == 1 && kOrient == 0) {
            if (k1_whole_cu(a.g, a.solo)) {
                if (ex) return launch_timed(t, fdct_kernel<true, kK1WavesSolo, kFilt, kN>, dim3(grid), dim3(kK1WavesSolo * 64), s, fs);
                else return launch_timed(t, fdct_kernel<false, kK1WavesSolo, kFilt, kN>, dim3(grid), dim3(kK1WavesSolo * 64), s, fs);
            }
        }
        if (ex) return launch_timed(t, fdct_kernel<true, kK1WavesShared, kFilt, kN>, dim3(grid), dim3(kK1WavesShared * 64), s, fs);
        else return launch_timed(t, fdct_kernel<false, kK1WavesShared, kFilt, kN>, dim3(grid), dim3(kK1WavesShared * 64), s, fs);
    }
}

// This build's kernel for a validated set (launch_fdct_fs) of grid workgroups.
template <int kN>
static hipError_t launch_k1(const FrameSet<FdctArgs, kN>& fs, uint32_t grid, hipStream_t s, const KTimer* t) {
    const FdctArgs& a = fs.a[0];
    // the kernels assume these shapes (kernels.hpp Geometry)
    if constexpr (kGray) {
        // one component: one-block MCUs, whatever the subsampling mode
        if (!a.g.gray() || a.g.yh != 1) return hipErrorInvalidValue;
        return launch_row8<1, kN>(fs, grid, s, t);
    } else if constexpr (kYuv420) {
        // the chroma planes are the S420_m planes already: the instance that takes each 2x2
        // cell's first staged word (all four hold the cell's sample) applies no filter
        if (a.g.row8() || a.g.yh != 2 || a.g.bpm != 6 || a.g.cfilt != kFiltS420m) return hipErrorInvalidValue;
        return launch_420<kFiltS420, kN>(fs, grid, s, t);
    } else {
        if (a.g.row8()) {
            // (the transposed builds have fdct_kernel only)
            if constexpr (kOrTrans) return hipErrorInvalidValue;
            else switch (a.g.yh) {
                // (launch_timed returns the launch's error: hipGetLastError has already consumed it)
                case 1: return a.g.bpm != 3 ? hipErrorInvalidValue : launch_row8<1, kN>(fs, grid, s, t);
                case 2: return a.g.bpm != 4 ? hipErrorInvalidValue : launch_row8<2, kN>(fs, grid, s, t);
                case 4: return a.g.bpm != 6 ? hipErrorInvalidValue : launch_row8<4, kN>(fs, grid, s, t);
                default: return hipErrorInvalidValue;
            }
        }
        if (a.g.yh != 2 || a.g.bpm != 6) return hipErrorInvalidValue;
        switch (a.g.cfilt) {
            case kFiltS420m: return launch_420<kFiltS420m, kN>(fs, grid, s, t);
            case kFiltS420lm: return launch_420<kFiltS420lm, kN>(fs, grid, s, t);
            case kFiltS420: return launch_420<kFiltS420, kN>(fs, grid, s, t);
            default: return hipErrorInvalidValue;
        }
    }
}

#if JPGE_K1_SHAPE != 0 || JPGE_K1_DS != 1 || JPGE_K1_ORIENT != 0 || JPGE_K1_LUT != 0
// this load shape's entry point (JPGE_K1_ENTRY: launch_fdct_bgr8 / _x4 / _planar / _nv12 / _i420 / _yuv444 / _gray /
// _packed422 / _nv16 / _i422 / _p010 / _i010 / _y210 / _p210 / _i210 / _v210 / _bayer8; the downscaling builds: launch_fdct_rgb8_d2 / _d4, _bgr8_d2, ...;
// the oriented builds: launch_fdct_rgb8_o1 .. _o4, _bgr8_o1, ...; the channel tables' builds: launch_fdct_rgb8_lut, _bgr8_lut, _x4_lut, _bayer8_lut)
hipError_t JPGE_K1_ENTRY(const FrameSet<FdctArgs, kMaxSet>& fs, uint32_t grid, hipStream_t s, const KTimer* t) {
    return launch_k1<kMaxSet>(fs, grid, s, t);
}
#if JPGE_K1_SHAPE >= 11 && JPGE_K1_SHAPE != 17
// the 10-bit shapes also have the lone frame's instance (launch_fdct_p010_one / _i010_one / _y210_one / ...), as the RGB8 shape has
#define JPGE_K1_CAT_(a, b) a##b
#define JPGE_K1_CAT(a, b) JPGE_K1_CAT_(a, b)
hipError_t JPGE_K1_CAT(JPGE_K1_ENTRY, _one)(const FrameSet<FdctArgs, 1>& fs, uint32_t grid, hipStream_t s, const KTimer* t) {
    return launch_k1<1>(fs, grid, s, t);
}
#endif
#else
hipError_t launch_fdct_bgr8(const FrameSet<FdctArgs, kMaxSet>& fs, uint32_t grid, hipStream_t s, const KTimer* t);
hipError_t launch_fdct_x4(const FrameSet<FdctArgs, kMaxSet>& fs, uint32_t grid, hipStream_t s, const KTimer* t);
hipError_t launch_fdct_planar(const FrameSet<FdctArgs, kMaxSet>& fs, uint32_t grid, hipStream_t s, const KTimer* t);
hipError_t launch_fdct_nv12(const FrameSet<FdctArgs, kMaxSet>& fs, uint32_t grid, hipStream_t s, const KTimer* t);
hipError_t launch_fdct_i420(const FrameSet<FdctArgs, kMaxSet>& fs, uint32_t grid, hipStream_t s, const KTimer* t);
hipError_t launch_fdct_yuv444(const FrameSet<FdctArgs, kMaxSet>& fs, uint32_t grid, hipStream_t s, const KTimer* t);
hipError_t launch_fdct_gray(const FrameSet<FdctArgs, kMaxSet>& fs, uint32_t grid, hipStream_t s, const KTimer* t);
hipError_t launch_fdct_packed422(const FrameSet<FdctArgs, kMaxSet>& fs, uint32_t grid, hipStream_t s, const KTimer* t);
hipError_t launch_fdct_nv16(const FrameSet<FdctArgs, kMaxSet>& fs, uint32_t grid, hipStream_t s, const KTimer* t);
hipError_t launch_fdct_i422(const FrameSet<FdctArgs, kMaxSet>& fs, uint32_t grid, hipStream_t s, const KTimer* t);
hipError_t launch_fdct_p010(const FrameSet<FdctArgs, kMaxSet>& fs, uint32_t grid, hipStream_t s, const KTimer* t);
hipError_t launch_fdct_i010(const FrameSet<FdctArgs, kMaxSet>& fs, uint32_t grid, hipStream_t s, const KTimer* t);
hipError_t launch_fdct_p010_one(const FrameSet<FdctArgs, 1>& fs, uint32_t grid, hipStream_t s, const KTimer* t);
hipError_t launch_fdct_i010_one(const FrameSet<FdctArgs, 1>& fs, uint32_t grid, hipStream_t s, const KTimer* t);
hipError_t launch_fdct_y210(const FrameSet<FdctArgs, kMaxSet>& fs, uint32_t grid, hipStream_t s, const KTimer* t);
hipError_t launch_fdct_p210(const FrameSet<FdctArgs, kMaxSet>& fs, uint32_t grid, hipStream_t s, const KTimer* t);
hipError_t launch_fdct_i210(const FrameSet<FdctArgs, kMaxSet>& fs, uint32_t grid, hipStream_t s, const KTimer* t);
hipError_t launch_fdct_y210_one(const FrameSet<FdctArgs, 1>& fs, uint32_t grid, hipStream_t s, const KTimer* t);
hipError_t launch_fdct_p210_one(const FrameSet<FdctArgs, 1>& fs, uint32_t grid, hipStream_t s, const KTimer* t);
hipError_t launch_fdct_i210_one(const FrameSet<FdctArgs, 1>& fs, uint32_t grid, hipStream_t s, const KTimer* t);
hipError_t launch_fdct_v210(const FrameSet<FdctArgs, kMaxSet>& fs, uint32_t grid, hipStream_t s, const KTimer* t);
hipError_t launch_fdct_v210_one(const FrameSet<FdctArgs, 1>& fs, uint32_t grid, hipStream_t s, const KTimer* t);
hipError_t launch_fdct_bayer8(const FrameSet<FdctArgs, kMaxSet>& fs, uint32_t grid, hipStream_t s, const KTimer* t);
// the downscaling builds (FdctArgs::ds 2, 4) of the shapes that have them
hipError_t launch_fdct_rgb8_d2(const FrameSet<FdctArgs, kMaxSet>& fs, uint32_t grid, hipStream_t s, const KTimer* t);
hipError_t launch_fdct_rgb8_d4(const FrameSet<FdctArgs, kMaxSet>& fs, uint32_t grid, hipStream_t s, const KTimer* t);
hipError_t launch_fdct_bgr8_d2(const FrameSet<FdctArgs, kMaxSet>& fs, uint32_t grid, hipStream_t s, const KTimer* t);
hipError_t launch_fdct_bgr8_d4(const FrameSet<FdctArgs, kMaxSet>& fs, uint32_t grid, hipStream_t s, const KTimer* t);
hipError_t launch_fdct_x4_d2(const FrameSet<FdctArgs, kMaxSet>& fs, uint32_t grid, hipStream_t s, const KTimer* t);
hipError_t launch_fdct_x4_d4(const FrameSet<FdctArgs, kMaxSet>& fs, uint32_t grid, hipStream_t s, const KTimer* t);
hipError_t launch_fdct_nv12_d2(const FrameSet<FdctArgs, kMaxSet>& fs, uint32_t grid, hipStream_t s, const KTimer* t);
hipError_t launch_fdct_nv12_d4(const FrameSet<FdctArgs, kMaxSet>& fs, uint32_t grid, hipStream_t s, const KTimer* t);
// the oriented builds (FdctArgs::orient, kernels.hpp orient_class 1..4) of the shapes that have them
#define JPGE_K1_ORIENT_ENTRIES(shape)                                                                                  \
    hipError_t launch_fdct_##shape##_o1(const FrameSet<FdctArgs, kMaxSet>& fs, uint32_t grid, hipStream_t s, const KTimer* t); \
    hipError_t launch_fdct_##shape##_o2(const FrameSet<FdctArgs, kMaxSet>& fs, uint32_t grid, hipStream_t s, const KTimer* t); \
    hipError_t launch_fdct_##shape##_o3(const FrameSet<FdctArgs, kMaxSet>& fs, uint32_t grid, hipStream_t s, const KTimer* t); \
    hipError_t launch_fdct_##shape##_o4(const FrameSet<FdctArgs, kMaxSet>& fs, uint32_t grid, hipStream_t s, const KTimer* t);
JPGE_K1_ORIENT_ENTRIES(rgb8)
JPGE_K1_ORIENT_ENTRIES(bgr8)
JPGE_K1_ORIENT_ENTRIES(x4)
#undef JPGE_K1_ORIENT_ENTRIES
// the channel tables' builds (kernels.hpp fdct_lut) of the shapes that have them
hipError_t launch_fdct_rgb8_lut(const FrameSet<FdctArgs, kMaxSet>& fs, uint32_t grid, hipStream_t s, const KTimer* t);
hipError_t launch_fdct_bgr8_lut(const FrameSet<FdctArgs, kMaxSet>& fs, uint32_t grid, hipStream_t s, const KTimer* t);
hipError_t launch_fdct_x4_lut(const FrameSet<FdctArgs, kMaxSet>& fs, uint32_t grid, hipStream_t s, const KTimer* t);
hipError_t launch_fdct_bayer8_lut(const FrameSet<FdctArgs, kMaxSet>& fs, uint32_t grid, hipStream_t s, const KTimer* t);

uint32_t fdct_grid(const Geometry& g, bool solo, uint32_t override_wgs, uint32_t ds, uint32_t orient) {
    const uint32_t tiles = k1_tiles(g);
    if (k1_whole_cu(g, solo, ds, orient)) {  // one whole-CU workgroup per CU (MI355X: 256 CUs)
        const uint32_t cap = 256u * (16u / (uint32_t)kK1WavesSolo);
        return tiles < cap ? tiles : cap;
    }
    // the 4-wave shape, a tile per wave at a time: four per CU alone, at most
    // kK1SharedCap beside other lanes
    const uint32_t wgs = (tiles + kK1WavesShared - 1) / kK1WavesShared;
    const uint32_t cap = override_wgs ? override_wgs : solo ? 1024u : kK1SharedCap;
    return wgs < cap ? wgs : cap;
}

// fdct_grid's last argument for a frame: non-zero rules the whole-CU shape out, for an oriented
// frame, a Bayer one and one with channel tables (their builds have the 4-wave workgroups only)
static uint32_t k1_small(const FdctArgs& a) { return fmt_bayer(a.fmt) || fdct_lut(a) ? 1u : a.orient; }

// A set of frames of one geometry, colour path and workgroup shape (one launch).
template <int kN>
static hipError_t launch_fdct_fs(const FrameSet<FdctArgs, kN>& fs, hipStream_t s, const KTimer* t) {
    const FdctArgs& a = fs.a[0];
    for (uint32_t f = 0; f < fs.n; ++f) {
        const FdctArgs& m = fs.a[f];
        // 32-bit buffer offsets: the frame's pixels and coefficients must stay below kOob
        // (a 16384^2 frame needs 805 MB of each)
        // (planar: each plane has its own descriptor, so the extent is one plane's)
        // (the 4:2:0, NV16 and I422 layouts' chroma planes have descriptors of their own, with no larger extents)
        // (a one-component geometry goes with the gray layout, and only with it)
        if (!fmt_valid(m.fmt) || m.g.height == 0 || ((fmt_yuv(m.fmt) || fmt_gray(m.fmt)) && m.maxval != 255) ||
            fmt_gray(m.fmt) != m.g.gray())
            return hipErrorInvalidValue;
        // (a Bayer frame: a 2x2 cell at least, so that a reflected neighbour exists; one plane; the
        // exact colour path.  The members of a set may differ in CFA phase: each reads its own.)
        if (fmt_bayer(m.fmt) && (m.g.width < 2 || m.g.height < 2 || m.maxval != 255 || m.plane_stride)) return hipErrorInvalidValue;
        // (channel tables: the exact colour path, at full size and as the frame lies; a set is all
        // with tables or all without: the setting is a context's, and a group's members share it)
        if (fdct_lut(m) && (m.maxval != 255 || m.ds > 1 || m.orient)) return hipErrorInvalidValue;
        if ((fdct_lut(m) != nullptr) != (fdct_lut(a) != nullptr)) return hipErrorInvalidValue;
        static_assert(kK1OffsetBound == kOob, "the host's bound is the kernel's out-of-range offset");
        // a downscaled frame: g is the frame of ceil(src / ds) pixels; the offsets span the source
        Geometry src = m.g;
        if (m.ds > 1) {
            if (!ds_valid((int)m.ds) || !ds_fmt(m.fmt) || !m.src_w || !m.src_h || m.g.width != ds_dim(m.src_w, (int)m.ds) ||
                m.g.height != ds_dim(m.src_h, (int)m.ds))
                return hipErrorInvalidValue;
            src.width = m.src_w;
            src.height = m.src_h;
        }
        // an oriented frame: g is O's; the offsets span the source.  The interleaved RGB layouts, no
        // downscale; the transposed orientations in the 16x16-MCU modes.  A set shares one
        // orientation and one source size.
        if (m.orient) {
            if (!orient_valid((int)m.orient) || !orient_fmt(m.fmt) || m.ds > 1 || !m.src_w || !m.src_h ||
                m.g.width != orient_w(m.src_w, m.src_h, (int)m.orient) || m.g.height != orient_h(m.src_w, m.src_h, (int)m.orient) ||
                (orient_transposed((int)m.orient) && m.g.row8()))
                return hipErrorInvalidValue;
            src.width = m.src_w;
            src.height = m.src_h;
        }
        if (!k1_offsets_fit(m.fmt, src, m.stride)) return hipErrorInvalidValue;
        if ((m.ds > 1 ? m.ds : 1u) != (a.ds > 1 ? a.ds : 1u) || (m.ds > 1 && (m.src_w != a.src_w || m.src_h != a.src_h)))
            return hipErrorInvalidValue;
        if (m.orient != a.orient || (m.orient && (m.src_w != a.src_w || m.src_h != a.src_h))) return hipErrorInvalidValue;
        // 10-bit layouts: 16-bit words (even addresses and pitches), and always the sample transform
        if (fmt_yuv10(m.fmt) && ((((uintptr_t)m.rgb | m.stride | m.plane_stride) & 1) || !m.xf_on)) return hipErrorInvalidValue;
        // (v210: 32-bit words, one plane, no downscaling build)
        if (m.fmt == kFmtV210 && ((((uintptr_t)m.rgb | m.stride) & 3) || m.plane_stride)) return hipErrorInvalidValue;
        if (std::memcmp(&m.g, &a.g, sizeof(Geometry)) != 0 || (m.maxval == 255) != (a.maxval == 255) ||
            fmt_shape(m.fmt) != fmt_shape(a.fmt) || (m.xf_on != 0) != (a.xf_on != 0) ||
            m.solo != a.solo || fs.wg0[f + 1] - fs.wg0[f] != fdct_grid(m.g, m.solo, m.wgs, m.ds, k1_small(m)))
            return hipErrorInvalidValue;
    }
    const uint32_t grid = fs.wg0[fs.n];
    const bool lut = fdct_lut(a) != nullptr;
    if (a.ds <= 1 && !a.orient && !lut && fmt_shape(a.fmt) == kShapeRgb8) return launch_k1(fs, grid, s, t);
    if constexpr (kN == 1) {
        if (fmt_shape(a.fmt) == kShapeP010) return launch_fdct_p010_one(fs, grid, s, t);
        if (fmt_shape(a.fmt) == kShapeI010) return launch_fdct_i010_one(fs, grid, s, t);
        if (fmt_shape(a.fmt) == kShapeY210) return launch_fdct_y210_one(fs, grid, s, t);
        if (fmt_shape(a.fmt) == kShapeP210) return launch_fdct_p210_one(fs, grid, s, t);
        if (fmt_shape(a.fmt) == kShapeI210) return launch_fdct_i210_one(fs, grid, s, t);
        if (fmt_shape(a.fmt) == kShapeV210) return launch_fdct_v210_one(fs, grid, s, t);
    }
    // the other load shapes have the frame-set instance only (a lone frame is a set of one)
    FrameSet<FdctArgs, kMaxSet> w{};
    w.n = fs.n;
    for (uint32_t f = 0; f < fs.n; ++f) w.a[f] = fs.a[f];
    for (uint32_t f = 0; f <= fs.n; ++f) w.wg0[f] = fs.wg0[f];
    if (a.orient) {
        const int c = orient_class((int)a.orient);
        switch (fmt_shape(a.fmt)) {
            case kShapeRgb8: return c == 1 ? launch_fdct_rgb8_o1(w, grid, s, t) : c == 2 ? launch_fdct_rgb8_o2(w, grid, s, t) : c == 3 ? launch_fdct_rgb8_o3(w, grid, s, t) : launch_fdct_rgb8_o4(w, grid, s, t);
            case kShapeBgr8: return c == 1 ? launch_fdct_bgr8_o1(w, grid, s, t) : c == 2 ? launch_fdct_bgr8_o2(w, grid, s, t) : c == 3 ? launch_fdct_bgr8_o3(w, grid, s, t) : launch_fdct_bgr8_o4(w, grid, s, t);
            case kShapeX4: return c == 1 ? launch_fdct_x4_o1(w, grid, s, t) : c == 2 ? launch_fdct_x4_o2(w, grid, s, t) : c == 3 ? launch_fdct_x4_o3(w, grid, s, t) : launch_fdct_x4_o4(w, grid, s, t);
            default: return hipErrorInvalidValue;
        }
    }
    if (a.ds > 1) {
        const bool d2 = a.ds == 2;
        switch (fmt_shape(a.fmt)) {
            case kShapeRgb8: return d2 ? launch_fdct_rgb8_d2(w, grid, s, t) : launch_fdct_rgb8_d4(w, grid, s, t);
            case kShapeBgr8: return d2 ? launch_fdct_bgr8_d2(w, grid, s, t) : launch_fdct_bgr8_d4(w, grid, s, t);
            case kShapeX4: return d2 ? launch_fdct_x4_d2(w, grid, s, t) : launch_fdct_x4_d4(w, grid, s, t);
            case kShapeNv12: return d2 ? launch_fdct_nv12_d2(w, grid, s, t) : launch_fdct_nv12_d4(w, grid, s, t);
            default: return hipErrorInvalidValue;
        }
    }
    if (lut) {
        switch (fmt_shape(a.fmt)) {
            case kShapeRgb8: return launch_fdct_rgb8_lut(w, grid, s, t);
            case kShapeBgr8: return launch_fdct_bgr8_lut(w, grid, s, t);
            case kShapeX4: return launch_fdct_x4_lut(w, grid, s, t);
            case kShapeBayer8: return launch_fdct_bayer8_lut(w, grid, s, t);
            default: return hipErrorInvalidValue;
        }
    }
    switch (fmt_shape(a.fmt)) {
        case kShapeBgr8: return launch_fdct_bgr8(w, grid, s, t);
        case kShapeX4: return launch_fdct_x4(w, grid, s, t);
        case kShapeNv12: return launch_fdct_nv12(w, grid, s, t);
        case kShapeI420: return launch_fdct_i420(w, grid, s, t);
        case kShapeYuv444: return launch_fdct_yuv444(w, grid, s, t);
        case kShapeGray: return launch_fdct_gray(w, grid, s, t);
        case kShapePacked422: return launch_fdct_packed422(w, grid, s, t);
        case kShapeNv16: return launch_fdct_nv16(w, grid, s, t);
        case kShapeI422: return launch_fdct_i422(w, grid, s, t);
        case kShapeP010: return launch_fdct_p010(w, grid, s, t);
        case kShapeI010: return launch_fdct_i010(w, grid, s, t);
        case kShapeY210: return launch_fdct_y210(w, grid, s, t);
        case kShapeP210: return launch_fdct_p210(w, grid, s, t);
        case kShapeI210: return launch_fdct_i210(w, grid, s, t);
        case kShapeV210: return launch_fdct_v210(w, grid, s, t);
        case kShapeBayer8: return launch_fdct_bayer8(w, grid, s, t);
        default: return launch_fdct_planar(w, grid, s, t);
    }
}

hipError_t launch_fdct(const FdctArgs& a, hipStream_t s, const KTimer* t) {
    return launch_fdct_fs(frame_set<1>(&a, 1, fdct_grid(a.g, a.solo, a.wgs, a.ds, k1_small(a))), s, t);
}

hipError_t launch_fdct_set(const FdctArgs* a, int n, hipStream_t s, const KTimer* t) {
    if (n < 1 || n > kMaxSet) return hipErrorInvalidValue;
    return launch_fdct_fs(frame_set(a, n, fdct_grid(a[0].g, a[0].solo, a[0].wgs, a[0].ds, k1_small(a[0]))), s, t);
}
#endif  // JPGE_K1_SHAPE == 0

}  // namespace jpge
