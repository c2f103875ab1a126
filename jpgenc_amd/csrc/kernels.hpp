// Device-side interface of the jpge HIP kernels (gfx950).  Host code fills
// these parameter blocks; fdct.hip / stats.hip / entropy.hip own the launch
// geometry.
//
// Data layout in HBM (per frame):
//   rgb   : the frame's pixels in one of the input layouts below, row pitch `stride`
//           (16-byte aligned pitch/base/plane pitch = fast path)
//   coef  : int16 [nmcu][6][64]  quantised coefficients, NATURAL order inside a block,
//           blocks in MCU-interleave order Y00 Y01 Y10 Y11 Cb Cr (= entropy order)
//   hist  : u32 cnt[kHistReplicas][4][256], u64 key[4][256] (~first-occurrence key)
//   ubuf  : u8 [G][kEntropyRegionBytes] each entropy workgroup's bit stream before
//           byte alignment and 0xFF stuffing, written and re-read by that workgroup
#pragma once
#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime_api.h>

#if defined(__HIPCC__)
#define JPGE_HD __host__ __device__
#else
#define JPGE_HD
#endif

namespace jpge {

// Frame geometry (reference: Image.cpp:480-531 pads to 16, Image.cpp:311-312
// halves the chroma planes).  One MCU = 16x16 px = Y00 Y01 Y10 Y11 Cb Cr.
// An MCU is yh x yv Y blocks (row by row) + one Cb + one Cr block, bpm = yh*yv + 2:
//   4:2:0 (the reference's S420_m, and the S420 / S420_lm filters): 2x2, 16x16 px;
//   4:4:4: 1x1, 8x8 px;  4:2:2: 2x1, 16x8 px;  4:1:1: 4x1, 32x8 px.
// One component (kFmtGray8): bpm = 1 with yh = 1, an MCU is one block and there is no
// chroma; blocks, the DC chain and the texts run in block raster order.
// cfilt selects the 4:2:0 chroma filter of applySubsampling (Image.cpp:279-306).
constexpr uint32_t kFiltS420m = 0, kFiltS420lm = 1, kFiltS420 = 2;
struct Geometry {
    uint32_t width = 0, height = 0;  // real size
    uint32_t mw = 0, mh = 0;         // MCUs per row / column
    uint32_t bpm = 6;
    uint32_t yh = 2;                 // Y blocks across an MCU (1, 2, 4)
    uint32_t cfilt = kFiltS420m;
    JPGE_HD uint32_t nmcu() const { return mw * mh; }
    JPGE_HD uint32_t nblocks() const { return nmcu() * bpm; }
    JPGE_HD bool gray() const { return bpm == 1; }          // one component: no chroma slots
    JPGE_HD uint32_t ny() const { return gray() ? 1u : bpm - 2; }  // Y blocks of an MCU
    JPGE_HD uint32_t yv() const { return ny() / yh; }  // Y blocks down an MCU (1, 2)
    JPGE_HD bool s444() const { return bpm == 3; }
    JPGE_HD bool row8() const { return ny() == yh; }  // MCUs one block row high
    JPGE_HD uint32_t mcu_w() const { return 8 * yh; }   // MCU size in pixels
    JPGE_HD uint32_t mcu_h() const { return 8 * yv(); }
};
// component of MCU slot k: 0 = Y, 1 = Cb, 2 = Cr (the last two slots are the chroma;
// bpm = 1: the one slot is Y)
JPGE_HD inline int block_comp(int k, uint32_t bpm) { return bpm == 1 || k < (int)bpm - 2 ? 0 : k - ((int)bpm - 3); }

// Input layouts (jpge.h JPGE_FMT_*, the same values) and K1's load shapes: what a lane
// loads for its 16-pixel run.  Each shape is one build of fdct.hip (JPGE_K1_SHAPE).  layouts.hpp has
// each layout's row: its shape, row and plane arithmetic, families and capabilities (host code).
constexpr int kFmtRgb8 = 0, kFmtBgr8 = 1, kFmtRgba8 = 2, kFmtBgra8 = 3, kFmtRgb8Planar = 4, kFmtCount = 5;
// full-range 8-bit Y, Cb, Cr samples (no colour conversion; a sample v is the fp64 value v - 128):
// NV12 (Y plane + one plane of interleaved Cb,Cr at half size), I420 (Y, Cb, Cr planes,
// chroma at half size), planar 4:4:4 (addressed as kFmtRgb8Planar)
constexpr int kFmtNv12 = 16, kFmtI420 = 17, kFmtYuv444Planar = 18;
// 4:2:2 frames of the same samples, one Cb and one Cr per horizontal pixel pair (cell x >> 1) of
// every row: packed groups Y0 Cb Y1 Cr (YUYV) or Cb Y0 Cr Y1 (UYVY), NV16 (Y plane + a plane of
// interleaved Cb,Cr rows), I422 (Y, Cb, Cr planes).  A frame is the planar 4:4:4 frame whose
// chroma planes hold c[y][x >> 1] at pixel (y, x), in every subsampling mode.
constexpr int kFmtYuyv = 20, kFmtUyvy = 21, kFmtNv16 = 22, kFmtI422 = 23;
// 10-bit 4:2:0 frames of little-endian 16-bit words: P010 (NV12's planes, a sample in the top 10
// bits of its word) and I010 (I420's planes, a sample in the low 10 bits).  A sample s is the
// exact fp64 value s / 4 in 8-bit units, and always goes through the sample transform.
constexpr int kFmtP010 = 32, kFmtI010 = 33;
// 10-bit 4:2:2 frames of the same words, one Cb and one Cr per horizontal pixel pair of every row:
// Y210 (packed groups Y0 Cb Y1 Cr of four words, a sample in its word's top 10 bits), P210 (NV16's
// planes, top 10 bits), I210 (I422's planes, low 10 bits).  A frame is the frame of samples
// s_y[y][x], s_cb[y][x >> 1], s_cr[y][x >> 1], each s / 4, in every subsampling mode.
constexpr int kFmtY210 = 40, kFmtP210 = 41, kFmtI210 = 42;
// v210 (10-bit SDI capture): the same samples packed three to a little-endian 32-bit word (bits
// 0-9, 10-19, 20-29), a row the stream Cb0 Y0 Cr0 Y1 Cb1 Y2 Cr1 Y3 ...: pixel x has its Y at stream
// index 2x + 1, cell c its Cb at 4c and its Cr at 4c + 2; six pixels are a group of four words.
constexpr int kFmtV210 = 48;
// one plane of 8-bit luminance samples (a sample v is the fp64 value v - 128, as a Y sample
// above): a one-component stream, Geometry::gray(), whatever the subsampling mode
constexpr int kFmtGray8 = 8;
// 8-bit Bayer mosaics (camera raw, white balance and gamma applied in the camera): one plane of one
// byte per pixel, the name the colours of the 2x2 cell at rows 0-1, columns 0-1, read row by row.
// The frame codes as the RGB8 frame of its bilinear demosaic (jpge.h; bayer_rgb below), built in
// K1's tile staging.  code - kFmtBayerRggb8 is the phase: bit 0 the column parity of the R sites,
// bit 1 their row parity.
constexpr int kFmtBayerRggb8 = 10, kFmtBayerGrbg8 = 11, kFmtBayerGbrg8 = 12, kFmtBayerBggr8 = 13;
JPGE_HD inline bool fmt_bayer(int fmt) { return fmt >= kFmtBayerRggb8 && fmt <= kFmtBayerBggr8; }
JPGE_HD inline uint32_t bayer_phase(int fmt) { return (uint32_t)(fmt - kFmtBayerRggb8); }
// a neighbour's coordinate, reflected without repeating the edge (n >= 2): -1 is 1, n is n - 2
JPGE_HD inline uint32_t bayer_before(uint32_t i) { return i ? i - 1 : 1u; }
JPGE_HD inline uint32_t bayer_after(uint32_t i, uint32_t n) { return i + 1 < n ? i + 1 : n - 2; }
// R | G << 8 | B << 16 of site (y, x) from its 3x3 neighbourhood: l, m, r are columns x - 1, x,
// x + 1 (reflected), each V(y - 1) | V(y) << 8 | V(y + 1) << 16.  The rule of jpge.h in integers;
// jpge_demosaic_frame and K1's byte path both call it.
JPGE_HD inline uint32_t bayer_rgb(uint32_t phase, uint32_t y, uint32_t x, uint32_t l, uint32_t m, uint32_t r) {
    const uint32_t dy = (y ^ (phase >> 1)) & 1, dx = (x ^ phase) & 1;  // (0, 0): an R site; (1, 1): a B site
    const uint32_t lm = (l >> 8) & 0xFF, rm = (r >> 8) & 0xFF;
    uint32_t lo, mid, hi;  // on an R row: R, G, B; on a B row lo and hi trade places
    if (dx == dy) {  // R or B: its own colour, G of the four beside it, the other colour of the diagonals
        lo = (m >> 8) & 0xFF;
        mid = ((m & 0xFF) + (m >> 16) + lm + rm + 2) >> 2;
        hi = ((l & 0xFF) + (l >> 16) + (r & 0xFF) + (r >> 16) + 2) >> 2;
    } else {  // G: its row's colour left and right, its column's colour above and below
        lo = (lm + rm + 1) >> 1;
        mid = (m >> 8) & 0xFF;
        hi = ((m & 0xFF) + (m >> 16) + 1) >> 1;
    }
    return dy ? hi | (mid << 8) | (lo << 16) : lo | (mid << 8) | (hi << 16);
}
constexpr int kShapeRgb8 = 0;    // 48 bytes R,G,B,...: three b128 loads
constexpr int kShapeBgr8 = 1;    // the same loads, bytes 2,1,0 of each pixel
constexpr int kShapeX4 = 2;      // RGBA8 / BGRA8: 64 bytes, four b128 loads, a wave-uniform byte selector
constexpr int kShapePlanar = 3;  // 16 bytes of each of the planes R, G, B: three b128 loads
constexpr int kShapeNv12 = 4;    // 16 Y bytes + the 16 Cb,Cr bytes (8 samples of both) under them: two b128 loads
constexpr int kShapeI420 = 5;    // 16 Y bytes + 16 Cb bytes + 16 Cr bytes (the lane uses 8 of each): three b128 loads
constexpr int kShapeYuv444 = 6;  // the planar shape's loads of the planes Y, Cb, Cr
constexpr int kShapeGray = 7;    // 16 Y bytes: one b128 load (no chroma: Geometry::gray())
constexpr int kShapePacked422 = 8;  // YUYV / UYVY: the run's 32 bytes, two b128 loads, wave-uniform byte selectors
constexpr int kShapeNv16 = 9;    // the NV12 shape's two loads, the Cb,Cr row that of the pixels
constexpr int kShapeI422 = 10;   // the I420 shape's three loads, the chroma rows those of the pixels
constexpr int kShapeP010 = 11;   // 32 Y bytes (16 words) + the 32 bytes of Cb,Cr word pairs under them: four b128 loads
constexpr int kShapeI010 = 12;   // 32 Y bytes + the 16 Cb bytes + the 16 Cr bytes of the run's 8 cells: four b128 loads
constexpr int kShapeY210 = 13;   // the run's 64 bytes (8 groups of four words): four b128 loads
constexpr int kShapeP210 = 14;   // the P010 shape's four loads, the Cb,Cr row that of the pixels
constexpr int kShapeI210 = 15;   // the I010 shape's four loads, the chroma rows those of the pixels
constexpr int kShapeV210 = 16;   // the three or four 16-byte groups that hold the run: four b128 loads, a per-lane phase
constexpr int kShapeBayer8 = 17; // 16 raw bytes of rows y - 1, y, y + 1 and the six bytes beside them: three b128 and six byte loads
JPGE_HD inline uint32_t chroma_dim(uint32_t n) { return (n + 1) / 2; }
// K1's out-of-range buffer offset (fdct.hip kOob), the bound of layouts.hpp k1_offsets_fit
constexpr uint64_t kK1OffsetBound = 0xFFFFFF00u;

constexpr int kHistReplicas = 8;  // spread of the global histogram atomics
constexpr int kStatsTile = 128;           // blocks per statistics tile (4 lanes each)
constexpr int kEntropyTile = 128;         // blocks per entropy tile (4 lanes each)
constexpr int kEntropyMaxTilesPerWg = 4;  // tiles a persistent entropy workgroup may own
constexpr int kStageBytesPerBlock = 216;  // >= worst-case 1665 bits of one block
constexpr int kStampSlots = 16;           // diagnostic stamp words per workgroup (JPGE_STAMPS builds)
constexpr int kEntropyRecordBytes = 48;   // per entropy workgroup: bits, edge bits, 0xFF counts

// Tables: 0 Y-DC, 1 Y-AC, 2 C-DC, 3 C-AC.
struct HistPtrs {
    uint32_t* cnt;
    uint64_t* key;
};

struct FdctArgs {
    const uint8_t* rgb;
    uint64_t stride;
    Geometry g;
    int maxval;      // 255 -> exact integer colour path
    bool solo;       // the kernel has the GPU to itself: whole-CU workgroups (else 4-wave ones)
    uint32_t wgs;    // pipeline grid override (0: the default cap; experiments, JPGE_FDCT_WGS)
    // box downscale (jpge_set_downscale): 2 or 4 = g is the frame of ceil(src / ds) pixels whose
    // samples are the rounded means of ds x ds source samples, read from a src_w x src_h frame
    // (the downscaling load shapes, fdct.hip JPGE_K1_DS); 0 or 1: none, g is the frame at rgb.
    // (in the padding before q, src_w and src_h in the padding before xf: no field moves, and
    // the block keeps its size)
    uint32_t ds = 1;
    // orientation (jpge_set_orientation, kOrient* below): non-zero = g is the oriented frame O, read
    // from the src_w x src_h frame at rgb (the oriented load shapes, fdct.hip JPGE_K1_ORIENT).
    // (in the last padding word before q)
    uint32_t orient = 0;
    // luma then chroma quantisers, natural order (bytes: a small kernarg block; 16-byte
    // aligned so the kernels fetch it with scalar loads, see fdct.hip q_entry)
    alignas(16) uint8_t q[128];
    int16_t* coef;
    uint32_t* zero;       // the frame's control block, zeroed by this kernel (it runs first)
    uint32_t zero_words;
    // carried duty: import another frame's tables + headers from mapped host memory
    // (workgroup 0; 0 units = none)
    const uint4* imp_src;
    uint4* imp_dst;
    uint32_t imp_n16;
    uint64_t* dbg;   // diagnostic phase stamps (JPGE_STAMPS builds), else unused
    // input layout (kFmt*); planar: plane c's rows start at rgb + c * plane_stride
    // (NV12, I420, NV16, I422 and the 10-bit planar layouts: the chroma starts at rgb + plane_stride, see fmt_chroma_pitch)
    int fmt = kFmtRgb8;
    // 1: the Y, Cb, Cr and gray shapes convert each sample by xf (jpge_set_yuv_transform, a
    // preset other than FULL_601): their !kExact instances.  The other shapes ignore it.
    // (in the padding after fmt; xf at the block's end: no earlier field moves)
    uint32_t xf_on = 0;
    uint64_t plane_stride = 0;
    uint32_t src_w = 0, src_h = 0;  // ds > 1 or orient != 0: the source frame's size (stride and plane_stride are its pitches)
    // y_off, m0..m6 (host_io.hpp YuvXf); fetched with scalar loads, like q
    alignas(16) double xf[8] = {0, 1, 0, 0, 1, 0, 0, 1};
};

static_assert(sizeof(FdctArgs) == 336 && offsetof(FdctArgs, q) == 64 && offsetof(FdctArgs, xf) == 272,
              "the downscale fields sit in padding: the argument block's layout is unchanged");
static_assert(offsetof(FdctArgs, ds) == 56 && offsetof(FdctArgs, orient) == 60, "the orientation sits in padding too");
// (The block has no padding left.  A Bayer frame's CFA phase needs no field: it is bayer_phase(fmt),
// which each member of a frame set reads from its own block, as the 4-byte shape reads its channel order.)

// Per-channel lookup tables (jpge.h jpge_set_channel_lut): kLutBytes bytes, T[256 c + v] the value of
// channel c (0 R, 1 G, 2 B) for the sample v.  A frame codes as the RGB8 frame M with
// M[y][x][c] = T[256 c + D[y][x][c]], D the frame's RGB8 pixels (a Bayer frame: its demosaic), mapped
// in K1's tile staging (fdct.hip JPGE_K1_LUT).  The interleaved RGB layouts and the Bayer ones, at
// full size and as they lie.  The RGB and Bayer shapes never read xf, so the device pointer of the
// context's table lives in that field's first 8 bytes: all zero bits (the default, xf[0] = 0.0) is
// "no table", and the host writes it only when a table is on.  Each member of a frame set reads
// its own.
constexpr int kLutBytes = 768;
JPGE_HD inline bool lut_fmt(int fmt) { return (fmt >= kFmtRgb8 && fmt <= kFmtBgra8) || fmt_bayer(fmt); }
JPGE_HD inline const uint8_t* fdct_lut_raw(const FdctArgs& a) {
    return reinterpret_cast<const uint8_t*>(__builtin_bit_cast(uint64_t, a.xf[0]));
}
// (the other shapes' xf is their sample transform)
JPGE_HD inline const uint8_t* fdct_lut(const FdctArgs& a) { return lut_fmt(a.fmt) ? fdct_lut_raw(a) : nullptr; }
inline void fdct_set_lut(FdctArgs& a, const uint8_t* d_lut) { a.xf[0] = __builtin_bit_cast(double, (uint64_t)reinterpret_cast<uintptr_t>(d_lut)); }

// Box downscale by 2 or 4 inside K1 (jpge.h jpge_set_downscale): the interleaved RGB layouts in
// every subsampling mode, and NV12 (whose Cb,Cr plane is averaged in its own domain).
JPGE_HD inline bool ds_valid(int ds) { return ds == 1 || ds == 2 || ds == 4; }
JPGE_HD inline uint32_t ds_dim(uint32_t n, int ds) { return (n + (uint32_t)ds - 1) / (uint32_t)ds; }

// Orientation applied inside K1 (jpge.h jpge_set_orientation, the same values): the coded frame
// O of a sw x sh source S.  Three properties describe all eight: transposed (O is sh x sw and its
// rows are the source's columns), mirrored (the source's columns run backwards) and rows_back (the
// source's rows run backwards).  The interleaved RGB layouts only; 4-7 in the 16x16-MCU modes only.
constexpr int kOrientNone = 0, kOrientFlipH = 1, kOrientRot180 = 2, kOrientFlipV = 3, kOrientTranspose = 4,
              kOrientRot90 = 5, kOrientTransverse = 6, kOrientRot270 = 7;
JPGE_HD inline bool orient_valid(int o) { return o >= 0 && o <= 7; }
JPGE_HD inline bool orient_transposed(int o) { return o >= 4; }
JPGE_HD inline bool orient_mirrored(int o) { return ((0xC6u >> o) & 1u) != 0; }   // 1, 2, 6, 7
JPGE_HD inline bool orient_rows_back(int o) { return ((0x6Cu >> o) & 1u) != 0; }  // 2, 3, 5, 6
JPGE_HD inline uint32_t orient_w(uint32_t w, uint32_t h, int o) { return orient_transposed(o) ? h : w; }
JPGE_HD inline uint32_t orient_h(uint32_t w, uint32_t h, int o) { return orient_transposed(o) ? w : h; }
// the source pixel (row sr, column sc) of O(y, x)
JPGE_HD inline void orient_src(int o, uint32_t sw, uint32_t sh, uint32_t y, uint32_t x, uint32_t& sr, uint32_t& sc) {
    const uint32_t r = orient_transposed(o) ? x : y, c = orient_transposed(o) ? y : x;
    sr = orient_rows_back(o) ? sh - 1 - r : r;
    sc = orient_mirrored(o) ? sw - 1 - c : c;
}
// K1's build for an orientation (fdct.hip JPGE_K1_ORIENT): 0 none, 1 rows (3), 2 mirrored (1, 2),
// 3 transposed (4, 5), 4 transposed and mirrored (6, 7); rows_back is a run-time scalar in each
JPGE_HD inline int orient_class(int o) {
    return o == 0 ? 0 : orient_transposed(o) ? (orient_mirrored(o) ? 4 : 3) : (orient_mirrored(o) ? 2 : 1);
}

// Stripe context of a frame (a row stripe of a larger image); the
// defaults describe a whole frame.
struct DcSeed {
    int v[3] = {0, 0, 0};  // DC chain predecessors of the first Y / Cb / Cr block (Image.cpp:638-678)
};

// Restart intervals (DRI / RSTn; opt-in, not in the reference):
// every `mcus` MCUs the DC predictions restart at 0, and the entropy stream is
// 1-filled to a byte boundary and followed by an RSTn marker (n = interval - 1 mod 8).
// mcus = 0: off (the reference's single interval).  mcu0: the frame's first MCU in
// the image's numbering (a stripe starts at an interval boundary).
struct Restart {
    uint32_t mcus = 0;
    uint32_t mcu0 = 0;
};

// The entropy kernels' partition of a frame: segments (restart intervals; one
// segment when restart is off), each cut into tiles of <= kEntropyTile blocks
// (balanced: tile i of a segment of nb blocks in tps tiles is blocks
// [i*nb/tps, (i+1)*nb/tps)), each run of tiles owned by one workgroup.  A
// workgroup's stream never crosses a segment boundary, so every segment starts
// byte-aligned after its predecessor's fill.
struct SegLayout {
    uint32_t nseg = 1;                    // segments
    uint32_t sblk = 0, tps = 0, wps = 0;  // a full segment: blocks, tiles, workgroups
    uint32_t lblk = 0, ltps = 0, lwps = 0;  // the last segment (the frame's tail)
    JPGE_HD uint32_t grid() const { return (nseg - 1) * wps + lwps; }
};

// Workgroup w's tiles: tiles [t0, t0 + nt) of segment seg (blocks [b0, b0 + nb) of
// the frame, in tps tiles).
struct WgTiles {
    uint64_t b0;
    uint32_t nb, tps, t0, nt, seg;
    bool first, last;  // the segment's first / last workgroup
    JPGE_HD uint64_t tile_b0(uint32_t i) const { return b0 + (uint64_t)i * nb / tps; }
    JPGE_HD uint32_t tile_nb(uint32_t i) const {
        return (uint32_t)((uint64_t)(i + 1) * nb / tps - (uint64_t)i * nb / tps);
    }
};
JPGE_HD inline WgTiles wg_tiles(const SegLayout& L, uint32_t w) {
    WgTiles r;
    uint32_t j, wps;
    if (w < (L.nseg - 1) * L.wps) {
        r.seg = w / L.wps; j = w % L.wps; r.tps = L.tps; wps = L.wps; r.nb = L.sblk;
    } else {
        r.seg = L.nseg - 1; j = w - (L.nseg - 1) * L.wps; r.tps = L.ltps; wps = L.lwps; r.nb = L.lblk;
    }
    r.b0 = (uint64_t)r.seg * L.sblk;
    r.t0 = (uint32_t)((uint64_t)j * r.tps / wps);
    r.nt = (uint32_t)((uint64_t)(j + 1) * r.tps / wps) - r.t0;
    r.first = j == 0;
    r.last = j == wps - 1;
    return r;
}

// Symbol records (K2 -> K3): the entropy-coded symbols of a tile in stream order,
// 16 bits each (round 6; 32-bit records had been 38% of a 4K frame's HBM bytes):
//   table << 14 | run << 10 | size << 6 | x     (table 0 Y-DC, 1 Y-AC, 2 C-DC, 3 C-AC;
//   a DC symbol is its category with run 0; EOB run 0 size 0; ZRL run 15 size 0), x = the
//   top min(size, 6) of the symbol's extra bits;
//   continuation: the component's AC table << 14 | n << 10 | the n (1..5) low extra bits
//   the record before it could not hold (size >= 7); run n with size 0 is no JPEG symbol
//   (Coding.hpp:148-196 codes zero runs only as ZRL and EOB), so it never collides with one.
// The code kernel indexes one 64-bit LDS entry per record by record >> 6.  A block codes
// at most 64 symbols (DC + 63 AC, or DC + 62 AC + EOB; a zero run long enough for a ZRL
// removes a coefficient), each with at most one continuation, so a tile's records fit
// kTileRecords halfwords; tile t's sit at recs + t * kTileRecords.  Tiles are the entropy
// partition's (seg_layout), numbered segment by segment.
constexpr int kRecPerBlock = 128;
constexpr int kTileRecords = kEntropyTile * kRecPerBlock;
constexpr uint32_t kRecXBits = 6;  // extra bits a head record holds
// A tile's records are written as kRecSub sub-streams, one per wave of the
// statistics kernel: sub-stream j of a tile of nb blocks holds blocks
// [j*nb/kRecSub, (j+1)*nb/kRecSub) of the tile, at recs + t*kTileRecords +
// j*kSubRecords, its count at tcount[t*kRecSub + j].  The code kernel reads a
// tile's sub-streams in order, so they form the tile's one record stream.
constexpr int kRecSub = 4;
constexpr int kSubRecords = kTileRecords / kRecSub;
static_assert(kTileRecords % kRecSub == 0, "sub-streams divide a tile's records");

struct StatsArgs {
    const int16_t* coef;
    Geometry g;
    HistPtrs hist;
    DcSeed seed;
    Restart rst;
    // first-occurrence key bases in the whole image's texts (Image.cpp:888-906):
    // Y raster index of the stripe's first Y block, Cb raster index of its first
    // Cb block, and the image's Cb block count (every Cr key follows all Cb keys)
    uint64_t key_y0 = 0, key_c0 = 0, key_ncb = 0;
    SegLayout seg;       // the entropy partition: the tiles the records are written in
    uint16_t* recs;      // [tiles][kTileRecords] symbol records
    uint32_t* tcount;    // [tiles][kRecSub] records per sub-stream
    uint32_t wgs = 0;    // workgroup count (0 = 3 per CU; the pipeline passes its own, stats_grid)
    // 1: fixed Huffman tables (jpge_set_huffman): the instance without histograms, which
    // reads none of hist, key_*, done, host_* and seq (in the padding after wgs: the
    // argument block's layout is unchanged)
    uint32_t fixed = 0;
    uint64_t* dbg;
    // Set (single frames): the last workgroup to finish exports the histograms into
    // mapped host memory (export_hist), in place of a hist_export_kernel launch.  `done`
    // counts finished workgroups (zeroed per frame by K1).
    uint32_t* done = nullptr;
    uint32_t* host_cnt = nullptr;
    uint64_t* host_key = nullptr;
    uint64_t* host_seq = nullptr;
    uint64_t seq = 0;
};

// Where each entropy workgroup's bytes go (entropy_scan_kernel -> pack kernel).
struct alignas(16) WgPlace {
    uint64_t P;       // global bit offset of the workgroup's stream
    uint64_t Q;       // 0x00 stuffing bytes before its first owned byte
    uint32_t ftotal;  // 0xFF bytes it owns (its stuffing count)
    uint32_t split;   // value of its first byte when shared with the predecessor (P & 7 != 0)
    uint32_t fill;    // its 1-filled final byte (the last workgroup of a restart interval / the image)
    uint32_t seg;     // restart mode: its segment; the RST markers before its bytes = seg + seg_markers0
};

// A stripe's entropy summary (entropy_scan_kernel, summary mode): enough for the
// stripes to place their bytes after one all-gather.
struct StripeSummary {
    uint64_t bits;   // length of the stripe's stream (restart intervals: its bytes, markers and fills included)
    uint32_t ff[8];  // ff[a]: 0xFF bytes wholly inside the stripe when it starts at bit a (mod 8),
                     // the byte shared with the previous stripe and the final fill byte excluded
    uint32_t head;   // its first 8 bits (MSB-first byte)
    uint32_t tail;   // its last 8 bits
    uint32_t restart;  // 1: restart-interval stripe (byte-aligned; bits = byte length)
    uint32_t pad;
};

constexpr uint32_t kStripeFirst = 1u;  // holds the image's first bit: writes the headers
constexpr uint32_t kStripeLast = 2u;   // holds the last bit: 1-fill and EOI
constexpr uint32_t kExtPlace = 4u;     // pack kernel reads WgPlace (entropy_scan_kernel) instead of scanning

struct EntropyArgs {
    const int16_t* coef;
    const uint16_t* recs;    // the statistics kernel's symbol records (kTileRecords per tile)
    const uint32_t* tcount;  // records per tile
    Geometry g;
    const uint32_t* tables;  // [4][256] (len << 16) | code, followed by the header bytes
    uint8_t* out;            // whole .jpg; the kernel writes the header to [0, hdr_len)
    uint64_t hdr_len;
    uint64_t out_cap;
    uint8_t* ubuf;           // per-workgroup unstuffed regions (entropy_ubuf_bytes)
    uint8_t* rec;            // [entropy_grid][kEntropyRecordBytes] code -> pack kernel records
    uint32_t* done = nullptr;  // (zeroed per frame) code workgroups finished: the last one places all
    // (zeroed per frame) pack workgroups finished, then the last workgroup's end offset
    // (u64 at [2]) and no-space flag ([4]): the last to finish hands the result over
    uint32_t* pack_done = nullptr;
    uint64_t* host_result;   // mapped pinned host memory: [0] .jpg bytes, [1] no-space (4),
                             // [2] reserved (0), [3] = seq, written last, once every
                             // workgroup's output stores have completed (pack_done)
    uint64_t seq;            // the frame's sequence number
    // carried duty of the code kernel: export another frame's histograms to mapped
    // host memory (workgroup 0; exp_cnt == nullptr: none)
    HistPtrs exp_hist;
    uint32_t* exp_cnt;
    uint64_t* exp_key;
    uint64_t* exp_seq;
    uint64_t exp_seqv;
    uint32_t wgs;            // workgroup count override (0 = automatic; tests)
    DcSeed seed;             // DC chain predecessors (stripes)
    // placement (stripes / large grids): stream starts at global bit p_ext with q_ext
    // stuffing bytes before it; head_split = its first byte when p_ext & 7 != 0
    uint64_t p_ext = 0, q_ext = 0;
    uint32_t head_split = 0;
    uint32_t flags = kStripeFirst | kStripeLast;
    WgPlace* place = nullptr;          // [seg.grid()] (kExtPlace)
    StripeSummary* summary = nullptr;  // summary mode output
    Restart rst;                       // restart intervals (rst.mcus = 0: none)
    SegLayout seg;                     // workgroup partition (host: seg_layout)
    uint32_t seg_markers0 = 0;         // RST markers in this output before the frame's first segment (stripes)
    uint32_t seg_index0 = 0;           // the image's interval index of the frame's first segment (stripes)
    uint64_t out_base = 0;             // restart stripes: bytes of earlier stripes after the header
    uint64_t* dbg;
};

// tiles of a partition, and tile gt's blocks (the global tile number of segment s's
// tile i is s * tps + i)
JPGE_HD inline uint32_t seg_tiles(const SegLayout& L) { return (L.nseg - 1) * L.tps + L.ltps; }
JPGE_HD inline void seg_tile(const SegLayout& L, uint32_t gt, uint64_t& b0, uint32_t& nb) {
    uint32_t seg, i, tps, nbs;
    if (gt < (L.nseg - 1) * L.tps) {
        seg = gt / L.tps; i = gt % L.tps; tps = L.tps; nbs = L.sblk;
    } else {
        seg = L.nseg - 1; i = gt - seg * L.tps; tps = L.ltps; nbs = L.lblk;
    }
    b0 = (uint64_t)seg * L.sblk + (uint64_t)i * nbs / tps;
    nb = (uint32_t)((uint64_t)(i + 1) * nbs / tps - (uint64_t)i * nbs / tps);
}
// record sub-stream s (tile s / kRecSub, part s % kRecSub) and its blocks
JPGE_HD inline void sub_tile(const SegLayout& L, uint32_t s, uint64_t& b0, uint32_t& nb) {
    uint64_t tb;
    uint32_t tn;
    seg_tile(L, s / kRecSub, tb, tn);
    const uint32_t j = s % kRecSub;
    b0 = tb + j * tn / kRecSub;
    nb = (j + 1) * tn / kRecSub - j * tn / kRecSub;
}

inline uint32_t entropy_tiles(const Geometry& g) {
    return (g.nblocks() + kEntropyTile - 1) / kEntropyTile;
}
// bytes of one entropy workgroup's private region: its bit stream (workgroup-
// local offsets, worst case) plus slack, a whole number of 128-byte lines
constexpr uint64_t kEntropyRegionBytes = (uint64_t)kEntropyMaxTilesPerWg * kEntropyTile * kStageBytesPerBlock + 128;

// Kernel timing (sampled frames only): when given, the launch goes through
// hipExtLaunchKernel with these events, which the runtime binds to the kernel's own
// dispatch (its start and end timestamps, the ones rocprofv3 reports), so their
// elapsed time is the kernel's execution without launch gaps or marker packets.
struct KTimer {
    hipEvent_t start = nullptr, stop = nullptr;
};

// Frames launched together (frame sets): member f of a set owns workgroups
// [wg0[f], wg0[f + 1]) of one launch and runs exactly as if launched alone with its
// own arguments and wg0[f + 1] - wg0[f] workgroups.  The members share a geometry
// (one kernel shape).  Small frames go in sets: a 1080p frame's kernels alone leave
// most of the GPU idle while their fixed latencies (launch, first loads, last
// workgroup) pass, so 4 frames per launch do 4 frames' work in about one frame's
// latency.  Every kernel takes a set; a lone frame is a set of one.
constexpr int kMaxSet = 4;
// (N: the kernel instance's capacity; lone frames launch the N = 1 instance, whose
// kernel arguments are a quarter the size: a launch copies them whole)
template <typename A, int N = kMaxSet>
struct FrameSet {
    A a[N];
    uint32_t wg0[N + 1];
    uint32_t n;
};
// the member that owns workgroup b (uniform: scalar code; a fixed trip count, so the
// N = 1 instance reduces to member 0)
// (K2 keeps the rolled form: with it the compiler gives the statistics kernel 62 VGPRs
// instead of 69-70, and the kernel runs 4% faster)
JPGE_HD inline uint32_t set_member_rolled(const uint32_t* wg0, uint32_t n, uint32_t b) {
    uint32_t f = 0;
    for (uint32_t i = 1; i < n; ++i) f += b >= wg0[i] ? 1u : 0u;
    return f;
}
template <int N>
JPGE_HD inline uint32_t set_member(const uint32_t* wg0, uint32_t n, uint32_t b) {
    uint32_t f = 0;
    for (int i = 1; i < N; ++i) f += (i < (int)n && b >= wg0[i]) ? 1u : 0u;
    return f;
}
template <int N = kMaxSet, typename A>
inline FrameSet<A, N> frame_set(const A* a, int n, uint32_t grid_each) {
    FrameSet<A, N> s{};
    s.n = (uint32_t)n;
    for (int f = 0; f < n; ++f) {
        s.a[f] = a[f];
        s.wg0[f] = (uint32_t)f * grid_each;
    }
    s.wg0[n] = (uint32_t)n * grid_each;
    return s;
}

// (ds: FdctArgs::ds, a downscaled frame runs the 4-wave workgroups at every size; orient:
// FdctArgs::orient, an oriented frame likewise)
uint32_t fdct_grid(const Geometry& g, bool solo, uint32_t override_wgs = 0, uint32_t ds = 1, uint32_t orient = 0);
// statistics workgroups: wgs (0: 3 per CU), within the tile-table bound and the tile count
uint32_t stats_grid(const SegLayout& L, uint32_t wgs = 0);
// entropy partition of a frame: restart_mcus = 0 -> one segment over 128-block tiles
// (2..kEntropyMaxTilesPerWg per workgroup, about 384 workgroups or wgs_override)
SegLayout seg_layout(const Geometry& g, uint32_t restart_mcus, uint32_t wgs_override);
inline uint32_t entropy_grid(const Geometry& g, uint32_t wgs_override) { return seg_layout(g, 0, wgs_override).grid(); }

inline uint64_t entropy_ubuf_bytes(const SegLayout& L) { return (uint64_t)L.grid() * kEntropyRegionBytes; }

// Segment concatenation (concat.hip): segment k's len[k] bytes from src[k] to dst + off[k];
// workgroups [chunk0[k], chunk0[k+1]) copy segment k (concat_chunks(len, dst + off) each)
constexpr uint32_t kConcatMax = 96;  // segments per launch (the arguments stay under 4 KB)
struct ConcatArgs {
    uint8_t* dst;
    uint32_t n;
    uint32_t chunk0[kConcatMax + 1];
    const uint8_t* src[kConcatMax];
    uint64_t off[kConcatMax];
    uint64_t len[kConcatMax];
};
uint32_t concat_chunks(uint64_t len, uintptr_t dst);
hipError_t launch_concat(const ConcatArgs& a, uint32_t nchunks, hipStream_t s);

hipError_t launch_fdct(const FdctArgs& a, hipStream_t s, const KTimer* t = nullptr);
hipError_t launch_stats(const StatsArgs& a, hipStream_t s, const KTimer* t = nullptr);
// frame sets (kMaxSet frames of one geometry, one launch per kernel): the members'
// arguments as launch_fdct / launch_stats / launch_entropy take them
hipError_t launch_fdct_set(const FdctArgs* a, int n, hipStream_t s, const KTimer* t = nullptr);
hipError_t launch_stats_set(const StatsArgs* a, int n, hipStream_t s, const KTimer* t = nullptr);
// (every member placed by its code kernel's last workgroup: a.done set, no restart)
hipError_t launch_entropy_set(const EntropyArgs* a, int n, hipStream_t s, const KTimer* code = nullptr,
                              const KTimer* pack = nullptr);
// [4][256] summed counts and keys into (mapped) host memory, then *host_seq = seq
hipError_t launch_hist_export(const HistPtrs& h, uint32_t* host_cnt, uint64_t* host_key, uint64_t* host_seq,
                              uint64_t seq, hipStream_t s);
// code + pack kernels (with the placement scan between them when kExtPlace)
hipError_t launch_entropy(const EntropyArgs& a, hipStream_t s, const KTimer* code = nullptr,
                          const KTimer* pack = nullptr);
// its two halves: the code kernel does not read hdr_len, so it can be queued before the
// header is known (encoder.cpp, encode()'s gate); the pack kernel (and placement)
hipError_t launch_entropy_code(const EntropyArgs& a, hipStream_t s, const KTimer* code = nullptr);
// encode()'s gate: wait (one workgroup, at most timeout_ticks of the 100 MHz realtime
// counter, then *fail = 1 and no copy) until *gate == value (mapped host memory), then copy
// n16 16-byte units src -> dst (src: device view of mapped host memory)
hipError_t launch_gate_copy(const uint32_t* gate, uint32_t value, const void* src, void* dst, uint32_t n16,
                            uint64_t* fail, uint64_t timeout_ticks, hipStream_t s);
hipError_t launch_entropy_pack(const EntropyArgs& a, hipStream_t s, const KTimer* pack = nullptr);
// stripes: code kernel + summary scan; then placement scan + pack kernel
hipError_t launch_entropy_code_summary(const EntropyArgs& a, hipStream_t s);
hipError_t launch_entropy_place_pack(const EntropyArgs& a, hipStream_t s);
// grids above this many workgroups place by a separate scan (each pack workgroup
// scanning every record would read G^2 records)
constexpr uint32_t kInlineScanMaxWgs = 1024;
// Grids the last code workgroup places (entropy_code_kernel, EntropyArgs::done).
// Hardware assumption (gfx950), not the HIP memory model's letter: each workgroup
// publishes its 48-byte record with agent-scope relaxed atomic stores, which gfx950
// issues write-through (sc1) to the agent's coherence point, waits for their
// completion (s_waitcnt vmcnt(0)), and only then counts itself with a device atomic
// performed at that point; the workgroup completing the count takes an agent-scope
// acquire fence (buffer_inv sc1) before reading every record.  The formal alternative,
// a release fence per workgroup, writes back the whole L2 (measured 26% slower).
// Covered by the GPU tests that run multi-lane batches and compare every frame with
// the oracle (test_gpu_parity.py: placement in code at 1..G workgroups, batches).
constexpr uint32_t kPlaceInCodeMaxWgs = 4096;

}  // namespace jpge
