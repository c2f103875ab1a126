/*
 * jpge — MI355X-native JPEG baseline encoder, C ABI (the drop-in boundary).
 *
 * The reference (Nuos/jpgEnc) has no FFI: its encode path is the C++ API of the
 * static library jpgEncLib (src/CMakeLists.txt:6-11) consumed by src/main.cpp.
 * Each entry point below replaces one piece of that API; the C++ facade in
 * jpgenc_amd/csrc/jpge_image.hpp re-exposes them under the reference's names.
 *
 * Conventions: every function returns a jpge_status (0 = ok); no exceptions or
 * C++ types cross this boundary; all buffers are owned by the caller; a context
 * (one HIP device + its streams and workspace) may be shared between threads: its
 * calls run one at a time (each call holds the context).  Output bytes are
 * bit-identical to the reference encoder.
 */
#ifndef JPGE_H_
#define JPGE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    JPGE_OK = 0,
    JPGE_E_ARG = 1,       /* invalid argument */
    JPGE_E_NOSPACE = 2,   /* output buffer too small; *len receives the size needed */
    JPGE_E_HIP = 3,       /* HIP runtime failure */
    JPGE_E_NODEV = 4,     /* no GPU / bad device index */
    JPGE_E_FORMAT = 5,    /* not a P3/P6 PPM (reference: std::runtime_error, Image.cpp:449-450) */
    JPGE_E_IO = 6,        /* cannot open/read/write a file (Image.cpp:427-428) */
    JPGE_E_TRUNC = 7,     /* PPM sample data shorter than width*height*3 */
    JPGE_E_RANGE = 8,     /* maxval outside 1..255 (Image.cpp:462) or sample > 255 */
    JPGE_E_TIMEOUT = 9,   /* device-side scan protocol did not complete */
    JPGE_E_RCCL = 10,     /* RCCL failure (multi-GPU paths) */
    JPGE_E_INTERNAL = 11
} jpge_status;

#define JPGE_DEVICE_INPUT 1u  /* rgb points to device memory */
#define JPGE_DEVICE_OUTPUT 2u /* out points to device memory */

typedef struct jpge_ctx jpge_ctx;

/* One frame of a batch (jpge_encode_batch). */
typedef struct {
    const uint8_t* rgb; /* interleaved RGB8 (host, or device with JPGE_DEVICE_INPUT) */
    uint32_t width, height;
    size_t stride;      /* bytes per row, 0 = width*3; stride * height (of one plane) must stay below
                           0xFFFFFF00, the transform kernel's 32-bit offset range, else JPGE_E_ARG */
    int maxval;         /* PPM maxval, 1..255; samples are scaled by 255./maxval (Image.cpp:465) */
    uint8_t* out;       /* .jpg destination */
    size_t cap;         /* capacity of out */
    size_t len;         /* [out] bytes written */
    int status;         /* [out] jpge_status of this frame */
} jpge_frame;

/* Per-kernel device times of the last timed frame (ms; see jpge_set_timing for
 * sampling).  Each kernel of a timed frame is launched with its own pair of HIP
 * events bound to its dispatch (hipExtLaunchKernel), so a kernel's figure is its
 * execution time as rocprofv3 reports it, without launch gaps. */
typedef struct {
    float fdct;     /* K1: colour + 4:2:0 + FDCT + quantise */
    float dc_stats; /* K2: DC chain + RLE/category symbol histograms + first-occurrence keys */
    float entropy;  /* K3: code kernel start .. pack kernel end (Huffman emission, MCU interleave, fill, stuffing) */
    float total;    /* K1 start .. K3 end of that frame (includes the queued work of other frames) */
    double fdct_sum, dc_stats_sum, entropy_sum; /* accumulated since jpge_reset_timing (ms) */
    uint64_t frames;                            /* frames accumulated */
    uint64_t symbols; /* Huffman-coded symbols of those frames (= K2's 4-byte symbol records); counted from the
                         histograms, so frames of a fixed Huffman mode (jpge_set_huffman) do not advance it */
    double code_sum, pack_sum; /* K3's entropy_code_kernel and entropy_pack_kernel alone (ms, accumulated) */
    uint64_t launches;         /* timed launches of each kernel (batches of small frames launch frame sets:
                                  one launch per kernel for up to 4 frames; the sums are per launch) */
    uint64_t gate_timeouts;    /* single-frame calls whose table gate timed out on the device and were
                                  re-coded ungated (jpge_encode_rgb8; not reset by jpge_reset_timing) */
} jpge_timing;

const char* jpge_strerror(int status);
int jpge_version(void);
int jpge_device_count(int* n);

/* Context lifetime (replaces nothing in the reference: its encoder is stateless). */
int jpge_open(int device, jpge_ctx** ctx);
/* jpge_open with an explicit lane count (0 = JPGE_LANES or the default 4; at most 8;
 * 1 = a single pipeline, e.g. to time kernels without other frames beside them). */
int jpge_open_ex(int device, int lanes, jpge_ctx** ctx);
/* Contexts and groups still open when the process exits are released by the library
 * itself (an std::atexit handler registered at the first jpge_open): their threads,
 * streams and memory are freed, but the handle stays valid, so a jpge_close or
 * jpge_group_close the caller makes later (e.g. from its own exit handler) is a no-op,
 * and any other call on it returns JPGE_E_ARG. */
int jpge_close(jpge_ctx* ctx);
/* Kernel timing with HIP events on the encoder's stream: every = 0 off, N >= 1
 * times the kernels of every N-th frame (1 = all; events cost GPU time). */
int jpge_set_timing(jpge_ctx* ctx, int every);
int jpge_get_timing(jpge_ctx* ctx, jpge_timing* t);
int jpge_reset_timing(jpge_ctx* ctx);
/* Pipelines ("lanes") the context runs a batch on: each lane is a HIP stream with
 * its own frame slots and host thread; a batch's frames are dealt round-robin to
 * them (env JPGE_LANES at jpge_open, default 4). */
int jpge_get_lanes(jpge_ctx* ctx, int* lanes);

/* Restart intervals for the context's following encodes (jpge_encode_rgb8, _batch,
 * _file): every `mcus` MCUs the DC predictions restart and the entropy stream is
 * 1-filled and followed by an RSTn marker, announced by a DRI segment before SOS
 * (ITU T.81 B.2.4.4, F.1.2.3).  0 (the default) = none: the reference's stream,
 * bit-identical to it.  Replaces nothing in the reference (writeJPEG never emits
 * DRI/RSTn, Image.cpp:931-972); its decoded pixels equal the mcus = 0 output's.
 * 1..65535, else JPGE_E_ARG; the stripe phases (jpge_stripe_*) need mcus = 0. */
int jpge_set_restart_interval(jpge_ctx* ctx, uint32_t mcus);

/* Subsampling modes: the SubsamplingMode enum of Image.hpp:44-52, as passed to
 * Image::applySubsampling (Image.cpp:237-319). */
#define JPGE_S420_M 420  /* mean of 2x2 (writeJPEG's mode; the default)        MCU 16x16, Y 2x2 */
#define JPGE_S444 444    /* no subsampling                                    MCU  8x8,  Y 1x1 */
#define JPGE_S422 422    /* every second pixel of a row                       MCU 16x8,  Y 2x1 */
#define JPGE_S411 411    /* every fourth pixel of a row                       MCU 32x8,  Y 4x1 */
#define JPGE_S420 4200   /* every second pixel of every second row            MCU 16x16, Y 2x2 */
#define JPGE_S420_LM 4201 /* mean of the two rows' left pixels                MCU 16x16, Y 2x2 */

/* Chroma subsampling for the context's following encodes.  JPGE_S420_M (the
 * default) is applySubsampling(S420_m) as writeJPEG hard-codes it (Image.cpp:842),
 * bit-identical to the reference.  The other modes follow Image::subsample
 * (Image.cpp:198-235) for the masks of applySubsampling; writeJPEG cannot emit
 * them, so the oracle's composition of the pinned stages defines their bytes: the
 * frame edge-replicated to whole MCUs, MCU = the Y blocks row by row + Cb + Cr,
 * SOF0 declaring Y as H x V.  Unknown modes: JPGE_E_ARG.  jpge_fdct_quant then
 * returns the mode's planes; the stripe phases (jpge_stripe_*) need JPGE_S420_M. */
int jpge_set_subsampling(jpge_ctx* ctx, int mode);

/* Input layouts of 8-bit frames.  The .jpg of a frame in any of them is, byte for
 * byte, the .jpg of the same pixels rearranged to interleaved RGB: only the
 * transform kernel's loads differ, no repack pass runs. */
#define JPGE_FMT_RGB8 0        /* interleaved R,G,B, 3 bytes per pixel (the default) */
#define JPGE_FMT_BGR8 1        /* interleaved B,G,R */
#define JPGE_FMT_RGBA8 2       /* interleaved R,G,B,A, 4 bytes per pixel; alpha ignored */
#define JPGE_FMT_BGRA8 3       /* interleaved B,G,R,A; alpha ignored */
#define JPGE_FMT_RGB8_PLANAR 4 /* planes R, G, B of `height` rows of `stride` bytes, 1 byte per
                                  pixel, at rgb, rgb + plane_stride, rgb + 2*plane_stride */
/* Frames of full-range (JFIF) 8-bit Y, Cb, Cr samples, a video decoder's output: no
 * colour conversion runs, a sample v enters the transform as the value v - 128 (the
 * reference Image's plane after convertToColorSpace(YCbCr)).  `rgb` points at the Y
 * plane and `stride` is its row pitch; maxval must be 255 (else JPGE_E_ARG, in a batch
 * the frame's status).  With cw = ceil(width / 2), ch = ceil(height / 2):
 *   NV12: the Cb,Cr plane at rgb + plane_stride (0 = stride * height), ch rows of pitch
 *     `stride`, Cb at even bytes and Cr at odd bytes; stride 0 = width rounded up to even.
 *   I420: the Cb plane at rgb + plane_stride (0 = stride * height), ch rows of pitch
 *     cs = (stride + 1) / 2; the Cr plane at Cb + cs * ch; stride 0 = width.
 *   YUV444_PLANAR: addressed exactly as JPGE_FMT_RGB8_PLANAR; the context's subsampling
 *     mode (any of the six) filters Cb and Cr as it does after a colour conversion.
 * NV12 and I420 chroma is subsampled already: the planes are taken as the output of the
 * 4:2:0 averaging (Y edge-replicated to whole 16x16 MCUs, each chroma plane
 * edge-replicated, in the chroma domain, to half that), and the context must be in
 * JPGE_S420_M (the default): in another mode the encode calls return JPGE_E_ARG.  The
 * fast path needs every plane's base and pitch 16-byte aligned (I420: a stride that is
 * a multiple of 32). */
#define JPGE_FMT_NV12 16
#define JPGE_FMT_I420 17
#define JPGE_FMT_YUV444_PLANAR 18
/* 4:2:2 frames of the same samples (capture cards and webcams, SDI paths, 4:2:2 decoders):
 * one Cb and one Cr sample per horizontal pixel pair of every row.  maxval must be 255.
 * With cw = ceil(width / 2); `rgb` points at the frame's first byte (NV16, I422: the Y plane):
 *   YUYV: one plane, `height` rows of cw 4-byte groups Y0 Cb Y1 Cr: pixel x has Y at byte
 *     2x, Cb at 4(x>>1)+1, Cr at 4(x>>1)+3 of its row; stride 0 = 4 * cw; plane_stride 0.
 *   UYVY: the same with groups Cb Y0 Cr Y1: Y at 2x+1, Cb at 4(x>>1), Cr at 4(x>>1)+2.
 *   NV16: the Y plane, then at rgb + plane_stride (0 = stride * height) a Cb,Cr plane of
 *     `height` rows of pitch `stride`, Cb at even bytes; stride 0 = width rounded up to even.
 *   I422: the Y plane, then at rgb + plane_stride (0 = stride * height) the Cb plane, `height`
 *     rows of pitch cs = (stride + 1) / 2; the Cr plane at Cb + cs * height; stride 0 = width.
 * Such a frame is, byte for byte of the .jpg, the JPGE_FMT_YUV444_PLANAR frame whose chroma
 * planes hold c[y][x >> 1] at pixel (y, x): in every subsampling mode (none is refused;
 * JPGE_S422 is the native one: it keeps each cell's sample and runs no filter), with every
 * jpge_set_yuv_transform setting (per pixel, then the mode's filter), Huffman mode and
 * restart interval.  So the chroma is edge-replicated in the chroma domain.  With an odd
 * width the last group's second Y byte is storage only: its value never reaches the output.
 * The fast path needs base, stride and plane_stride 16-byte aligned (I422: a stride that is
 * a multiple of 32); anything else works, slower. */
#define JPGE_FMT_YUYV 20
#define JPGE_FMT_UYVY 21
#define JPGE_FMT_NV16 22
#define JPGE_FMT_I422 23
/* 10-bit 4:2:0 frames (HEVC Main10, AV1, VP9 profile 2 decoders): little-endian 16-bit words,
 * NV12's and I420's planes.  `rgb` points at the Y plane and `stride` is its pitch in BYTES.
 * With cw = ceil(width / 2), ch = ceil(height / 2):
 *   P010: a sample is s = word >> 6; the low six bits are never read (P012 and P016 data is
 *     taken at its top 10 bits).  The Cb,Cr plane at rgb + plane_stride (0 = stride * height):
 *     ch rows of pitch `stride`, Cb in the even words and Cr in the odd words; stride 0 =
 *     2 * (width rounded up to even).
 *   I010 (yuv420p10le): a sample is s = word & 0x3FF; the high six bits are never read.  The
 *     Cb plane at rgb + plane_stride (0 = stride * height): ch rows of pitch
 *     cs = 2 * ceil(stride / 4); the Cr plane at Cb + cs * ch; stride 0 = 2 * width.
 * The base, `stride` and `plane_stride` must be even and the stride not below the least for
 * the width (else JPGE_E_ARG).  maxval must be 255 and the context in JPGE_S420_M, as for
 * NV12; jpge_stripe_transform and jpge_group_encode_striped refuse the layouts.  The fast
 * path needs base, stride and plane_stride 16-byte aligned (I010: a stride that is a multiple
 * of 32); anything else that is even works, slower.
 * Conversion: no sample is rounded to 8 bits.  A pixel's s_y, s_cb, s_cr (the chroma of its
 * 2x2 cell, edge-replicated in the chroma domain as for NV12) enter as the exact values
 *   yc = 0.25 * s_y - y_off,  u = 0.25 * s_cb - 128,  v = 0.25 * s_cr - 128
 * and the three lines of jpge_set_yuv_transform (each product and sum rounded on its own,
 * the clamps included) are applied ALWAYS: under JPGE_YUV_FULL_601 with the identity
 * coefficients, which gives Y' = min(0.25 * s_y, 255) - 128 and Cb' = min(0.25 * s_cb - 128, 127).
 * Studio swing in 10 bits (64..940, 64..960) is 4 times the 8-bit one, so the presets mean
 * what they mean in 8 bits.  Full-range 10-bit data by ITU-T H.273 has white at 1023, which the
 * identity clamps to 255; a caller who wants 1023 at 255 exactly passes JPGE_YUV_CUSTOM with
 * m[0] = 1020.0 / 1023.
 * A frame whose samples are all multiples of 4 gives, byte for byte, the .jpg of the NV12 / I420
 * frame of s / 4: under every transform setting, Huffman mode and restart interval. */
#define JPGE_FMT_P010 32
#define JPGE_FMT_I010 33
/* 10-bit 4:2:2 frames (SDI capture; ProRes, DNxHR, XAVC-Intra and HEVC RExt 4:2:2 decoders):
 * little-endian 16-bit words, one Cb and one Cr sample per horizontal pixel pair of every row.
 * `rgb` points at the frame's first byte and `stride` is the Y (or only) plane's pitch in BYTES.
 * With cw = ceil(width / 2):
 *   Y210: one plane, `height` rows of cw 8-byte groups Y0 Cb Y1 Cr; a sample is s = word >> 6,
 *     the low six bits are never read (Y212 and Y216 data is taken at its top 10 bits); stride
 *     0 = 8 * cw; plane_stride must be 0.  With an odd width the last group's Y1 word is storage
 *     only: its value never reaches the output.
 *   P210: the Y plane, then at rgb + plane_stride (0 = stride * height) a Cb,Cr plane of
 *     `height` rows of pitch `stride`, Cb in the even words and Cr in the odd words; a sample is
 *     s = word >> 6 (P212 and P216 likewise); stride 0 = 2 * (width rounded up to even).
 *   I210 (yuv422p10le): a sample is s = word & 0x3FF; the high six bits are never read.  The
 *     Cb plane at rgb + plane_stride (0 = stride * height): `height` rows of pitch
 *     cs = 2 * ceil(stride / 4); the Cr plane at Cb + cs * height; stride 0 = 2 * width.
 * The base, `stride` and `plane_stride` must be even, the stride not below the least for the
 * width, and maxval 255 (else JPGE_E_ARG, or the frame's status in a batch).
 * A frame in one of these layouts is the Y, Cb, Cr frame in which pixel (y, x) has the samples
 * s_y[y][x], s_cb[y][x >> 1], s_cr[y][x >> 1], each entering as the exact value s / 4:
 *   yc = 0.25 * s_y - y_off,  u = 0.25 * s_cb - 128,  v = 0.25 * s_cr - 128
 * with the three lines of jpge_set_yuv_transform applied ALWAYS and per pixel (each product and
 * sum rounded on its own, the clamps included; under JPGE_YUV_FULL_601 with the identity
 * coefficients, as for P010), and after that the context's subsampling mode.  All six modes are
 * accepted; JPGE_S422 is the native one: it keeps each cell's sample and runs no filter
 * arithmetic.  This holds under every Huffman mode and restart interval, alone, in batches and
 * frame sets, and through jpge_group_encode_batch.  The chroma is edge-replicated in the chroma
 * domain: the clamped pixel's cell is the clamped cell.  Two consequences:
 *   - a frame whose samples are all multiples of 4 gives, byte for byte, the .jpg of the 8-bit
 *     YUYV / NV16 / I422 frame of s / 4, in every mode and setting;
 *   - the three layouts of the same samples give the same bytes.
 * jpge_stripe_transform and jpge_group_encode_striped refuse the three layouts, and so does an
 * encode under jpge_set_downscale with a factor above 1 (JPGE_E_ARG, before anything is
 * queued).  The fast path needs base, stride and plane_stride 16-byte aligned (I210: a stride
 * that is a multiple of 32); anything else that is even works, slower. */
#define JPGE_FMT_Y210 40
#define JPGE_FMT_P210 41
#define JPGE_FMT_I210 42
/* v210: the 10-bit 4:2:2 frames that SDI capture hardware writes and that QuickTime / AVI
 * "uncompressed 10-bit" files and ffmpeg's v210 codec hold.  One plane; `rgb` points at the
 * frame's first byte and `stride` is the row pitch in BYTES.  A row is a sequence of 32-bit
 * little-endian words, each holding three 10-bit samples at bits 0-9, 10-19 and 20-29; bits
 * 30-31 are never read.  The samples of a row, in word-and-field order, form the stream
 *   Cb0 Y0 Cr0 Y1 Cb1 Y2 Cr1 Y3 ...
 * so that pixel x has its Y at stream index 2x + 1, cell c = x >> 1 its Cb at index 4c and its Cr
 * at 4c + 2, and stream index k is field k % 3 of word k / 3.  Six pixels make a group of four
 * words (16 bytes), and a row occupies jpge_v210_row_bytes(width) = 16 * ceil(width / 6) bytes:
 * stride 0 means that; the conventional pitch 128 * ceil(width / 48) is one valid stride, not a
 * requirement.  Samples of the last group beyond pixel width - 1 and its cell are storage only and
 * never reach the output (with an odd width the last cell's Cb and Cr are real).
 * The frame means exactly what the Y210, P210 or I210 frame of the same samples s_y, s_cb, s_cr
 * means (above): yc = 0.25 s_y - y_off, u = 0.25 s_cb - 128, v = 0.25 s_cr - 128, the three lines
 * of jpge_set_yuv_transform per pixel, always (JPGE_YUV_FULL_601: the identity, for its clamps),
 * then the context's subsampling mode, the chroma edge-replicated in the chroma domain.  So
 *   - a v210 frame gives, byte for byte, the .jpg of the Y210, P210 or I210 frame of its samples;
 *   - a v210 frame whose samples are all multiples of 4 gives the .jpg of the 8-bit YUYV / NV16 /
 *     I422 frame of s / 4.
 * Accepted: all six subsampling modes (JPGE_S422 is the native one), every Huffman mode and restart
 * interval, single frames, batches and frame sets, jpge_group_encode_batch, device and host
 * input.  Refused with JPGE_E_ARG (or the frame's status in a batch) before anything is queued,
 * the context staying usable: a base or stride that is not a multiple of 4, a stride below
 * jpge_v210_row_bytes(width), maxval != 255, a non-zero plane_stride, a downscale factor above 1,
 * jpge_stripe_transform and jpge_group_encode_striped.  The fast path needs base and stride
 * 16-byte aligned; any other multiples of 4 work, slower.
 * jpge_input_format_info reports bytes_per_pixel 0 for this layout: a row is not a whole number
 * of bytes per pixel; use jpge_v210_row_bytes. */
#define JPGE_FMT_V210 48
/* One plane of 8-bit luminance: `height` rows of `stride` bytes (0 = width), one byte per
 * pixel; a sample v enters the transform as the value v - 128, as a Y sample above.
 * maxval must be 255 and plane_stride 0 (else JPGE_E_ARG).  The output is a baseline JPEG
 * with ONE component in a non-interleaved scan (ITU T.81 A.2.2): SOI APP0 DQT(qy) SOF0
 * (1 component, 1x1, table 0) DHT(DC 0) DHT(AC 0) [DRI] SOS <entropy> EOI.  The MCU is
 * one 8x8 block: the plane is edge-replicated to whole blocks, blocks and the DC chain run
 * in block raster order, and a restart interval counts blocks.  qc is not read (it may be
 * NULL in the encode and stage entries) and the context's subsampling mode does not enter:
 * there is no chroma.  jpge_fdct_quant fills coef_y only (coef_cb, coef_cr may be NULL);
 * jpge_symbol_stats returns zeros and ~0 keys for tables 2 and 3.  The fast path needs the
 * pointer and the stride 16-byte aligned. */
#define JPGE_FMT_GRAY8 8

/* 8-bit Bayer mosaics (an addition): what machine-vision and embedded sensors deliver (GenICam
 * BayerRG8 / BayerGR8 / BayerGB8 / BayerBG8, V4L2 SRGGB8 / SGRBG8 / SGBRG8 / SBGGR8), white balance
 * and gamma already applied in the camera.  One plane of `height` rows of `width` bytes, pitch
 * `stride` (0 = width), plane_stride 0.  The name gives the colours of the 2x2 cell at rows 0-1,
 * columns 0-1, read row by row (RGGB: row 0 is R,G and row 1 is G,B); the site at (y, x) has colour
 * cell[y & 1][x & 1].
 *
 * The frame codes as the RGB8 frame D = jpge_demosaic_frame(frame), a bilinear demosaic in integers
 * built inside the transform kernel as it stages a tile (no pass writes D):
 *   V(y, x) is the raw byte at coordinates reflected without repeating the edge, i < 0 -> -i and
 *   i >= n -> 2 (n - 1) - i, which keeps a site's colour parity.
 *   At an R or B site:  own colour = V(y, x)
 *                       G = (V(y-1,x) + V(y+1,x) + V(y,x-1) + V(y,x+1) + 2) >> 2
 *                       the opposite colour = (V(y-1,x-1) + V(y-1,x+1) + V(y+1,x-1) + V(y+1,x+1) + 2) >> 2
 *   At a G site:        G = V(y, x)
 *                       the colour of its row's other sites = (V(y,x-1) + V(y,x+1) + 1) >> 1
 *                       the colour of its column's other sites = (V(y-1,x) + V(y+1,x) + 1) >> 1
 * The .jpg is, byte for byte, that of D coded as JPGE_FMT_RGB8 on the same context, under every
 * other setting (quality tables, the six subsampling modes, restart interval, Huffman mode, frame
 * sets and lanes, jpge_encode_batch, jpge_group_encode_batch); jpge_fdct_quant and
 * jpge_symbol_stats return D's coefficients and histograms.  Padding to whole MCUs replicates D's
 * right and bottom edge pixels: a coordinate is clamped in D first, and the clamped pixel is then
 * demosaiced with its reflected neighbours.
 * JPGE_E_ARG, before anything is queued (a batch: the frame's status): width or height below 2,
 * maxval other than 255, a plane_stride other than 0, a downscale factor above 1, an orientation
 * other than JPGE_ORIENT_NONE, jpge_stripe_transform and jpge_group_encode_striped.
 * jpge_encode_planes and the plane stages ignore the layout.  The fast path needs the pointer and
 * the stride 16-byte aligned.  Not built: other demosaic filters, deeper or packed raw and a colour
 * matrix; white balance gains and a gamma curve are jpge_set_channel_lut's
 * tables, applied to the demosaiced pixel. */
#define JPGE_FMT_BAYER_RGGB8 10
#define JPGE_FMT_BAYER_GRBG8 11
#define JPGE_FMT_BAYER_GBRG8 12
#define JPGE_FMT_BAYER_BGGR8 13
/* The rule above in plain C++ on the host: the `height` rows of `width` raw bytes at `src`, pitch
 * `stride` (0 = width), in Bayer layout `format`, to the RGB8 frame D at dst_rgb8, pitch dst_stride
 * (0 = 3 * width).  JPGE_E_ARG: another layout, a dimension below 2, a NULL pointer, or a stride
 * below a row's bytes; a refused call writes nothing.  (An addition.) */
int jpge_demosaic_frame(int format, const uint8_t* src, uint32_t width, uint32_t height, size_t stride,
                        uint8_t* dst_rgb8, size_t dst_stride);

/* Input layout for the context's following jpge_encode_rgb8, jpge_encode_batch,
 * jpge_fdct_quant and jpge_symbol_stats calls (their `rgb` then points at a frame in
 * that layout), also on a group member's context (jpge_group_context), and so for
 * jpge_group_encode_batch.  plane_stride: the planar layouts' bytes between planes
 * (NV12, I420, NV16, I422: from the Y plane to the chroma), 0 = stride * height of each frame
 * (contiguous CHW); non-zero with an interleaved layout, or an unknown layout: JPGE_E_ARG.  A frame's stride of 0 means width * the
 * layout's bytes per pixel (planar: width); a smaller stride is JPGE_E_ARG.  maxval
 * scales the three colour channels as before.  The fast path needs the pointer, the
 * stride and the plane stride 16-byte aligned; anything else works, slower.
 * The PPM entries (jpge_encode_file, jpge_encode_files) and the fp64 plane entries
 * ignore the setting.  jpge_stripe_transform takes the four interleaved layouts (the
 * stripe pointer stays "first pixel row of the stripe") and returns JPGE_E_ARG for
 * the planar ones (RGB8_PLANAR, NV12, I420, YUV444_PLANAR), for the four 4:2:2 layouts, the two 10-bit 4:2:0 and the three 10-bit 4:2:2 layouts, v210, the four Bayer layouts and for
 * JPGE_FMT_GRAY8 (stripes are three-component 4:2:0 of interleaved colour); jpge_group_encode_striped needs JPGE_FMT_RGB8. */
int jpge_set_input_format(jpge_ctx* ctx, int format, size_t plane_stride);
/* the current setting (plane_stride may be NULL) */
int jpge_get_input_format(jpge_ctx* ctx, int* format, size_t* plane_stride);
/* bytes per pixel along a row and number of planes of a layout (host only; either
 * pointer may be NULL); unknown layout: JPGE_E_ARG.  JPGE_FMT_V210: 0 bytes per pixel, meaning
 * "not a whole number": its rows are jpge_v210_row_bytes(width) */
int jpge_input_format_info(int format, int* bytes_per_pixel, int* planes);
/* Bytes of a v210 row of `width` pixels: 16 * ceil(width / 6).  Host only.  (An addition.) */
size_t jpge_v210_row_bytes(uint32_t width);
/* The layout rule of JPGE_FMT_V210 in plain C++ on the host: the samples of the `height` rows of
 * pitch `stride` (0 = jpge_v210_row_bytes(width)) at `src` as planes y (height x width), cb and cr
 * (height x ceil(width / 2)), contiguous.  A caller can produce the planes and check: the frame's
 * .jpg is that of the I210 frame of these planes.  JPGE_E_ARG: a NULL pointer, a zero dimension,
 * a stride below a row's bytes.  (An addition.) */
int jpge_v210_unpack(const uint8_t* src, uint32_t width, uint32_t height, size_t stride, uint16_t* y, uint16_t* cb,
                     uint16_t* cr);

/* ---- Huffman tables of the output (an addition; replaces nothing in the reference) ----
 * JPGE_HUFF_OPTIMAL builds per-image tables as writeJPEG does (Image.cpp:888-930): the
 * reference's stream, bit-identical, and a device -> host -> device round trip in every
 * frame (histograms out, tables back).  The fixed modes code with tables known before the
 * frame arrives, as libjpeg without `optimize` and MJPEG cameras do: a few per cent more
 * bytes, and no host work between a frame's statistics and entropy kernels. */
#define JPGE_HUFF_OPTIMAL  0   /* per-image tables, the reference's stream (default) */
#define JPGE_HUFF_STANDARD 1   /* ITU T.81 Annex K tables K.3-K.6 */
#define JPGE_HUFF_CUSTOM   2   /* caller's tables */
/* A table in DHT form (ITU T.81 B.2.4.2): bits[l - 1] = number of codes of length l
 * (1..16), huffval = the symbols in order of increasing code length; codes are assigned
 * canonically (T.81 Annex C).  (An addition; replaces nothing in the reference.) */
typedef struct { uint8_t bits[16]; uint8_t huffval[256]; } jpge_huff_spec;
/* Huffman mode of the context's following jpge_encode_rgb8, jpge_encode_batch and
 * jpge_encode_file(s) calls (an output property: the PPM entries honour it), also on a
 * group member's context (jpge_group_context), and so for jpge_group_encode_batch.  specs:
 * Y-DC, Y-AC, C-DC, C-AC; read only for JPGE_HUFF_CUSTOM (a one-component stream uses
 * specs 0 and 1 and writes two DHT segments).  JPGE_E_ARG for an unknown mode, CUSTOM with
 * specs == NULL, and a spec with more than 256 symbols, a repeated symbol, a Kraft sum
 * (sum of bits[l - 1] * 2^(16 - l)) of 2^16 or more (a code of all ones, T.81 C.2), or one
 * that is incomplete for 8-bit baseline data: a DC table must hold categories 0..11, an AC
 * table 0x00, 0xF0 and every run 0..15 x size 1..10 (in a fixed mode no frame's symbols
 * are looked at before they are coded, so no symbol may lack a code).  The setting is
 * orthogonal to the subsampling mode, the restart interval, the input layout, frame sets
 * and lanes.  The segment order is unchanged, each DHT carries the table as given, and
 * every other header byte is the optimal mode's.  In a fixed mode jpge_stripe_*,
 * jpge_group_encode_striped and jpge_encode_planes return JPGE_E_ARG (stripes share one
 * image's tables through the histogram all-reduce); the stage entries (jpge_fdct_quant,
 * jpge_symbol_stats, ...) behave the same in every mode; jpge_timing.symbols does not
 * advance (its source is the histogram).  (An addition; replaces nothing in the reference.) */
int jpge_set_huffman(jpge_ctx* ctx, int mode, const jpge_huff_spec specs[4]);
/* The current mode and, in a fixed mode, its four tables (specs may be NULL;
 * JPGE_HUFF_OPTIMAL fills nothing).  (An addition; replaces nothing in the reference.) */
int jpge_get_huffman(jpge_ctx* ctx, int* mode, jpge_huff_spec specs[4]);
/* Annex K table 0 Y-DC (K.3), 1 Y-AC (K.5), 2 C-DC (K.4), 3 C-AC (K.6); host only.
 * (An addition; replaces nothing in the reference.) */
int jpge_standard_huffman(int table /*0..3*/, jpge_huff_spec* spec);

/* ---- Sample transform of Y, Cb, Cr input (an addition; replaces nothing in the reference) ----
 * A JFIF file holds full-range BT.601 samples, and by default a Y, Cb, Cr frame is taken
 * to hold exactly those.  A video decoder's output is usually studio swing (Y 16..235,
 * Cb and Cr 16..240) and, above SD, BT.709: the presets below convert such samples to
 * full-range BT.601 inside the transform kernel, in fp64 with no intermediate rounding to
 * 8 bits and no pass over the frame.  (All additions.) */
#define JPGE_YUV_FULL_601     0  /* the default: a sample v is v - 128 (today's stream) */
#define JPGE_YUV_LIMITED_601  1  /* studio swing, BT.601 matrix: range expansion only   */
#define JPGE_YUV_LIMITED_709  2  /* studio swing, BT.709 matrix -> full-range BT.601    */
#define JPGE_YUV_FULL_709     3  /* full range, BT.709 matrix -> full-range BT.601      */
#define JPGE_YUV_CUSTOM       4  /* the caller's coefficients                           */
/* With bytes (y, cb, cr) of one pixel (NV12, I420: cb, cr of the pixel's 2x2 cell),
 * yc = (double)y - y_off, u = (double)cb - 128, v = (double)cr - 128 (all exact), the fp64
 * planes that enter the pipeline (the reference Image's planes after convertToColorSpace) are
 *   Y'  = min(max((m[0]*yc + m[1]*u) + m[2]*v, 0), 255) - 128
 *   Cb' = min(max( m[3]*u + m[4]*v, -128), 127)
 *   Cr' = min(max( m[5]*u + m[6]*v, -128), 127)
 * each product and each sum rounded to fp64 on its own, in the order of the brackets (no
 * fused multiply-add): these rules define the output bytes.  The clamps keep every sample in
 * the interval of an 8-bit one whatever the input (super-white and out-of-gamut samples
 * are legal in video), so the coefficient bounds the fixed Huffman tables rest on hold.
 * (An addition.) */
typedef struct { double y_off; double m[7]; } jpge_yuv_transform;
/* The transform of the context's following jpge_encode_rgb8, jpge_encode_batch,
 * jpge_fdct_quant and jpge_symbol_stats calls on frames in JPGE_FMT_NV12, _I420,
 * _YUV444_PLANAR (transform per pixel, then the subsampling mode's filter) and _GRAY8 (y_off
 * and m[0] only: a video's Y plane as a grayscale file); also on a group member's context
 * (jpge_group_context), and so for jpge_group_encode_batch.  The RGB layouts ignore it.
 * custom is read for JPGE_YUV_CUSTOM only.  JPGE_E_ARG for an unknown preset, CUSTOM with
 * custom == NULL, a non-finite value, y_off outside 0..255 or an |m[i]| above 4; the
 * setting is then unchanged.  Orthogonal to the subsampling mode, the restart interval,
 * the Huffman mode, lanes and frame sets; the header bytes do not depend on it; maxval must
 * still be 255, and every refusal of the layouts stands.  JPGE_YUV_FULL_601 runs the same
 * kernels as a context that never called this.  (An addition.) */
int jpge_set_yuv_transform(jpge_ctx* ctx, int preset, const jpge_yuv_transform* custom);
/* The current preset and its coefficients (t may be NULL).  (An addition.) */
int jpge_get_yuv_transform(jpge_ctx* ctx, int* preset, jpge_yuv_transform* t);
/* A preset's coefficients; host only, no context.  LIMITED_*: y_off 16, m[0] = 255/219,
 * the chroma entries scaled by 255/224; *_709: the matrix A601 . inverse(A709) of the
 * BT.601 (0.299, 0.587, 0.114) and BT.709 (0.2126, 0.7152, 0.0722) luma weights;
 * JPGE_YUV_FULL_601: the identity (y_off 0, m[0] = m[3] = m[6] = 1).  JPGE_E_ARG for
 * JPGE_YUV_CUSTOM and unknown presets.  (An addition.) */
int jpge_yuv_preset(int preset, jpge_yuv_transform* t);

/* ---- Box downscale of the input (an addition; replaces nothing in the reference) ----
 * With factor s = 2 or 4 a width x height frame is coded at dw = ceil(width / s),
 * dh = ceil(height / s): the transform kernel averages s x s source samples into each
 * sample it reads, so a 4K or 8K surface becomes a 1080p .jpg without a resize pass and
 * without a second surface.  Every 8-bit sample of the downscaled frame D is the integer
 * mean, rounded half up, of its source samples, their coordinates clamped to the plane:
 *
 *   D[y][x][c] = (sum_{j<s, i<s} S[min(s*y + j, H-1)][min(s*x + i, W-1)][c] + s*s/2) / (s*s)
 *
 * NV12: the Y plane over width x height, and the Cb,Cr plane the same way in its own
 * domain (ceil(width / 2) x ceil(height / 2), Cb and Cr separately).  RGBA8 / BGRA8: alpha
 * is ignored.  The .jpg of a frame coded with factor s is, byte for byte, the .jpg of D
 * (jpge_downscale_frame) coded with factor 1 in the same layout, under every other
 * setting; SOF0 carries dw x dh.
 *
 * The factor applies to the context's following jpge_encode_rgb8, jpge_encode_batch,
 * jpge_encode_file(s), jpge_fdct_quant and jpge_symbol_stats calls (the last two return
 * D's planes and histograms), and on a group member's context to jpge_group_encode_batch.
 * Layouts with s > 1: JPGE_FMT_RGB8, _BGR8, _RGBA8, _BGRA8 in every subsampling mode and
 * JPGE_FMT_NV12; with any other layout those calls return JPGE_E_ARG (a batch: the frame's
 * status) before anything is queued, as do jpge_stripe_transform and
 * jpge_group_encode_striped.  jpge_encode_planes and the plane stages ignore the setting.
 * The limits on width, height and stride are the source's; jpge_max_jpeg_bytes(dw, dh)
 * bounds the output.
 *
 * 1 (the default), 2 or 4; anything else, or a NULL context: JPGE_E_ARG, the setting
 * unchanged. */
int jpge_set_downscale(jpge_ctx* ctx, int factor);
int jpge_get_downscale(jpge_ctx* ctx, int* factor);
/* dw, dh of a width x height frame; host only.  JPGE_E_ARG: a factor other than 1, 2, 4,
 * a zero dimension or a NULL pointer. */
int jpge_downscaled_size(uint32_t width, uint32_t height, int factor, uint32_t* dw, uint32_t* dh);
/* The rule above in plain C++, host only: src (width x height in `format`, row pitch
 * stride, 0 = dense; NV12: the Cb,Cr plane plane_stride bytes after the Y plane, 0 =
 * stride * height) to dst (dw x dh in the same layout, dst_stride and dst_plane_stride
 * likewise).  Factor 1 copies the rows; with 2 or 4 a 4-byte layout's fourth byte is 255.
 * JPGE_E_ARG: a layout without a downscaling kernel, another factor, a zero dimension, a
 * NULL pointer, a stride below a row's bytes or a plane stride below the Y plane's. */
int jpge_downscale_frame(int format, const uint8_t* src, uint32_t width, uint32_t height, size_t stride,
                         size_t plane_stride, int factor, uint8_t* dst, size_t dst_stride, size_t dst_plane_stride);

/* ---- Orientation of the input (an addition; replaces nothing in the reference) ----
 * A frame whose rows are not the picture's rows (a sensor mounted sideways, portrait video,
 * a mirrored front camera) is coded flipped, rotated or transposed: the transform kernel
 * reads the source in the turned order while it stages a tile, so no transpose or flip pass
 * runs and no second surface exists.  The stream stays plain JFIF, without an orientation
 * tag: the pixels are turned.  The values name the operation applied to the pixels.  With the
 * source S of Ws x Hs pixels, S(r, c) its pixel at row r, column c, the coded frame O is
 * ow x oh:
 *
 *   value  name                       ow x oh   O(y, x) =              numpy
 *   0      JPGE_ORIENT_NONE (default) Ws x Hs   S(y, x)                a
 *   1      JPGE_ORIENT_FLIP_H         Ws x Hs   S(y, Ws-1-x)           a[:, ::-1]
 *   2      JPGE_ORIENT_ROT180         Ws x Hs   S(Hs-1-y, Ws-1-x)      a[::-1, ::-1]
 *   3      JPGE_ORIENT_FLIP_V         Ws x Hs   S(Hs-1-y, x)           a[::-1]
 *   4      JPGE_ORIENT_TRANSPOSE      Hs x Ws   S(x, y)                a.transpose(1, 0, 2)
 *   5      JPGE_ORIENT_ROT90          Hs x Ws   S(Hs-1-x, y)           np.rot90(a, -1)   (clockwise)
 *   6      JPGE_ORIENT_TRANSVERSE     Hs x Ws   S(Hs-1-x, Ws-1-y)      np.rot90(a, 2).transpose(1, 0, 2)
 *   7      JPGE_ORIENT_ROT270         Hs x Ws   S(x, Ws-1-y)           np.rot90(a, 1)    (counter-clockwise)
 *
 * The .jpg of a frame coded with orientation o is, byte for byte, the .jpg of O
 * (jpge_orient_frame) coded with JPGE_ORIENT_NONE in the same layout, under every other
 * setting: quality tables, maxval, subsampling mode, restart interval, Huffman mode, frame
 * sets and lanes.  SOF0 carries ow x oh; the padding to whole MCUs replicates O's right and
 * bottom edge (the kernel clamps in O's coordinates first and maps to the source second);
 * alpha is ignored.
 *
 * The setting applies to the calls jpge_set_downscale applies to: jpge_encode_rgb8,
 * jpge_encode_batch, jpge_encode_file(s), jpge_fdct_quant and jpge_symbol_stats (the last two
 * return O's planes and histograms), and on a group member's context jpge_group_encode_batch.
 * Layouts with o != 0: JPGE_FMT_RGB8, _BGR8, _RGBA8, _BGRA8.  Orientations 1-3 in every
 * subsampling mode; 4-7 in the three modes with 16x16 MCUs (JPGE_S420_M, JPGE_S420,
 * JPGE_S420_LM).  Everything else with o != 0 returns JPGE_E_ARG (a batch: the frame's status)
 * before anything is queued: any other layout, 4-7 in JPGE_S444 / _S422 / _S411, a downscale
 * factor above 1 together with o != 0, jpge_stripe_transform and jpge_group_encode_striped.
 * jpge_encode_planes and the plane stages ignore the setting.  The limits on width, height and
 * stride, and the 32-bit offset check, are the source's; jpge_max_jpeg_bytes(ow, oh) bounds the
 * output.
 *
 * Speed: the fast path needs base and stride 16-byte aligned, as without an orientation.  The
 * mirrored orientations (1, 2, 6, 7) read each row's runs from its far end, so they need in
 * addition a row of a multiple of 16 bytes: Ws % 16 == 0 for 3-byte pixels, Ws % 4 == 0 for
 * 4-byte pixels.  A mirrored frame whose width misses that is read pixel by pixel on every
 * tile: correct, at about twice the transform kernel's time.
 *
 * 0..7; anything else, or a NULL context: JPGE_E_ARG, the setting unchanged. */
#define JPGE_ORIENT_NONE 0
#define JPGE_ORIENT_FLIP_H 1
#define JPGE_ORIENT_ROT180 2
#define JPGE_ORIENT_FLIP_V 3
#define JPGE_ORIENT_TRANSPOSE 4
#define JPGE_ORIENT_ROT90 5
#define JPGE_ORIENT_TRANSVERSE 6
#define JPGE_ORIENT_ROT270 7
int jpge_set_orientation(jpge_ctx* ctx, int orientation);
int jpge_get_orientation(jpge_ctx* ctx, int* orientation);
/* ow, oh of a width x height frame; host only.  JPGE_E_ARG: a value outside 0..7, a zero
 * dimension or a NULL pointer. */
int jpge_oriented_size(uint32_t width, uint32_t height, int orientation, uint32_t* ow, uint32_t* oh);
/* The table above in plain C++, host only: src (width x height in `format`, row pitch stride,
 * 0 = dense) to dst (ow x oh in the same layout, dst_stride likewise; src and dst must not
 * overlap).  A 4-byte layout's fourth byte is copied.  Bytes of dst outside its rows' pixels
 * are not written.  JPGE_E_ARG: a layout other than the four above, a value outside 0..7, a
 * zero dimension, a NULL pointer or a stride below a row's bytes. */
int jpge_orient_frame(int format, const uint8_t* src, uint32_t width, uint32_t height, size_t stride, int orientation,
                      uint8_t* dst, size_t dst_stride);

/* Per-channel lookup tables (an addition): a tone curve applied inside the transform kernel as it
 * stages a tile -- black level, per-channel gain (white balance), gamma or an sRGB curve, contrast
 * stretch, inversion -- with no pass over the surface in front of the encode.
 *
 * lut is 768 bytes T: T[0..255] for R, T[256..511] for G, T[512..767] for B.  Take a frame F in
 * layout L and let D(F) be its RGB8 frame: the pixels rearranged for JPGE_FMT_RGB8, _BGR8, _RGBA8
 * and _BGRA8, and jpge_demosaic_frame(F) for the four Bayer layouts.  With tables set, F codes as
 * the RGB8 frame M with
 *     M[y][x][c] = T[256 * c + D[y][x][c]]        c = 0 (R), 1 (G), 2 (B).
 * The table is chosen by colour, not by byte position (BGR8: the byte at offset 0 goes through
 * the B table); alpha is ignored, as without tables; a Bayer frame's tables act on the demosaiced
 * pixel (after the bilinear rule), not on the raw byte.  All of it is integer: the .jpg is, byte
 * for byte, that of M coded as JPGE_FMT_RGB8 with no tables on the same context, under every other
 * setting (quality tables, the six subsampling modes, restart interval, Huffman mode, lanes and
 * frame sets, jpge_encode_batch, jpge_group_encode_batch); jpge_fdct_quant and jpge_symbol_stats
 * return M's coefficients and histograms.  Padding to whole MCUs replicates M's edge pixels (the
 * map is per pixel, so it commutes with the clamp).  The identity tables give the bytes of a
 * context without tables; a context that never calls the setter launches the kernels it launched
 * before this entry existed.
 *
 * jpge_set_channel_lut: NULL switches the tables off (the default).  The 768 bytes are copied, to
 * the host and to the device (on a stream of the context's own, awaited), so the caller's buffer
 * is free on return.  The setting applies to jpge_encode_rgb8, jpge_encode_batch, jpge_fdct_quant,
 * jpge_symbol_stats, jpge_encode_file(s) and, on a group member's context, jpge_group_encode_batch.
 * With tables set these return JPGE_E_ARG before anything is queued (a batch or a file list: the
 * frame's status; the context stays usable): a layout other than RGB8, BGR8, RGBA8, BGRA8 and the
 * four Bayer ones; maxval other than 255 (a PPM file's too); a downscale factor above 1; an
 * orientation other than JPGE_ORIENT_NONE; jpge_stripe_transform and jpge_group_encode_striped.
 * jpge_encode_planes and the plane stages ignore the setting.  Not built: planar RGB, GRAY8 and
 * the Y, Cb, Cr layouts, a 3x3 colour matrix, tables deeper than 8 bits.
 * jpge_get_channel_lut: *on is 0 or 1; lut (may be NULL) receives the bytes last set.
 * Speed: about the transform kernel's time without tables. */
int jpge_set_channel_lut(jpge_ctx* ctx, const uint8_t lut[768]);
int jpge_get_channel_lut(jpge_ctx* ctx, int* on, uint8_t lut[768]);
/* The rule above in plain C++, host only, for the four interleaved layouts: src (width x height
 * in `format`, row pitch stride, 0 = dense) to dst in the same layout (dst_stride likewise; dst
 * may be src).  A 4-byte layout's fourth byte is copied.  Bytes of dst outside its rows' pixels
 * are not written.  JPGE_E_ARG: another layout, a zero dimension, a NULL pointer, or a stride
 * below a row's bytes; a refused call writes nothing.  It has no Bayer case: compose it with
 * jpge_demosaic_frame. */
int jpge_lut_frame(int format, const uint8_t* src, uint32_t width, uint32_t height, size_t stride, const uint8_t lut[768],
                   uint8_t* dst, size_t dst_stride);

/* Worst-case .jpg size for a frame, in any subsampling mode (header + 2x
 * worst-case entropy + RST markers + EOI). */
size_t jpge_max_jpeg_bytes(uint32_t width, uint32_t height);

/* Quantisation tables for quality 1..100: the reference's Annex-K tables
 * (Image.cpp:850-869) scaled by the IJG rule; quality 50 returns them unchanged,
 * which is the only table pair the reference itself uses. Natural order. */
int jpge_quality_tables(int quality, uint8_t qy[64], uint8_t qc[64]);

/* Full encode — replaces Image::writeJPEG (Image.hpp:92, Image.cpp:831-976) for an
 * image as produced by loadPPM: SOI APP0 DQT DQT SOF0 DHTx4 SOS <entropy> EOI.
 * Returns once every output byte is in place: in host memory (host output), or in
 * device memory (JPGE_DEVICE_OUTPUT), readable from any stream.  On a 1-lane context
 * with device output the call returns as soon as the bytes are written, while the
 * context's stream may still be retiring the last kernel (later work on the context
 * is ordered after it). */
int jpge_encode_rgb8(jpge_ctx* ctx, const uint8_t* rgb, uint32_t width, uint32_t height, size_t stride,
                     int maxval, const uint8_t qy[64], const uint8_t qc[64], uint8_t* out, size_t cap,
                     size_t* len, uint32_t flags);

/* Many independent frames, pipelined on the context's stream (configs 3/4): the
 * transform of later frames is queued ahead of each frame's entropy kernel while
 * host threads build that frame's tables. */
int jpge_encode_batch(jpge_ctx* ctx, jpge_frame* frames, int n, const uint8_t qy[64], const uint8_t qc[64],
                      uint32_t flags);

/* Stage entry — convertToColorSpace + applySubsampling(S420_m) + applyDCT(Arai) +
 * applyQuantization (Image.cpp:839-871) on the GPU: quantised coefficients before
 * DC differencing, per component, blocks in raster order, 64 natural-order values
 * per block (host buffers of (W'/8)(H'/8)*64 and 2 x (W'/16)(H'/16)*64 int16; at
 * 4:4:4 three buffers of ceil(W/8)*ceil(H/8)*64 int16). */
int jpge_fdct_quant(jpge_ctx* ctx, const uint8_t* rgb, uint32_t width, uint32_t height, size_t stride,
                    int maxval, const uint8_t qy[64], const uint8_t qc[64], int16_t* coef_y, int16_t* coef_cb,
                    int16_t* coef_cr, uint32_t flags);

/* Stage entry — the symbol "texts" of writeJPEG (Image.cpp:888-906) as histograms:
 * counts[t*256+s] and first[t*256+s] = position key of the first occurrence
 * (~0 if absent); t = 0 Y-DC, 1 Y-AC, 2 C-DC, 3 C-AC. */
int jpge_symbol_stats(jpge_ctx* ctx, const uint8_t* rgb, uint32_t width, uint32_t height, size_t stride,
                      int maxval, const uint8_t qy[64], const uint8_t qc[64], uint32_t counts[1024],
                      uint64_t first[1024], uint32_t flags);

/* Host table build — replaces generateHuffmanCode (Huffman.hpp:53, Huffman.cpp:3-66)
 * for byte symbols given counts and first-occurrence keys.  bits[0..15] = number
 * of codes of length 1..16, huffval = DHT symbol order, code/len per symbol. */
int jpge_huffman_table(const uint32_t counts[256], const uint64_t first[256], uint8_t bits[16],
                       uint8_t huffval[256], int* nsym, uint32_t code[256], uint8_t len[256]);

/* Same for an arbitrary int symbol text (the reference signature, for tests and
 * tools): writes n distinct symbols as (symbol, length, code) in DHT order. */
int jpge_huffman_text(const int* text, size_t n, int* syms, int* lens, uint32_t* codes, int* nsym);

/* Concatenate n device byte segments (segs[k], lens[k] bytes) back to back into the
 * device buffer dst, in one kernel launch per 96 segments on `stream` (a hipStream_t;
 * NULL = the null stream), without waiting for it; *total (optional) = the sum of the
 * lengths.  device: the GPU the buffers live on (the caller's current device is kept).
 * Config 4's gather packs a rank's .jpg bytes with it (jpgenc_amd/gather.py) before
 * the one transfer to rank 0.  Replaces nothing in the reference (its encoder is one
 * process); an addition of this library.  Any alignments; segments below 2 GB. */
int jpge_concat_segments(int device, void* stream, const uint8_t* const* segs, const size_t* lens, int n,
                         uint8_t* dst, size_t* total);

/* ---- Decode-side verification utilities (host) ---- */

/* huffmanDecode (Huffman.hpp:62, Huffman.cpp:91-146): the symbol text coded in the
 * first nbits bits (MSB-first bytes) by the table of nsym (symbol, code, length)
 * entries, codes right-aligned as jpge_huffman_text returns them.  `bits` must hold
 * at least ceil(nbits / 8) bytes.  text = NULL: count only.  JPGE_E_FORMAT where no
 * code matches (the reference asserts). */
int jpge_huffman_decode(const uint8_t* bits, uint64_t nbits, const uint32_t* table_syms, const uint32_t* table_codes,
                        const uint8_t* table_lens, int nsym, int* text, size_t cap, size_t* n);

/* inverseDctMat (Dct.hpp:278-306) of one 8x8 block, row-major doubles:
 * (A^T X) A with A(k, n) = C(k) sqrt(2/8) cos((2n+1) k pi / 16). */
void jpge_idct8x8(const double in[64], double out[64]);

/* A decoded jpge stream's frame (jpge_decode_coeffs). */
typedef struct {
    uint32_t width, height;  /* SOF0: the real size */
    uint32_t yh, yv;         /* Y sampling factors (chroma is 1x1) */
    uint32_t restart;        /* DRI interval in MCUs, 0 = none */
    size_t y_blocks, c_blocks; /* coefficient blocks per plane */
    uint8_t qy[64], qc[64];  /* DQT tables, natural order */
} jpge_decoded;

/* Baseline entropy decode of a .jpg written by this library (SOF0; three
 * components, chroma 1x1, Y 1x1 / 2x1 / 4x1 / 2x2, or one component 1x1, the
 * JPGE_FMT_GRAY8 stream; optional DRI/RSTn): the
 * quantised coefficients with the DC differences undone (Image.cpp:638-678
 * inverted), natural order, blocks in raster order per component — the planes
 * jpge_fdct_quant returns.  y = NULL: fill *info only (sizes).  A one-component
 * stream reports yh = yv = 1, c_blocks = 0 (how a caller tells it) and a zero qc;
 * cb and cr may then be NULL and are not written.  Verification utility, not on
 * the encode path. */
int jpge_decode_coeffs(const uint8_t* jpg, size_t len, jpge_decoded* info, int16_t* y, int16_t* cb, int16_t* cr,
                       size_t cap_y_blocks, size_t cap_c_blocks);

/* PPM front end — replaces loadPPM (Image.hpp:28, Image.cpp:421-538) up to the
 * padding, which the GPU path performs by clamped addressing.  parse: rgb gets
 * width*height*3 unscaled samples (cap bytes available). */
int jpge_parse_ppm(const uint8_t* buf, size_t n, uint8_t* rgb, size_t cap, uint32_t* width, uint32_t* height,
                   int* maxval);
int jpge_ppm_info(const uint8_t* buf, size_t n, uint32_t* width, uint32_t* height, int* maxval);

/* Convenience: PPM file -> .jpg file at the given quality (the CLI path, main.cpp:8-32). */
int jpge_encode_file(jpge_ctx* ctx, const char* ppm_path, const char* jpg_path, int quality);

/* Many PPM files -> .jpg files (the CLI path over a list), pipelined: worker threads
 * read and parse each file into pinned memory while the previous group of frames is
 * encoded (H2D queued ahead of the kernels on each lane) and the one before is copied
 * back and written.  lens/statuses (optional, n entries) get each file's .jpg length
 * and jpge_status; returns the first failing status.  group = frames per stage
 * (0 = 8, at most 64).  Bytes equal jpge_encode_file's for every file. */
int jpge_encode_files(jpge_ctx* ctx, const char* const* ppm_paths, const char* const* jpg_paths, int n, int quality,
                      size_t* lens, int* statuses, int group);

/* Deterministic synthetic frame (kind 0 photo-like, 1 random bytes, 2 flat). */
int jpge_synth_rgb8(uint64_t seed, uint32_t width, uint32_t height, int kind, uint8_t* out, size_t stride);

/* The Arai constants compiled into the kernels (Dct.hpp:21-43), for verification:
 * a[0..4] = a1..a5, s[0..7] = s0..s7. */
void jpge_arai_constants(double a[5], double s[8]);

/* ---- Coding.hpp primitives (host; per block, as the reference's free functions) ----
 * The GPU path computes all of these inside its kernels; these entries serve the
 * facade's Coding.hpp functions (jpge_image.hpp) and their known-answer tests. */

/* zigzag(int) (Coding.hpp:57-81): the natural (row-major) index of zig-zag position
 * i (0..63); -1 for i outside 0..63 (the reference asserts). */
int jpge_zigzag_index(int i);
/* zigzag(matrix) (Coding.hpp:30-54): out[zig-zag position of (r, c)] = in[r * 8 + c]. */
int jpge_zigzag_block(const int32_t in[64], int32_t out[64]);
/* quantize (Coding.hpp:84-97): out[i] = (int)round(block[i] / table[i]), row-major. */
int jpge_quantize_block(const double block[64], const double table[64], int32_t out[64]);
/* RLE_AC (Coding.hpp:112-183): (run, value) pairs; pair 0 is (0, DC); a value after
 * more than 15 zeros is preceded by (15, 0) pairs; a trailing zero run ends with the
 * EOB pair (0, 0).  zigzag_scan = 0: the vector version over data[0..n) as given
 * (n >= 2); 1: the matrix version over a natural-order 8x8 block (n = 64) scanned in
 * zig-zag order.  *npairs receives the count (JPGE_E_NOSPACE if cap is smaller). */
int jpge_rle_ac(const int32_t* data, size_t n, int zigzag_scan, uint8_t* runs, int32_t* values, size_t cap,
                size_t* npairs);
/* getCategoryAndCode (Coding.hpp:197-262): category = bit length of |value| (0 for
 * 0), bits = value if > 0 else (2^category - 1) - |value| (the low `category` bits,
 * written MSB-first).  JPGE_E_RANGE for |value| >= 2^15 (the reference asserts). */
int jpge_category_code(int32_t value, uint16_t* category, uint32_t* bits);
/* encode_category (Coding.hpp:265-283): per pair, symbol = (run << 4) | category and
 * its extra bits (code, code_lens[i] = category). */
int jpge_encode_category(const uint8_t* runs, const int32_t* values, size_t n, uint8_t* symbols, uint32_t* codes,
                         uint8_t* code_lens);
/* applyDCdifferenceCoding (Image.cpp:638-678), in place on quantised int planes:
 * the Y DCs in MCU order (2x2 blocks of 8x8 per 16x16 MCU), each chroma plane's DCs
 * in block raster order; every chain starts at 0.  Y is rows x cols (multiples of
 * 16), the chroma planes crows x ccols (multiples of 8). */
int jpge_dc_difference(int32_t* y, uint32_t rows, uint32_t cols, int32_t* cb, int32_t* cr, uint32_t crows,
                       uint32_t ccols);

/* ---- Plane stages: the reference's Image stage methods on fp64 planes (GPU) ----
 * Row-major planes of doubles (Image's matrix<PixelDataType>); host buffers, or
 * device buffers with JPGE_DEVICE_INPUT / JPGE_DEVICE_OUTPUT.  Each call returns with
 * its results in place.  Bit-identical to the reference's loops. */
#define JPGE_TO_RGB 0
#define JPGE_TO_YCBCR 1
/* convertToColorSpace (Image.cpp:112-179) of n pixels: JPGE_TO_YCBCR takes R,G,B
 * planes to Y,Cb,Cr; JPGE_TO_RGB the reverse. */
int jpge_color_convert(jpge_ctx* ctx, const double* in0, const double* in1, const double* in2, double* out0,
                       double* out1, double* out2, size_t n, int target, uint32_t flags);
/* Image::subsample with applySubsampling's mask for `mode` (JPGE_S*; Image.cpp:
 * 198-319) on one rows x cols plane; out gets out_rows x out_cols (S444: a copy).
 * out = NULL: only the output size. */
int jpge_subsample_plane(jpge_ctx* ctx, const double* in, uint32_t rows, uint32_t cols, int mode, double* out,
                         uint32_t* out_rows, uint32_t* out_cols, uint32_t flags);
#define JPGE_DCT_SIMPLE 0 /* dctDirect (Dct.hpp:238-262) */
#define JPGE_DCT_MATRIX 1 /* dctMat (Dct.hpp:264-276) */
#define JPGE_DCT_ARAI 2   /* dctArai (Dct.hpp:47-215), writeJPEG's */
/* applyDCT(mode) (Image.cpp:540-595) on one plane of 8x8 blocks (rows, cols
 * multiples of 8). */
int jpge_dct_plane(jpge_ctx* ctx, const double* in, uint32_t rows, uint32_t cols, int dct_mode, double* out,
                   uint32_t flags);
/* applyQuantization's per-block quantize (Image.cpp:597-636, Coding.hpp:84-97) on
 * one plane of 8x8 blocks with one natural-order table. */
int jpge_quantize_plane(jpge_ctx* ctx, const double* in, uint32_t rows, uint32_t cols, const uint8_t table[64],
                        int32_t* out, uint32_t flags);
/* writeJPEG (Image.cpp:831-976) on an Image's three planes (rows x cols, multiples of
 * 16): colorspace JPGE_TO_RGB = the planes are R,G,B (converted first), JPGE_TO_YCBCR
 * = they are Y,Cb,Cr with full-size chroma; then S420_m, Arai, quantisation, DC/RLE/
 * category, per-image tables and emission, all on the GPU.  SOF0 carries
 * real_width x real_height.  The context's restart interval applies. */
int jpge_encode_planes(jpge_ctx* ctx, const double* p0, const double* p1, const double* p2, uint32_t rows,
                       uint32_t cols, int colorspace, uint32_t real_width, uint32_t real_height, const uint8_t qy[64],
                       const uint8_t qc[64], uint8_t* out, size_t cap, size_t* len, uint32_t flags);

/* ---- Row stripes of one large image across devices ----
 * The image (width x height, 4:2:0) is cut into stripes of whole MCU rows (16 px);
 * each stripe is encoded by its own context (one per GPU) in four phases, with
 * three small exchanges between them that the caller performs (RCCL all-gather /
 * all-reduce, or plain copies in one process).  The result is byte-identical to
 * encoding the whole image at once: the reference never emits restart markers, so
 * its DC chain (Image.cpp:638-678), its histograms (Image.cpp:888-906) and its
 * single bit stream (Image.cpp:957-972) run across stripe boundaries.
 *   1 jpge_stripe_transform  -> last_dc; exchange: all-gather, stripe r's seed = r-1's last_dc
 *   2 jpge_stripe_stats      -> counts/first; exchange: all-reduce counts (sum), first (min)
 *   3 jpge_stripe_code       -> summary; exchange: all-gather summaries
 *   4 jpge_stripe_pack       -> the stripe's bytes at their place in a whole-file device
 *                               buffer; then gather every [seg_off, seg_off + seg_len) to one rank.
 * With a restart interval set (jpge_set_restart_interval on every context) whose
 * boundaries include every stripe start, the stripes are independent but for the
 * shared tables: no DC seed is needed (phase 1's exchange can be skipped), and the
 * summaries only carry byte lengths — the output equals the whole-image restart
 * encode.  Replaces nothing in the reference (single-process, single-image encoder). */
typedef struct {
    uint64_t bits;    /* length of the stripe's bit stream (restart intervals: its byte length) */
    uint32_t ff[8];   /* 0xFF bytes wholly inside it when it starts at bit a (mod 8) */
    uint32_t head;    /* its first 8 bits */
    uint32_t tail;    /* its last 8 bits */
    uint32_t restart; /* 1: restart-interval stripe (every stripe starts an interval: its bytes
                         are self-contained, so placement is a prefix sum of byte lengths) */
    uint32_t pad;
} jpge_stripe_summary;

/* K1 on MCU rows [mcu_row0, mcu_row0 + mcu_rows) of the image; rgb = device pointer
 * to the stripe's first pixel row (image row 16*mcu_row0), stride bytes per row. */
int jpge_stripe_transform(jpge_ctx* ctx, const uint8_t* rgb, size_t stride, uint32_t width, uint32_t height,
                          uint32_t mcu_row0, uint32_t mcu_rows, int maxval, const uint8_t qy[64],
                          const uint8_t qc[64], int32_t last_dc[3]);
/* K2 with the DC chain seeded by the previous stripe's last Y/Cb/Cr DC (0,0,0 for
 * the first stripe); counts/first as jpge_symbol_stats, keys in the image's texts. */
int jpge_stripe_stats(jpge_ctx* ctx, const int32_t seed_dc[3], uint32_t counts[1024], uint64_t first[1024]);
/* Tables from the image's (summed) counts and (minimum) first keys, then the code
 * kernel; returns the stripe's summary and the header length. */
int jpge_stripe_code(jpge_ctx* ctx, const uint32_t counts[1024], const uint64_t first[1024],
                     jpge_stripe_summary* summary, size_t* header_len);
/* Host only: stripe `index`'s first output byte and the whole file's length. */
int jpge_stripe_place(const jpge_stripe_summary* all, int n, int index, size_t header_len, size_t* seg_off,
                      size_t* total_len);
/* Stuffed bytes of stripe `index` into out (device, whole-file capacity cap) at
 * [seg_off, seg_off + seg_len); stripe 0 includes the headers, the last one the
 * 1-fill and EOI. */
int jpge_stripe_pack(jpge_ctx* ctx, const jpge_stripe_summary* all, int n, int index, uint8_t* out, size_t cap,
                     size_t* seg_off, size_t* seg_len, size_t* total_len);

/* ---- Device groups: one process, several devices ----
 * A group owns one context per listed device and, when the devices are distinct, a
 * single-process RCCL clique (ncclCommInitAll) over xGMI.  A device listed more than
 * once (a rehearsal of N members on one GPU) makes the group exchange through host
 * memory and device copies instead; the bytes are the same.  Replaces nothing in
 * the reference (a single-threaded CPU encoder). */
typedef struct jpge_group jpge_group;
/* lanes: per member context, as jpge_open_ex.  JPGE_E_RCCL if librccl cannot be
 * loaded or the communicators cannot be created. */
int jpge_group_open(int ndev, const int* devices, int lanes, jpge_group** g);
int jpge_group_close(jpge_group* g);
/* members, and whether the exchanges ride RCCL (1) or host memory (0) */
int jpge_group_size(const jpge_group* g, int* n, int* uses_rccl);
/* member i's context (for per-member settings; owned by the group) */
int jpge_group_context(jpge_group* g, int member, jpge_ctx** ctx);
/* restart interval of every member (jpge_set_restart_interval) */
int jpge_group_set_restart_interval(jpge_group* g, uint32_t mcus);
/* Config 4: independent frames, frame i encoded by member i mod N (no collective);
 * with JPGE_DEVICE_INPUT / _OUTPUT frame i's buffers live on that member's device.
 * Per-frame len/status as jpge_encode_batch. */
int jpge_group_encode_batch(jpge_group* g, jpge_frame* frames, int n, const uint8_t qy[64], const uint8_t qc[64],
                            uint32_t flags);
/* Config 5: one 4:2:0 image (host RGB8) in row stripes of whole MCU rows over the
 * members — the jpge_stripe_* phases on every member at once, with an RCCL all-gather
 * of the DC seeds, all-reduce of the histograms (sum) and first-occurrence keys
 * (min), all-gather of the stripe summaries, and a grouped send/recv of the stuffed
 * segments to member 0 — then the whole .jpg to host memory.  Byte-identical to
 * jpge_encode_rgb8 on one device (with the group's restart interval, every stripe
 * starts an interval and the DC seed exchange drops out). */
int jpge_group_encode_striped(jpge_group* g, const uint8_t* rgb, uint32_t width, uint32_t height, size_t stride,
                              int maxval, const uint8_t qy[64], const uint8_t qc[64], uint8_t* out, size_t cap,
                              size_t* len);

#ifdef __cplusplus
}
#endif
#endif /* JPGE_H_ */
