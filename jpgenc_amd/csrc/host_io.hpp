// Host-side I/O around the GPU path: the PPM front end (reference loadPPM,
// Image.cpp:326-538), the JFIF segment writer (JpegSegments.hpp:55-377 as used by
// Image.cpp:933-954), quality-scaled quantisation tables, and the deterministic
// synthetic frame generator used by tests and the bench.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "huffman.hpp"

namespace jpge {

// Status codes shared with the C ABI (include/jpge.h).
enum Status : int {
    kOk = 0,
    kErrArg = 1,
    kErrNoSpace = 2,
    kErrHip = 3,
    kErrNoDevice = 4,
    kErrFormat = 5,
    kErrIo = 6,
    kErrTruncated = 7,
    kErrRange = 8,
    kErrTimeout = 9,
    kErrRccl = 10,
    kErrInternal = 11,
};

struct PpmImage {
    uint32_t width = 0, height = 0;
    int maxval = 0;
    std::vector<uint8_t> rgb;  // width*height*3 samples, unscaled (0..maxval)
};

// Parses P3/P6 with the reference tokenizer semantics (PPMFileBuffer::read_word,
// Image.cpp:334-390: whitespace skipping, '#' comment lines, fast_atoi for P3
// samples).  Differences, all on inputs where the reference has undefined
// or assert-only behaviour: truncated P6 data -> kErrTruncated; samples above
// maxval or maxval outside 1..255 -> kErrRange.
int parse_ppm(const uint8_t* buf, size_t n, PpmImage& out);
int load_ppm_file(const std::string& path, PpmImage& out);
// The same parse without a copy: P6 -> offset of the samples in buf; P3 -> the
// samples written over the text at buf[0..) (offset 0).
int parse_ppm_inplace(uint8_t* buf, size_t n, uint32_t& width, uint32_t& height, int& maxval, size_t& offset);

// Annex K tables (Image.cpp:850-869) scaled for quality 1..100 with the IJG rule
// (50 == the reference's tables unchanged).
void quality_tables(int quality, uint8_t qy[64], uint8_t qc[64]);

// Natural (row-major) index of zig-zag position i (Coding.hpp:57-81).
extern const uint8_t kZigzagToNatural[64];

// SOI, APP0, DQT(luma), DQT(chroma), SOF0, DHT x4, SOS, in that order
// (Image.cpp:936-954).  tables: Y-DC, Y-AC, C-DC, C-AC.  restart_mcus > 0 adds a DRI
// segment before SOS, s444 declares Y 1x1 (both not in the reference).
std::vector<uint8_t> jfif_headers(uint32_t real_width, uint32_t real_height, const uint8_t qy[64],
                                  const uint8_t qc[64], const HuffTable* const tables[4], uint32_t restart_mcus = 0,
                                  uint8_t ysamp = 0x22);
// The one-component (grayscale) stream's headers: SOI, APP0, DQT(luma), SOF0 with the one
// component 1x1 on table 0, DHT x2 (tables[0] Y-DC, tables[1] Y-AC), DRI if restart_mcus > 0
// (the interval counts blocks: a non-interleaved scan's MCU is one block, ITU T.81 A.2.2),
// and a one-component SOS.
std::vector<uint8_t> jfif_headers_gray(uint32_t real_width, uint32_t real_height, const uint8_t qy[64],
                                       const HuffTable* const tables[2], uint32_t restart_mcus = 0);

// ---- fixed Huffman tables (jpge_set_huffman; an addition, nothing in the reference) ----
// A table in DHT form, as jpge_huff_spec: bits[l - 1] codes of length l, then the symbols.
struct HuffSpec {
    uint8_t bits[16];
    uint8_t huffval[256];
};
// ITU T.81 Annex K tables K.3 (luminance DC), K.5 (luminance AC), K.4 (chrominance DC) and
// K.6 (chrominance AC), in the library's table order Y-DC, Y-AC, C-DC, C-AC.
extern const HuffSpec kAnnexKHuffman[4];
// A table the encoder may code any 8-bit baseline frame with, without looking at the frame:
// at most 256 symbols, none twice, Kraft sum (sum of bits[l-1] * 2^(16-l)) below 2^16 (so no
// code is all ones, T.81 C.2), and complete: a DC table (ac = false) holds categories
// 0..11, an AC table 0x00, 0xF0 and every run 0..15 x size 1..10.
bool huff_spec_valid(const HuffSpec& spec, bool ac);
// jpge_set_huffman's argument check: kOk, or kErrArg for an unknown mode, mode 2 (the
// caller's tables) without specs, or a spec of it that is not valid (specs 1 and 3 are AC).
int huff_setting_check(int mode, const HuffSpec* specs);
// Canonical codes (T.81 Annex C, figures C.1-C.3) of a valid spec: codes of one length
// count up in huffval order, and the first code of a length is the last one of the shorter
// length, plus one, shifted left.
void huff_spec_table(const HuffSpec& spec, HuffTable& out);

// ---- sample transform of Y, Cb, Cr input (jpge_set_yuv_transform; an addition) ----
// jpge_yuv_transform, the same layout.  With bytes (y, cb, cr) of a pixel, yc = y - y_off,
// u = cb - 128, v = cr - 128 (exact), the planes that enter the pipeline are
//   Y'  = min(max((m0 yc + m1 u) + m2 v, 0), 255) - 128
//   Cb' = min(max(m3 u + m4 v, -128), 127),  Cr' = min(max(m5 u + m6 v, -128), 127)
// every product and sum rounded to fp64 on its own, in this order (K1, fdct.hip XfK).
struct YuvXf {
    double y_off = 0;
    double m[7] = {1, 0, 0, 1, 0, 0, 1};
};
constexpr int kYuvFull601 = 0, kYuvLimited601 = 1, kYuvLimited709 = 2, kYuvFull709 = 3, kYuvCustom = 4;
// A preset's coefficients (false: no such preset; kYuvCustom has none).
bool yuv_preset(int preset, YuvXf& t);
// jpge_set_yuv_transform's argument check and the setting's coefficients: kOk, or kErrArg
// for an unknown preset, kYuvCustom without a struct, a non-finite value, y_off outside
// 0..255 or an |m[i]| above 4.
int yuv_setting_check(int preset, const YuvXf* custom, YuvXf& t);

// Deterministic synthetic RGB8 frame (integer-only, identical on every host):
// kind 0 = smooth gradients + texture + noise (photo-like), 1 = uniform random
// bytes (worst-case symbol statistics), 2 = flat colour.
void synth_rgb8(uint64_t seed, uint32_t width, uint32_t height, int kind, uint8_t* out, size_t stride);

}  // namespace jpge
