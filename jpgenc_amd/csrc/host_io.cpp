#include "host_io.hpp"
#include "host_par.hpp"

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <thread>

namespace jpge {

const uint8_t kZigzagToNatural[64] = {
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5,
    12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
    58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

namespace {

// Tokenizer with the reference's exact behaviour (Image.cpp:349-389), bounds-checked.
class Tokens {
  public:
    Tokens(const uint8_t* p, size_t n) : p_(p), n_(n) {}
    size_t pos() const { return pos_; }
    uint8_t byte() { return pos_ < n_ ? p_[pos_++] : (pos_++, 0); }
    std::string word() {
        uint8_t c = byte();
        if (std::isspace(c)) {
            while (pos_ < n_ && std::isspace(p_[pos_])) ++pos_;
            c = byte();
        }
        size_t first = pos_ - 1;
        for (;;) {
            if (c == '#') {
                while (pos_ < n_ && p_[pos_++] != '\n') {}
                first = pos_;
            } else if (std::isspace(c)) {
                return std::string(reinterpret_cast<const char*>(p_) + first, pos_ - 1 - first);
            } else if (pos_ >= n_) {
                size_t end = std::min(pos_, n_);
                return first < end ? std::string(reinterpret_cast<const char*>(p_) + first, end - first)
                                   : std::string();
            }
            c = byte();
        }
    }

  private:
    const uint8_t* p_;
    size_t n_, pos_ = 0;
};

bool to_int(const std::string& s, long& v) {
    if (s.empty()) return false;
    char* end = nullptr;
    v = std::strtol(s.c_str(), &end, 10);
    return end != s.c_str();
}

const uint8_t kLuma[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55,
                           14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                           18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                           49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const uint8_t kChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99,
                             24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                             99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                             99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

void put16(std::vector<uint8_t>& o, uint32_t v) {
    o.push_back((uint8_t)(v >> 8));
    o.push_back((uint8_t)v);
}

// splitmix64 (integer-only PRNG so the frames are identical on every host).
inline uint64_t mix(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

inline int tri(int x, int period) {  // triangle wave 0..255
    int p = x % period;
    if (p < 0) p += period;
    int h = period / 2;
    return (p < h ? p : period - p) * 255 / (h ? h : 1);
}

// loadP3PPM's fast_atoi (Image.cpp:393-408): digits accumulated without validation.
// The reference's int overflows (undefined) on long tokens; here an accumulator that
// leaves +-2^40 stops at -1, which every caller rejects as out of range, and every
// token that stays inside that range gets the reference's value.
inline long fast_atoi(const std::string& wd) {
    long v = 0;
    for (char c : wd) {
        v = v * 10 + (c - '0');
        if (v > (1l << 40) || v < -(1l << 40)) return -1;
    }
    return v;
}

}  // namespace

int parse_ppm(const uint8_t* buf, size_t n, PpmImage& out) {
    Tokens t(buf, n);
    std::string magic = t.word();
    if (magic != "P3" && magic != "P6") return kErrFormat;
    long w = 0, h = 0, mv = 0;
    if (!to_int(t.word(), w) || !to_int(t.word(), h) || !to_int(t.word(), mv)) return kErrFormat;
    if (w <= 0 || h <= 0 || w > 65535 || h > 65535) return kErrFormat;
    if (mv < 1 || mv > 255) return kErrRange;  // Image.cpp:462 asserts maxval < 256
    out.width = (uint32_t)w;
    out.height = (uint32_t)h;
    out.maxval = (int)mv;
    const size_t cnt = (size_t)w * (size_t)h * 3;
    out.rgb.resize(cnt);
    if (magic == "P6") {  // loadP6PPM, Image.cpp:411-418
        if (t.pos() + cnt > n) return kErrTruncated;
        std::memcpy(out.rgb.data(), buf + t.pos(), cnt);
        for (size_t i = 0; i < cnt; ++i)
            if (out.rgb[i] > mv) return kErrRange;
    } else {  // loadP3PPM, Image.cpp:393-408 (fast_atoi, no validation)
        for (size_t i = 0; i < cnt; ++i) {
            std::string wd = t.word();
            if (wd.empty() && t.pos() >= n) return kErrTruncated;
            const long v = fast_atoi(wd);
            if (v < 0 || v > mv) return kErrRange;
            out.rgb[i] = (uint8_t)v;
        }
    }
    return kOk;
}

int parse_ppm_inplace(uint8_t* buf, size_t n, uint32_t& width, uint32_t& height, int& maxval, size_t& offset) {
    Tokens t(buf, n);
    std::string magic = t.word();
    if (magic != "P3" && magic != "P6") return kErrFormat;
    long w = 0, h = 0, mv = 0;
    if (!to_int(t.word(), w) || !to_int(t.word(), h) || !to_int(t.word(), mv)) return kErrFormat;
    if (w <= 0 || h <= 0 || w > 65535 || h > 65535) return kErrFormat;
    if (mv < 1 || mv > 255) return kErrRange;
    width = (uint32_t)w;
    height = (uint32_t)h;
    maxval = (int)mv;
    const size_t cnt = (size_t)w * (size_t)h * 3;
    if (magic == "P6") {  // loadP6PPM, Image.cpp:411-418: the samples are the frame
        if (t.pos() + cnt > n) return kErrTruncated;
        offset = t.pos();
        if (mv < 255)
            for (size_t i = 0; i < cnt; ++i)
                if (buf[offset + i] > mv) return kErrRange;
        return kOk;
    }
    // loadP3PPM, Image.cpp:393-408: sample i is written over the text at byte i, which
    // the tokenizer has passed (every earlier sample took >= 2 characters)
    for (size_t i = 0; i < cnt; ++i) {
        std::string wd = t.word();
        if (wd.empty() && t.pos() >= n) return kErrTruncated;
        const long v = fast_atoi(wd);
        if (v < 0 || v > mv) return kErrRange;
        buf[i] = (uint8_t)v;
    }
    offset = 0;
    return kOk;
}

int load_ppm_file(const std::string& path, PpmImage& out) {
    std::ifstream f(path, std::ios::binary);
    if (!f.is_open()) return kErrIo;
    std::vector<uint8_t> buf((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    return parse_ppm(buf.data(), buf.size(), out);
}

void quality_tables(int q, uint8_t qy[64], uint8_t qc[64]) {
    q = std::min(100, std::max(1, q));
    const int s = q < 50 ? 5000 / q : 200 - 2 * q;
    for (int i = 0; i < 64; ++i) {
        qy[i] = (uint8_t)std::min(255, std::max(1, (kLuma[i] * s + 50) / 100));
        qc[i] = (uint8_t)std::min(255, std::max(1, (kChroma[i] * s + 50) / 100));
    }
}

// sSOI + sAPP0 (JpegSegments.hpp:55-109): JFIF 1.1, no units, density 1x1.
static const uint8_t kSoiApp0[20] = {0xFF, 0xD8, 0xFF, 0xE0, 0x00, 0x10, 'J', 'F', 'I', 'F',
                                     0x00, 0x01, 0x01, 0x00, 0x00, 0x01, 0x00, 0x01, 0x00, 0x00};

std::vector<uint8_t> jfif_headers(uint32_t rw, uint32_t rh, const uint8_t qy[64], const uint8_t qc[64],
                                  const HuffTable* const tables[4], uint32_t restart_mcus, uint8_t ysamp) {
    std::vector<uint8_t> o;
    o.reserve(700);
    o.insert(o.end(), kSoiApp0, kSoiApp0 + 20);
    // sDQT x2 (JpegSegments.hpp:259-319): one table per segment, zig-zag order.
    const uint8_t* qt[2] = {qy, qc};
    for (int id = 0; id < 2; ++id) {
        o.push_back(0xFF); o.push_back(0xDB); put16(o, 67); o.push_back((uint8_t)id);
        for (int i = 0; i < 64; ++i) o.push_back(qt[id][kZigzagToNatural[i]]);
    }
    // sSOF0 (JpegSegments.hpp:112-164): height before width, unpadded size;
    // Y 2x2 on table 0, Cb/Cr 1x1 on table 1 (Image.cpp:940-945); the other
    // subsampling modes declare Y as ysamp = (H << 4) | V.
    o.push_back(0xFF); o.push_back(0xC0); put16(o, 17); o.push_back(8);
    put16(o, rh & 0xFFFF); put16(o, rw & 0xFFFF);
    const uint8_t comp[10] = {3, 1, ysamp, 0, 2, 0x11, 1, 3, 0x11, 1};
    o.insert(o.end(), comp, comp + 10);
    // sDHT x4 (JpegSegments.hpp:167-256), Image.cpp:946-949.
    static const uint8_t kInfo[4] = {0x00, 0x10, 0x01, 0x11};
    for (int k = 0; k < 4; ++k) {
        const HuffTable& t = *tables[k];
        o.push_back(0xFF); o.push_back(0xC4); put16(o, (uint32_t)(2 + 17 + t.nsym)); o.push_back(kInfo[k]);
        for (int l = 1; l <= 16; ++l) o.push_back(t.bits[l]);
        o.insert(o.end(), t.huffval, t.huffval + t.nsym);
    }
    if (restart_mcus) {  // DRI (ITU T.81 B.2.4.4): restart interval in MCUs
        o.push_back(0xFF); o.push_back(0xDD); put16(o, 4); put16(o, restart_mcus & 0xFFFF);
    }
    // sSOS (JpegSegments.hpp:322-358): Y tables 0/0, Cb and Cr 1/1, Ss 0 Se 63 AhAl 0.
    static const uint8_t kSos[14] = {0xFF, 0xDA, 0x00, 0x0C, 0x03, 0x01, 0x00, 0x02, 0x11, 0x03, 0x11, 0x00, 0x3F, 0x00};
    o.insert(o.end(), kSos, kSos + 14);
    return o;
}

std::vector<uint8_t> jfif_headers_gray(uint32_t rw, uint32_t rh, const uint8_t qy[64],
                                       const HuffTable* const tables[2], uint32_t restart_mcus) {
    // SOI, APP0 and the luma DQT as in jfif_headers; SOF0, the two DHTs and SOS for one
    // component (1x1, quantiser 0, tables 0/0)
    std::vector<uint8_t> o;
    o.reserve(400);
    o.insert(o.end(), kSoiApp0, kSoiApp0 + 20);
    o.push_back(0xFF); o.push_back(0xDB); put16(o, 67); o.push_back(0);
    for (int i = 0; i < 64; ++i) o.push_back(qy[kZigzagToNatural[i]]);
    o.push_back(0xFF); o.push_back(0xC0); put16(o, 11); o.push_back(8);
    put16(o, rh & 0xFFFF); put16(o, rw & 0xFFFF);
    const uint8_t comp[4] = {1, 1, 0x11, 0};
    o.insert(o.end(), comp, comp + 4);
    static const uint8_t kInfo[2] = {0x00, 0x10};
    for (int k = 0; k < 2; ++k) {
        const HuffTable& t = *tables[k];
        o.push_back(0xFF); o.push_back(0xC4); put16(o, (uint32_t)(2 + 17 + t.nsym)); o.push_back(kInfo[k]);
        for (int l = 1; l <= 16; ++l) o.push_back(t.bits[l]);
        o.insert(o.end(), t.huffval, t.huffval + t.nsym);
    }
    if (restart_mcus) {
        o.push_back(0xFF); o.push_back(0xDD); put16(o, 4); put16(o, restart_mcus & 0xFFFF);
    }
    static const uint8_t kSos[10] = {0xFF, 0xDA, 0x00, 0x08, 0x01, 0x01, 0x00, 0x00, 0x3F, 0x00};
    o.insert(o.end(), kSos, kSos + 10);
    return o;
}

// ITU T.81 Annex K, tables K.3, K.5, K.4, K.6 (BITS and HUFFVAL as the standard lists them).
const HuffSpec kAnnexKHuffman[4] = {
    {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
     {0x00, 0x01, 0x02, 0x03, 0x04, 0x05, 0x06, 0x07, 0x08, 0x09, 0x0A, 0x0B}},
    {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125},
     {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
      0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0,
      0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28,
      0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
      0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
      0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
      0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7,
      0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5,
      0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2,
      0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8,
      0xF9, 0xFA}},
    {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
     {0x00, 0x01, 0x02, 0x03, 0x04, 0x05, 0x06, 0x07, 0x08, 0x09, 0x0A, 0x0B}},
    {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119},
     {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
      0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0,
      0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26,
      0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
      0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
      0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
      0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5,
      0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3,
      0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA,
      0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8,
      0xF9, 0xFA}},
};

bool huff_spec_valid(const HuffSpec& spec, bool ac) {
    uint32_t n = 0, kraft = 0;
    for (int l = 1; l <= 16; ++l) {
        n += spec.bits[l - 1];
        kraft += (uint32_t)spec.bits[l - 1] << (16 - l);
    }
    if (n > 256 || kraft >= (1u << 16)) return false;
    bool have[256] = {};
    for (uint32_t i = 0; i < n; ++i) {
        if (have[spec.huffval[i]]) return false;
        have[spec.huffval[i]] = true;
    }
    if (!ac) {
        for (int c = 0; c <= 11; ++c)
            if (!have[c]) return false;
        return true;
    }
    if (!have[0x00] || !have[0xF0]) return false;
    for (int run = 0; run < 16; ++run)
        for (int size = 1; size <= 10; ++size)
            if (!have[(run << 4) | size]) return false;
    return true;
}

int huff_setting_check(int mode, const HuffSpec* specs) {
    if (mode < 0 || mode > 2) return kErrArg;
    if (mode != 2) return kOk;  // (specs are read for the caller's tables only)
    if (!specs) return kErrArg;
    for (int t = 0; t < 4; ++t)
        if (!huff_spec_valid(specs[t], (t & 1) != 0)) return kErrArg;
    return kOk;
}

// The presets of the sample transform.  With luma weights (kr, kb), kg = 1 - kr - kb, a
// matrix's Y, Cb, Cr are Y = kr R + kg G + kb B, Cb = (B - Y) / (2 (1 - kb)),
// Cr = (R - Y) / (2 (1 - kr)).  A *_709 preset carries A601 . inverse(A709): both matrices
// send grey to (Y, 0, 0), so its first column is (1, 0, 0) and seven entries remain, the
// images of a unit of BT.709 Cb and of Cr.  Studio swing stores 219 Y / 255 + 16 and
// 224 C / 255 + 128: y_off 16, the Y column scaled by 255/219, the chroma columns by 255/224.
bool yuv_preset(int preset, YuvXf& t) {
    if (preset < kYuvFull601 || preset > kYuvFull709) return false;
    const bool limited = preset == kYuvLimited601 || preset == kYuvLimited709;
    const bool from709 = preset == kYuvLimited709 || preset == kYuvFull709;
    const double sy = limited ? 255.0 / 219.0 : 1.0, sc = limited ? 255.0 / 224.0 : 1.0;
    t = YuvXf();
    t.y_off = limited ? 16.0 : 0.0;
    t.m[0] = sy;
    t.m[3] = t.m[6] = sc;
    if (from709) {
        const double kr6 = 0.299, kb6 = 0.114, kg6 = 1.0 - kr6 - kb6;
        const double kr9 = 0.2126, kb9 = 0.0722, kg9 = 1.0 - kr9 - kb9;
        // R, G, B of a unit of BT.709 Cb, then of Cr
        const double rgb[2][3] = {{0.0, -2.0 * kb9 * (1.0 - kb9) / kg9, 2.0 * (1.0 - kb9)},
                                  {2.0 * (1.0 - kr9), -2.0 * kr9 * (1.0 - kr9) / kg9, 0.0}};
        for (int c = 0; c < 2; ++c) {
            const double y = kr6 * rgb[c][0] + kg6 * rgb[c][1] + kb6 * rgb[c][2];
            t.m[1 + c] = y * sc;
            t.m[3 + c] = (rgb[c][2] - y) / (2.0 * (1.0 - kb6)) * sc;
            t.m[5 + c] = (rgb[c][0] - y) / (2.0 * (1.0 - kr6)) * sc;
        }
    }
    return true;
}

int yuv_setting_check(int preset, const YuvXf* custom, YuvXf& t) {
    if (preset == kYuvCustom) {
        if (!custom) return kErrArg;
        t = *custom;
    } else if (!yuv_preset(preset, t)) {
        return kErrArg;
    }
    // (the comparisons are false for a NaN)
    if (!(t.y_off >= 0.0 && t.y_off <= 255.0)) return kErrArg;
    for (const double m : t.m)
        if (!(std::fabs(m) <= 4.0)) return kErrArg;
    return kOk;
}

void huff_spec_table(const HuffSpec& spec, HuffTable& out) {
    out = HuffTable();
    uint32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        out.bits[l] = spec.bits[l - 1];
        for (int i = 0; i < spec.bits[l - 1] && k < 256; ++i, ++k) {
            const uint8_t s = spec.huffval[k];
            out.huffval[k] = s;
            out.code[s] = code++;
            out.len[s] = (uint8_t)l;
        }
        code <<= 1;
    }
    out.nsym = k;
}

namespace {
int synth_threads(uint32_t h) {  // test-data synthesis: a few threads for large frames
    const unsigned hw = std::thread::hardware_concurrency();
    return h < 256 ? 1 : (int)std::min(8u, hw ? hw : 1u);
}
}  // namespace

void synth_rgb8(uint64_t seed, uint32_t w, uint32_t h, int kind, uint8_t* out, size_t stride) {
    const uint64_t s = mix(seed);
    if (kind == 2) {
        const uint8_t c[3] = {(uint8_t)s, (uint8_t)(s >> 8), (uint8_t)(s >> 16)};
        for (uint32_t y = 0; y < h; ++y)
            for (uint32_t x = 0; x < w; ++x) std::memcpy(out + (size_t)y * stride + x * 3, c, 3);
        return;
    }
    const int px = (int)(s % 977) + 200, py = (int)((s >> 10) % 743) + 150;
    const int tx = (int)((s >> 20) % 23) + 9, ty = (int)((s >> 30) % 19) + 7;
    parallel_for((long)h, synth_threads(h), [&](long yy) {
        const int y = (int)yy;
        uint8_t* row = out + (size_t)y * stride;
        for (uint32_t xu = 0; xu < w; ++xu) {
            const int x = (int)xu;
            const uint64_t r = mix(s ^ ((uint64_t)y << 32) ^ (uint64_t)x);
            if (kind == 1) {
                row[x * 3] = (uint8_t)r; row[x * 3 + 1] = (uint8_t)(r >> 8); row[x * 3 + 2] = (uint8_t)(r >> 16);
                continue;
            }
            // approx. gaussian noise, sigma ~ 12: sum of 4 uniform bytes
            int noise = ((int)(r & 0xFF) + (int)((r >> 8) & 0xFF) + (int)((r >> 16) & 0xFF) + (int)((r >> 24) & 0xFF) - 510) / 6;
            int texture = ((x / tx + y / ty) & 1) ? 18 : -18;
            int v[3];
            v[0] = (tri(x, px) * 3 + tri(y, py)) / 4;
            v[1] = (tri(x + y, px + py) + tri(y * 2, py)) / 2;
            v[2] = (tri(x - y, px) + 255 - tri(y, py / 2 + 1)) / 2;
            for (int c = 0; c < 3; ++c) {
                int val = v[c] + noise + (c == 1 ? texture : texture / 2) + (int)((r >> (32 + 8 * c)) & 7) - 3;
                row[x * 3 + c] = (uint8_t)std::min(255, std::max(0, val));
            }
        }
    });
}

}  // namespace jpge
