// Fixed Huffman tables (jpge_set_huffman), host side: the spec validation, the argument
// check of a setting, and the canonical code assignment (host_io.cpp).  Stand-alone: it
// links host_io.cpp only and touches no GPU.  Built plain (tests/cpp/bin/test_huffspec) and
// with -fsanitize=address,undefined (tests/cpp/bin/asan/test_huffspec, `make asan`);
// tests/test_fixedhuff_cpu.py runs both.
//
// Prints one "ok <case>" or "FAIL <case>" line per case, then "<n> cases, <m> failed".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "host_io.hpp"

using jpge::HuffSpec;
using jpge::HuffTable;

static int g_cases = 0, g_fail = 0;
static void report(const char* name, bool ok) {
    ++g_cases;
    if (!ok) ++g_fail;
    std::printf("%s %s\n", ok ? "ok" : "FAIL", name);
}

static int nsym(const HuffSpec& s) {
    int n = 0;
    for (int l = 0; l < 16; ++l) n += s.bits[l];
    return n;
}

// the four Annex K tables as a caller's tables
static void annex_k(HuffSpec out[4]) {
    for (int t = 0; t < 4; ++t) out[t] = jpge::kAnnexKHuffman[t];
}

static bool rejected(const HuffSpec specs[4]) { return jpge::huff_setting_check(2, specs) == jpge::kErrArg; }

// Canonical codes of a valid spec: prefix-free, none all ones, lengths as the spec says,
// codes of one length consecutive in huffval order.
static bool codes_ok(const HuffSpec& s) {
    HuffTable t;
    jpge::huff_spec_table(s, t);
    const int n = nsym(s);
    if (t.nsym != n) return false;
    int k = 0;
    for (int l = 1; l <= 16; ++l)
        for (int i = 0; i < s.bits[l - 1]; ++i, ++k) {
            const uint8_t sym = s.huffval[k];
            if (t.len[sym] != l || t.huffval[k] != sym) return false;
            if (t.code[sym] == (1u << l) - 1u) return false;  // all ones
            if (i > 0 && t.code[sym] != t.code[s.huffval[k - 1]] + 1) return false;
        }
    for (int a = 0; a < n; ++a)
        for (int b = 0; b < n; ++b) {
            if (a == b) continue;
            const uint8_t x = s.huffval[a], y = s.huffval[b];
            if (t.len[x] <= t.len[y] && (t.code[y] >> (t.len[y] - t.len[x])) == t.code[x]) return false;  // x prefixes y
        }
    return true;
}

int main() {
    HuffSpec sp[4];

    // Annex K itself: valid, with the code lengths ITU T.81 prints for it
    annex_k(sp);
    report("annexk_valid", jpge::huff_setting_check(2, sp) == jpge::kOk && jpge::huff_setting_check(1, nullptr) == jpge::kOk &&
                               jpge::huff_setting_check(0, nullptr) == jpge::kOk);
    {
        bool ok = true;
        for (int t = 0; t < 4; ++t) ok = ok && codes_ok(sp[t]);
        HuffTable t;
        jpge::huff_spec_table(sp[1], t);
        // K.5: EOB 1010 (4 bits), 0/1 00 (2 bits), ZRL 11111111001 (11 bits), F/A 1111111111111110
        ok = ok && t.len[0x00] == 4 && t.code[0x00] == 0xA && t.len[0x01] == 2 && t.code[0x01] == 0 &&
             t.len[0xF0] == 11 && t.code[0xF0] == 0x7F9 && t.len[0xFA] == 16 && t.code[0xFA] == 0xFFFE;
        jpge::huff_spec_table(sp[0], t);
        // K.3: category 0 00, category 11 111111110
        ok = ok && t.len[0] == 2 && t.code[0] == 0 && t.len[11] == 9 && t.code[11] == 0x1FE;
        report("annexk_codes", ok);
    }

    // an incomplete AC table: one run/size pair (5/7) missing
    annex_k(sp);
    {
        HuffSpec& s = sp[1];
        const int n = nsym(s);
        int at = -1;
        for (int i = 0; i < n; ++i)
            if (s.huffval[i] == 0x57) at = i;
        bool ok = at >= 0;
        if (ok) {
            std::memmove(s.huffval + at, s.huffval + at + 1, (size_t)(n - at - 1));
            s.huffval[n - 1] = 0;
            s.bits[15] -= 1;  // (0x57 has a 16-bit code in K.5)
            ok = rejected(sp);
        }
        report("reject_incomplete_ac", ok);
    }
    // a DC table without category 11
    annex_k(sp);
    sp[2].bits[10] = 0;  // (K.4: category 11 is the one 11-bit code, the last symbol)
    report("reject_dc_without_11", nsym(sp[2]) == 11 && rejected(sp));
    // a repeated symbol
    annex_k(sp);
    sp[3].huffval[7] = sp[3].huffval[3];
    report("reject_repeated_symbol", rejected(sp));
    // Kraft sum exactly 2^16: K.3's 12 symbols as 4 codes of 3 bits and 8 of 4 bits
    annex_k(sp);
    std::memset(sp[0].bits, 0, 16);
    sp[0].bits[2] = 4;
    sp[0].bits[3] = 8;
    report("reject_kraft_full", nsym(sp[0]) == 12 && rejected(sp));
    // ... and one step below it (the last code 1110, not all ones) is accepted
    sp[0].bits[3] = 7;
    sp[0].bits[4] = 1;
    report("accept_kraft_below_full", jpge::huff_setting_check(2, sp) == jpge::kOk && codes_ok(sp[0]));
    // more than 256 symbols
    annex_k(sp);
    sp[1].bits[15] = 255;  // (162 - 125 + 255 = 292)
    report("reject_over_256_symbols", nsym(sp[1]) > 256 && rejected(sp));
    // an unknown mode; the caller's tables without specs
    annex_k(sp);
    report("reject_unknown_mode", jpge::huff_setting_check(3, sp) == jpge::kErrArg &&
                                      jpge::huff_setting_check(-1, sp) == jpge::kErrArg);
    report("reject_custom_null", jpge::huff_setting_check(2, nullptr) == jpge::kErrArg);
    // a DC spec in an AC slot (and the reverse) is incomplete there
    annex_k(sp);
    sp[1] = sp[0];
    report("reject_dc_in_ac_slot", rejected(sp));

    // accepted: complete tables whose longest codes are 16 bits: all 256 byte symbols, one
    // code each of lengths 1..8 and 248 of length 16 (Kraft 2^16 - 2^8 + 248)
    {
        HuffSpec s;
        std::memset(&s, 0, sizeof s);
        for (int l = 0; l < 8; ++l) s.bits[l] = 1;
        s.bits[15] = 248;
        for (int i = 0; i < 256; ++i) s.huffval[i] = (uint8_t)i;
        for (int t = 0; t < 4; ++t) sp[t] = s;
        HuffTable t;
        jpge::huff_spec_table(s, t);
        report("accept_16_bit_codes", jpge::huff_setting_check(2, sp) == jpge::kOk && codes_ok(s) && t.len[255] == 16 &&
                                          t.len[0] == 1 && t.nsym == 256);
    }

    // random specs (valid or not): the validation and, for the valid ones, the code
    // assignment read nothing out of bounds and agree with a direct check
    {
        std::mt19937_64 rng(5);
        bool ok = true;
        int valid = 0;
        for (int it = 0; it < 4000 && ok; ++it) {
            HuffSpec s;
            std::memset(&s, 0, sizeof s);
            const bool ac = rng() & 1;
            if (it % 4 == 0) {  // any bytes
                for (int l = 0; l < 16; ++l) s.bits[l] = (uint8_t)rng();
                for (int i = 0; i < 256; ++i) s.huffval[i] = (uint8_t)rng();
            } else {  // a shuffled complete symbol set with random lengths under the Kraft limit
                std::vector<uint8_t> syms;
                if (ac) {
                    syms = {0x00, 0xF0};
                    for (int r = 0; r < 16; ++r)
                        for (int z = 1; z <= 10; ++z) syms.push_back((uint8_t)((r << 4) | z));
                } else {
                    for (int c = 0; c <= 11; ++c) syms.push_back((uint8_t)c);
                }
                for (size_t i = syms.size(); i > 1; --i) std::swap(syms[i - 1], syms[rng() % i]);
                uint32_t room = (1u << 16) - 1;
                std::vector<int> lens;
                for (size_t i = 0; i < syms.size(); ++i) {
                    int l = (int)(rng() % 16) + 1;
                    while (l < 16 && (1u << (16 - l)) + (uint32_t)(syms.size() - i - 1) > room) ++l;
                    if ((1u << (16 - l)) > room) break;
                    room -= 1u << (16 - l);
                    lens.push_back(l);
                }
                int k = 0;
                for (int l = 1; l <= 16; ++l)
                    for (size_t i = 0; i < lens.size(); ++i)
                        if (lens[i] == l) {
                            s.bits[l - 1]++;
                            s.huffval[k++] = syms[i];
                        }
                if (it % 16 == 1) s.huffval[rng() % 12] = (uint8_t)rng();  // (may repeat or drop a symbol)
            }
            const bool v = jpge::huff_spec_valid(s, ac);
            if (v) {
                ++valid;
                ok = ok && codes_ok(s);
            }
        }
        report("random_specs", ok && valid > 1000);
    }

    std::printf("%d cases, %d failed\n", g_cases, g_fail);
    return g_fail ? 1 : 0;
}
