// jpge_set_yuv_transform's argument check and the presets (host_io.cpp yuv_setting_check,
// yuv_preset): host only, no GPU.  Built plain and under AddressSanitizer + UBSan;
// tests/test_yuvxf_cpu.py runs both and reads the "ok"/"FAIL" lines.
#include <cmath>
#include <cstdio>
#include <limits>

#include "host_io.hpp"

using jpge::YuvXf;

static int g_fail = 0;
static void report(const char* name, bool ok) {
    std::printf("%s %s\n", ok ? "ok" : "FAIL", name);
    if (!ok) ++g_fail;
}

static bool rejected(int preset, const YuvXf* c) {
    YuvXf t;
    t.y_off = -7.0;  // (a refused setting leaves no half-written result the caller would use)
    return jpge::yuv_setting_check(preset, c, t) == jpge::kErrArg;
}
static bool accepted(int preset, const YuvXf* c, YuvXf& t) { return jpge::yuv_setting_check(preset, c, t) == jpge::kOk; }

static bool same(const YuvXf& a, const YuvXf& b) {
    if (a.y_off != b.y_off) return false;
    for (int i = 0; i < 7; ++i)
        if (a.m[i] != b.m[i]) return false;
    return true;
}

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    YuvXf t, p;

    // the presets: every one accepted, and the setting carries the preset's coefficients
    {
        bool ok = true;
        for (int preset = jpge::kYuvFull601; preset <= jpge::kYuvFull709; ++preset)
            ok = ok && jpge::yuv_preset(preset, p) && accepted(preset, nullptr, t) && same(t, p);
        report("presets_accepted", ok);
    }
    // FULL_601 is the identity
    {
        const YuvXf id;
        report("full601_identity", jpge::yuv_preset(jpge::kYuvFull601, p) && same(p, id) && p.y_off == 0.0 && p.m[0] == 1.0 &&
                                       p.m[3] == 1.0 && p.m[6] == 1.0 && p.m[1] == 0.0 && p.m[2] == 0.0 && p.m[4] == 0.0 &&
                                       p.m[5] == 0.0);
    }
    // LIMITED_601: range expansion only
    report("limited601", jpge::yuv_preset(jpge::kYuvLimited601, p) && p.y_off == 16.0 && p.m[0] == 255.0 / 219.0 &&
                             p.m[3] == 255.0 / 224.0 && p.m[6] == 255.0 / 224.0 && p.m[1] == 0.0 && p.m[2] == 0.0 &&
                             p.m[4] == 0.0 && p.m[5] == 0.0);
    // the 709 presets: the limited one is the full one, scaled
    {
        YuvXf f, l;
        bool ok = jpge::yuv_preset(jpge::kYuvFull709, f) && jpge::yuv_preset(jpge::kYuvLimited709, l);
        ok = ok && f.y_off == 0.0 && l.y_off == 16.0 && f.m[0] == 1.0 && l.m[0] == 255.0 / 219.0;
        for (int i = 1; i < 7; ++i) ok = ok && std::fabs(l.m[i] - f.m[i] * (255.0 / 224.0)) <= 1e-15;
        ok = ok && std::fabs(f.m[1] - 0.1016) < 1e-3 && std::fabs(f.m[2] - 0.1961) < 1e-3 && std::fabs(f.m[3] - 0.9899) < 1e-3 &&
             std::fabs(f.m[4] + 0.1107) < 1e-3 && std::fabs(f.m[5] + 0.0725) < 1e-3 && std::fabs(f.m[6] - 0.9834) < 1e-3;
        report("presets_709", ok);
    }
    // no such preset; CUSTOM is no preset, and needs a struct
    report("reject_unknown_preset", rejected(-1, nullptr) && rejected(5, nullptr) && rejected(99, &p) &&
                                        !jpge::yuv_preset(jpge::kYuvCustom, p) && !jpge::yuv_preset(-1, p) &&
                                        !jpge::yuv_preset(5, p));
    report("reject_custom_null", rejected(jpge::kYuvCustom, nullptr));
    // a preset ignores the struct
    {
        YuvXf bad;
        bad.y_off = nan;
        report("preset_ignores_struct", accepted(jpge::kYuvLimited709, &bad, t) && jpge::yuv_preset(jpge::kYuvLimited709, p) && same(t, p));
    }
    // CUSTOM: the bounds are inclusive
    {
        YuvXf c;
        c.y_off = 255.0;
        for (int i = 0; i < 7; ++i) c.m[i] = (i & 1) ? -4.0 : 4.0;
        bool ok = accepted(jpge::kYuvCustom, &c, t) && same(t, c);
        c.y_off = 0.0;
        ok = ok && accepted(jpge::kYuvCustom, &c, t) && same(t, c);
        report("accept_bounds", ok);
    }
    // y_off outside 0..255
    {
        YuvXf c;
        bool ok = true;
        for (const double v : {-1.0, -1e-9, 255.0000001, 256.0, 1e300, -inf, inf, nan}) {
            c.y_off = v;
            ok = ok && rejected(jpge::kYuvCustom, &c);
        }
        report("reject_y_off", ok);
    }
    // every m[i]: above 4 in magnitude, or not finite
    {
        bool ok = true;
        for (int i = 0; i < 7; ++i)
            for (const double v : {4.0000001, -4.0000001, 1e300, -1e300, inf, -inf, nan}) {
                YuvXf c;
                c.m[i] = v;
                ok = ok && rejected(jpge::kYuvCustom, &c);
            }
        report("reject_m", ok);
    }
    // denormals and signed zeros are finite values inside the bounds
    {
        YuvXf c;
        c.y_off = -0.0;
        c.m[1] = std::numeric_limits<double>::denorm_min();
        c.m[2] = -0.0;
        report("accept_tiny", accepted(jpge::kYuvCustom, &c, t));
    }
    std::printf("%s\n", g_fail ? "FAILED" : "all ok");
    return g_fail ? 1 : 0;
}
