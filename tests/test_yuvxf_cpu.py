"""The sample transform of Y, Cb, Cr input (jpge_set_yuv_transform), the parts that need no GPU:

- jpge_yuv_preset against an independent numpy derivation (the BT.601 and BT.709 luma
  weights, A601 . inv(A709), 255/219 and 255/224), and its direction: limited-range BT.709
  samples of an RGB colour come back as that colour through JFIF's inverse;
- tests/_yuvxf.py, the GPU tests' source of expected planes: with the identity it is
  _yuv.pad_planes bit for bit, and its clamps are the ones jpge.h words;
- the setting's validation, in a stand-alone host program (tests/cpp/test_yuvxf.cpp), plain
  and under AddressSanitizer + UBSan;
- the version, the constants and the exported names.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _yuv as Y
import _yuvxf as X
import jpgenc_amd as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = (J.JPGE_YUV_FULL_601, J.JPGE_YUV_LIMITED_601, J.JPGE_YUV_LIMITED_709, J.JPGE_YUV_FULL_709)


def test_version_constants_and_exports():
    assert J.lib().jpge_version() >= 103
    assert (J.JPGE_YUV_FULL_601, J.JPGE_YUV_LIMITED_601, J.JPGE_YUV_LIMITED_709, J.JPGE_YUV_FULL_709,
            J.JPGE_YUV_CUSTOM) == (0, 1, 2, 3, 4)
    for name in ("jpge_set_yuv_transform", "jpge_get_yuv_transform", "jpge_yuv_preset"):
        assert name in J.EXPORTS and hasattr(J.lib(), name)
    assert ctypes.sizeof(J.YuvTransform) == 64
    t = J.YuvTransform.from_tuple(X.CUSTOM)
    assert t.as_tuple() == X.CUSTOM
    with pytest.raises(ValueError):
        J.YuvTransform.from_tuple((0.0, 1.0))


# ---- the presets ----
@pytest.mark.parametrize("preset", ALL)
def test_presets_match_the_derivation(preset):
    # fp64 evaluation-order differences are of order 1e-16; a wrong constant is off by 1e-3 or more
    got = J.yuv_preset(preset)
    want, m = X.derived(preset)
    assert np.allclose(m[:, 0], (1.0, 0.0, 0.0), rtol=0, atol=1e-12)  # grey stays grey: seven entries carry the matrix
    assert len(got) == 8
    for g, w in zip(got, want):
        assert abs(g - w) <= 1e-12 * abs(w), (preset, got, want)


def test_preset_shapes():
    assert J.yuv_preset(J.JPGE_YUV_FULL_601) == X.IDENTITY
    lim = J.yuv_preset(J.JPGE_YUV_LIMITED_601)
    assert lim == (16.0, 255.0 / 219.0, 0.0, 0.0, 255.0 / 224.0, 0.0, 0.0, 255.0 / 224.0)
    assert J.yuv_preset(J.JPGE_YUV_LIMITED_709)[0] == 16.0 and J.yuv_preset(J.JPGE_YUV_FULL_709)[0] == 0.0
    for bad in (-1, J.JPGE_YUV_CUSTOM, 5, 99):
        with pytest.raises(J.JpgeError) as ei:
            J.yuv_preset(bad)
        assert ei.value.status == 1
    assert J.lib().jpge_yuv_preset(J.JPGE_YUV_FULL_709, None) == 1


def _jfif_inverse(y, cb, cr):
    """R, G, B of full-range BT.601 planes (Y in 0..255, centred chroma): inv(A601)."""
    return np.einsum("ij,j...->i...", np.linalg.inv(X.A601), np.stack([y, cb, cr]))


@pytest.mark.parametrize("preset", [J.JPGE_YUV_LIMITED_709, J.JPGE_YUV_FULL_709, J.JPGE_YUV_LIMITED_601])
def test_direction(preset):
    # an algebraic identity (rounding near 1e-13): in-gamut RGB -> the preset's Y, Cb, Cr in
    # fp64, unrounded -> the preset's three lines -> JFIF's inverse gives the RGB back
    # (colours a step inside the cube: JFIF's chroma interval [-128, 127] ends half a step short
    # of a fully saturated blue or red, 127.5, which the clamp would cut)
    rgb = np.random.default_rng(3).uniform(2.0, 253.0, (3, 4000))
    a = X.A709 if preset != J.JPGE_YUV_LIMITED_601 else X.A601
    ycc = a @ rgb
    if preset != J.JPGE_YUV_FULL_709:  # studio swing
        y, cb, cr = 16.0 + ycc[0] * 219.0 / 255.0, 128.0 + ycc[1] * 224.0 / 255.0, 128.0 + ycc[2] * 224.0 / 255.0
    else:
        y, cb, cr = ycc[0], 128.0 + ycc[1], 128.0 + ycc[2]
    t = J.yuv_preset(preset)
    u, v = cb - 128.0, cr - 128.0
    back = _jfif_inverse(X.luma(y, u, v, t) + 128.0, X.chroma(u, v, t[4], t[5]), X.chroma(u, v, t[6], t[7]))
    assert np.abs(back - rgb).max() < 1e-9


# ---- the helper ----
@pytest.mark.parametrize("fmt", Y.FORMATS, ids=[Y.NAMES[f] for f in Y.FORMATS])
@pytest.mark.parametrize("w,h", [(1, 1), (33, 17), (80, 32)])
def test_helper_identity_is_pad_planes(fmt, w, h):
    p = Y.samples(fmt, 5, w, h)
    for mcu in ((16, 16), (8, 8), (32, 8)) if fmt == Y.YUV444 else ((16, 16),):
        got, want = X.planes(fmt, *p, X.IDENTITY, mcu=mcu), Y.pad_planes(fmt, *p, mcu=mcu)
        assert all(g.dtype == np.float64 and g.tobytes() == w_.tobytes() for g, w_ in zip(got, want))


def test_helper_identity_gray():
    import _gray
    y = _gray.plane("random", 17, 9)
    (got,) = X.planes(X.GRAY, y, None, None, J.yuv_preset(J.JPGE_YUV_FULL_601))
    assert got.tobytes() == _gray.pad(y).tobytes()
    b = X.gray_file(y, X.IDENTITY, J.quality_tables(90)[0])
    assert b.jpg == _gray.built("random", 17, 9, 90).jpg and _gray.pad(y).shape == (16, 24)  # (pad is restored)


def test_clamping():
    t = J.yuv_preset(J.JPGE_YUV_LIMITED_601)
    b = np.array([[0, 15, 16, 235, 236, 255]], np.uint8)
    want = [-128.0, -128.0, -128.0, 127.0, 127.0, 127.0]
    z = np.full_like(b, 128)
    assert X.planes(X.GRAY, b, None, None, t)[0][0, :6].tolist() == want
    assert X.planes(Y.YUV444, b, z, z, t, mcu=(8, 8))[0][0, :6].tolist() == want
    # chroma: 16 and 240 are the ends of studio swing, and everything outside clamps
    c = np.array([[0, 15, 16, 240, 241, 255]], np.uint8)
    _, cb, cr = X.planes(Y.YUV444, z, c, c[:, ::-1].copy(), t, mcu=(8, 8))
    lo = 255.0 / 224.0 * -112.0  # (-127.5 but for a rounding: inside the interval)
    assert -128.0 < lo < -127.0
    assert cb[0, :6].tolist() == [-128.0, -128.0, lo, 127.0, 127.0, 127.0]
    assert cr[0, :6].tolist() == [127.0, 127.0, 127.0, lo, -128.0, -128.0]
    # one step inside the range is not clamped
    assert X.planes(X.GRAY, np.array([[17, 234]], np.uint8), None, None, t)[0][0, :2].tolist() == [
        255.0 / 219.0 * 1.0 - 128.0, 255.0 / 219.0 * 218.0 - 128.0]


def test_custom_transform_uses_every_entry():
    p = Y.samples(Y.I420, 8, 33, 17)
    base = X.planes(Y.I420, *p, X.CUSTOM)
    for i in range(8):
        t = list(X.CUSTOM)
        t[i] += 0.03125
        other = X.planes(Y.I420, *p, t)
        changed = [not np.array_equal(a, b) for a, b in zip(base, other)]
        assert changed == [i < 4, i in (4, 5), i in (6, 7)], i


# ---- validation: the stand-alone host program ----
CASES = ("presets_accepted", "full601_identity", "limited601", "presets_709", "reject_unknown_preset", "reject_custom_null",
         "preset_ignores_struct", "accept_bounds", "reject_y_off", "reject_m", "accept_tiny")


@pytest.fixture(scope="module")
def yuvxf_plain():
    exe = os.path.join(ROOT, "tests", "cpp", "bin", "test_yuvxf")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout + r.stderr


@pytest.mark.parametrize("case", CASES)
def test_validation(yuvxf_plain, case):
    rc, out = yuvxf_plain
    assert f"ok {case}" in out.splitlines(), out[-2000:]
    assert rc == 0 and out.rstrip().endswith("all ok") and out.count("\nok ") + 1 == len(CASES), out[-2000:]


def test_validation_sanitized():
    # built as the other sanitized host programs are (make asan's flags), this one target only
    exe = os.path.join("tests", "cpp", "bin", "asan", "test_yuvxf")
    r = subprocess.run(["make", "-s", exe], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(ROOT, exe)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out, out[-6000:]
    assert r.returncode == 0 and "all ok" in out and "FAIL" not in out, out[-4000:]
