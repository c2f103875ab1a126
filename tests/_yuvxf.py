"""Helpers of the sample-transform tests (jpge.h jpge_set_yuv_transform): the fp64 planes a
frame of 8-bit Y, Cb, Cr samples stands for under a transform t = (y_off, m0, ..., m6), by the
three lines of jpge.h restated with numpy (separate multiplications and additions on arrays,
np.clip, nothing fused), in _yuv.pad_planes' form, so that _yuv.want_coeffs and
Encoder.encode_planes give the expected coefficients and files as they do for the
untransformed layouts.  The coefficients are always the ones the library returned
(jpgenc_amd.yuv_preset) or was given.  test_yuvxf_cpu.py checks this file against
_yuv.pad_planes (identity), the clamps, and the presets against an independent derivation."""

import numpy as np

import _gray
import _yuv
import jpgenc_amd as J

GRAY = J.JPGE_FMT_GRAY8
IDENTITY = (0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0)
#: a custom transform with all eight entries non-trivial (inside the accepted ranges)
CUSTOM = (11.5, 1.0625, -0.21, 0.173, 0.93, 0.087, -0.119, 1.21)
PRESETS = {"limited601": J.JPGE_YUV_LIMITED_601, "limited709": J.JPGE_YUV_LIMITED_709, "full709": J.JPGE_YUV_FULL_709}


def coeffs(name: str):
    """(preset, coefficients or None for set_yuv_transform, the eight coefficients in force)."""
    if name == "custom":
        return J.JPGE_YUV_CUSTOM, CUSTOM, CUSTOM
    if name == "identity":
        return J.JPGE_YUV_CUSTOM, IDENTITY, IDENTITY
    return PRESETS[name], None, J.yuv_preset(PRESETS[name])


def luma(y, u, v, t):
    """Y' of byte arrays y and centred chroma u, v (fp64): every product and sum on its own."""
    y_off, m0, m1, m2 = (float(x) for x in t[:4])
    yc = np.asarray(y, np.float64) - y_off
    if u is None:  # one component: y_off and m0 only
        s = m0 * yc
    else:
        a = m0 * yc
        b = m1 * u
        c = m2 * v
        s = a + b
        s = s + c
    return np.clip(s, 0.0, 255.0) - 128.0


def chroma(u, v, ku, kv):
    a = float(ku) * u
    b = float(kv) * v
    return np.clip(a + b, -128.0, 127.0)


def planes(fmt: int, y, cb, cr, t, mcu=(16, 16)):
    """The fp64 planes [Y', Cb', Cr'] (full size, whole MCUs) of a frame under transform t, in
    _yuv.pad_planes' form: the samples are edge-replicated first (the 4:2:0 layouts' chroma
    in the chroma domain, then repeated 2x2, so that a pixel sees its cell's chroma) and then
    converted pixel by pixel; replication and a per-pixel map commute.  GRAY8 (cb, cr None):
    [Y'] alone, replicated to whole mcu = (8, 8) blocks."""
    if fmt == GRAY:
        b = _yuv.pad_planes(_yuv.YUV444, y, y, y, mcu=(8, 8))[0] + 128.0  # the padded bytes
        return [luma(b, None, None, t)]
    yb, u, v = _yuv.pad_planes(fmt, y, cb, cr, mcu=mcu)  # samples - 128, replicated
    return [luma(yb + 128.0, u, v, t), chroma(u, v, t[4], t[5]), chroma(u, v, t[6], t[7])]


def gray_file(y, t, qy, restart: int = 0) -> _gray.Built:
    """_gray.build of an (h, w) uint8 plane under transform t: the builder takes its fp64
    plane from _gray.pad, which is pointed at the transformed plane for the call (everything
    after the plane is the builder's own)."""
    yplane = planes(GRAY, y, None, None, t)[0]
    saved = _gray.pad
    _gray.pad = lambda _plane: yplane
    try:
        return _gray.build(np.ascontiguousarray(y, np.uint8), qy, restart)
    finally:
        _gray.pad = saved


# ---- an independent derivation of the presets (numpy only) ----
def _matrix(kr: float, kb: float) -> np.ndarray:
    """RGB -> Y, Cb, Cr for luma weights (kr, 1 - kr - kb, kb), full range, centred chroma."""
    kg = 1.0 - kr - kb
    return np.array([[kr, kg, kb],
                     [-kr / (2 * (1 - kb)), -kg / (2 * (1 - kb)), 0.5],
                     [0.5, -kg / (2 * (1 - kr)), -kb / (2 * (1 - kr))]], np.float64)


A601 = _matrix(0.299, 0.114)
A709 = _matrix(0.2126, 0.0722)


def derived(preset: int):
    """(y_off, m0..m6) of a preset from A601 . inv(A709), 255/219 and 255/224."""
    limited = preset in (J.JPGE_YUV_LIMITED_601, J.JPGE_YUV_LIMITED_709)
    m = A601 @ np.linalg.inv(A709) if preset in (J.JPGE_YUV_LIMITED_709, J.JPGE_YUV_FULL_709) else np.eye(3)
    sy, sc = (255.0 / 219.0, 255.0 / 224.0) if limited else (1.0, 1.0)
    return (16.0 if limited else 0.0, m[0, 0] * sy, m[0, 1] * sc, m[0, 2] * sc, m[1, 1] * sc, m[1, 2] * sc,
            m[2, 1] * sc, m[2, 2] * sc), m
