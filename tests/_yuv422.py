"""Helpers of the 4:2:2 input-layout tests (jpge.h JPGE_FMT_YUYV, _UYVY, _NV16, _I422): the
layouts built with numpy (and taken apart again), and the chroma-repeated 4:4:4 planes that
define what such a frame means: the JPGE_FMT_YUV444_PLANAR frame whose chroma planes hold
c[y][x >> 1] at pixel (y, x).  Everything after that is _yuv.py's (pad_planes, want_coeffs)
and the oracle's.  test_yuv422_cpu.py checks the builders and the repeated planes, so the GPU
tests' expectations do not rest on unchecked code."""

import numpy as np

import _yuv
import jpgenc_amd as J

YUYV, UYVY, NV16, I422 = J.JPGE_FMT_YUYV, J.JPGE_FMT_UYVY, J.JPGE_FMT_NV16, J.JPGE_FMT_I422
FORMATS = (YUYV, UYVY, NV16, I422)
PACKED = (YUYV, UYVY)
NAMES = {YUYV: "yuyv", UYVY: "uyvy", NV16: "nv16", I422: "i422"}


def cw_of(w: int) -> int:
    return (w + 1) // 2


def least_stride(fmt: int, w: int) -> int:
    return {YUYV: 4 * cw_of(w), UYVY: 4 * cw_of(w), NV16: 2 * cw_of(w), I422: w}[fmt]


def repeat(c: np.ndarray, w: int) -> np.ndarray:
    """An (h, cw) chroma plane as the (h, w) plane with c[y][x >> 1] at (y, x)."""
    c = np.asarray(c)
    return np.ascontiguousarray(c[:, np.arange(w) >> 1])


def repeated(y, cb, cr):
    """(y, Cb, Cr): the three (h, w) planes of the YUV444_PLANAR frame that the frame is."""
    w = y.shape[1]
    return y, repeat(cb, w), repeat(cr, w)


def pad_chroma_domain(y, cb, cr, mcu=(16, 8)):
    """The fp64 planes of a 4:2:2 frame with the chroma edge-replicated in the chroma domain, as
    jpge.h words the edge rule: the Y plane to whole MCUs, the chroma planes to that height
    and half that width, then each sample repeated across its cell."""
    y, cb, cr = (np.asarray(p, np.float64) - 128.0 for p in (y, cb, cr))
    h, w = y.shape
    H, W = -(-h // mcu[1]) * mcu[1], -(-w // mcu[0]) * mcu[0]
    edge = lambda p, r, c: np.pad(p, ((0, r - p.shape[0]), (0, c - p.shape[1])), mode="edge")
    return [edge(y, H, W)] + [np.repeat(edge(c, H, W // 2), 2, axis=1) for c in (cb, cr)]


def samples(seed: int, w: int, h: int, kind: str = "random"):
    """(y, cb, cr) uint8 planes, chroma (h, cw): random bytes, or every sample 0 / 255."""
    cw = cw_of(w)
    if kind == "random":
        g = np.random.default_rng(seed)
        return (g.integers(0, 256, (h, w), dtype=np.uint8), g.integers(0, 256, (h, cw), dtype=np.uint8),
                g.integers(0, 256, (h, cw), dtype=np.uint8))
    v = {"zeros": 0, "ones": 255}[kind]
    return np.full((h, w), v, np.uint8), np.full((h, cw), v, np.uint8), np.full((h, cw), v, np.uint8)


def build(fmt: int, y, cb, cr):
    """The frame Encoder.encode takes in layout fmt: a pack_yuv422 frame."""
    return J.pack_yuv422(fmt, y, cb, cr)[0]


def raw(fmt: int, y, cb, cr, stride: int = 0, plane_stride: int = 0, offset: int = 0, seed: int = 9, spare=None):
    """The frame written sample by sample, as jpge.h words the layouts, into a flat buffer of
    random bytes: rows of pitch `stride` from `offset`; NV16's and I422's chroma plane_stride
    bytes later.  spare: the value of an odd-width packed frame's last second Y byte of each
    row (None: the buffer's random byte stays).  Returns (buffer, stride, plane stride) with the
    defaults (0) resolved (packed: plane stride 0)."""
    y, cb, cr = (np.asarray(p, np.uint8) for p in (y, cb, cr))
    h, w = y.shape
    cw = cw_of(w)
    stride = stride or least_stride(fmt, w)
    packed = fmt in PACKED
    ps = 0 if packed else plane_stride or stride * h
    cs = (stride + 1) // 2
    size = offset + stride * h + (0 if packed else ps + 2 * max(cs, stride) * h) + 64
    buf = np.random.default_rng(seed).integers(0, 256, size, dtype=np.uint8)
    for r in range(h):
        o = offset + r * stride
        if packed:
            yo, co = (0, 1) if fmt == YUYV else (1, 0)
            for x in range(w):
                buf[o + 2 * x + yo] = y[r, x]
            if w % 2 and spare is not None:
                buf[o + 2 * w + yo] = spare
            for c in range(cw):
                buf[o + 4 * c + co], buf[o + 4 * c + co + 2] = cb[r, c], cr[r, c]
            continue
        buf[o:o + w] = y[r]
        if fmt == NV16:
            c0 = offset + ps + r * stride
            buf[c0:c0 + 2 * cw:2], buf[c0 + 1:c0 + 2 * cw:2] = cb[r], cr[r]
        else:
            c0 = offset + ps + r * cs
            buf[c0:c0 + cw], buf[c0 + cs * h:c0 + cs * h + cw] = cb[r], cr[r]
    return buf, stride, ps


def split(fmt: int, frame, w: int, h: int, stride: int = 0, plane_stride: int = 0, offset: int = 0):
    """(y, cb, cr) of a frame in layout fmt, read by the address rules of jpge.h."""
    a = np.asarray(frame, np.uint8).reshape(-1)
    cw = cw_of(w)
    stride = stride or least_stride(fmt, w)
    ps = plane_stride or stride * h
    y, cb, cr = np.zeros((h, w), np.uint8), np.zeros((h, cw), np.uint8), np.zeros((h, cw), np.uint8)
    for r in range(h):
        o = offset + r * stride
        for x in range(w):
            if fmt == YUYV:
                y[r, x], cb[r, x >> 1], cr[r, x >> 1] = a[o + 2 * x], a[o + 4 * (x >> 1) + 1], a[o + 4 * (x >> 1) + 3]
            elif fmt == UYVY:
                y[r, x], cb[r, x >> 1], cr[r, x >> 1] = a[o + 2 * x + 1], a[o + 4 * (x >> 1)], a[o + 4 * (x >> 1) + 2]
            elif fmt == NV16:
                c0 = offset + ps + r * stride + 2 * (x >> 1)
                y[r, x], cb[r, x >> 1], cr[r, x >> 1] = a[o + x], a[c0], a[c0 + 1]
            else:
                cs = (stride + 1) // 2
                c0 = offset + ps + r * cs + (x >> 1)
                y[r, x], cb[r, x >> 1], cr[r, x >> 1] = a[o + x], a[c0], a[c0 + cs * h]
    return y, cb, cr


def yuv444(y, cb, cr):
    """The YUV444_PLANAR frame (3, H, W) of the repeated planes."""
    return _yuv.build(_yuv.YUV444, *repeated(y, cb, cr))
