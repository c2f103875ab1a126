"""Helpers of the limit tests (test_limits_cpu.py, test_gpu_limits.py): the frames at the
65535-pixel limit, their expected bytes and coefficients from the C oracle's whole-frame
entries (no per-block Python loop: these frames have 25-50 thousand blocks), the restart
intervals worth trying on them, and builders that lay a frame out inside random bytes with
numpy views (what _formats.padded, _yuv.raw and _yuv422.raw do row by row or sample by
sample; test_limits_cpu.py checks that they agree).

Pillow (libjpeg's 65500-pixel dimension limit) decodes the oracle's streams up to 65500
pixels and refuses them from 65520 on ("broken data stream"), in either dimension: above
65500 the decode-side check is the project's own decode_coeffs."""
import functools

import numpy as np

import _oracle
import _yuv as Y
import _yuv422 as Z
import jpgenc_amd as J

#: one row, one column, one and a bit MCU rows / columns, a ragged 8-px edge, Pillow's largest
LIMIT_SHAPES = [(65535, 1), (1, 65535), (65535, 17), (17, 65535), (65521, 9), (65500, 33)]
LONG = [(65535, 17), (17, 65535)]
#: in 4:4:4 at a restart interval of 1: 8192 x 9 = 73 728 segments, more than 16 bits count
MANY_SEGMENTS = (65535, 65)
MODES = (420, 444, 422, 411, 4200, 4201)
#: the transform kernel's 32-bit offset bound (fdct.hip kOob, kernels.hpp kK1OffsetBound):
#: stride * height of a frame read in place stays below it
K_OOB = 0xFFFFFF00
PILLOW_MAX = 65500
E_ARG = 1

KIND = {"photo": 0, "random": 1}


def ids(shapes):
    return [f"{w}x{h}" for w, h in shapes]


@functools.lru_cache(maxsize=None)
def frame(kind: str, w: int, h: int, seed: int = 0) -> np.ndarray:
    """synth_rgb8's photo-like frame or random bytes, read-only, computed once."""
    rgb = J.synth_rgb8(seed or (w * 31 + h), w, h, kind=KIND[kind])
    rgb.setflags(write=False)
    return rgb


def scaled(rgb: np.ndarray, maxval: int) -> np.ndarray:
    return (rgb.astype(np.uint32) * maxval // 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def want(kind, w, h, quality=90, mode=420, restart=0, maxval=255, seed=0) -> bytes:
    rgb = frame(kind, w, h, seed)
    return _oracle.encode(rgb if maxval == 255 else scaled(rgb, maxval), quality, maxval=maxval, restart=restart,
                          subsampling=mode)


@functools.lru_cache(maxsize=None)
def want_coeffs(kind, w, h, quality=90, mode=420, maxval=255, seed=0):
    rgb = frame(kind, w, h, seed)
    return _oracle.stage_coeffs_mode(rgb if maxval == 255 else scaled(rgb, maxval), mode, quality, maxval)


def mcus(w: int, h: int, mode: int) -> tuple[int, int]:
    """(MCUs across, MCUs down)"""
    yh, yv = _oracle.SHAPES[mode]
    return -(-w // (8 * yh)), -(-h // (8 * yv))


def restarts(w: int, h: int, mode: int) -> list[int]:
    """1, one MCU row, the DRI limit, and an interval that does not divide the row (a row of
    one MCU has no such interval above 1: then 3, which does not divide the MCU count)."""
    mw, mh = mcus(w, h, mode)
    odd = next(r for r in (7, 5, 3, 2) if (mw % r if mw > 1 else (mw * mh) % r))
    out = []
    for r in (1, mw, 65535, odd):
        if r not in out:
            out.append(r)
    return out


def same(got, wanted) -> bool:
    assert len(got) == len(wanted)
    return all(np.array_equal(g, w) for g, w in zip(got, wanted))


# ---- frames inside random bytes, written through strided views ----
def _noise(size: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, size, dtype=np.uint8)


def rows(buf: np.ndarray, off: int, h: int, n: int, stride: int, step: int = 1) -> np.ndarray:
    """A writable (h, n) view of buf: row r's sample k at off + r * stride + k * step."""
    assert off >= 0 and off + (h - 1) * stride + (n - 1) * step < buf.size
    return np.lib.stride_tricks.as_strided(buf[off:], shape=(h, n), strides=(stride, step))


def padded(a: np.ndarray, fmt: int, stride: int, plane_stride: int = 0, offset: int = 0, seed: int = 9):
    """_formats.padded: (buffer, offset of the first pixel, plane stride used)."""
    planar = fmt == J.JPGE_FMT_RGB8_PLANAR
    planes = a if planar else a[None].reshape(1, a.shape[0], -1)
    n, h, row = planes.shape
    assert stride >= row
    ps = plane_stride or stride * h
    assert not planar or ps >= stride * (h - 1) + row
    buf = _noise(offset + (n - 1) * ps + stride * (h - 1) + row + 64, seed)
    for c in range(n):
        rows(buf, offset + c * ps, h, row, stride)[:] = planes[c]
    return buf, offset, (ps if planar else 0)


def yuv_raw(fmt: int, y, cb, cr, stride: int = 0, plane_stride: int = 0, offset: int = 0, seed: int = 9):
    """_yuv.raw (NV12, I420, YUV444_PLANAR): (buffer, stride, plane stride)."""
    y, cb, cr = (np.asarray(p, np.uint8) for p in (y, cb, cr))
    h, w = y.shape
    ch, cw = Y.chroma_shape(fmt, w, h)
    stride = stride or (2 * cw if fmt == Y.NV12 else w)
    ps = plane_stride or stride * h
    cs = {Y.NV12: stride, Y.I420: (stride + 1) // 2, Y.YUV444: stride}[fmt]
    buf = _noise(offset + ps + 2 * max(cs * ch, ps) + 64, seed)
    rows(buf, offset, h, w, stride)[:] = y
    o = offset + ps
    if fmt == Y.NV12:
        rows(buf, o, ch, cw, cs, 2)[:] = cb
        rows(buf, o + 1, ch, cw, cs, 2)[:] = cr
    elif fmt == Y.I420:
        rows(buf, o, ch, cw, cs)[:] = cb
        rows(buf, o + cs * ch, ch, cw, cs)[:] = cr
    else:
        rows(buf, o, ch, cw, cs)[:] = cb
        rows(buf, o + ps, ch, cw, cs)[:] = cr
    return buf, stride, ps


def yuv422_raw(fmt: int, y, cb, cr, stride: int = 0, plane_stride: int = 0, offset: int = 0, seed: int = 9):
    """_yuv422.raw with spare=None (YUYV, UYVY, NV16, I422): (buffer, stride, plane stride)."""
    y, cb, cr = (np.asarray(p, np.uint8) for p in (y, cb, cr))
    h, w = y.shape
    cw = Z.cw_of(w)
    stride = stride or Z.least_stride(fmt, w)
    packed = fmt in Z.PACKED
    ps = 0 if packed else plane_stride or stride * h
    cs = (stride + 1) // 2
    buf = _noise(offset + stride * h + (0 if packed else ps + 2 * max(cs, stride) * h) + 64, seed)
    if packed:
        yo, co = (0, 1) if fmt == Z.YUYV else (1, 0)
        rows(buf, offset + yo, h, w, stride, 2)[:] = y
        rows(buf, offset + co, h, cw, stride, 4)[:] = cb
        rows(buf, offset + co + 2, h, cw, stride, 4)[:] = cr
        return buf, stride, 0
    rows(buf, offset, h, w, stride)[:] = y
    o = offset + ps
    if fmt == Z.NV16:
        rows(buf, o, h, cw, stride, 2)[:] = cb
        rows(buf, o + 1, h, cw, stride, 2)[:] = cr
    else:
        rows(buf, o, h, cw, cs)[:] = cb
        rows(buf, o + cs * h, h, cw, cs)[:] = cr
    return buf, stride, ps


def rgb_planes(rgb: np.ndarray):
    """loadPPM's fp64 R, G, B planes of an 8-bit frame, edge-replicated to whole 16x16 MCUs
    (what encode_planes takes with JPGE_TO_RGB)."""
    h, w = rgb.shape[:2]
    p = np.pad(rgb, ((0, -h % 16), (0, -w % 16), (0, 0)), mode="edge").astype(np.float64)
    return [np.ascontiguousarray(p[..., c]) for c in range(3)]
