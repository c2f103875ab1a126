"""Helpers of the Y, Cb, Cr input-layout tests (jpge.h JPGE_FMT_NV12, _I420, _YUV444_PLANAR):
the layouts built with numpy (and taken apart again), the fp64 planes a frame of 8-bit
samples stands for, and the coefficients expected of them, from the oracle's primitives
only (subsample_mode, orc_dct_arai, orc_quantize, quality_tables).  test_yuv_cpu.py checks
the builders and pad_planes, so the GPU tests' expectations do not rest on unchecked code."""

import numpy as np

import _oracle
import jpgenc_amd as J

NV12, I420, YUV444 = J.JPGE_FMT_NV12, J.JPGE_FMT_I420, J.JPGE_FMT_YUV444_PLANAR
FORMATS = (NV12, I420, YUV444)
HALF = (NV12, I420)  # chroma planes of ceil(H/2) x ceil(W/2)
NAMES = {NV12: "nv12", I420: "i420", YUV444: "yuv444"}


def chroma_shape(fmt: int, w: int, h: int) -> tuple[int, int]:
    return ((h + 1) // 2, (w + 1) // 2) if fmt in HALF else (h, w)


def _edge(p: np.ndarray, rows: int, cols: int) -> np.ndarray:
    return np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode="edge")


def pad_planes(fmt: int, y, cb, cr, mcu=(16, 16)):
    """The three fp64 planes (Y, Cb, Cr; full size) that a frame of 8-bit samples is: each
    sample v the value v - 128, the Y plane edge-replicated to whole MCUs (mcu: its width
    and height, 16x16 unless a YUV444_PLANAR test picks another subsampling mode); the 4:2:0
    layouts' chroma edge-replicated in the chroma domain to half that size, then each sample
    repeated 2x2 (the S420_m average of four equal values is that value); YUV444_PLANAR's
    chroma edge-replicated like Y."""
    y, cb, cr = (np.asarray(p, np.float64) - 128.0 for p in (y, cb, cr))
    h, w = y.shape
    H, W = -(-h // mcu[1]) * mcu[1], -(-w // mcu[0]) * mcu[0]
    out = [_edge(y, H, W)]
    for c in (cb, cr):
        assert c.shape == chroma_shape(fmt, w, h)
        if fmt in HALF:
            out.append(np.repeat(np.repeat(_edge(c, H // 2, W // 2), 2, axis=0), 2, axis=1))
        else:
            out.append(_edge(c, H, W))
    return out


def _blocks(plane: np.ndarray, q: np.ndarray) -> np.ndarray:
    """orc_dct_arai + orc_quantize of each 8x8 block, raster block order -> (blocks, 64) int16."""
    L = _oracle.orc()
    H, W = plane.shape
    assert H % 8 == 0 and W % 8 == 0
    q32 = np.ascontiguousarray(q, np.int32)
    out = np.zeros(((H // 8) * (W // 8), 64), np.int16)
    src, dct, qi = np.zeros(64, np.float64), np.zeros(64, np.float64), np.zeros(64, np.int32)
    for by in range(H // 8):
        for bx in range(W // 8):
            src[:] = plane[8 * by:8 * by + 8, 8 * bx:8 * bx + 8].reshape(64)
            L.orc_dct_arai(src.ctypes.data, dct.ctypes.data)
            L.orc_quantize(dct.ctypes.data, q32.ctypes.data, qi.ctypes.data)
            out[by * (W // 8) + bx] = qi
    return out


def want_coeffs(planes, mode: int, quality: int):
    """(Y, Cb, Cr) quantised coefficients of pad_planes' planes in subsampling mode `mode`:
    _oracle.subsample_mode on the chroma planes, then the oracle's DCT and quantiser."""
    qy, qc = _oracle.quality_tables(quality)
    y, cb, cr = (np.ascontiguousarray(p, np.float64) for p in planes)
    return (_blocks(y, qy), _blocks(_oracle.subsample_mode(cb, mode), qc),
            _blocks(_oracle.subsample_mode(cr, mode), qc))


def mcu_size(mode: int) -> tuple[int, int]:
    yh, yv = _oracle.SHAPES[mode]
    return 8 * yh, 8 * yv


# ---- layouts ----
def build(fmt: int, y, cb, cr):
    """The frame Encoder.encode takes in layout fmt: a pack_yuv420 frame, or (3, H, W)."""
    if fmt in HALF:
        return J.pack_yuv420(fmt, y, cb, cr)[0]
    return np.ascontiguousarray(np.stack([y, cb, cr]), np.uint8)


def raw(fmt: int, y, cb, cr, stride: int = 0, plane_stride: int = 0, offset: int = 0, seed: int = 9):
    """The frame written plane by plane, as jpge.h words the layouts, into a flat buffer of
    random bytes: Y rows of pitch `stride` from `offset`; the chroma plane_stride bytes
    later.  Returns (buffer, stride, plane stride) with the defaults (0) resolved."""
    y, cb, cr = (np.asarray(p, np.uint8) for p in (y, cb, cr))
    h, w = y.shape
    ch, cw = chroma_shape(fmt, w, h)
    stride = stride or (2 * cw if fmt == NV12 else w)
    ps = plane_stride or stride * h
    cs = {NV12: stride, I420: (stride + 1) // 2, YUV444: stride}[fmt]
    buf = np.random.default_rng(seed).integers(0, 256, offset + ps + 2 * max(cs * ch, ps) + 64, dtype=np.uint8)
    for r in range(h):
        buf[offset + r * stride:offset + r * stride + w] = y[r]
    for r in range(ch):
        o = offset + ps + r * cs
        if fmt == NV12:
            buf[o:o + 2 * cw:2], buf[o + 1:o + 2 * cw:2] = cb[r], cr[r]
        elif fmt == I420:
            buf[o:o + cw], buf[o + cs * ch:o + cs * ch + cw] = cb[r], cr[r]
        else:
            buf[o:o + cw], buf[o + ps:o + ps + cw] = cb[r], cr[r]
    return buf, stride, ps


def split(fmt: int, frame, w: int, h: int):
    """(y, cb, cr) of a frame in layout fmt with the least stride and plane stride 0."""
    ch, cw = chroma_shape(fmt, w, h)
    if fmt == YUV444:
        return tuple(np.array(frame[c]) for c in range(3))
    a = np.asarray(frame, np.uint8).reshape(-1)
    if fmt == NV12:
        s = 2 * cw
        c = a[s * h:s * (h + ch)].reshape(ch, cw, 2)
        return a[:s * h].reshape(h, s)[:, :w].copy(), c[:, :, 0].copy(), c[:, :, 1].copy()
    n = w * h
    return a[:n].reshape(h, w).copy(), a[n:n + cw * ch].reshape(ch, cw).copy(), a[n + cw * ch:].reshape(ch, cw).copy()


def samples(fmt: int, seed: int, w: int, h: int, kind: str = "random"):
    """(y, cb, cr) uint8 planes for layout fmt: random bytes, or every sample 0 / 255."""
    ch, cw = chroma_shape(fmt, w, h)
    if kind == "random":
        g = np.random.default_rng(seed)
        return (g.integers(0, 256, (h, w), dtype=np.uint8), g.integers(0, 256, (ch, cw), dtype=np.uint8),
                g.integers(0, 256, (ch, cw), dtype=np.uint8))
    v = {"zeros": 0, "ones": 255}[kind]
    return np.full((h, w), v, np.uint8), np.full((ch, cw), v, np.uint8), np.full((ch, cw), v, np.uint8)


def upsample(c, w: int, h: int) -> np.ndarray:
    """A half-size chroma plane repeated 2x2, cropped to h x w."""
    return np.ascontiguousarray(np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)[:h, :w])
