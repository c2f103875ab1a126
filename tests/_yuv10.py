"""Helpers of the 10-bit 4:2:0 input-layout tests (jpge.h JPGE_FMT_P010, _I010): the layouts
built with numpy (and taken apart again), and the fp64 planes a frame of 10-bit samples stands
for: every sample s the exact value s / 4, edge-replicated as _yuv.pad_planes replicates the
half layouts, then the three lines of jpge_set_yuv_transform (_yuvxf.luma, _yuvxf.chroma) with
the coefficients the library returned, the identity for FULL_601: the transform, and so its
clamps, always runs.  test_yuv10_cpu.py checks this file, so the GPU tests' expectations do not
rest on unchecked code."""

import numpy as np

import _yuv
import _yuvxf
import jpgenc_amd as J

P010, I010 = J.JPGE_FMT_P010, J.JPGE_FMT_I010
FORMATS = (P010, I010)
NAMES = {P010: "p010", I010: "i010"}
EIGHT = {P010: _yuv.NV12, I010: _yuv.I420}  # the 8-bit layout of the same planes
IDENTITY = _yuvxf.IDENTITY


def chroma_shape(w: int, h: int) -> tuple[int, int]:
    return (h + 1) // 2, (w + 1) // 2


def least_stride(fmt: int, w: int) -> int:
    return 4 * ((w + 1) // 2) if fmt == P010 else 2 * w


def chroma_pitch(fmt: int, stride: int) -> int:
    return stride if fmt == P010 else 2 * ((stride + 3) // 4)


def planes(y, cb, cr, t=IDENTITY):
    """The fp64 planes [Y', Cb', Cr'] (full size, whole 16x16 MCUs) of uint16 planes of 10-bit
    samples under transform t = (y_off, m0..m6), in _yuv.pad_planes' form."""
    q = [np.asarray(p, np.float64) / 4.0 for p in (y, cb, cr)]  # exact
    yb, u, v = _yuv.pad_planes(_yuv.I420, *q)  # samples / 4 - 128, replicated
    return [_yuvxf.luma(yb + 128.0, u, v, t), _yuvxf.chroma(u, v, t[4], t[5]), _yuvxf.chroma(u, v, t[6], t[7])]


def build(fmt: int, y, cb, cr):
    """The frame Encoder.encode takes in layout fmt: a pack_yuv420p10 frame."""
    return J.pack_yuv420p10(fmt, y, cb, cr)[0]


def words(fmt: int, p, junk=None):
    """The 16-bit words of a plane of samples: P010 in the top 10 bits, I010 in the low 10; the
    six other bits zero, or taken from junk (an array of values 0..63)."""
    p = np.asarray(p, np.uint16)
    j = np.zeros_like(p) if junk is None else np.asarray(junk, np.uint16)
    return ((p << 6) | j) if fmt == P010 else (p | (j << 10))


def raw(fmt: int, y, cb, cr, stride: int = 0, plane_stride: int = 0, offset: int = 0, seed: int = 9, junk_seed=None):
    """The frame written plane by plane, as jpge.h words the layouts, into a flat buffer of
    random bytes: Y rows of pitch `stride` (bytes) from `offset`; the chroma plane_stride bytes
    later.  junk_seed: random values in the bits the layout never reads.  Returns (buffer,
    stride, plane stride) with the defaults (0) resolved."""
    y, cb, cr = (np.asarray(p, np.uint16) for p in (y, cb, cr))
    h, w = y.shape
    ch, cw = chroma_shape(w, h)
    stride = stride or least_stride(fmt, w)
    ps = plane_stride or stride * h
    cs = chroma_pitch(fmt, stride)
    g = np.random.default_rng(seed)
    buf = g.integers(0, 256, offset + ps + 2 * max(cs * ch, ps) + 64, dtype=np.uint8)
    jg = None if junk_seed is None else np.random.default_rng(junk_seed)

    def put(o, row):
        j = None if jg is None else jg.integers(0, 64, row.shape, dtype=np.uint16)
        b = words(fmt, row, j).astype("<u2").view(np.uint8)
        buf[o:o + b.size] = b

    for r in range(h):
        put(offset + r * stride, y[r])
    for r in range(ch):
        o = offset + ps + r * cs
        if fmt == P010:
            put(o, np.stack([cb[r], cr[r]], axis=1).reshape(-1))
        else:
            put(o, cb[r])
            put(o + cs * ch, cr[r])
    return buf, stride, ps


def split(fmt: int, frame, w: int, h: int):
    """(y, cb, cr) uint16 samples of a frame of bytes in layout fmt with the least stride and
    plane stride 0."""
    ch, cw = chroma_shape(w, h)
    a = np.asarray(frame, np.uint8).reshape(-1).view("<u2").astype(np.uint16)
    if fmt == P010:
        s = 2 * cw  # words per row
        c = a[s * h:s * (h + ch)].reshape(ch, cw, 2) >> 6
        return (a[:s * h].reshape(h, s)[:, :w] >> 6).copy(), c[:, :, 0].copy(), c[:, :, 1].copy()
    n = w * h
    a = a & 0x3FF
    return a[:n].reshape(h, w).copy(), a[n:n + cw * ch].reshape(ch, cw).copy(), a[n + cw * ch:].reshape(ch, cw).copy()


def samples(seed: int, w: int, h: int, kind: str = "random"):
    """(y, cb, cr) uint16 planes of 10-bit samples: random over 0..1023, or every sample 0 / 1023."""
    ch, cw = chroma_shape(w, h)
    if kind == "random":
        g = np.random.default_rng(seed)
        return (g.integers(0, 1024, (h, w), dtype=np.uint16), g.integers(0, 1024, (ch, cw), dtype=np.uint16),
                g.integers(0, 1024, (ch, cw), dtype=np.uint16))
    v = {"zeros": 0, "ones": 1023}[kind]
    return np.full((h, w), v, np.uint16), np.full((ch, cw), v, np.uint16), np.full((ch, cw), v, np.uint16)
