"""Helpers of the 10-bit 4:2:2 input-layout tests (jpge.h JPGE_FMT_Y210, _P210, _I210): the
layouts built with numpy by the header's wording (and taken apart again), and the fp64 planes a
frame of 10-bit samples stands for: every sample s the exact value s / 4, a cell's chroma in
both of its pixels (_yuv422.repeat), edge-replicated to whole MCUs of the subsampling mode, then
the three lines of jpge_set_yuv_transform (_yuvxf.luma, _yuvxf.chroma) with the coefficients the
library returned, the identity for FULL_601: the transform, and so its clamps, always runs.
Expected coefficients are _yuv.want_coeffs of those planes, expected files _stream3.build3 of
them: no GPU code runs in an expectation.  test_yuv422p10_cpu.py checks this file."""

import numpy as np

import _yuv
import _yuv422
import _yuvxf
import jpgenc_amd as J

Y210, P210, I210 = J.JPGE_FMT_Y210, J.JPGE_FMT_P210, J.JPGE_FMT_I210
FORMATS = (Y210, P210, I210)
NAMES = {Y210: "y210", P210: "p210", I210: "i210"}
EIGHT = {Y210: _yuv422.YUYV, P210: _yuv422.NV16, I210: _yuv422.I422}  # the 8-bit layout of the same planes
HIGH = (Y210, P210)  # a sample is its word's top 10 bits
IDENTITY = _yuvxf.IDENTITY
MODES = (420, 444, 422, 411, 4200, 4201)


def cw_of(w: int) -> int:
    return (w + 1) // 2


def least_stride(fmt: int, w: int) -> int:
    return {Y210: 8 * cw_of(w), P210: 4 * cw_of(w), I210: 2 * w}[fmt]


def chroma_pitch(fmt: int, stride: int) -> int:
    return 2 * ((stride + 3) // 4) if fmt == I210 else stride


def planes(y, cb, cr, t=IDENTITY, mcu=(16, 16)):
    """The fp64 planes [Y', Cb', Cr'] (full size, whole MCUs of size mcu = (width, height)) of
    uint16 planes of 10-bit samples, chroma (h, cw), under transform t = (y_off, m0..m6), in
    _yuv.pad_planes' form."""
    q = [np.asarray(p, np.float64) / 4.0 for p in (y, cb, cr)]  # exact
    w = q[0].shape[1]
    q = [q[0], _yuv422.repeat(q[1], w), _yuv422.repeat(q[2], w)]
    yb, u, v = _yuv.pad_planes(_yuv.YUV444, *q, mcu=mcu)  # samples / 4 - 128, replicated
    return [_yuvxf.luma(yb + 128.0, u, v, t), _yuvxf.chroma(u, v, t[4], t[5]), _yuvxf.chroma(u, v, t[6], t[7])]


def build(fmt: int, y, cb, cr):
    """The frame Encoder.encode takes in layout fmt: a pack_yuv422p10 frame."""
    return J.pack_yuv422p10(fmt, y, cb, cr)[0]


def words(fmt: int, p, junk=None):
    """The 16-bit words of samples: Y210 and P210 in the top 10 bits, I210 in the low 10; the six
    other bits zero, or taken from junk (an array of values 0..63)."""
    p = np.asarray(p, np.uint16)
    j = np.zeros_like(p) if junk is None else np.asarray(junk, np.uint16)
    return ((p << 6) | j) if fmt in HIGH else (p | (j << 10))


def raw(fmt: int, y, cb, cr, stride: int = 0, plane_stride: int = 0, offset: int = 0, seed: int = 9, junk_seed=None,
        spare=None):
    """The frame written word by word, as jpge.h words the layouts, into a flat buffer of random
    bytes: rows of pitch `stride` (bytes) from `offset`; P210's and I210's chroma plane_stride
    bytes later.  junk_seed: random values in the six bits of each word the layout never reads.
    spare: the 16-bit word stored as an odd-width Y210 frame's last Y1 of each row (None: the
    buffer's random bytes stay).  Returns (buffer, stride, plane stride) with the defaults (0)
    resolved (Y210: plane stride 0)."""
    y, cb, cr = (np.asarray(p, np.uint16) for p in (y, cb, cr))
    h, w = y.shape
    cw = cw_of(w)
    assert cb.shape == (h, cw) == cr.shape
    stride = stride or least_stride(fmt, w)
    ps = 0 if fmt == Y210 else plane_stride or stride * h
    cs = chroma_pitch(fmt, stride)
    size = offset + stride * h + (0 if fmt == Y210 else ps + 2 * max(cs, stride) * h) + 64
    buf = np.random.default_rng(seed).integers(0, 256, size, dtype=np.uint8)
    jg = None if junk_seed is None else np.random.default_rng(junk_seed)

    def put(o, row, step=2):
        """the samples of row as words at byte o, o + step, ..."""
        j = None if jg is None else jg.integers(0, 64, row.shape, dtype=np.uint16)
        b = words(fmt, row, j).astype("<u2").view(np.uint8).reshape(-1, 2)
        at = o + step * np.arange(b.shape[0])
        buf[at], buf[at + 1] = b[:, 0], b[:, 1]

    for r in range(h):
        o = offset + r * stride
        if fmt == Y210:  # groups Y0 Cb Y1 Cr of four words
            put(o, y[r], 4)
            put(o + 2, cb[r], 8)
            put(o + 6, cr[r], 8)
            if w % 2 and spare is not None:
                buf[o + 4 * w:o + 4 * w + 2] = np.array([spare], "<u2").view(np.uint8)
            continue
        put(o, y[r])
        if fmt == P210:  # Cb in the even words, Cr in the odd words, pitch stride
            c0 = offset + ps + r * stride
            put(c0, cb[r], 4)
            put(c0 + 2, cr[r], 4)
        else:  # the Cb plane, then the Cr plane cs * h bytes later
            c0 = offset + ps + r * cs
            put(c0, cb[r])
            put(c0 + cs * h, cr[r])
    return buf, stride, ps


def split(fmt: int, frame, w: int, h: int, stride: int = 0, plane_stride: int = 0, offset: int = 0):
    """(y, cb, cr) uint16 samples of a frame of bytes in layout fmt, read by the address rules of
    jpge.h."""
    a = np.asarray(frame, np.uint8).reshape(-1)
    cw = cw_of(w)
    stride = stride or least_stride(fmt, w)
    ps = plane_stride or stride * h
    cs = chroma_pitch(fmt, stride)
    word = lambda o: int(a[o]) | (int(a[o + 1]) << 8)
    s = (lambda o: word(o) >> 6) if fmt in HIGH else (lambda o: word(o) & 0x3FF)
    y, cb, cr = np.zeros((h, w), np.uint16), np.zeros((h, cw), np.uint16), np.zeros((h, cw), np.uint16)
    for r in range(h):
        o = offset + r * stride
        for x in range(w):
            c = x >> 1
            if fmt == Y210:
                y[r, x], cb[r, c], cr[r, c] = s(o + 8 * c + 4 * (x & 1)), s(o + 8 * c + 2), s(o + 8 * c + 6)
            elif fmt == P210:
                c0 = offset + ps + r * stride + 4 * c
                y[r, x], cb[r, c], cr[r, c] = s(o + 2 * x), s(c0), s(c0 + 2)
            else:
                c0 = offset + ps + r * cs + 2 * c
                y[r, x], cb[r, c], cr[r, c] = s(o + 2 * x), s(c0), s(c0 + cs * h)
    return y, cb, cr


def samples(seed: int, w: int, h: int, kind: str = "random"):
    """(y, cb, cr) uint16 planes of 10-bit samples, chroma (h, cw): random over 0..1023, or every
    sample 0 / 1023."""
    cw = cw_of(w)
    if kind == "random":
        g = np.random.default_rng(seed)
        return (g.integers(0, 1024, (h, w), dtype=np.uint16), g.integers(0, 1024, (h, cw), dtype=np.uint16),
                g.integers(0, 1024, (h, cw), dtype=np.uint16))
    v = {"zeros": 0, "ones": 1023}[kind]
    return np.full((h, w), v, np.uint16), np.full((h, cw), v, np.uint16), np.full((h, cw), v, np.uint16)
