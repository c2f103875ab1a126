"""Helpers of the v210 input-layout tests (jpge.h JPGE_FMT_V210): the layout rule stated on its
own in numpy, one loop over a row's stream index (sample k of the stream Cb0 Y0 Cr0 Y1 Cb1 Y2 Cr1
Y3 ... is field k % 3 of the row's 32-bit little-endian word k / 3; pixel x has its Y at 2x + 1,
cell c its Cb at 4c and its Cr at 4c + 2), a writer that places a frame inside random bytes by the
same rule, and the fp64 planes a frame of 10-bit samples stands for, which are _yuv422p10's: a v210
frame means what the I210 frame of its samples means.  Expected coefficients are _yuv.want_coeffs
of those planes, expected files _stream3.build3 of them: no GPU code runs in an expectation.
test_v210_cpu.py checks this file."""

import numpy as np

import _yuv422p10 as T
import jpgenc_amd as J

V210 = J.JPGE_FMT_V210
IDENTITY = T.IDENTITY
MODES = T.MODES
cw_of = T.cw_of
samples = T.samples  # (y, cb, cr) uint16 planes of 10-bit samples, chroma (h, cw)
planes = T.planes    # the fp64 planes of such samples under a transform, whole MCUs


def row_bytes(w: int) -> int:
    """Six pixels in 16 bytes, whole groups."""
    return 16 * ((w + 5) // 6)


def conventional_stride(w: int) -> int:
    """The pitch capture hardware uses: rows of 48 pixels in 128 bytes."""
    return 128 * ((w + 47) // 48)


def stream(frame, w: int, h: int, stride: int = 0, offset: int = 0):
    """(h, n) uint16: the n = 12 * ceil(w / 6) samples of every row's stream, one loop over the
    stream index."""
    a = np.asarray(frame, np.uint8).reshape(-1)
    stride = stride or row_bytes(w)
    n = 3 * (row_bytes(w) // 4)
    rows = offset + stride * np.arange(h)
    out = np.zeros((h, n), np.uint16)
    for k in range(n):
        o = rows + 4 * (k // 3)
        word = a[o].astype(np.uint32) | (a[o + 1].astype(np.uint32) << 8) | (a[o + 2].astype(np.uint32) << 16) | \
            (a[o + 3].astype(np.uint32) << 24)
        out[:, k] = (word >> (10 * (k % 3))) & 0x3FF
    return out


def unpack(frame, w: int, h: int, stride: int = 0, offset: int = 0):
    """(y, cb, cr) uint16 samples of a frame of bytes, by the stream rule."""
    s = stream(frame, w, h, stride, offset)
    cw = cw_of(w)
    y = np.stack([s[:, 2 * x + 1] for x in range(w)], axis=1)
    cb = np.stack([s[:, 4 * c] for c in range(cw)], axis=1)
    cr = np.stack([s[:, 4 * c + 2] for c in range(cw)], axis=1)
    return y, cb, cr


def used(w: int) -> np.ndarray:
    """Which stream indices of a row hold a sample of the frame."""
    n = 3 * (row_bytes(w) // 4)
    u = np.zeros(n, bool)
    u[[2 * x + 1 for x in range(w)]] = True
    u[[4 * c for c in range(cw_of(w))]] = True
    u[[4 * c + 2 for c in range(cw_of(w))]] = True
    return u


def raw(y, cb, cr, stride: int = 0, offset: int = 0, seed: int = 9, junk_seed=None, tail: int = 64):
    """The frame written sample by sample into a flat buffer of random bytes: rows of pitch
    `stride` (bytes, 0: the least) from `offset`, `tail` more bytes after the last row's last
    group.  junk_seed None: bits 30-31 of every word and the last group's unused samples are zero;
    else they are random.  The padding between rows keeps the buffer's random bytes either way.
    Returns (buffer, stride)."""
    y, cb, cr = (np.asarray(p, np.uint32) for p in (y, cb, cr))
    h, w = y.shape
    cw = cw_of(w)
    assert cb.shape == (h, cw) == cr.shape
    row = row_bytes(w)
    stride = stride or row
    assert stride >= row
    n = 3 * (row // 4)
    buf = np.random.default_rng(seed).integers(0, 256, offset + stride * (h - 1) + row + tail, dtype=np.uint8)
    jg = None if junk_seed is None else np.random.default_rng(junk_seed)
    s = np.zeros((h, n), np.uint32) if jg is None else jg.integers(0, 1024, (h, n), dtype=np.uint32)
    for x in range(w):
        s[:, 2 * x + 1] = y[:, x]
    for c in range(cw):
        s[:, 4 * c], s[:, 4 * c + 2] = cb[:, c], cr[:, c]
    top = np.zeros((h, n // 3), np.uint32) if jg is None else jg.integers(0, 4, (h, n // 3), dtype=np.uint32)
    words = (s[:, 0::3] | (s[:, 1::3] << 10) | (s[:, 2::3] << 20) | (top << 30)).astype("<u4")
    for r in range(h):
        o = offset + r * stride
        buf[o:o + row] = words[r].view(np.uint8)
    return buf, stride


def build(y, cb, cr, stride: int = 0):
    """The frame Encoder.encode takes: a pack_v210 frame."""
    return J.pack_v210(y, cb, cr, stride)[0]
