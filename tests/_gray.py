"""The one-component (JPGE_FMT_GRAY8) stream built from the oracle's primitives only
(orc_dct_arai, orc_quantize, orc_rle_block, _oracle.huffman, _oracle.pack_bits) and numpy:
the expected bytes of the gray tests.  The stream (jpge.h JPGE_FMT_GRAY8): the plane
edge-replicated to whole 8x8 blocks, a sample v the fp64 value v - 128, blocks in raster
order, one DC chain over them (reset at every restart interval's first block), the two
luma texts and their per-image tables, SOI APP0 DQT SOF0(1 component) DHT DHT [DRI] SOS,
the bits of each interval 1-filled and 0xFF-stuffed, RSTn between intervals, EOI.
test_gray_cpu.py ties the coefficients to the Y plane of the YUV helpers (_yuv) and the
file to the host decoder and to PIL."""

from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import _oracle
import jpgenc_amd as J

GRAY = J.JPGE_FMT_GRAY8
SOI_APP0 = bytes([0xFF, 0xD8, 0xFF, 0xE0, 0x00, 0x10]) + b"JFIF" + bytes([0, 1, 1, 0, 0, 1, 0, 1, 0, 0])
SOS = bytes([0xFF, 0xDA, 0x00, 0x08, 0x01, 0x01, 0x00, 0x00, 0x3F, 0x00])


@dataclass(frozen=True)
class Built:
    jpg: bytes
    coef: np.ndarray   # (blocks, 64) int16 quantised coefficients before DC differencing, raster order
    blocks: tuple      # per block: ((symbol, nbits, bits), ...), the DC symbol first
    dc_text: tuple     # the DC text: one category per block
    ac_text: tuple     # the AC text: every block's AC symbols, in block order
    mw: int
    mh: int


def pad(plane: np.ndarray) -> np.ndarray:
    """The fp64 plane: v - 128, edge-replicated to multiples of 8."""
    p = np.asarray(plane)
    assert p.ndim == 2 and p.dtype == np.uint8 and p.size
    h, w = p.shape
    return np.pad(p.astype(np.float64) - 128.0, ((0, -h % 8), (0, -w % 8)), mode="edge")


def coefficients(plane: np.ndarray, qy) -> np.ndarray:
    L = _oracle.orc()
    p = pad(plane)
    H, W = p.shape
    q32 = np.ascontiguousarray(qy, np.int32)
    out = np.zeros(((H // 8) * (W // 8), 64), np.int16)
    src, dct, qi = np.zeros(64, np.float64), np.zeros(64, np.float64), np.zeros(64, np.int32)
    for by in range(H // 8):
        for bx in range(W // 8):
            src[:] = p[8 * by:8 * by + 8, 8 * bx:8 * bx + 8].reshape(64)
            L.orc_dct_arai(src.ctypes.data, dct.ctypes.data)
            L.orc_quantize(dct.ctypes.data, q32.ctypes.data, qi.ctypes.data)
            out[by * (W // 8) + bx] = qi
    return out


def _dht(info: int, table) -> bytes:
    """A DHT segment from _oracle.huffman's (symbol, length, code) list (DHT order)."""
    bits = [0] * 16
    for _, ln, _ in table:
        bits[ln - 1] += 1
    n = 2 + 17 + len(table)
    return bytes([0xFF, 0xC4, n >> 8, n & 255, info]) + bytes(bits) + bytes(s for s, _, _ in table)


def headers(w: int, h: int, qy, dc_table, ac_table, restart: int) -> bytes:
    zz = [_oracle.orc().orc_zigzag_to_natural(i) for i in range(64)]
    q = np.asarray(qy, np.uint8)
    out = SOI_APP0 + bytes([0xFF, 0xDB, 0x00, 0x43, 0x00]) + bytes(int(q[zz[i]]) for i in range(64))
    out += bytes([0xFF, 0xC0, 0x00, 0x0B, 0x08, h >> 8, h & 255, w >> 8, w & 255, 0x01, 0x01, 0x11, 0x00])
    out += _dht(0x00, dc_table) + _dht(0x10, ac_table)
    if restart:
        out += bytes([0xFF, 0xDD, 0x00, 0x04, restart >> 8, restart & 255])
    return out + SOS


def build(plane: np.ndarray, qy, restart: int = 0) -> Built:
    """The whole file of an (h, w) uint8 plane with luma table qy (natural order) and a
    restart interval in blocks (0: none)."""
    L = _oracle.orc()
    h, w = plane.shape
    coef = coefficients(plane, qy)
    nb = coef.shape[0]
    blk = np.zeros(64, np.int32)
    runs, vals, syms, nbits = (np.zeros(64, np.int32) for _ in range(4))
    bits = np.zeros(64, np.uint32)
    blocks = []
    pred = 0
    for g in range(nb):
        if restart and g % restart == 0:
            pred = 0
        blk[:] = coef[g]
        blk[0] = int(coef[g, 0]) - pred
        pred = int(coef[g, 0])
        n = L.orc_rle_block(blk.ctypes.data, runs.ctypes.data, vals.ctypes.data, syms.ctypes.data, nbits.ctypes.data,
                            bits.ctypes.data)
        blocks.append(tuple(zip(syms[:n].tolist(), nbits[:n].tolist(), bits[:n].tolist())))
    dc_text = tuple(b[0][0] for b in blocks)
    ac_text = tuple(s[0] for b in blocks for s in b[1:])
    dc_table, ac_table = _oracle.huffman(dc_text), _oracle.huffman(ac_text)
    dc_code = {s: (c, ln) for s, ln, c in dc_table}
    ac_code = {s: (c, ln) for s, ln, c in ac_table}
    out = bytearray(headers(w, h, qy, dc_table, ac_table, restart))
    step = restart if restart else nb
    for i, g0 in enumerate(range(0, nb, step)):
        if i:
            out += bytes([0xFF, 0xD0 + ((i - 1) & 7)])
        v, n = [], []
        for b in blocks[g0:g0 + step]:
            for k, (s, sb, xb) in enumerate(b):
                c, ln = (dc_code if k == 0 else ac_code)[s]
                v.append(c)
                n.append(ln)
                if sb:
                    v.append(xb)
                    n.append(sb)
        out += _oracle.pack_bits(v, n, do_fill=True)[0]
    out += bytes([0xFF, 0xD9])
    return Built(bytes(out), coef, tuple(blocks), dc_text, ac_text, (w + 7) // 8, (h + 7) // 8)


# ---- inputs ----
KINDS = ("random", "photo", "zeros", "ones")


def plane(kind: str, w: int, h: int, seed: int = 1) -> np.ndarray:
    """Random bytes, jpge_synth_rgb8's photo-like green channel, all 0 or all 255."""
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "photo":
        return np.ascontiguousarray(J.synth_rgb8(seed, w, h)[:, :, 1])
    return np.full((h, w), {"zeros": 0, "ones": 255}[kind], np.uint8)


@functools.lru_cache(maxsize=None)
def built(kind: str, w: int, h: int, quality: int, restart: int = 0, seed: int = 1) -> Built:
    """build() of plane(kind, w, h, seed) at a quality's luma table, computed once."""
    return build(plane(kind, w, h, seed), _oracle.quality_tables(quality)[0], restart)


def hist(b: Built):
    """(counts[2][256], order[2]): the DC and AC texts' symbol counts, and their symbols in
    order of first occurrence (what the table build consumes)."""
    counts = np.zeros((2, 256), np.uint32)
    order = []
    for t, text in enumerate((b.dc_text, b.ac_text)):
        np.add.at(counts[t], np.asarray(text, np.int64), 1)
        order.append(list(dict.fromkeys(text)))
    return counts, order
