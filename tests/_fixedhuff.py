"""Expected bytes of a stream coded with GIVEN Huffman tables (jpge.h jpge_set_huffman),
restated from parts that are pinned already, without touching the oracle:

  1. the quantised coefficients: _oracle.stage_coeffs_mode (RGB frames), or for a plane of
     8-bit samples _gray.coefficients (the one-component stream; a plane of a 4:4:4 Y, Cb,
     Cr frame);
  2. the DC differences, predictions restarting with every restart interval;
  3. zig-zag, RLE_AC and the category code through jpgenc_amd's host C ABI entries
     (jpge_rle_ac, jpge_encode_category: pinned to the reference by test_coding.py);
  4. canonical codes from the table's (bits, huffval) (ITU T.81 Annex C);
  5. one _oracle.pack_bits call per restart segment (the 1-fill and the 0xFF stuffing);
  6. RSTn between the segments;
  7. the optimal-mode header of a frame of the same geometry, quantisers, sampling and
     restart interval, with its DHT segments swapped for the given tables (every other
     header byte does not depend on the pixels).

test_fixedhuff_cpu.py feeds it the per-image optimal tables and gets _oracle.encode's bytes
back, which pins steps 1 to 7 to the reference before the helper judges anything.

A table ("spec") is (bits, huffval): 16 counts of codes of length 1..16 and the symbols in
DHT order, as jpgenc_amd.standard_huffman returns it; specs = [Y-DC, Y-AC, C-DC, C-AC]."""

from __future__ import annotations

import functools
import json
import os

import numpy as np

import _gray
import _oracle
import jpgenc_amd as J

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "annexk_huffman.json")


# ---- tables ----
def canonical(spec) -> dict:
    """symbol -> (code, length): codes of one length count up in huffval order; the first
    code of a length is the last code of the shorter length, plus one, shifted left."""
    bits, vals = spec
    out, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(int(bits[ln - 1])):
            out[int(vals[k])] = (code, ln)
            code += 1
            k += 1
        code <<= 1
    assert k == len(vals)
    return out


def golden_specs() -> list:
    """Annex K tables K.3, K.5, K.4, K.6 as the committed fixture holds them."""
    with open(GOLDEN) as f:
        return [(t["bits"], t["huffval"]) for t in json.load(f)["tables"]]


def dht_specs(jpg: bytes) -> list:
    """The tables of a stream's DHT segments, by slot Y-DC, Y-AC, C-DC, C-AC (None: absent)."""
    out = [None] * 4
    for marker, body in segments(jpg)[0]:
        if marker != 0xC4:
            continue
        p = 0
        while p < len(body):
            info, bits = body[p], list(body[p + 1:p + 17])
            n = sum(bits)
            out[2 * (info & 15) + (info >> 4)] = (bits, list(body[p + 17:p + 17 + n]))
            p += 17 + n
    return out


def optimal_specs(rgb: np.ndarray, quality: int) -> list:
    """The per-image tables of a 4:2:0 frame without restart intervals: the host table
    builder (jpge_huffman_table) on the oracle's histograms and first-occurrence keys."""
    counts, first = _oracle.stage_hist(rgb, quality)
    out = []
    for t in range(4):
        bits, hv, _, _ = J.huffman_table(counts[t], first[t].astype(np.uint64))
        out.append((bits.tolist(), hv))
    return out


# ---- marker segments ----
def segments(jpg: bytes):
    """([(marker, payload)] from after SOI up to and including SOS, offset of the scan)."""
    assert jpg[:2] == b"\xff\xd8"
    out, i = [], 2
    while True:
        assert jpg[i] == 0xFF, hex(jpg[i])
        m, n = jpg[i + 1], (jpg[i + 2] << 8) | jpg[i + 3]
        out.append((m, jpg[i + 4:i + 2 + n]))
        i += 2 + n
        if m == 0xDA:
            return out, i


def _segment(marker: int, body: bytes) -> bytes:
    n = len(body) + 2
    return bytes([0xFF, marker, n >> 8, n & 255]) + body


def swap_dht(header: bytes, specs) -> bytes:
    """The header (SOI .. SOS) with each DHT segment's table replaced by its slot's spec."""
    out = bytearray(b"\xff\xd8")
    for m, body in segments(header)[0]:
        if m == 0xC4:
            info = body[0]
            assert len(body) == 17 + sum(body[1:17]), "one table per DHT segment"
            bits, vals = specs[2 * (info & 15) + (info >> 4)]
            body = bytes([info]) + bytes(int(b) for b in bits) + bytes(int(v) for v in vals)
        out += _segment(m, body)
    return bytes(out)


@functools.lru_cache(maxsize=None)
def _optimal_header(w: int, h: int, qy: bytes, qc: bytes, mode: int, restart: int) -> bytes:
    # (the header of any frame of this geometry: only its DHT payloads depend on the pixels)
    jpg = _oracle.encode(np.zeros((h, w, 3), np.uint8), qy=np.frombuffer(qy, np.uint8), qc=np.frombuffer(qc, np.uint8),
                         restart=restart, subsampling=mode)
    return jpg[:segments(jpg)[1]]


def header(w: int, h: int, qy, qc, specs, mode: int = 420, restart: int = 0) -> bytes:
    """Three components: the optimal-mode header with the given tables."""
    hdr = _optimal_header(w, h, np.asarray(qy, np.uint8).tobytes(), np.asarray(qc, np.uint8).tobytes(), mode, restart)
    return swap_dht(hdr, specs)


def header_gray(w: int, h: int, qy, specs, restart: int = 0) -> bytes:
    """One component: _gray.headers with the luma pair (two DHT segments)."""
    tabs = [[(s, ln, c) for s, (c, ln) in canonical(sp).items()] for sp in specs[:2]]
    return _gray.headers(w, h, qy, tabs[0], tabs[1], restart)


# ---- the scan ----
def _block_symbols(blk: np.ndarray):
    """[(symbol, extra bits, bit count)] of a natural-order block whose DC is already the
    difference: the DC pair first, then the AC pairs (ZRL, EOB included)."""
    return J.encode_category(J.rle_ac(blk, zigzag_scan=True))


def mcu_blocks(y, cb, cr, w: int, h: int, mode: int):
    """[(component, coefficients)] in scan order: per MCU its Y blocks row by row, Cb, Cr.
    cb is None: one component, blocks in raster order."""
    if cb is None:
        return [[(0, b)] for b in y]
    yh, yv = _oracle.SHAPES[mode]
    mw, mh = -(-w // (8 * yh)), -(-h // (8 * yv))
    ybw = mw * yh
    out = []
    for mr in range(mh):
        for mc in range(mw):
            m = [(0, y[(mr * yv + k // yh) * ybw + mc * yh + k % yh]) for k in range(yh * yv)]
            m += [(1, cb[mr * mw + mc]), (2, cr[mr * mw + mc])]
            out.append(m)
    return out


def scan(mcus, specs, restart: int = 0) -> bytes:
    """The entropy-coded segment(s) of MCUs (mcu_blocks) with RSTn between restart
    intervals (restart: MCUs per interval, 0 = one interval), without EOI."""
    codes = [canonical(s) if s is not None else None for s in specs]
    out = bytearray()
    step = restart if restart else max(1, len(mcus))
    blk = np.zeros(64, np.int32)
    for i, m0 in enumerate(range(0, len(mcus), step)):
        if i:
            out += bytes([0xFF, 0xD0 + ((i - 1) & 7)])
        pred = [0, 0, 0]
        v, n = [], []
        for mcu in mcus[m0:m0 + step]:
            for comp, coef in mcu:
                blk[:] = coef
                blk[0] = int(coef[0]) - pred[comp]
                pred[comp] = int(coef[0])
                for k, (sym, xb, nb) in enumerate(_block_symbols(blk)):
                    c, ln = codes[2 * (comp != 0) + (k != 0)][sym]
                    v.append(c)
                    n.append(ln)
                    if nb:
                        v.append(xb)
                        n.append(nb)
        out += _oracle.pack_bits(v, n, do_fill=True)[0]
    return bytes(out)


# ---- whole files ----
def expected_rgb(rgb: np.ndarray, quality: int, specs, mode: int = 420, restart: int = 0) -> bytes:
    """An RGB frame at a quality's tables in a subsampling mode."""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    h, w = rgb.shape[:2]
    qy, qc = _oracle.quality_tables(quality)
    y, cb, cr = _oracle.stage_coeffs_mode(rgb, mode, quality)
    return header(w, h, qy, qc, specs, mode, restart) + scan(mcu_blocks(y, cb, cr, w, h, mode), specs, restart) + b"\xff\xd9"


def expected_coeffs(y, cb, cr, w: int, h: int, qy, qc, specs, mode: int = 420, restart: int = 0) -> bytes:
    """Three planes of quantised coefficients ((blocks, 64), raster block order) of a
    w x h frame in a subsampling mode."""
    return header(w, h, qy, qc, specs, mode, restart) + scan(mcu_blocks(y, cb, cr, w, h, mode), specs, restart) + b"\xff\xd9"


def expected_gray(plane: np.ndarray, qy, specs, restart: int = 0) -> bytes:
    """The one-component stream of an (h, w) plane (restart: blocks per interval)."""
    h, w = plane.shape
    coef = _gray.coefficients(plane, qy)
    return header_gray(w, h, qy, specs, restart) + scan(mcu_blocks(coef, None, None, w, h, 444), specs, restart) + b"\xff\xd9"


def expected_yuv444(planes, qy, qc, specs, restart: int = 0) -> bytes:
    """A 4:4:4 frame of three (h, w) planes of Y, Cb, Cr samples (JPGE_FMT_YUV444_PLANAR in
    JPGE_S444): each plane the one-component stream's coefficients at its table."""
    h, w = planes[0].shape
    y, cb, cr = (_gray.coefficients(p, q) for p, q in zip(planes, (qy, qc, qc)))
    return header(w, h, qy, qc, specs, 444, restart) + scan(mcu_blocks(y, cb, cr, w, h, 444), specs, restart) + b"\xff\xd9"


# ---- engineered tables ----
def long_code_spec(spec, keep: int = 0):
    """The same symbols, recoded so that all but `keep` of them carry 15- and 16-bit
    codes: bits = [0]*14 + [a, b] with the symbols' order reversed, so the symbols Annex K
    gives its shortest codes (the frequent ones) get the 16-bit codes.  Complete because the
    symbol set is unchanged; Kraft sum 2a + b < 2^16."""
    _, vals = spec
    vals = list(vals)
    head, rest = vals[:keep], vals[keep:][::-1]
    a = min(len(rest) // 2, 60)
    bits = [0] * 16
    for i in range(keep):  # the kept symbols: one code each of lengths 2, 3, ...
        bits[1 + i] = 1
    bits[14], bits[15] = a, len(rest) - a
    return bits, head + rest


def permuted_spec(spec, seed: int = 7):
    """A valid permutation of the table's symbol order: the same bits, the symbols shuffled
    (so most symbols change their code, and some their length)."""
    bits, vals = spec
    p = np.random.default_rng(seed).permutation(len(vals))
    return list(bits), [int(vals[i]) for i in p]
