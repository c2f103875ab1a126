"""Frames engineered in the coefficient domain for the symbol streams the statistics
kernel's record writer and the code kernel have special cases for: four long records side
by side, blocks of 128 records, every zero run across the 16-position parts of a block,
long codes and continuations in the chroma tables.  numpy and the oracle only.

Construction: 64 quantised values in zig-zag order, times a uniform table full(64, q),
through the inverse DCT (A^T X A with A(k, n) = C(k) sqrt(2/8) cos((2n+1) k pi / 16), the
matrix of jpge_idct8x8), + 128, rounded to uint8.  Where a frame needs exact symbols the
block is passed through the oracle's own DCT and quantiser when it is built and drawn
again (other signs and magnitudes) until it gives back its values, so pixel rounding
(sigma 0.29 on a coefficient, against a half step of q / 2) has not moved one.  The
oracle, not this construction, defines the truth: test_adversarial_cpu.py recomputes every
property from _gray.build of the finished frame.

The record model (a test-side restatement; kernels.hpp, "Symbol records (K2 -> K3)"):
    "table << 14 | run << 10 | size << 6 | x ... x = the top min(size, 6) of the symbol's
    extra bits; continuation: the component's AC table << 14 | n << 10 | the n (1..5) low
    extra bits the record before it could not hold (size >= 7)" ... "A block codes at most
    64 symbols (DC + 63 AC, or DC + 62 AC + EOB ...), each with at most one continuation"
so a symbol's head record codes its Huffman code plus min(size, 6) bits, and a symbol of
size 7 and up is followed by a continuation record of size - 6 bits.  The code kernel joins
the 4 adjacent records of a thread in a 64-bit word and takes a per-record path when they
total more than 64 bits; a group starts at a multiple of 4 within a record sub-stream, and
sub-streams start at block boundaries, so 7 consecutive records of >= 17 bits inside one
block always hold a whole group over 64 bits."""

from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import _gray as G
import _oracle

LONG = 17        # four records of at least this many bits pass 64
REC_X_BITS = 6   # extra bits a head record holds (kRecXBits)


@functools.lru_cache(maxsize=None)
def _zz() -> np.ndarray:
    """natural index of each zig-zag position"""
    return np.array([_oracle.orc().orc_zigzag_to_natural(i) for i in range(64)])


@functools.lru_cache(maxsize=None)
def _A() -> np.ndarray:
    k, n = np.mgrid[0:8, 0:8]
    a = np.sqrt(2.0 / 8.0) * np.cos((2 * n + 1) * k * np.pi / 16.0)
    a[0] /= np.sqrt(2.0)
    return a


def pixels(zz_vals, q: int, dither=None):
    """(8x8 uint8 block, whether it needed no clipping) of 64 quantised zig-zag values
    (dither: an 8x8 offset added before rounding)."""
    x = np.zeros(64)
    x[_zz()] = np.asarray(zz_vals, np.float64) * q
    p = np.rint(_A().T @ x.reshape(8, 8) @ _A() + 128.0 + (0.0 if dither is None else dither))
    return np.clip(p, 0, 255).astype(np.uint8), bool(p.min() >= 0 and p.max() <= 255)


def quantised(block: np.ndarray, q: int) -> np.ndarray:
    """The oracle's quantised zig-zag values of one 8x8 uint8 block."""
    return G.coefficients(block, np.full(64, q, np.uint8))[0][_zz()].astype(np.int64)


def make_block(draw, q: int, rng, accept=None, tries: int = 4000) -> np.ndarray:
    """A block of draw(rng)'s values that needs no clipping and that the oracle quantises
    back to them (accept: another test of the oracle's values, for blocks that only need a
    property).  Plain rounding first; its error follows a sparse block's few waves and
    lands on their own coefficients (a lone value of 1 at step 2 moves no pixel by half),
    so the further attempts round with a uniform dither of +-1/2, whose error is spread
    over all 64 coefficients (sigma 0.41 each)."""
    for t in range(tries):
        want = np.asarray(draw(rng), np.int64)
        for d in range(1 if rng is None else 4):
            px, ok = pixels(want, q, rng.uniform(-0.5, 0.5, (8, 8)) if d else None)
            if not ok:
                continue
            got = quantised(px, q)
            if accept(got) if accept else np.array_equal(got, want):
                return px
    raise AssertionError("no block found")


def _mag(rng, size: int) -> int:
    """a value of the size (category), either sign"""
    return int(rng.integers(1 << (size - 1), 1 << size)) * (1 if rng.integers(2) else -1)


def flat_block(dc: int = 0, q: int = 2) -> np.ndarray:
    v = np.zeros(64, np.int64)
    v[0] = dc
    return make_block(lambda r: v, q, None)


def run_block(run: int, size: int, n: int, q: int, rng, dc: int = 0) -> np.ndarray:
    """n symbols (run, size): non-zero at zig-zag (run + 1) k, k = 1..n."""
    def draw(r):
        v = np.zeros(64, np.int64)
        v[0] = dc
        for k in range(1, n + 1):
            v[(run + 1) * k] = _mag(r, size)
        return v
    return make_block(draw, q, rng)


def rare_block(q: int, rng, dc: int = 0, size: int = 6) -> np.ndarray:
    """The eight symbols (r, size), r = 0..7, once each (values +-2^(size-1)), then EOB."""
    def draw(r):
        v = np.zeros(64, np.int64)
        v[0] = dc
        p = 0
        for run in range(8):
            p += run + 1
            v[p] = (1 << (size - 1)) * (1 if r.integers(2) else -1)
        return v
    return make_block(draw, q, rng)


def chain_blocks(chain, q: int, rng) -> list:
    """Whole blocks of one symbol each: symbol (run, size) `count` times for every
    ((run, size), count) of the chain (63 // (run + 1) per block, the rest in a last one)."""
    out = []
    for (run, size), count in chain:
        cap = 63 // (run + 1)
        while count > 0:
            out.append(run_block(run, size, min(cap, count), q, rng))
            count -= cap
    return out


def full_variants(q: int, rng, n: int = 4, dc: int = 70) -> tuple:
    """Two lists of n blocks whose 63 AC values all have size 7 and whose DC values are
    near +dc and -dc (|dc| >= 64: every DC difference between the two kinds, and from 0,
    has category >= 7).  At q = 1 rounding moves values by one, so the block is accepted on
    what the oracle finds (every AC size 7, |DC| >= 66), not on exact values."""
    def draw(sign):
        def f(r):
            v = r.integers(65, 70, 64) * np.where(r.integers(0, 2, 64) == 1, 1, -1)
            v[0] = sign * dc
            return v
        return f

    def accept(sign):
        return lambda g: bool(np.all(np.abs(g[1:]) >= 64) and np.all(np.abs(g[1:]) <= 127) and sign * g[0] >= 66)
    return tuple([make_block(draw(s), q, rng, accept(s), tries=100000) for _ in range(n)] for s in (1, -1))


def sparse7_variants(q: int, rng, dc: int = 32) -> tuple:
    """Two blocks of eight (0, 7) symbols and an EOB with DC +dc and -dc: continuation
    records at a step where a block of 63 such values cannot exist."""
    def draw(sign):
        def f(r):
            v = np.zeros(64, np.int64)
            v[1:9] = r.integers(66, 80, 8) * np.where(r.integers(0, 2, 8) == 1, 1, -1)
            v[0] = sign * dc
            return v
        return f
    return tuple(make_block(draw(s), q, rng) for s in (1, -1))


def assemble(blocks: list, bw: int, bh: int) -> np.ndarray:
    """bw x bh blocks in raster order -> the (8 bh, 8 bw) plane"""
    assert len(blocks) == bw * bh
    return np.ascontiguousarray(np.stack(blocks).reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(8 * bh, 8 * bw))


@dataclass(frozen=True)
class Frame:
    name: str
    plane: np.ndarray       # (h, w) uint8
    q: int                  # the uniform luma table's step
    meta: dict = field(default_factory=dict)

    @property
    def qy(self) -> np.ndarray:
        return np.full(64, self.q, np.uint8)

    @property
    def size(self) -> tuple:
        return self.plane.shape[1], self.plane.shape[0]


# ---- F1 "long groups" ----
F1_CHAIN = [((r, s), 8 << (13 - j)) for j, (r, s) in
            enumerate([(r, s) for r in range(4) for s in (1, 2, 3)] + [(4, 1), (4, 2)])]


def _f1(name: str, rare_at, seed: int) -> Frame:
    bw = bh = 50
    rng = np.random.default_rng(seed)
    body = chain_blocks(F1_CHAIN, 2, rng)
    nb = bw * bh
    assert len(body) + len(rare_at) <= nb
    body += [flat_block()] * (nb - len(rare_at) - len(body))
    for at in sorted(rare_at):
        body.insert(at, rare_block(2, rng))
    return Frame(name, assemble(body, bw, bh), 2, {"rare": tuple(sorted(rare_at))})


@functools.lru_cache(maxsize=None)
def f1() -> Frame:
    """400x400: the chain, one rare block in the middle of the block order."""
    return _f1("F1", (1250,), 11)


@functools.lru_cache(maxsize=None)
def f1p() -> Frame:
    """400x400: rare blocks at the frame's first and last block and at block 127."""
    return _f1("F1'", (0, 127, 2499), 12)


# ---- F2 "full blocks" ----
@functools.lru_cache(maxsize=None)
def _f2_variants(seed: int):
    return full_variants(1, np.random.default_rng(seed))


def _f2(name: str, bw: int, bh: int, seed: int) -> Frame:
    pos, neg = _f2_variants(seed)
    blocks = [(pos if g % 2 == 0 else neg)[(g // 2) % len(pos)] for g in range(bw * bh)]
    return Frame(name, assemble(blocks, bw, bh), 1)


@functools.lru_cache(maxsize=None)
def f2a(seed: int = 21) -> Frame:
    """1024x16: 256 blocks, two whole tiles of alternating variants."""
    return _f2("F2a" if seed == 21 else f"F2a/{seed}", 128, 2, seed)


@functools.lru_cache(maxsize=None)
def f2b() -> Frame:
    """1032x24: 387 blocks, a ragged last tile."""
    return _f2("F2b", 129, 3, 21)


# ---- F3 "run sweep" ----
F3_DC = (0, 1, -2, 5, -9, 20, -40, 90, -90, 300, 3)


@functools.lru_cache(maxsize=None)
def f3() -> Frame:
    """520x256 = 2080 blocks: every pair i < j of zig-zag positions 1..63 alone in a block,
    every single position, one block of all 63, the rest flat; sizes 1 to 3."""
    bw, bh = 65, 32
    rng = np.random.default_rng(31)
    support = [(i, j) for i in range(1, 64) for j in range(i + 1, 64)] + [(i,) for i in range(1, 64)]
    support.append(tuple(range(1, 64)))
    support += [()] * (bw * bh - len(support))
    blocks = []
    for g, pos in enumerate(support):
        def draw(r, pos=pos, g=g):
            v = np.zeros(64, np.int64)
            v[0] = F3_DC[g % len(F3_DC)]
            for p in pos:
                v[p] = _mag(r, int(r.integers(1, 4)))
            return v
        blocks.append(make_block(draw, 2, rng))
    return Frame("F3", assemble(blocks, bw, bh), 2, {"support": tuple(support)})


# ---- F4 "chroma": three planes for JPGE_FMT_YUV444_PLANAR at 4:4:4 ----
# (a chain that grows like Fibonacci numbers: the deepest tree for the fewest symbols,
# so that it fits 96 blocks)
F4_CHAIN = list(zip([(0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 1), (2, 2), (2, 3), (3, 1), (3, 2)],
                    [712, 440, 272, 168, 104, 64, 40, 24, 16, 8, 8]))


@dataclass(frozen=True)
class Frame3:
    name: str
    planes: tuple           # Y, Cb, Cr: (h, w) uint8
    qy: np.ndarray
    qc: np.ndarray

    @property
    def size(self) -> tuple:
        return self.planes[0].shape[1], self.planes[0].shape[0]

    @property
    def frame(self) -> np.ndarray:
        return np.ascontiguousarray(np.stack(self.planes))


@functools.lru_cache(maxsize=None)
def f4() -> Frame3:
    """96x64, qc = full(64, 2): Y flat 128; Cb the chain; Cr the rare block, then pairs of
    blocks with eight size-7 values and DC differences of category 7."""
    bw, bh = 12, 8
    rng = np.random.default_rng(41)
    cb = chain_blocks(F4_CHAIN, 2, rng)
    cb += [flat_block()] * (bw * bh - len(cb))
    pos, neg = sparse7_variants(2, rng)
    cr = [rare_block(2, rng, dc=-32)] + [pos, neg] * 8
    cr += [flat_block(dc=-32)] * (bw * bh - len(cr))
    y = np.full((8 * bh, 8 * bw), 128, np.uint8)
    return Frame3("F4", (y, assemble(cb, bw, bh), assemble(cr, bw, bh)), np.ones(64, np.uint8), np.full(64, 2, np.uint8))


@functools.lru_cache(maxsize=None)
def f4full() -> Frame3:
    """96x64, qc all ones: Y flat 128; Cb and Cr F2's alternating full blocks.  (A block
    whose 63 AC values all quantise to 64 or more at step 2 needs coefficients of at least
    127 each: 63 * 127^2 + a DC is more than 98 % of the 64 * 128^2 that 64 pixels in
    [-128, 127] can hold at all, so the 128-record chroma block takes a table of ones.)"""
    bw, bh = 12, 8
    pos, neg = _f2_variants(21)
    cb = [(pos if g % 2 == 0 else neg)[(g // 2) % len(pos)] for g in range(bw * bh)]
    cr = [(neg if g % 2 == 0 else pos)[(g // 3) % len(pos)] for g in range(bw * bh)]
    y = np.full((8 * bh, 8 * bw), 128, np.uint8)
    return Frame3("F4full", (y, assemble(cb, bw, bh), assemble(cr, bw, bh)), np.ones(64, np.uint8), np.ones(64, np.uint8))


GRAY_FRAMES = {"F1": f1, "F1'": f1p, "F2a": f2a, "F2b": f2b, "F3": f3}


@functools.lru_cache(maxsize=None)
def built(name: str, restart: int = 0, seed: int = 0) -> G.Built:
    """_gray.build of a gray frame at its table, computed once."""
    f = f2a(seed) if seed else GRAY_FRAMES[name]()
    return G.build(f.plane, f.qy, restart)


# ---- the record model ----
def lengths(text) -> dict:
    """symbol -> code length of the oracle's table for a text"""
    return {s: ln for s, ln, _ in _oracle.huffman(text)}


def records(blocks, dc_len: dict, ac_len: dict) -> list:
    """Per block, the bit counts of its records in stream order (blocks: _gray.Built.blocks)."""
    out = []
    for b in blocks:
        r = []
        for k, (sym, size, _) in enumerate(b):
            r.append((dc_len if k == 0 else ac_len)[sym] + min(size, REC_X_BITS))
            if size > REC_X_BITS:
                r.append(size - REC_X_BITS)
        out.append(r)
    return out


@dataclass(frozen=True)
class Metrics:
    widest4: int        # the widest sum over 4 consecutive records of the stream
    long_run: int       # the longest run of consecutive records of >= LONG bits
    block_long_run: int  # the longest such run inside one block
    max_records: int    # the most records of one block
    full_blocks: int    # blocks of 128 records


def metrics(recs: list) -> Metrics:
    flat = np.array([n for r in recs for n in r], np.int64)
    c = np.concatenate([[0], np.cumsum(flat)])
    widest = int((c[4:] - c[:-4]).max()) if flat.size >= 4 else int(flat.sum())

    def longest(a):
        best = cur = 0
        for n in a:
            cur = cur + 1 if n >= LONG else 0
            best = max(best, cur)
        return best
    return Metrics(widest, longest(flat), max(longest(r) for r in recs), max(len(r) for r in recs),
                   sum(len(r) == 128 for r in recs))


def gray_metrics(b: G.Built) -> Metrics:
    return metrics(records(b.blocks, lengths(b.dc_text), lengths(b.ac_text)))


@dataclass(frozen=True)
class Chroma:
    cb: G.Built
    cr: G.Built
    dc_text: tuple      # the C-DC text: every Cb block's category, then every Cr block's
    ac_text: tuple      # the C-AC text, in the same order
    metrics: Metrics    # of the chroma records (tables 2 and 3), each component's blocks in order


@functools.lru_cache(maxsize=None)
def chroma(name: str) -> Chroma:
    f = {"F4": f4, "F4full": f4full}[name]()
    cb, cr = G.build(f.planes[1], f.qc), G.build(f.planes[2], f.qc)
    dc_text, ac_text = cb.dc_text + cr.dc_text, cb.ac_text + cr.ac_text
    return Chroma(cb, cr, dc_text, ac_text, metrics(records(cb.blocks + cr.blocks, lengths(dc_text), lengths(ac_text))))


def rgb(plane: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(np.repeat(plane[:, :, None], 3, 2))
