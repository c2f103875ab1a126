"""The three-component file built on the CPU: the expected bytes of every Y, Cb, Cr layout's
whole-file test, in whose making no GPU code runs.

build3 takes padded fp64 planes (the form of _yuv.pad_planes) and restates writeJPEG's steps
after the planes from parts that are pinned already:

  1. the quantised coefficients: _yuv.want_coeffs' steps at given tables (the oracle's
     subsample_mode, DCT and quantiser);
  2. the DC differences in MCU order (Image.cpp:638-678: an MCU's Y blocks row by row; the
     predictions restart with every restart interval);
  3. zig-zag, RLE_AC and the category code through the host C ABI entries that _fixedhuff uses
     (jpge_rle_ac, jpge_encode_category: pinned to the reference by test_coding.py);
  4. the four texts in the order the reference builds them (Image.cpp:888-906): Y-DC and
     Y-AC over the Y plane's blocks in raster order (the plane's, not the MCUs': the
     differences of step 2 are taken in MCU order and then read in raster order); C-DC and
     C-AC over every Cb block in raster order, then every Cr block (the component order that
     _adversarial.chroma restates);
  5. the per-image tables: _oracle.huffman of each text, as (bits, huffval);
  6. the header and the scan: _fixedhuff.expected_coeffs with those tables.

test_stream3_cpu.py pins build3 to _oracle.encode in all six subsampling modes, with and
without restart intervals, before it judges anything, and shows that the frames of CONTENT
hold the symbols they are meant to hold.

The second half of the file is the list of inputs that test_gpu_stream3.py encodes (CASES,
CONTENT, PLANES): each a Case, whose samples, frame, planes and expected file come from here,
so that the CPU test can decode every expected file before a GPU sees its input."""

from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import _adversarial as A
import _downscale as D
import _fixedhuff as F
import _oracle
import _yuv as Y
import _yuv10 as T
import _yuv422 as Z
import _yuvxf as X
import jpgenc_amd as J


@dataclass(frozen=True)
class Built3:
    jpg: bytes
    coef: tuple        # (Y, Cb, Cr): (blocks, 64) int16 before DC differencing, raster block order
    texts: tuple       # (Y-DC, Y-AC, C-DC, C-AC): tuples of symbols
    specs: tuple       # the four tables the file carries: (bits, huffval) each
    chroma_blocks: tuple  # symbols of each chroma block (DC included): every Cb block, then every Cr block


# ---- the builder ----
def spec_of(table) -> tuple:
    """(bits, huffval) of _oracle.huffman's [(symbol, length, code)] (DHT order)."""
    bits = [0] * 16
    for _, ln, _ in table:
        bits[ln - 1] += 1
    return tuple(bits), tuple(s for s, _, _ in table)


def dc_differences(y, cb, cr, w: int, h: int, mode: int, restart: int = 0):
    """The three coefficient arrays with each block's DC replaced by its difference: the
    chains of Image.cpp:638-678 in MCU order, all three reset at the first MCU of every
    restart interval (restart: MCUs per interval, 0 = one interval)."""
    yh, yv = _oracle.SHAPES[mode]
    mw, mh = -(-w // (8 * yh)), -(-h // (8 * yv))
    ybw = mw * yh
    out = [np.array(p, np.int32) for p in (y, cb, cr)]
    assert out[0].shape[0] == ybw * mh * yv and out[1].shape[0] == out[2].shape[0] == mw * mh
    pred = [0, 0, 0]
    for m in range(mw * mh):
        if restart and m % restart == 0:
            pred = [0, 0, 0]
        mr, mc = divmod(m, mw)
        at = [[(mr * yv + k // yh) * ybw + mc * yh + k % yh for k in range(yh * yv)], [m], [m]]
        for c in range(3):
            for g in at[c]:
                v = int(out[c][g, 0])
                out[c][g, 0] = v - pred[c]
                pred[c] = v
    return out


def coefficients(planes, mode: int, qy, qc):
    """_yuv.want_coeffs at given tables instead of a quality's: _oracle.subsample_mode on the
    chroma planes, then the oracle's DCT and quantiser (test_stream3_cpu.py holds the two equal
    at a quality's tables)."""
    y, cb, cr = (np.ascontiguousarray(p, np.float64) for p in planes)
    return (Y._blocks(y, qy), Y._blocks(_oracle.subsample_mode(cb, mode), qc),
            Y._blocks(_oracle.subsample_mode(cr, mode), qc))


def block_symbols(blocks) -> list:
    """Per block (DC already a difference) its symbols: the DC category, then the AC symbols."""
    return [tuple(s for s, _, _ in J.encode_category(J.rle_ac(b, zigzag_scan=True))) for b in blocks]


def build3(planes, w: int, h: int, qy, qc, mode: int = 420, restart: int = 0, specs=None) -> Built3:
    """The whole file of a w x h frame given as three padded fp64 planes (Y, Cb, Cr; whole
    MCUs of the mode, chroma at full size as _yuv.pad_planes returns it), at tables qy, qc
    (natural order), with per-image tables (specs None) or the four given."""
    qy, qc = np.ascontiguousarray(qy, np.uint8), np.ascontiguousarray(qc, np.uint8)
    y, cb, cr = coefficients(planes, mode, qy, qc)
    sy, scb, scr = (block_symbols(p) for p in dc_differences(y, cb, cr, w, h, mode, restart))
    chroma = scb + scr
    texts = (tuple(b[0] for b in sy), tuple(s for b in sy for s in b[1:]),
             tuple(b[0] for b in chroma), tuple(s for b in chroma for s in b[1:]))
    if specs is None:
        specs = [spec_of(_oracle.huffman(t)) for t in texts]
    specs = tuple((tuple(int(b) for b in s[0]), tuple(int(v) for v in s[1])) for s in specs)
    jpg = F.expected_coeffs(y, cb, cr, w, h, qy, qc, specs, mode, restart)
    return Built3(jpg, (y, cb, cr), texts, specs, tuple(chroma))


def where(jpg: bytes, i: int) -> str:
    """The part of a file that byte i lies in: a header segment by name, or the scan."""
    names = {0xE0: "APP0", 0xDB: "DQT", 0xC0: "SOF0", 0xC4: "DHT", 0xDD: "DRI", 0xDA: "SOS"}
    if i < 2:
        return "in SOI"
    segs, scan = F.segments(jpg)
    if i >= scan:
        return f"in the scan, byte {i - scan} of {len(jpg) - 2 - scan}" if i < len(jpg) - 2 else "in EOI"
    p, dht = 2, 0
    for m, body in segs:
        n = len(body) + 4
        if m == 0xC4:
            dht += 1
        if i < p + n:
            if m == 0xC4:
                return f"in DHT segment {dht} ({('Y-DC', 'Y-AC', 'C-DC', 'C-AC')[2 * (body[0] & 15) + (body[0] >> 4)]}), byte {i - p}"
            return f"in the header, segment {names.get(m, hex(m))}, byte {i - p}"
        p += n
    return ""


def difference(got: bytes, want: bytes) -> str:
    """'' when equal; otherwise the first differing byte and where in the expected file it lies."""
    if got == want:
        return ""
    n = min(len(got), len(want))
    i = next((k for k in range(n) if got[k] != want[k]), n)
    return (f"{len(got)} bytes for {len(want)}, first difference at byte {i} "
            f"({got[i:i + 4].hex()} for {want[i:i + 4].hex()}) {where(want, min(i, len(want) - 1))}")


# ---- planes ----
def planes_of(fmt: int, frame_or_samples, transform=None, mode: int = 420):
    """The padded fp64 planes [Y, Cb, Cr] of a frame in layout fmt, for build3 and
    Encoder.encode_planes: a thin dispatcher over _yuv, _yuv422, _yuv10, _yuvxf and _downscale.
    frame_or_samples: the (y, cb, cr) samples in the layout's own chroma shape, or an NV12
    frame as pack_yuv420 / downscale_frame returns it.  transform: the eight coefficients of
    jpge_set_yuv_transform in force (None: FULL_601)."""
    mcu = Y.mcu_size(mode)
    if fmt == Y.NV12 and hasattr(frame_or_samples, "width"):
        p = D.nv12_planes(frame_or_samples)[1:]
    else:
        p = tuple(frame_or_samples)
    if fmt in T.FORMATS:
        assert mode == 420
        return T.planes(*p, T.IDENTITY if transform is None else tuple(transform))
    if fmt in Z.FORMATS:
        fmt, p = Y.YUV444, Z.repeated(*p)
    assert fmt in Y.FORMATS
    if transform is None:
        return Y.pad_planes(fmt, *p, mcu=mcu)
    return X.planes(fmt, *p, tuple(transform), mcu=mcu)


def rgb_planes(rgb: np.ndarray, mode: int, maxval: int = 255):
    """The padded planes of an RGB frame: every pixel through the oracle's colour conversion
    (orc_ycc of byte * 255 / maxval), then edge-replicated to the mode's MCU (replication and
    a per-pixel map commute)."""
    L = _oracle.orc()
    rgb = np.ascontiguousarray(rgb, np.uint8)
    h, w = rgb.shape[:2]
    s = rgb.astype(np.float64) * (255. / maxval)
    out = np.zeros((h, w, 3), np.float64)
    px = np.zeros(3, np.float64)
    for r in range(h):
        for c in range(w):
            L.orc_ycc(s[r, c, 0], s[r, c, 1], s[r, c, 2], px.ctypes.data)
            out[r, c] = px
    mw, mh = Y.mcu_size(mode)
    return [np.pad(out[:, :, k], ((0, -h % mh), (0, -w % mw)), mode="edge") for k in range(3)]


# ---- the inputs of the GPU tests ----
HALF, FULL, P422, P10 = "half", "full", "422", "10"
CONTENT_SIZE = (96, 64)   # F4's and F4full's size


def family(fmt: int) -> str:
    return HALF if fmt in Y.HALF else FULL if fmt == Y.YUV444 else P422 if fmt in Z.FORMATS else P10


FMT_NAMES = {**Y.NAMES, **Z.NAMES, **T.NAMES}


@dataclass(frozen=True)
class Case:
    fmt: int
    w: int                  # the frame handed to the encoder (the source of a downscaled one)
    h: int
    kind: str = "random"    # random, photo, checker, edges, noise, F4, F4full
    quality: int = 90       # (F4 carries its own tables)
    mode: int = 420
    restart: int = 0
    xf: str = "full601"     # full601, or a name _yuvxf.coeffs takes
    huff: str = "optimal"   # optimal, standard (Annex K)
    scale: int = 1          # jpge_set_downscale (NV12)
    seed: int = 0

    @property
    def name(self) -> str:
        s = f"{FMT_NAMES[self.fmt]}-{self.w}x{self.h}-{self.kind}-q{self.quality}-{self.mode}"
        s += f"-r{self.restart}" if self.restart else ""
        s += f"-{self.xf}" if self.xf != "full601" else ""
        s += "-std" if self.huff == "standard" else ""
        s += f"-d{self.scale}" if self.scale != 1 else ""
        return s + (f"-s{self.seed}" if self.seed else "")

    @property
    def size(self) -> tuple:
        """The coded frame's size."""
        return J.downscaled_size(self.w, self.h, self.scale) if self.scale != 1 else (self.w, self.h)


@functools.lru_cache(maxsize=None)
def _photo(w: int, h: int):
    """Photo-like Y, Cb, Cr bytes: jpge_synth_rgb8 through the oracle's conversion, + 128,
    rounded and clipped."""
    return tuple(np.clip(np.rint(p[:h, :w] + 128.0), 0, 255).astype(np.uint8) for p in rgb_planes(J.synth_rgb8(w + h, w, h, kind=0), 444))


def _pattern(kind: str, ch: int, cw: int, rng):
    """Chroma planes (Cb, Cr) of CONTENT's frames: 8x8 cells of 0 / 255 as a checkerboard
    (adjacent blocks' DC values 2040 apart at a table of ones), the same cells moved by 4
    samples across (Cb) or down (Cr) (every block half 0, half 255: one AC value near 924),
    or random bytes (at a table of ones nearly no AC value rounds to 0)."""
    yy, xx = np.mgrid[0:ch, 0:cw]
    if kind == "checker":
        a = (yy // 8 + xx // 8) % 2
        return (255 * a).astype(np.uint8), (255 * (1 - a)).astype(np.uint8)
    if kind == "edges":
        return ((255 * ((yy // 8 + (xx + 4) // 8) % 2)).astype(np.uint8),
                (255 * (((yy + 4) // 8 + xx // 8) % 2)).astype(np.uint8))
    assert kind == "noise"
    return rng.integers(0, 256, (ch, cw), dtype=np.uint8), rng.integers(0, 256, (ch, cw), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _samples(fam: str, w: int, h: int, kind: str, seed: int):
    """(y, cb, cr) samples in the family's chroma shape (uint8; the 10-bit family uint16)."""
    rng = np.random.default_rng(7919 * w + 31 * h + seed)
    if kind in ("F4", "F4full"):
        assert fam == FULL and (w, h) == CONTENT_SIZE
        return tuple({"F4": A.f4, "F4full": A.f4full}[kind]().planes)
    if fam == P10:
        y, cb, cr = (np.array(p) for p in T.samples(7919 * w + 31 * h + seed, w, h))
        # the top of the range and the three values that are no multiple of 4, whatever the draw
        y.flat[0], cb.flat[0], cr.flat[-1] = 1023, 1023, 1023
        y.flat[-1], cb.flat[-1], cr.flat[0] = 1, 2, 3
        return y, cb, cr
    ch, cw = {HALF: ((h + 1) // 2, (w + 1) // 2), FULL: (h, w), P422: (h, (w + 1) // 2)}[fam]
    if kind == "photo":
        y, cb, cr = _photo(w, h)
        sy, sx = (2 if fam == HALF else 1), (1 if fam == FULL else 2)
        return y, cb[::sy, ::sx].copy(), cr[::sy, ::sx].copy()
    y = rng.integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "random":
        return y, rng.integers(0, 256, (ch, cw), dtype=np.uint8), rng.integers(0, 256, (ch, cw), dtype=np.uint8)
    return (y,) + _pattern(kind, ch, cw, rng)


@functools.lru_cache(maxsize=None)
def _source(c: Case):
    """The NV12 source frame of a downscaled case and its downscaled frame D (host code:
    jpge_downscale_frame, pinned by test_downscale_cpu.py)."""
    src = D.make(D.NV12, c.w, c.h, c.kind, 60 + c.seed, c.scale)
    return src, J.downscale_frame(src, D.NV12, c.scale)


def samples(c: Case):
    if c.scale != 1:
        return D.nv12_planes(_source(c)[1])[1:]
    return _samples(family(c.fmt), c.w, c.h, c.kind, c.seed)


def frame(c: Case):
    """What Encoder.encode takes for the case."""
    if c.scale != 1:
        return _source(c)[0]
    p = samples(c)
    if c.fmt in Z.FORMATS:
        return Z.build(c.fmt, *p)
    if c.fmt in T.FORMATS:
        return T.build(c.fmt, *p)
    return Y.build(c.fmt, *p)


def transform(c: Case):
    """(preset, the coefficients to hand to set_yuv_transform or None, those in force or None)."""
    return (J.JPGE_YUV_FULL_601, None, None) if c.xf == "full601" else X.coeffs(c.xf)


def tables(c: Case):
    if c.kind == "F4":
        return A.f4().qy, A.f4().qc
    return _oracle.quality_tables(c.quality)


@functools.lru_cache(maxsize=None)
def _planes(fam: str, w: int, h: int, kind: str, seed: int, xf: str, mode: int, scale: int):
    c = Case({HALF: Y.NV12, FULL: Y.YUV444, P422: Z.I422, P10: T.I010}[fam], w, h, kind, xf=xf, mode=mode, scale=scale, seed=seed)
    return planes_of(c.fmt, samples(c), transform(c)[2], mode)


def planes(c: Case):
    """The case's padded planes (one computation for the layouts of a family)."""
    return _planes(family(c.fmt), c.w, c.h, c.kind, c.seed, c.xf, c.mode, c.scale)


@functools.lru_cache(maxsize=None)
def _built(fam, w, h, kind, seed, xf, mode, scale, quality, restart, huff) -> Built3:
    c = Case({HALF: Y.NV12, FULL: Y.YUV444, P422: Z.I422, P10: T.I010}[fam], w, h, kind, quality, mode, restart, xf, huff, scale, seed)
    qy, qc = tables(c)
    return build3(planes(c), *c.size, qy, qc, mode, restart, F.golden_specs() if huff == "standard" else None)


def built(c: Case) -> Built3:
    """build3 of the case, computed once (the layouts of a family share it)."""
    return _built(family(c.fmt), c.w, c.h, c.kind, c.seed, c.xf, c.mode, c.scale,
                  0 if c.kind == "F4" else c.quality, c.restart, c.huff)


def configure(e, c: Case) -> None:
    """The case's settings on a context (an Encoder or a Group member's setters)."""
    preset, given, _ = transform(c)
    e.set_input_format(c.fmt)
    e.set_subsampling(c.mode)
    e.set_restart(c.restart)
    e.set_huffman(J.JPGE_HUFF_STANDARD if c.huff == "standard" else J.JPGE_HUFF_OPTIMAL)
    e.set_yuv_transform(preset, given)
    e.set_downscale(c.scale)


# a 4:2:0 tile is 64x16 px (test_gpu_yuv.py): one pixel, one MCU, one full tile, full + partial
# tile on two MCU rows, odd, several tiles
SIZES = [(1, 1), (16, 16), (64, 16), (80, 32), (33, 17), (130, 50)]
MODES = [444, 422, 411, 4200, 4201]
ALL_MODES = [420] + MODES
MODE_SIZES = [(9, 9), (136, 24)]         # the row-8 kernels' tile is 128x8 px
SIZES_422 = [(136 + 5, 24 + 3), (9, 9)]  # a ragged last tile; less than one block each way


def _cases() -> list:
    out = []
    # NV12, I420, YUV444_PLANAR (test_gpu_yuv.py)
    for fmt in Y.FORMATS:
        for w, h in SIZES:
            out += [Case(fmt, w, h, "photo" if q == 90 else "random", q) for q in (50, 90, 100)]
        out.append(Case(fmt, 130, 50, restart=3))
    out += [Case(Y.YUV444, w, h, mode=m) for m in MODES for w, h in MODE_SIZES]
    # YUYV, UYVY, NV16, I422 (test_gpu_yuv422.py)
    for fmt in Z.FORMATS:
        out += [Case(fmt, w, h, mode=m) for m in ALL_MODES for w, h in SIZES_422]
        out += [Case(fmt, *SIZES_422[0], "photo", mode=m, restart=3) for m in (422, 420)]
    # P010, I010 (test_gpu_yuv10.py)
    for fmt in T.FORMATS:
        for xf in ("full601", "limited709"):
            out += [Case(fmt, w, h, xf=xf) for w, h in ((33, 17), (130, 50))]
            out.append(Case(fmt, 130, 50, xf=xf, restart=3))
    # jpge_set_yuv_transform (test_gpu_yuvxf.py; its gray files come from _gray's builder already)
    for xf in ("limited601", "limited709", "full709", "custom"):
        out += [Case(Y.NV12, 130, 50, xf=xf), Case(Y.YUV444, 130, 50, xf=xf, mode=444)]
    out.append(Case(Y.NV12, 130, 50, xf="limited709", restart=3))
    # NV12 downscale (test_gpu_downscale.py): D is about 50 x 23, the source no multiple of the factor
    out += [Case(Y.NV12, 48 * s + 3, 20 * s + 5, scale=s) for s in D.FACTORS]
    # fixed tables on these layouts
    for w, h in ((33, 17), (130, 50)):
        out += [Case(Y.NV12, w, h, huff="standard"), Case(Z.YUYV, w, h, mode=422, huff="standard")]
    return out


CASES = _cases()

#: the frames whose chroma texts hold what random and photo-like frames never do (the
#: properties are asserted from built()'s texts in test_stream3_cpu.py), by chroma path
CONTENT = {
    HALF: [Case(fmt, *CONTENT_SIZE, k, 100) for fmt in Y.HALF for k in ("checker", "edges", "noise")],
    FULL: [Case(Y.YUV444, *CONTENT_SIZE, k, 100, mode=444) for k in ("checker", "edges", "noise", "F4full", "F4")],
}

#: planes handed to Encoder.encode_planes itself: random chroma bytes, 10-bit quarter steps,
#: the fp64 outputs of LIMITED_709; each again at restart 3
PLANES = [Case(fmt, 130, 50, xf=xf, restart=r) for fmt, xf in ((Y.NV12, "full601"), (T.P010, "full601"), (Y.NV12, "limited709"))
          for r in (0, 3)]


def every_case() -> list:
    """Every distinct expected file of the GPU tests."""
    seen, out = set(), []
    for c in CASES + CONTENT[HALF] + CONTENT[FULL] + PLANES:
        k = (family(c.fmt),) + tuple(getattr(c, f) for f in ("w", "h", "kind", "quality", "mode", "restart", "xf", "huff", "scale", "seed"))
        if k not in seen:
            seen.add(k)
            out.append(c)
    return out
