"""tests/_stream3.py, the GPU tests' CPU-built three-component file, is right before it judges
anything (no GPU here):

- fed an RGB frame's planes (every pixel through the oracle's colour conversion) it gives
  _oracle.encode's bytes in all six subsampling modes, at several qualities, with and without
  restart intervals: this pins the DC chains, the four texts and their order, the per-image
  tables, the header and the scan to the reference;
- every expected file of test_gpu_stream3.py decodes (the host decoder) to build3's own
  coefficients, and Pillow opens it;
- given its own tables back as specs it returns the same bytes;
- the frames of CONTENT hold, in the texts build3 returns, the symbols they are there for."""
import io

import numpy as np
import pytest

import _adversarial as A
import _oracle
import _stream3 as S
import _yuv as Y
import _yuv10 as T
import jpgenc_amd as J

SIZES = [(1, 1), (16, 16), (33, 17), (130, 50)]
BIG = 60000  # a restart interval above every MCU count here
# (quality, restart): restart 0, 1, 3 and one value above the MCU count; qualities 50, 90, 100
SETTINGS = [(50, 0), (90, 0), (100, 0), (90, 1), (100, 3), (50, 3), (90, BIG)]


@pytest.fixture(scope="module")
def rgb_planes():
    cache = {}

    def get(w, h, mode, maxval=255):
        # (the conversion once per frame; the padding depends on the mode's MCU)
        k = (w, h, maxval)
        if k not in cache:
            rgb = (J.synth_rgb8(3 * w + h, w, h).astype(np.uint32) * maxval // 255).astype(np.uint8)
            cache[k] = (rgb, S.rgb_planes(rgb, 444, maxval))
        rgb, p = cache[k]
        mw, mh = Y.mcu_size(mode)
        return rgb, [np.pad(a[:h, :w], ((0, -h % mh), (0, -w % mw)), mode="edge") for a in p]
    return get


# ---- 1. oracle parity ----
def test_rgb_planes_are_the_oracles():
    # the Y plane and the S420_m chroma planes of the oracle's own stage dump
    w, h = 33, 17
    rgb = J.synth_rgb8(5, w, h)
    y, cb, cr = S.rgb_planes(rgb, 420)
    want = [np.zeros((32, 48)), np.zeros((16, 24)), np.zeros((16, 24))]
    _oracle.orc().orc_stage_ycc(_oracle._p(rgb), w, h, 255, *(_oracle._p(a) for a in want))
    assert np.array_equal(y, want[0])
    assert np.array_equal(_oracle.subsample_mode(cb, 420), want[1]) and np.array_equal(_oracle.subsample_mode(cr, 420), want[2])


@pytest.mark.parametrize("mode", S.ALL_MODES)
@pytest.mark.parametrize("w,h", SIZES)
def test_build3_equals_the_oracle(rgb_planes, mode, w, h):
    rgb, planes = rgb_planes(w, h, mode)
    for quality, restart in SETTINGS:
        qy, qc = _oracle.quality_tables(quality)
        b = S.build3(planes, w, h, qy, qc, mode, restart)
        want = _oracle.encode(rgb, quality, restart=restart, subsampling=mode)
        assert not S.difference(b.jpg, want), (quality, restart, S.difference(b.jpg, want))
        assert (b.jpg.count(b"\xff\xdd") >= 1) == bool(restart)


@pytest.mark.parametrize("mode", S.ALL_MODES)
def test_build3_equals_the_oracle_maxval_100(rgb_planes, mode):
    w, h = 33, 17
    rgb, planes = rgb_planes(w, h, mode, maxval=100)
    assert rgb.max() <= 100
    for restart in (0, 3):
        qy, qc = _oracle.quality_tables(90)
        b = S.build3(planes, w, h, qy, qc, mode, restart)
        d = S.difference(b.jpg, _oracle.encode(rgb, 90, maxval=100, restart=restart, subsampling=mode))
        assert not d, (restart, d)


def test_coefficients_are_want_coeffs():
    c = S.Case(S.Z.YUYV, 141, 27, mode=411)
    want = Y.want_coeffs(S.planes(c), 411, 75)
    got = S.coefficients(S.planes(c), 411, *_oracle.quality_tables(75))
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


def test_texts_are_the_oracles_histograms():
    # 4:2:0 without restart: the oracle's own counts and first occurrences of the four texts
    rgb = J.synth_rgb8(9, 80, 48)
    b = S.build3(S.rgb_planes(rgb, 420), 80, 48, *_oracle.quality_tables(75))
    counts, first = _oracle.stage_hist(rgb, 75)
    for t in range(4):
        got = np.zeros(256, np.int64)
        np.add.at(got, np.asarray(b.texts[t], np.int64), 1)
        assert np.array_equal(got, counts[t])
        for s in np.nonzero(got)[0]:
            assert b.texts[t].index(int(s)) == first[t][s]


def test_difference_names_the_part():
    rgb = J.synth_rgb8(2, 40, 24)
    jpg = S.build3(S.rgb_planes(rgb, 420), 40, 24, *_oracle.quality_tables(75)).jpg
    segs, scan = S.F.segments(jpg)
    assert S.difference(jpg, jpg) == ""
    flip = lambda i: jpg[:i] + bytes([jpg[i] ^ 1]) + jpg[i + 1:]  # noqa: E731
    assert "segment DQT" in S.difference(flip(30), jpg)
    dht = jpg.index(b"\xff\xc4")
    assert "DHT segment 1 (Y-DC)" in S.difference(flip(dht + 6), jpg)
    last = len(jpg) - 2 - jpg[::-1].index(b"\xc4\xff")  # the last DHT marker
    assert "DHT segment 4 (C-AC)" in S.difference(flip(last + 6), jpg)
    assert "in the scan, byte 3 " in S.difference(flip(scan + 3), jpg)
    assert "in the scan" in S.difference(jpg[:-5], jpg)


# ---- 2. every expected file of the GPU tests ----
ALL = S.every_case()


@pytest.mark.parametrize("case", ALL, ids=[c.name for c in ALL])
def test_expected_file_decodes(case):
    b = S.built(case)
    w, h = case.size
    info, y, cb, cr = J.decode_coeffs(b.jpg)
    assert (info.width, info.height) == (w, h)
    assert (info.yh, info.yv) == _oracle.SHAPES[case.mode]
    for got, want in zip((y, cb, cr), b.coef):
        assert np.array_equal(got, want)
    Image = pytest.importorskip("PIL.Image")
    im = Image.open(io.BytesIO(b.jpg))
    im.load()
    assert im.size == (w, h) and im.layers == 3


def test_the_cases_cover_what_they_claim():
    names = [c.name for c in S.CASES]
    assert len(set(names)) == len(names)
    assert max(c.size[0] for c in ALL) <= 200 and max(c.size[1] for c in ALL) <= 100
    assert max(c.w for c in ALL) <= 200 and max(c.h for c in ALL) <= 100
    # the samples have the frame's size, in the layout's chroma shape
    for c in ALL:
        if c.scale == 1:
            y, cb, cr = S.samples(c)
            ch, cw = {S.HALF: ((c.h + 1) // 2, (c.w + 1) // 2), S.FULL: (c.h, c.w), S.P422: (c.h, (c.w + 1) // 2),
                      S.P10: ((c.h + 1) // 2, (c.w + 1) // 2)}[S.family(c.fmt)]
            assert y.shape == (c.h, c.w) and cb.shape == cr.shape == (ch, cw), c.name
    # the 10-bit frames hold 1023 and samples that are no multiple of 4, in every plane
    for c in ALL:
        if c.fmt in T.FORMATS:
            for p in S.samples(c):
                assert p.max() == 1023 and (p % 4 != 0).sum() > p.size // 2
    # a restart case really has several intervals, a fixed-table case Annex K's tables
    for c in ALL:
        b = S.built(c)
        if c.restart:
            assert b.jpg.count(b"\xff\xd0") >= 1 and b.jpg.count(b"\xff\xd1") >= 1
        if c.huff == "standard":
            assert [tuple(map(list, s)) for s in b.specs] == [tuple(map(list, J.standard_huffman(t))) for t in range(4)]
    # the downscaled cases: D's size, and D is not the source
    for c in ALL:
        if c.scale != 1:
            d = S._source(c)[1]
            assert c.size == (-(-c.w // c.scale), -(-c.h // c.scale)) == (d.width, d.height)
            assert c.w % c.scale and c.h % c.scale  # (the last cell of a row and of a column is clamped)


# ---- 3. consistency ----
@pytest.mark.parametrize("case", [S.Case(Y.NV12, 33, 17), S.Case(Y.YUV444, 136, 24, mode=411),
                                  S.Case(S.Z.YUYV, 141, 27, "photo", mode=422, restart=3),
                                  S.CONTENT[S.HALF][2], S.CONTENT[S.FULL][4]], ids=lambda c: c.name)
def test_own_tables_given_back(case):
    b = S.built(case)
    again = S.build3(S.planes(case), *case.size, *S.tables(case), case.mode, case.restart, specs=b.specs)
    assert again.jpg == b.jpg and again.texts == b.texts
    assert S.F.dht_specs(b.jpg) == [(list(s[0]), list(s[1])) for s in b.specs]


# ---- 4. what the content frames hold ----
def _properties(b: S.Built3) -> dict:
    return {"dc11": 11 in b.texts[2],
            "ac10": any(s & 15 == 10 for s in b.texts[3]),
            "full": any(len(blk) == 64 for blk in b.chroma_blocks)}


@pytest.mark.parametrize("path", [S.HALF, S.FULL])
def test_content_conditions(path):
    assert np.all(_oracle.quality_tables(100)[0] == 1) and np.all(_oracle.quality_tables(100)[1] == 1)
    props = {c.name: _properties(S.built(c)) for c in S.CONTENT[path]}
    by_kind = {}
    for c in S.CONTENT[path]:
        by_kind.setdefault(c.kind, []).append(props[c.name])
    # each property, from the texts of the file: in its own frame, and so in the list
    assert all(p["dc11"] for p in by_kind["checker"])
    assert all(p["ac10"] for p in by_kind["edges"])
    assert all(p["full"] for p in by_kind["noise"])
    for k in ("dc11", "ac10", "full"):
        assert any(p[k] for p in props.values()), k
    for c in S.CONTENT[path]:
        assert c.mode == (420 if path == S.HALF else 444) and S.family(c.fmt) == path


def test_content_f4_frames_are_the_adversarial_ones():
    # the 4:4:4 chroma texts of F4 and F4full as _adversarial.chroma restates them
    for c in S.CONTENT[S.FULL]:
        if c.kind in ("F4", "F4full"):
            b, a = S.built(c), A.chroma(c.kind)
            assert b.texts[2] == a.dc_text and b.texts[3] == a.ac_text
            assert np.array_equal(b.coef[1], a.cb.coef) and np.array_equal(b.coef[2], a.cr.coef)
    full = S.built(S.CONTENT[S.FULL][3])
    assert S.CONTENT[S.FULL][3].kind == "F4full" and all(len(blk) == 64 for blk in full.chroma_blocks)
