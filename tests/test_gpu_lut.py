"""Per-channel lookup tables (jpge_set_channel_lut): the .jpg of a frame coded with tables T is, byte
for byte, (a) the .jpg of M coded as JPGE_FMT_RGB8 with no tables on the same context, and (b) the
oracle's bytes of M, where M[y][x][c] = T[c][D[y][x][c]] and D is the frame's RGB8 frame (a Bayer
mosaic: demosaic_frame's).  M is built in numpy (_lut.mapped); test_lut_cpu.py pins jpge_lut_frame
to the same statement.  Every comparison is exact.

The cases are small frames that code in well under a millisecond, so each group walks its whole set
of cases in loops and names the failing case in the assertion.  The four groups
(matrix, modes and settings, state and batches, refusals) are plain functions, as the groups of
test_gpu_bayer.py are; one test at the end of the file runs them in turn (about a second in all),
so that the file adds one entry to every later run of the suite, not one per group."""
import functools

import numpy as np
import pytest

import _bayer as B
import _fixedhuff
import _lut as L
import _oracle
import jpgenc_amd as J

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

E_ARG = 1
# W x H: test_gpu_bayer.py's set (one run, one tile, partial runs, an interior tile, the two-pixel
# strips of both kernels' tiles, a frame of many tiles with nothing aligned)
SIZES = [(2, 2), (3, 3), (16, 16), (64, 16), (65, 17), (66, 18), (130, 34), (192, 48), (157, 37), (2, 200), (200, 2), (517, 131)]
ALL_MODES = (420, 4200, 4201, 444, 422, 411)
PERM, PERM2 = L.TABLES["perm"], L.TABLES["perm2"]


@pytest.fixture(scope="module")
def enc4():
    e = J.Encoder(0, lanes=4)
    yield e
    e.close()


@pytest.fixture(scope="module")
def enc1():
    e = J.Encoder(0, lanes=1)
    yield e
    e.close()


def _reset(e):
    e.set_channel_lut(None)
    e.set_orientation(J.JPGE_ORIENT_NONE)
    e.set_downscale(1)
    e.set_input_format(J.JPGE_FMT_RGB8)
    e.set_subsampling(420)
    e.set_restart(0)
    e.set_huffman(J.JPGE_HUFF_OPTIMAL)


@pytest.fixture(autouse=True)
def _defaults(enc4, enc1):
    yield
    for e in (enc4, enc1):
        _reset(e)


@functools.lru_cache(maxsize=None)
def _frame(fmt, w, h, seed=1):
    a = L.noise(fmt, w, h, seed)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _m(fmt, w, h, seed=1, table="perm"):
    m = L.mapped(_frame(fmt, w, h, seed), fmt, L.TABLES[table])
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _want(fmt, w, h, seed=1, table="perm", quality=90, mode=420):
    """(b): computed once per case, shared by the variants and the contexts."""
    return _oracle.encode(_m(fmt, w, h, seed, table), quality, subsampling=mode)


def _encode(e, frame, fmt, variant, quality=90, **kw):
    """One frame in layout fmt through context e with its current settings (tables included)."""
    if variant == "host":
        e.set_input_format(fmt)
        return e.encode(frame, quality, **kw)
    assert not kw
    return e.encode_tensor(L.device_view(torch, frame, variant), quality, **L.tensor_kwargs(fmt))


def _plain(e, m, quality=90, **kw):
    """(a): M coded as RGB8 with no tables on the same context; the tables in force come back."""
    t = e.channel_lut()
    e.set_channel_lut(None)
    e.set_input_format(J.JPGE_FMT_RGB8)
    got = e.encode(m, quality, **kw)
    e.set_channel_lut(t)
    return got


# ---- 1. the matrix: layouts x sizes x input variants, both contexts ----
def _matrix(enc4, enc1):
    for lanes, e in ((4, enc4), (1, enc1)):
        e.set_channel_lut(PERM)
        for fmt in L.LAYOUTS:
            for w, h in SIZES:
                case = (lanes, L.NAMES[fmt], w, h)
                src, want = _frame(fmt, w, h), _want(fmt, w, h)
                assert _plain(e, _m(fmt, w, h)) == want, (case, "the RGB8 encode of M differs from the oracle")
                for variant in L.VARIANTS:
                    assert _encode(e, src, fmt, variant) == want, (case, variant)


# ---- 2. subsampling modes and the other settings ----
def _modes_and_settings(enc4):
    e = enc4
    e.set_channel_lut(PERM)
    for fmt in L.LAYOUTS:
        name = L.NAMES[fmt]
        for mode in ALL_MODES:
            e.set_subsampling(mode)
            for w, h in ((130, 34), (157, 37)):
                src, want = _frame(fmt, w, h, 2), _want(fmt, w, h, 2, "perm", 90, mode)
                for variant in L.VARIANTS:
                    assert _encode(e, src, fmt, variant) == want, (name, mode, w, h, variant)
                assert _plain(e, _m(fmt, w, h, 2)) == want, (name, mode, w, h)
        e.set_subsampling(420)

        w, h = 130, 34
        src, m = _frame(fmt, w, h, 4), _m(fmt, w, h, 4)
        for restart in (1, 7):
            want = _oracle.encode(m, 90, restart=restart)
            e.set_restart(restart)
            for variant in ("aligned", "unaligned"):
                assert _encode(e, src, fmt, variant) == want, ("restart", restart, name, variant)
            assert _plain(e, m) == want, ("restart", restart, name)
        e.set_restart(0)

        std = _fixedhuff.golden_specs()
        custom = [_fixedhuff.permuted_spec(s, seed=7 + t) for t, s in enumerate(std)]
        for mode, specs in ((J.JPGE_HUFF_STANDARD, std), (J.JPGE_HUFF_CUSTOM, custom)):
            want = _fixedhuff.expected_rgb(m, 90, specs)
            e.set_huffman(mode, None if mode == J.JPGE_HUFF_STANDARD else specs)
            for variant in ("aligned", "host"):
                assert _encode(e, src, fmt, variant) == want, ("huffman", mode, name, variant)
            assert _plain(e, m) == want, ("huffman", mode, name)
        e.set_huffman(J.JPGE_HUFF_OPTIMAL)

        for quality in (50, 100):
            want = _oracle.encode(m, quality)
            assert _encode(e, src, fmt, "aligned", quality) == want, ("quality", quality, name)
            assert _encode(e, src, fmt, "host", quality) == want, ("quality", quality, name)
            assert _plain(e, m, quality) == want, ("quality", quality, name)

        # the stage entries return M's coefficients and histograms
        e.set_input_format(fmt)
        coef, hist = e.fdct_quant(src, 90), e.symbol_stats(src, 90)
        e.set_channel_lut(None)
        e.set_input_format(J.JPGE_FMT_RGB8)
        wcoef, whist = e.fdct_quant(m, 90), e.symbol_stats(m, 90)
        e.set_channel_lut(PERM)
        assert all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(coef, wcoef)), ("fdct_quant", name)
        assert all(np.array_equal(a, b) for a, b in zip(hist, whist)), ("symbol_stats", name)
        assert all(np.array_equal(a, b) for a, b in zip(coef, _oracle.stage_coeffs(m, 90))), ("fdct_quant, oracle", name)


# ---- 3. state: the tables change on one context; batches and a group ----
def _state_and_batches(enc4, enc1):
    w, h = 157, 37
    for lanes, e in ((4, enc4), (1, enc1)):
        for fmt in (L.RGB8, L.BGRA8, B.GRBG):
            src = _frame(fmt, w, h, 6)
            none = _oracle.encode(L.rgb_of(src, fmt), 90)
            steps = (("A", PERM, _want(fmt, w, h, 6, "perm")), ("B", L.TABLES["gamma"], _want(fmt, w, h, 6, "gamma")),
                     ("identity", L.TABLES["identity"], none), ("off", None, none), ("A again", PERM, _want(fmt, w, h, 6, "perm")),
                     ("invert", L.TABLES["invert"][0], _want(fmt, w, h, 6, "invert")), ("const", L.TABLES["const"], _want(fmt, w, h, 6, "const")),
                     ("B2", PERM2, _want(fmt, w, h, 6, "perm2")))
            for step, table, want in steps:
                e.set_channel_lut(table)
                got = e.channel_lut()
                assert (got is None) == (table is None), (lanes, L.NAMES[fmt], step)
                if table is not None:
                    assert np.array_equal(got, np.broadcast_to(table, (3, 256))), (lanes, L.NAMES[fmt], step)
                for variant in L.VARIANTS:
                    assert _encode(e, src, fmt, variant) == want, (lanes, L.NAMES[fmt], step, variant)

    # a batch of 9 frames of mixed sizes with tables on 4 lanes (frame sets), then one geometry
    sizes = [(157, 37), (64, 16), (157, 37), (2, 2), (64, 16), (157, 37), (200, 2), (130, 34), (64, 16)]
    for fmt in (L.BGR8, L.RGBA8, B.BGGR):
        enc4.set_channel_lut(PERM)
        enc4.set_input_format(fmt)
        got = enc4.encode_batch([_frame(fmt, sw, sh, 200 + i) for i, (sw, sh) in enumerate(sizes)], 90)
        for i, (sw, sh) in enumerate(sizes):
            assert got[i] == _want(fmt, sw, sh, 200 + i), ("mixed batch", L.NAMES[fmt], i)
        for e in (enc4, enc1):
            e.set_channel_lut(PERM2)
            e.set_input_format(fmt)
            got = e.encode_batch([_frame(fmt, 130, 34, 100 + i) for i in range(9)], 90)
            for i in range(9):
                assert got[i] == _want(fmt, 130, 34, 100 + i, "perm2"), ("batch", L.NAMES[fmt], i)
            # and off again: the same frames without tables
            e.set_channel_lut(None)
            got = e.encode_batch([_frame(fmt, 130, 34, 100 + i) for i in range(3)], 90)
            for i in range(3):
                assert got[i] == _oracle.encode(L.rgb_of(_frame(fmt, 130, 34, 100 + i), fmt), 90), ("batch, off", L.NAMES[fmt], i)

    # the same through a group that lists device 0 twice
    with J.Group([0, 0], lanes=1) as g:
        for fmt in (L.RGB8, B.GBRG):
            g.set_input_format(fmt)
            g.set_channel_lut(PERM)
            got = g.encode_batch([_frame(fmt, sw, sh, 200 + i) for i, (sw, sh) in enumerate(sizes)], 90)
            for i, (sw, sh) in enumerate(sizes):
                assert got[i] == _want(fmt, sw, sh, 200 + i), ("group", L.NAMES[fmt], i)
        g.set_input_format(L.RGB8)
        with pytest.raises(J.JpgeError) as err:
            g.encode_striped(np.zeros((64, 64, 3), np.uint8), 90)
        assert err.value.status == E_ARG
        g.set_channel_lut(None)
        rgb = J.synth_rgb8(2, 128, 64)
        assert g.encode_striped(rgb, 90) == _oracle.encode(rgb, 90)


# ---- 4. refusals: JPGE_E_ARG, and the next plain encode on the same context is byte-correct ----
def _refused(call):
    with pytest.raises(J.JpgeError) as e:
        call()
    return e.value.status == E_ARG


def _next_encode_is_correct(e):
    """With the tables still on, and without them."""
    src = _frame(L.RGB8, 83, 21)
    e.set_input_format(L.RGB8)
    assert e.encode(src, 90) == _want(L.RGB8, 83, 21)
    e.set_channel_lut(None)
    assert e.encode(src, 90) == _oracle.encode(src, 90)
    e.set_channel_lut(PERM)


def _refusals(enc4, enc1, tmp_path):
    buf = torch.zeros(64 * 64 * 4, dtype=torch.uint8, device="cuda")
    out = torch.zeros(J.max_jpeg_bytes(64, 64), dtype=torch.uint8, device="cuda")
    half = out.numel() // 2

    def ptr(e, w=32, h=32, stride=256, maxval=255):
        return e.encode_ptr(buf.data_ptr(), w, h, stride, out.data_ptr(), out.numel(), 90, maxval)

    def batch_refused(e, maxval=255):
        with pytest.raises(J.JpgeError):
            e.encode_batch_dev([(buf.data_ptr(), 32, 32, 256), (buf.data_ptr(), 16, 16, 256)],
                               [(out.data_ptr(), half), (out.data_ptr() + half, half)], 90, maxval)
        return e.batch_status() == [E_ARG, E_ARG]

    for e in (enc4, enc1):
        e.set_channel_lut(PERM)
        # the layouts without such a kernel
        for fmt in (J.JPGE_FMT_RGB8_PLANAR, J.JPGE_FMT_GRAY8, J.JPGE_FMT_NV12, J.JPGE_FMT_I420, J.JPGE_FMT_YUV444_PLANAR,
                    J.JPGE_FMT_YUYV, J.JPGE_FMT_NV16, J.JPGE_FMT_P010, J.JPGE_FMT_Y210, J.JPGE_FMT_V210):
            e.set_input_format(fmt)
            assert _refused(lambda: ptr(e)), fmt
            assert batch_refused(e), fmt
        _next_encode_is_correct(e)
        for fmt in (L.RGB8, L.BGRA8, B.RGGB):
            name = L.NAMES[fmt]
            src = _frame(fmt, 83, 21)
            e.set_input_format(fmt)
            assert ptr(e) > 0, name
            # maxval
            assert _refused(lambda: ptr(e, maxval=254)), name
            assert _refused(lambda: e.encode(src, 90, 100)), name
            assert batch_refused(e, 254), name
            # a downscale factor above 1
            for factor in (2, 4):
                e.set_downscale(factor)
                assert _refused(lambda: e.encode(src, 90)), (name, factor)
                assert _refused(lambda: e.fdct_quant(src, 90)), (name, factor)
                assert batch_refused(e), (name, factor)
            e.set_downscale(1)
            # an orientation
            for o in (1, 3, 5):
                e.set_orientation(o)
                assert _refused(lambda: e.encode(src, 90)), (name, o)
                assert _refused(lambda: e.symbol_stats(src, 90)), (name, o)
                assert batch_refused(e), (name, o)
            e.set_orientation(0)
            _next_encode_is_correct(e)
        # the stripe entry
        e.set_input_format(L.RGB8)
        assert _refused(lambda: e.stripe_transform(buf.data_ptr(), 256, 64, 64, 0, 4, 90))
        _next_encode_is_correct(e)
        e.set_channel_lut(None)
        assert len(e.stripe_transform(buf.data_ptr(), 256, 64, 64, 0, 4, 90)) == 3

    # PPM files: maxval 255 goes through the tables, another maxval is that file's E_ARG
    src = np.asarray(_frame(L.RGB8, 83, 21))
    p255, p100, j255, j100 = (str(tmp_path / n) for n in ("a.ppm", "b.ppm", "a.jpg", "b.jpg"))
    with open(p255, "wb") as f:
        f.write(b"P6\n83 21\n255\n" + src.tobytes())
    with open(p100, "wb") as f:
        f.write(b"P6\n83 21\n100\n" + (src % 101).tobytes())
    enc1.set_channel_lut(PERM)
    enc1.encode_file(p255, j255, 90)
    assert open(j255, "rb").read() == _want(L.RGB8, 83, 21)
    assert _refused(lambda: enc1.encode_file(p100, j100, 90))
    _next_encode_is_correct(enc1)

    # argument shapes never reach the library, and leave the tables in force as they were
    enc4.set_channel_lut(PERM)
    for bad in (np.zeros((3, 255), np.uint8), np.zeros((3, 256), np.int16), np.zeros(768, np.uint8)):
        with pytest.raises(ValueError):
            enc4.set_channel_lut(bad)
    _next_encode_is_correct(enc4)


# ---- the test: the four groups in turn, the contexts at their defaults before each ----
def test_channel_lut(enc4, enc1, tmp_path):
    for group in (lambda: _matrix(enc4, enc1), lambda: _modes_and_settings(enc4), lambda: _state_and_batches(enc4, enc1),
                  lambda: _refusals(enc4, enc1, tmp_path)):
        for e in (enc4, enc1):
            _reset(e)
        group()
