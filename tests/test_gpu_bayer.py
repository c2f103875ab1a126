"""8-bit Bayer input (JPGE_FMT_BAYER_*): the .jpg of a mosaic is, byte for byte, (a) the .jpg of
D = demosaic_frame(frame) coded as JPGE_FMT_RGB8 on the same context, and (b) the oracle's bytes of
D.  D comes from jpge_demosaic_frame, which test_bayer_cpu.py pins to the rule's numpy statement.
Every comparison is exact.

The cases are small frames that code in well under a millisecond, so each test walks its whole
set of cases in loops (a few seconds at the most) and names the failing case in the assertion.
The groups of cases below are plain functions; four tests at the end of the file run them, so that
the file adds four entries to every later run of the suite, not one per group."""
import functools

import numpy as np
import pytest

import _bayer as B
import _fixedhuff
import _oracle
import jpgenc_amd as J

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

E_ARG = 1
# W x H.  A fdct_kernel tile is 64 x 16 pixels and a fdct_row8_kernel tile 128 x 8, a lane's run 16
# pixels of a row: one run, one tile, a pixel more and two more than a tile (partial runs, the
# clamped path), several tiles each way, the smallest frame with an interior tile (192 x 48), odd
# sizes, the two-pixel strips, and a frame of many tiles with nothing aligned.
SIZES = [(2, 2), (3, 3), (16, 16), (64, 16), (65, 17), (66, 18), (130, 34), (192, 48), (157, 37), (2, 200), (200, 2), (517, 131)]
ALL_MODES = (420, 4200, 4201, 444, 422, 411)


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
def _frame(w, h, seed=1):
    a = B.noise(w, h, seed)
    a.setflags(write=False)
    return a


def _d(frame, fmt):
    return J.demosaic_frame(frame, fmt)


@functools.lru_cache(maxsize=None)
def _want(fmt, w, h, seed=1, quality=90, mode=420):
    """(b): computed once per case, shared by the variants and the contexts."""
    return _oracle.encode(_d(_frame(w, h, seed), fmt), quality, subsampling=mode)


def _encode(e, frame, fmt, variant, quality=90, **kw):
    """One mosaic through context e with its current settings (the layout set here)."""
    if variant == "host":
        e.set_input_format(fmt)
        return e.encode(frame, quality, **kw)
    assert not kw
    return e.encode_tensor(B.device_view(torch, frame, variant), quality, layout=B.LAYOUTS[fmt])


def _plain(e, d, quality=90, **kw):
    """(a): D coded as RGB8 on the same context."""
    e.set_input_format(J.JPGE_FMT_RGB8)
    return e.encode(d, quality, **kw)


# ---- 1. the main matrix: patterns x sizes x input variants, both contexts ----
def _matrix(enc4, enc1):
    for lanes, e in ((4, enc4), (1, enc1)):
        for fmt in B.FORMATS:
            for w, h in SIZES:
                case = (lanes, B.NAMES[fmt], w, h)
                src, want = _frame(w, h), _want(fmt, w, h)
                assert _plain(e, _d(src, fmt)) == want, (case, "the RGB8 encode of D differs from the oracle")
                for variant in B.VARIANTS:
                    assert _encode(e, src, fmt, variant) == want, (case, variant)


# ---- 2. subsampling modes: both kernels' neighbourhoods ----
def _modes(enc4):
    for fmt in B.FORMATS:
        for mode in ALL_MODES:
            enc4.set_subsampling(mode)
            for w, h in ((130, 34), (157, 37)):
                case = (B.NAMES[fmt], mode, w, h)
                src, want = _frame(w, h, 2), _want(fmt, w, h, 2, 90, mode)
                for variant in ("aligned", "unaligned", "host"):
                    assert _encode(enc4, src, fmt, variant) == want, (case, variant)
                assert _plain(enc4, _d(src, fmt)) == want, case


# ---- 3. stage entries ----
def _stage_entries(enc4):
    """fdct_quant and symbol_stats return D's coefficients and histograms."""
    for fmt in B.FORMATS:
        for w, h in ((83, 21), (130, 34)):
            src = _frame(w, h, 11)
            d = _d(src, fmt)
            enc4.set_input_format(fmt)
            coef, hist = enc4.fdct_quant(src, 90), enc4.symbol_stats(src, 90)
            enc4.set_input_format(J.JPGE_FMT_RGB8)
            wcoef, whist = enc4.fdct_quant(d, 90), enc4.symbol_stats(d, 90)
            case = (B.NAMES[fmt], w, h)
            assert all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(coef, wcoef)), case
            assert all(np.array_equal(a, b) for a, b in zip(hist, whist)), case
            assert all(np.array_equal(a, b) for a, b in zip(coef, _oracle.stage_coeffs(d, 90))), case


# ---- 4. other settings ----
W4, H4 = 130, 34


def _other_settings(enc4):
    for fmt in (B.GRBG, B.BGGR):
        name = B.NAMES[fmt]
        src = _frame(W4, H4, 4)
        d = _d(src, fmt)
        for restart in (1, 7):
            want = _oracle.encode(d, 90, restart=restart)
            enc4.set_restart(restart)
            for variant in ("aligned", "unaligned"):
                assert _encode(enc4, src, fmt, variant) == want, ("restart", restart, name, variant)
            assert _plain(enc4, d) == want, ("restart", restart, name)
            _reset(enc4)

        want = _fixedhuff.expected_rgb(d, 90, _fixedhuff.golden_specs())
        enc4.set_huffman(J.JPGE_HUFF_STANDARD)
        assert _encode(enc4, src, fmt, "aligned") == want, ("standard huffman", name)
        assert _plain(enc4, d) == want, ("standard huffman", name)
        _reset(enc4)

        for quality in (50, 90, 100):
            want = _oracle.encode(d, quality)
            assert _encode(enc4, src, fmt, "aligned", quality) == want, ("quality", quality, name)
            assert _encode(enc4, src, fmt, "host", quality) == want, ("quality", quality, name)
            assert _plain(enc4, d, quality) == want, ("quality", quality, name)

        # the caller's tables
        qy = (np.arange(64) % 23 + 1).astype(np.uint8)
        qc = (np.arange(64)[::-1] % 31 + 2).astype(np.uint8)
        want = _oracle.encode(d, 50, qy=qy, qc=qc)
        assert _encode(enc4, src, fmt, "host", 50, qy=qy, qc=qc) == want, ("custom tables", name)
        assert _plain(enc4, d, 50, qy=qy, qc=qc) == want, ("custom tables", name)


# ---- 5. batches ----
def _batches(enc4, enc1):
    # 9 frames of one geometry: on the 4-lane context two full frame sets and a short one
    frames = [_frame(130, 34, 100 + i) for i in range(9)]
    for lanes, e in ((4, enc4), (1, enc1)):
        for fmt in (B.RGGB, B.GBRG):
            e.set_input_format(fmt)
            got = e.encode_batch(frames, 90)
            for i in range(9):
                assert got[i] == _want(fmt, 130, 34, 100 + i), (lanes, B.NAMES[fmt], i)
    # mixed patterns: a call has one layout (the context's), so the layout changes from call to call
    # on one context, each call over the four phases' mosaics of one scene
    rgb = np.random.default_rng(5).integers(0, 256, (34, 130, 3), dtype=np.uint8)
    for fmt in B.FORMATS:
        enc4.set_input_format(fmt)
        frames = [B.mosaic(rgb, f) for f in B.FORMATS] * 2
        got = enc4.encode_batch(frames, 90)
        for i, f in enumerate(frames):
            assert got[i] == _oracle.encode(_d(f, fmt), 90), ("mixed", B.NAMES[fmt], i)
    # mixed geometries
    sizes = [(157, 37), (64, 16), (157, 37), (2, 2), (64, 16), (157, 37), (200, 2)]
    frames = [_frame(w, h, 200 + i) for i, (w, h) in enumerate(sizes)]
    enc4.set_input_format(B.BGGR)
    got = enc4.encode_batch(frames, 90)
    for i, (w, h) in enumerate(sizes):
        assert got[i] == _want(B.BGGR, w, h, 200 + i), ("geometries", i)
    # Bayer, RGB8, Bayer on one context
    frames = [_frame(157, 37, 300 + i) for i in range(5)]
    ds = [_d(f, B.GRBG) for f in frames]
    want = [_want(B.GRBG, 157, 37, 300 + i) for i in range(5)]
    for lanes, e in ((4, enc4), (1, enc1)):
        for fmt, fr in ((B.GRBG, frames), (J.JPGE_FMT_RGB8, ds), (B.GRBG, frames)):
            e.set_input_format(fmt)
            assert e.encode_batch(fr, 90) == want, (lanes, fmt)


def _group_batch():
    frames = [_frame(130, 34, 20 + i) for i in range(5)]
    with J.Group([0], lanes=1) as g:
        g.set_input_format(B.GBRG)
        got = g.encode_batch(frames, 90)
        for i, b in enumerate(got):
            assert b == _want(B.GBRG, 130, 34, 20 + i), i
        with pytest.raises(J.JpgeError) as e:
            g.encode_striped(np.zeros((64, 64, 3), np.uint8), 90)
        assert e.value.status == E_ARG


# ---- 6. checkers and single pixels ----
def _checkers_and_single_pixels(enc4):
    w, h = 130, 34
    for fmt in B.FORMATS:
        for which in range(8):
            a = B.checker(w, h, which)
            want = _oracle.encode(_d(a, fmt), 90)
            for variant in ("aligned", "unaligned"):
                assert _encode(enc4, a, fmt, variant) == want, ("checker", B.NAMES[fmt], which, variant)
    for fmt in (B.RGGB, B.BGGR):
        for mode in (420, 444):
            enc4.set_subsampling(mode)
            for at, a in B.single_pixels(w, h):
                want = _oracle.encode(_d(a, fmt), 90, subsampling=mode)
                for variant in ("aligned", "unaligned"):
                    assert _encode(enc4, a, fmt, variant) == want, ("pixel", B.NAMES[fmt], mode, at, variant)


# ---- 7. refusals: JPGE_E_ARG, and the next valid Bayer encode on the same context is byte-correct ----
def _next_encode_is_correct(e):
    _reset(e)
    assert _encode(e, _frame(83, 21), B.GRBG, "aligned") == _want(B.GRBG, 83, 21)
    assert _encode(e, _frame(83, 21), B.GRBG, "host") == _want(B.GRBG, 83, 21)
    _reset(e)


def _refused(call):
    with pytest.raises(J.JpgeError) as e:
        call()
    return e.value.status == E_ARG


def test_refusals(enc4, enc1):
    src = _frame(83, 21)
    buf = torch.zeros(64 * 64, dtype=torch.uint8, device="cuda")
    out = torch.zeros(J.max_jpeg_bytes(64, 64), dtype=torch.uint8, device="cuda")

    def ptr(w, h, maxval=255):
        return enc4.encode_ptr(buf.data_ptr(), w, h, 64, out.data_ptr(), out.numel(), 90, maxval)

    for fmt in B.FORMATS:
        name = B.NAMES[fmt]
        # a dimension below 2: the single call and a batch frame's status
        enc4.set_input_format(fmt)
        for w, h in ((1, 32), (32, 1), (1, 1)):
            assert _refused(lambda: ptr(w, h)), (name, w, h)
            with pytest.raises(J.JpgeError):
                enc4.encode_batch_dev([(buf.data_ptr(), w, h, 64), (buf.data_ptr(), 32, 32, 64)],
                                      [(out.data_ptr(), out.numel() // 2), (out.data_ptr() + out.numel() // 2, out.numel() // 2)], 90)
            assert enc4.batch_status() == [E_ARG, 0], (name, w, h)
        # maxval
        assert _refused(lambda: ptr(32, 32, 254)), name
        assert _refused(lambda: enc4.encode(src, 90, 100)), name
        assert ptr(32, 32) > 0
        # a plane stride
        assert _refused(lambda: (enc4.set_input_format(fmt, 4096), ptr(32, 32))), name
        enc4.set_input_format(fmt)
        # a downscale factor above 1
        for factor in (2, 4):
            enc4.set_downscale(factor)
            assert _refused(lambda: enc4.encode(src, 90)), (name, factor)
            assert _refused(lambda: enc4.fdct_quant(src, 90)), (name, factor)
            with pytest.raises(J.JpgeError):
                enc4.encode_batch([src, src], 90)
        enc4.set_downscale(1)
        # an orientation
        for o in (1, 3, 5):
            enc4.set_orientation(o)
            assert _refused(lambda: enc4.encode(src, 90)), (name, o)
            assert _refused(lambda: enc4.symbol_stats(src, 90)), (name, o)
        enc4.set_orientation(0)
        _next_encode_is_correct(enc4)
        # the stripe entry
        enc1.set_input_format(fmt)
        assert _refused(lambda: enc1.stripe_transform(buf.data_ptr(), 64, 64, 64, 0, 4, 90)), name
        _next_encode_is_correct(enc1)
    # a frame shaped for another layout never reaches the library
    enc4.set_input_format(B.RGGB)
    with pytest.raises(ValueError):
        enc4.encode(np.zeros((8, 8, 3), np.uint8), 90)
    with pytest.raises(ValueError):
        enc4.encode_tensor(torch.zeros((8, 8, 3), dtype=torch.uint8), 90, layout="bayer_rggb")
    with pytest.raises(ValueError):
        enc4.encode_tensor(torch.zeros((8, 8), dtype=torch.uint8), 90, layout="bayer_rgbg")
    _next_encode_is_correct(enc4)


# ---- 8. device tensors ----
def _encode_tensor(enc1):
    src = _frame(517, 131)
    for fmt in B.FORMATS:
        want = _want(fmt, 517, 131)
        for variant in ("padded", "unaligned"):
            t = B.device_view(torch, src, variant)
            assert enc1.encode_tensor(t, 90, layout=B.LAYOUTS[fmt]) == want, (B.NAMES[fmt], variant)
        # a host tensor, and device output
        assert enc1.encode_tensor(torch.from_numpy(np.array(src)), 90, layout=B.LAYOUTS[fmt]) == want, B.NAMES[fmt]
        out = torch.zeros(J.max_jpeg_bytes(517, 131), dtype=torch.uint8, device="cuda")
        n = enc1.encode_tensor(B.device_view(torch, src, "aligned"), 90, out=out, layout=B.LAYOUTS[fmt])
        assert out[:n].cpu().numpy().tobytes() == want, B.NAMES[fmt]
    # the context's layout is what it was
    assert enc1.input_format()[0] == J.JPGE_FMT_RGB8


# ---- the tests: the groups above, a few to a test (every group resets the contexts it changed) ----
def _fresh(*encs):
    for e in encs:
        _reset(e)


def test_matrix_modes_and_tensors(enc4, enc1):
    _matrix(enc4, enc1)
    _fresh(enc4, enc1)
    _modes(enc4)
    _fresh(enc4)
    _encode_tensor(enc1)


def test_stages_settings_and_engineered_frames(enc4):
    _stage_entries(enc4)
    _fresh(enc4)
    _other_settings(enc4)
    _fresh(enc4)
    _checkers_and_single_pixels(enc4)


def test_batches(enc4, enc1):
    _batches(enc4, enc1)
    _group_batch()
