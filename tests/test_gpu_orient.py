"""Orientation inside K1 (jpge_set_orientation): the .jpg of a frame coded with orientation o
is, byte for byte, (a) the .jpg of O = orient_frame(frame) coded with JPGE_ORIENT_NONE in the
same layout on the same context, and (b) the oracle's bytes of O's R, G, B.  O comes from
jpge_orient_frame, which test_orient_cpu.py pins to the table's numpy expressions.  Every
comparison is exact.

The cases are small frames that code in well under a millisecond, so each test walks its whole
set of cases in loops (a few seconds at the most) and names the failing case in the assertion,
where a parametrised test would add thousands of entries to every later run of the suite."""
import functools
import os
import subprocess

import numpy as np
import pytest

import _fixedhuff
import _oracle
import _orient as O
import jpgenc_amd as J

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

VARIANTS = ("host", "aligned", "unaligned", "padded")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = 1

# Source sizes (W x H), the smallest that reach every path: a tile is 64 x 16 output pixels, so a
# transposed tile is 16 x 64 source pixels.  (160, 48): mirrored runs aligned in every layout;
# (168, 40): 3-byte mirrored runs at an 8-byte offset, 4-byte ones aligned; (157, 37): nothing
# aligned, partial tiles both ways.
SIZES = [(1, 1), (16, 16), (64, 16), (16, 64), (160, 48), (168, 40), (157, 37), (83, 21), (1, 200), (200, 1), (517, 131)]
ALL_MODES = (420, 4200, 4201, 444, 422, 411)
# orientations 1-3 in all six subsampling modes, 4-7 in the other two with 16x16 MCUs (S420_M: the matrix)
MODE_CASES = [(o, m) for o in (1, 2, 3) for m in ALL_MODES] + [(o, m) for o in O.TRANSPOSED for m in (4200, 4201)]


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
    e.set_yuv_transform(J.JPGE_YUV_FULL_601)


@pytest.fixture(autouse=True)
def _defaults(enc4, enc1):
    yield
    for e in (enc4, enc1):
        _reset(e)


@functools.lru_cache(maxsize=None)
def _frame(fmt, w, h, seed=1):
    a = O.make(fmt, w, h, seed)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _oriented(fmt, w, h, o, seed=1):
    a = J.orient_frame(_frame(fmt, w, h, seed), fmt, o)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _oracle_bytes(fmt, w, h, o, seed=1, quality=90, mode=420):
    """(b): computed once per case, shared by the variants and the contexts."""
    return _oracle.encode(O.to_rgb(_oriented(fmt, w, h, o, seed), fmt), quality, subsampling=mode)


def _encode(e, frame, fmt, variant, quality=90, maxval=255):
    """One frame through context e with its current settings (the layout set here)."""
    if variant == "host":
        e.set_input_format(fmt)
        return e.encode(frame, quality, maxval)
    t = O.device_view(torch, frame, variant)
    return e.encode_tensor(t, quality, order="bgr" if fmt in (O.BGR8, O.BGRA8) else "rgb", maxval=maxval)


def _plain(e, d, fmt, quality=90, maxval=255):
    """(a): O coded with JPGE_ORIENT_NONE on the same context (the orientation put back)."""
    o = e.orientation
    e.set_orientation(J.JPGE_ORIENT_NONE)
    try:
        return _encode(e, d, fmt, "host", quality, maxval)
    finally:
        e.set_orientation(o)


# ---- 1. the main matrix: orientations x layouts x sizes x input variants, both contexts ----
def test_matrix(enc4, enc1):
    for lanes, e in ((4, enc4), (1, enc1)):
        for fmt in O.FORMATS:
            for o in O.ORIENTS:
                for w, h in SIZES:
                    case = (lanes, O.NAMES[fmt], O.ONAMES[o], w, h)
                    src, d = _frame(fmt, w, h), _oriented(fmt, w, h, o)
                    want = _oracle_bytes(fmt, w, h, o)
                    e.set_orientation(o)
                    assert _plain(e, d, fmt) == want, (case, "the plain encode of O differs from the oracle")
                    for variant in VARIANTS:
                        assert _encode(e, src, fmt, variant) == want, (case, variant)


# ---- 2. subsampling modes ----
def test_modes(enc4):
    for fmt in O.FORMATS:
        for o, mode in MODE_CASES:
            enc4.set_subsampling(mode)
            for w, h in ((160, 48), (157, 37)):
                case = (O.NAMES[fmt], O.ONAMES[o], mode, w, h)
                src, d = _frame(fmt, w, h, 2), _oriented(fmt, w, h, o, 2)
                want = _oracle_bytes(fmt, w, h, o, 2, 90, mode)
                enc4.set_orientation(o)
                for variant in ("aligned", "unaligned"):
                    assert _encode(enc4, src, fmt, variant) == want, (case, variant)
                assert _plain(enc4, d, fmt) == want, case


# ---- 3. other settings (orientations 2 and 5, one size) ----
W3, H3 = 160, 48


def test_other_settings(enc4):
    for o in (2, 5):
        # maxval 100, the colour path that is not exact: its per-pixel scaling applies to O's pixels
        src = (_frame(O.RGB8, W3, H3, 3).astype(np.uint32) * 100 // 255).astype(np.uint8)
        d = J.orient_frame(src, O.RGB8, o)
        want = _oracle.encode(d, 90, maxval=100)
        enc4.set_orientation(o)
        for variant in ("aligned", "unaligned"):
            assert _encode(enc4, src, O.RGB8, variant, maxval=100) == want, ("maxval", o, variant)
        assert _plain(enc4, d, O.RGB8, maxval=100) == want, ("maxval", o)
        _reset(enc4)

        # a restart interval
        src, d = _frame(O.RGB8, W3, H3, 4), _oriented(O.RGB8, W3, H3, o, 4)
        want = _oracle.encode(d, 90, restart=3)
        enc4.set_restart(3)
        enc4.set_orientation(o)
        assert _encode(enc4, src, O.RGB8, "aligned") == want, ("restart", o)
        assert _plain(enc4, d, O.RGB8) == want, ("restart", o)
        _reset(enc4)

        # the Annex K tables
        src, d = _frame(O.RGB8, W3, H3, 5), _oriented(O.RGB8, W3, H3, o, 5)
        want = _fixedhuff.expected_rgb(d, 90, _fixedhuff.golden_specs())
        enc4.set_huffman(J.JPGE_HUFF_STANDARD)
        enc4.set_orientation(o)
        assert _encode(enc4, src, O.RGB8, "aligned") == want, ("standard huffman", o)
        assert _plain(enc4, d, O.RGB8) == want, ("standard huffman", o)
        _reset(enc4)

        # Q50 and Q100
        for quality in (50, 100):
            src, d = _frame(O.RGB8, W3, H3, 6), _oriented(O.RGB8, W3, H3, o, 6)
            want = _oracle.encode(d, quality)
            enc4.set_orientation(o)
            assert _encode(enc4, src, O.RGB8, "aligned", quality) == want, ("quality", quality, o)
            assert _plain(enc4, d, O.RGB8, quality) == want, ("quality", quality, o)
            _reset(enc4)


# ---- 4. batches ----
def test_batches(enc4, enc1):
    # 9 frames of one size: on the 4-lane context two full frame sets and a short one
    frames = [_frame(O.RGB8, 168, 40, 100 + i) for i in range(9)]
    for lanes, e in ((4, enc4), (1, enc1)):
        for o in (1, 5, 6):
            e.set_orientation(o)
            got = e.encode_batch(frames, 90)
            for i, f in enumerate(frames):
                assert got[i] == e.encode(f, 90), (lanes, o, i, "differs from the frame coded alone")
                assert got[i] == _oracle_bytes(O.RGB8, 168, 40, o, 100 + i), (lanes, o, i)
        _reset(e)
    # a batch that mixes two source sizes
    sizes = [(157, 37), (64, 16), (157, 37), (64, 16), (64, 16), (157, 37)]
    frames = [_frame(O.BGRA8, w, h, 200 + i) for i, (w, h) in enumerate(sizes)]
    enc4.set_input_format(O.BGRA8)
    for o in (2, 7):
        enc4.set_orientation(o)
        got = enc4.encode_batch(frames, 90)
        for i, (w, h) in enumerate(sizes):
            assert got[i] == _oracle_bytes(O.BGRA8, w, h, o, 200 + i), (o, i)


def test_device_input_and_output(enc1):
    src = _frame(O.RGB8, 517, 131)
    t = torch.from_numpy(np.array(src)).cuda()
    out = torch.zeros(J.max_jpeg_bytes(*J.oriented_size(517, 131, 5)), dtype=torch.uint8, device="cuda")
    enc1.set_orientation(5)
    n = enc1.encode_tensor(t, 90, out=out)
    assert out[:n].cpu().numpy().tobytes() == _oracle_bytes(O.RGB8, 517, 131, 5)


def test_group_batch_on_a_repeated_device():
    frames = [_frame(O.RGB8, 200, 90, 20 + i) for i in range(5)]
    with J.Group([0, 0], lanes=1) as g:
        g.set_orientation(J.JPGE_ORIENT_ROT90)
        got = g.encode_batch(frames, 90)
        for i, b in enumerate(got):
            assert b == _oracle_bytes(O.RGB8, 200, 90, 5, 20 + i)
        with pytest.raises(J.JpgeError) as e:
            g.encode_striped(frames[0], 90)
        assert e.value.status == E_ARG
        g.set_orientation(J.JPGE_ORIENT_NONE)
        assert g.encode_striped(frames[0], 90) == _oracle.encode(frames[0], 90)


# ---- 5. stage entries ----
def test_stage_entries(enc4):
    """fdct_quant and symbol_stats with orientation 5 return O's coefficients and histograms."""
    for fmt in O.FORMATS:
        src, d = _frame(fmt, 83, 21, 11), _oriented(fmt, 83, 21, 5, 11)
        enc4.set_input_format(fmt)
        enc4.set_orientation(5)
        coef, hist = enc4.fdct_quant(src, 90), enc4.symbol_stats(src, 90)
        enc4.set_orientation(0)
        wcoef, whist = enc4.fdct_quant(d, 90), enc4.symbol_stats(d, 90)
        assert all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(coef, wcoef)), O.NAMES[fmt]
        assert all(np.array_equal(a, b) for a, b in zip(hist, whist)), O.NAMES[fmt]
        assert all(np.array_equal(a, b) for a, b in zip(coef, _oracle.stage_coeffs(O.to_rgb(d, fmt), 90))), O.NAMES[fmt]


# ---- 6. refusals: JPGE_E_ARG, and the next valid encode on the same context is byte-correct ----
def _next_encode_is_correct(e):
    _reset(e)
    e.set_orientation(5)
    assert _encode(e, _frame(O.RGB8, 83, 21), O.RGB8, "aligned") == _oracle_bytes(O.RGB8, 83, 21, 5)
    _reset(e)


def _refused(call):
    with pytest.raises(J.JpgeError) as e:
        call()
    return e.value.status == E_ARG


def test_refusals(enc4, enc1):
    src = _frame(O.RGB8, 83, 21)
    # the layouts without an oriented kernel: the single call and a batch frame's status
    buf = torch.zeros(64 * 64 * 4, dtype=torch.uint8, device="cuda")
    out = torch.zeros(J.max_jpeg_bytes(32, 32), dtype=torch.uint8, device="cuda")
    for fmt in (J.JPGE_FMT_NV12, J.JPGE_FMT_GRAY8, J.JPGE_FMT_RGB8_PLANAR):
        enc4.set_input_format(fmt)
        enc4.set_orientation(1)
        assert _refused(lambda: enc4.encode_ptr(buf.data_ptr(), 32, 32, 32, out.data_ptr(), out.numel(), 90)), fmt
        with pytest.raises(J.JpgeError):
            enc4.encode_batch_dev([(buf.data_ptr(), 32, 32, 32)] * 2, [(out.data_ptr(), out.numel())] * 2, 90)
        assert enc4.batch_status() == [E_ARG, E_ARG], fmt
        enc4.set_orientation(0)
        assert enc4.encode_ptr(buf.data_ptr(), 32, 32, 32, out.data_ptr(), out.numel(), 90) > 0, fmt
        _next_encode_is_correct(enc4)
    # the transposed orientations in the modes whose MCUs are one block row high
    for mode in (444, 422, 411):
        enc4.set_subsampling(mode)
        for o in O.TRANSPOSED:
            enc4.set_orientation(o)
            assert _refused(lambda: enc4.encode(src, 90)), (mode, o)
            assert _refused(lambda: enc4.fdct_quant(src, 90)), (mode, o)
        _next_encode_is_correct(enc4)
    # together with a downscale factor above 1
    enc4.set_orientation(1)
    enc4.set_downscale(2)
    assert _refused(lambda: enc4.encode(src, 90))
    with pytest.raises(J.JpgeError):
        enc4.encode_batch([src, src], 90)
    enc4.set_orientation(0)  # (each setting alone still works)
    assert enc4.encode(src, 90) == _oracle.encode(J.downscale_frame(src, O.RGB8, 2), 90)
    _next_encode_is_correct(enc4)
    # the stripe entry
    t = torch.zeros((64, 64, 3), dtype=torch.uint8, device="cuda")
    enc1.set_orientation(1)
    assert _refused(lambda: enc1.stripe_transform(t.data_ptr(), 64 * 3, 64, 64, 0, 4, 90))
    enc1.set_orientation(0)
    assert len(enc1.stripe_transform(t.data_ptr(), 64 * 3, 64, 64, 0, 4, 90)) == 3
    _next_encode_is_correct(enc1)
    # an invalid value leaves the setting unchanged
    enc4.set_orientation(6)
    for bad in (-1, 8, 9, 255):
        assert _refused(lambda: enc4.set_orientation(bad)), bad
        assert enc4.orientation == 6
    enc4.set_input_format(J.JPGE_FMT_I420)  # (the setter takes a value whatever the layout)
    enc4.set_orientation(3)
    assert enc4.orientation == 3
    with J.Encoder(0, lanes=1) as fresh:
        assert fresh.orientation == J.JPGE_ORIENT_NONE


# ---- 7. switching on one context ----
def test_switching(enc4, enc1):
    """0, 5, 0, 2 in turn: no per-frame state survives a frame."""
    src = _frame(O.RGB8, 157, 37)
    for lanes, e in ((4, enc4), (1, enc1)):
        for o in (0, 5, 0, 2):
            e.set_orientation(o)
            assert _encode(e, src, O.RGB8, "aligned") == _oracle_bytes(O.RGB8, 157, 37, o), (lanes, o)
            assert _encode(e, src, O.RGB8, "host") == _oracle_bytes(O.RGB8, 157, 37, o), (lanes, o)


# ---- 8. the command line and the PPM entries ----
def test_cli_orient(enc1, tmp_path):
    src = _frame(O.RGB8, 203, 77, 50)
    ppm, jpg = tmp_path / "in.ppm", tmp_path / "out.jpg"
    ppm.write_bytes(b"P6\n203 77\n255\n" + src.tobytes())
    exe = os.path.join(ROOT, "jpgenc_amd", "bin", "jpgenc")
    r = subprocess.run([exe, "--orient", "rot90", "-q", "90", str(ppm), str(jpg)], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    enc1.set_orientation(J.JPGE_ORIENT_ROT90)
    want = enc1.encode(src, 90)
    assert want == _oracle_bytes(O.RGB8, 203, 77, 5, 50)
    assert jpg.read_bytes() == want
    r = subprocess.run([exe, "--orient", "rot90", "--gpus", "1", str(ppm), str(jpg)], capture_output=True, timeout=120)
    assert r.returncode == 1
    r = subprocess.run([exe, "--orient", "sideways", str(ppm), str(jpg)], capture_output=True, timeout=120)
    assert r.returncode == 1
    out = tmp_path / "f.jpg"  # the PPM entries honour the context's orientation
    enc1.encode_file(str(ppm), str(out), 90)
    assert out.read_bytes() == want
