"""Input layouts (jpge_set_input_format): BGR8, RGBA8, BGRA8 and planar RGB8 frames must
encode, byte for byte, to the .jpg of the same pixels as interleaved RGB — the oracle's
bytes for the RGB frame.  Inputs are built with numpy (_formats.py, checked by
test_formats_cpu.py): channel flip, an alpha plane of random bytes, transpose(2, 0, 1)."""
import functools
import os

import numpy as np
import pytest

import _formats as F
import _oracle
import jpgenc_amd as J
from jpgenc_amd import stripes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FMT = pytest.mark.parametrize("fmt", F.NEW_FORMATS, ids=[F.NAMES[f] for f in F.NEW_FORMATS])
INTERLEAVED = (J.JPGE_FMT_BGR8, J.JPGE_FMT_RGBA8, J.JPGE_FMT_BGRA8)


@functools.lru_cache(maxsize=None)
def _frame(seed, w, h, kind=1):
    rgb = J.synth_rgb8(seed, w, h, kind=kind)
    rgb.setflags(write=False)
    return rgb


@functools.lru_cache(maxsize=None)
def _want(seed, w, h, quality, kind=1, restart=0, subsampling=420):
    return _oracle.encode(_frame(seed, w, h, kind), quality, restart=restart, subsampling=subsampling)


@pytest.fixture(scope="module")
def enc():
    e = J.Encoder(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def enc1():
    e = J.Encoder(0, lanes=1)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def _default_format(enc, enc1):
    yield
    for e in (enc, enc1):
        e.set_input_format(J.JPGE_FMT_RGB8)
        e.set_subsampling(420)
        e.set_restart(0)


# ---- 1. sizes: fast path, ragged edges, one tile, a tile plus an MCU, more than one workgroup ----
SIZES = [(1, 1), (9, 7), (17, 33), (64, 16), (80, 16), (100, 60), (333, 211), (1040, 8), (8, 1040), (1920, 1080)]


@FMT
@pytest.mark.parametrize("w,h", SIZES)
def test_sizes(enc, fmt, w, h):
    enc.set_input_format(fmt)
    assert enc.encode(F.to_format(_frame(w + h, w, h), fmt), quality=90) == _want(w + h, w, h, 90)


# ---- 2. strides, through encode_ptr on device memory; all padding is random bytes ----
def _encode_dev(e, buf, off, w, h, stride, quality=90):
    dev = torch.from_numpy(buf).cuda()
    out = torch.zeros(J.max_jpeg_bytes(w, h), dtype=torch.uint8, device="cuda")
    n = e.encode_ptr(dev.data_ptr() + off, w, h, stride, out.data_ptr(), out.numel(), quality)
    torch.cuda.synchronize()
    return out[:n].cpu().numpy().tobytes()


def _row(fmt, w):
    return w * J.input_format_info(fmt)[0]


@FMT
@pytest.mark.parametrize("w,h", [(320, 48), (333, 211)])
@pytest.mark.parametrize("case", ["aligned", "odd", "offset1"])
def test_strides(enc, fmt, w, h, case):
    a = F.to_format(_frame(7, w, h), fmt)
    row = _row(fmt, w)
    stride = {"aligned": (row + 15) // 16 * 16 + 32, "odd": (row + 12) | 1, "offset1": (row + 15) // 16 * 16 + 16}[case]
    buf, off, ps = F.padded(a, fmt, stride, offset=1 if case == "offset1" else 0)
    enc.set_input_format(fmt, 0)  # (planar: the planes stride * height apart)
    assert _encode_dev(enc, buf, off, w, h, stride) == _want(7, w, h, 90)


@pytest.mark.parametrize("w,h", [(320, 48), (333, 211)])
@pytest.mark.parametrize("case", ["aligned", "unaligned"])
def test_plane_strides(enc, w, h, case):
    fmt = J.JPGE_FMT_RGB8_PLANAR
    a = F.to_format(_frame(7, w, h), fmt)
    stride = (w + 15) // 16 * 16 + 16
    ps = stride * h + (48 if case == "aligned" else 7)
    buf, off, ps = F.padded(a, fmt, stride, plane_stride=ps)
    enc.set_input_format(fmt, ps)
    assert enc.input_format() == (fmt, ps)
    assert _encode_dev(enc, buf, off, w, h, stride) == _want(7, w, h, 90)


# ---- 3. the other K1 kernels: the row-of-blocks MCUs (each kYh) and the other 4:2:0 filters ----
@FMT
@pytest.mark.parametrize("mode", [444, 422, 411, 4200, 4201])
@pytest.mark.parametrize("w,h", [(203, 117), (128, 16)])
def test_subsampling_modes(enc, fmt, mode, w, h):
    enc.set_input_format(fmt)
    enc.set_subsampling(mode)
    got = enc.encode(F.to_format(_frame(mode, w, h), fmt), quality=90)
    assert got == _want(mode, w, h, 90, subsampling=mode)


# ---- 4. the non-exact colour path (maxval != 255) ----
@FMT
@pytest.mark.parametrize("maxval", [1, 100, 254])
def test_maxval(enc, fmt, maxval):
    rgb = (_frame(5 + maxval, 120, 72).astype(np.uint32) * maxval // 255).astype(np.uint8)
    enc.set_input_format(fmt)
    assert enc.encode(F.to_format(rgb, fmt), quality=75, maxval=maxval) == _oracle.encode(rgb, 75, maxval=maxval)


@FMT
@pytest.mark.parametrize("mode", [444, 411])
def test_maxval_row8(enc, fmt, mode):
    rgb = (_frame(31, 120, 72).astype(np.uint32) * 100 // 255).astype(np.uint8)
    enc.set_input_format(fmt)
    enc.set_subsampling(mode)
    want = _oracle.encode(rgb, 75, maxval=100, subsampling=mode)
    assert enc.encode(F.to_format(rgb, fmt), quality=75, maxval=100) == want


# ---- 5. coefficients and symbol statistics ----
@FMT
def test_coefficients(enc, fmt):
    rgb = _frame(11, 203, 117)
    enc.set_input_format(fmt)
    got = enc.fdct_quant(F.to_format(rgb, fmt), quality=90)
    for g, w in zip(got, _oracle.stage_coeffs(rgb, 90)):
        assert np.array_equal(g, w)


@FMT
def test_symbol_statistics(enc, fmt):
    rgb = _frame(12, 200, 136)
    enc.set_input_format(fmt)
    counts, first = enc.symbol_stats(F.to_format(rgb, fmt), quality=90)
    enc.set_input_format(J.JPGE_FMT_RGB8)
    rcounts, rfirst = enc.symbol_stats(rgb, quality=90)
    assert np.array_equal(counts, _oracle.stage_hist(rgb, 90)[0])
    assert np.array_equal(counts, rcounts) and np.array_equal(first, rfirst)


# ---- 6. batches: 9 frames, 5 of one size (sets of 4 form), on 4 lanes and on 1 ----
BATCH = [(320, 240) if i % 2 == 0 else (100 + 16 * i, 60 + i) for i in range(9)]


@FMT
@pytest.mark.parametrize("lanes", [4, 1])
def test_batch_host(enc, enc1, fmt, lanes):
    e = enc if lanes == 4 else enc1
    assert e.lanes() == lanes
    e.set_input_format(fmt)
    outs = e.encode_batch([F.to_format(_frame(100 + i, w, h), fmt) for i, (w, h) in enumerate(BATCH)], quality=90)
    for i, (w, h) in enumerate(BATCH):
        assert outs[i] == _want(100 + i, w, h, 90), i


@FMT
@pytest.mark.parametrize("lanes", [4, 1])
def test_batch_device(enc, enc1, fmt, lanes):
    e = enc if lanes == 4 else enc1
    e.set_input_format(fmt)
    devs = [torch.from_numpy(F.to_format(_frame(100 + i, w, h), fmt)).cuda() for i, (w, h) in enumerate(BATCH)]
    outs = [torch.zeros(J.max_jpeg_bytes(w, h), dtype=torch.uint8, device="cuda") for w, h in BATCH]
    lens = e.encode_batch_dev([(d.data_ptr(), w, h, _row(fmt, w)) for d, (w, h) in zip(devs, BATCH)],
                              [(o.data_ptr(), o.numel()) for o in outs], quality=90)
    torch.cuda.synchronize()
    for i, (w, h) in enumerate(BATCH):
        assert outs[i][:lens[i]].cpu().numpy().tobytes() == _want(100 + i, w, h, 90), i


@FMT
def test_group_batch(fmt):
    with J.Group([0, 0]) as g:
        g.set_input_format(fmt)
        outs = g.encode_batch([F.to_format(_frame(100 + i, w, h), fmt) for i, (w, h) in enumerate(BATCH[:5])],
                              quality=90)
    for i, (w, h) in enumerate(BATCH[:5]):
        assert outs[i] == _want(100 + i, w, h, 90), i


# ---- 7. restart intervals ----
@FMT
def test_restart(enc, fmt):
    enc.set_input_format(fmt)
    enc.set_restart(42)
    assert enc.encode(F.to_format(_frame(8, 333, 211), fmt), quality=90) == _want(8, 333, 211, 90, restart=42)


# ---- 8. stripes ----
def _encode_striped(a, fmt, w, h, n, quality):
    dev = torch.from_numpy(a.reshape(-1)).cuda()
    stride = _row(fmt, w)
    rows = stripes.stripe_rows((h + 15) // 16, n)
    ptrs = [(dev.data_ptr() + r0 * 16 * stride, stride) for r0, _ in rows]
    cap = J.max_jpeg_bytes(w, h)
    out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    encs = [J.Encoder(0, lanes=1) for _ in range(n)]
    try:
        for e in encs:
            e.set_input_format(fmt)
        total = stripes.encode_stripes_local(encs, ptrs, w, h, quality, out.data_ptr(), cap, rows=rows)
    finally:
        for e in encs:
            e.close()
    torch.cuda.synchronize()
    return out[:total].cpu().numpy().tobytes()


@pytest.mark.parametrize("fmt", [J.JPGE_FMT_RGBA8, J.JPGE_FMT_BGR8, J.JPGE_FMT_BGRA8],
                         ids=["rgba8", "bgr8", "bgra8"])
def test_stripes(fmt):
    w, h = 256, 128
    assert _encode_striped(F.to_format(_frame(21, w, h), fmt), fmt, w, h, 4, 90) == _want(21, w, h, 90)


def test_stripes_refuse_planar(enc1):
    enc1.set_input_format(J.JPGE_FMT_RGB8_PLANAR)
    dev = torch.zeros(3 * 256 * 128, dtype=torch.uint8, device="cuda")
    with pytest.raises(J.JpgeError):
        enc1.stripe_transform(dev.data_ptr(), 256, 256, 128, 0, 2, 90)


@pytest.mark.parametrize("fmt", [J.JPGE_FMT_BGR8, J.JPGE_FMT_RGB8_PLANAR], ids=["bgr8", "planar"])
def test_group_striped_needs_rgb8(fmt):
    rgb = _frame(22, 256, 128)
    with J.Group([0, 0], lanes=1) as g:
        g.set_input_format(fmt)
        with pytest.raises(J.JpgeError):
            g.encode_striped(rgb, quality=90)
        g.set_input_format(J.JPGE_FMT_RGB8)
        assert g.encode_striped(rgb, quality=90) == _want(22, 256, 128, 90)


# ---- 9. the tensor entry ----
def test_tensor_planar_padded(enc1):
    w, h = 333, 211
    big = torch.randint(0, 256, (3, h + 5, w + 51), dtype=torch.uint8, device="cuda")
    t = big[:, 2:2 + h, 16:16 + w]  # padded row and plane strides, an aligned base
    t.copy_(torch.from_numpy(F.to_format(_frame(8, w, h), J.JPGE_FMT_RGB8_PLANAR)).cuda())
    assert t.stride() == ((h + 5) * (w + 51), w + 51, 1) and t.data_ptr() % 16 == 0
    enc1.set_input_format(J.JPGE_FMT_BGR8)
    assert enc1.encode_tensor(t, quality=90) == _want(8, w, h, 90)
    assert enc1.input_format() == (J.JPGE_FMT_BGR8, 0)  # unchanged
    u = big[:, 1:1 + h, 3:3 + w]  # an unaligned base: the clamped path
    u.copy_(t.clone())
    assert enc1.encode_tensor(u, quality=90) == _want(8, w, h, 90)


@pytest.mark.parametrize("order", ["rgb", "bgr"])
def test_tensor_four_bytes_device(enc1, order):
    w, h = 320, 48
    fmt = J.JPGE_FMT_RGBA8 if order == "rgb" else J.JPGE_FMT_BGRA8
    t = torch.from_numpy(F.to_format(_frame(7, w, h), fmt)).cuda()
    assert enc1.encode_tensor(t, quality=90, order=order) == _want(7, w, h, 90)
    out = torch.zeros(J.max_jpeg_bytes(w, h), dtype=torch.uint8, device="cuda")
    n = enc1.encode_tensor(t, quality=90, out=out, order=order)
    torch.cuda.synchronize()
    assert out[:n].cpu().numpy().tobytes() == _want(7, w, h, 90)
    assert enc1.input_format() == (J.JPGE_FMT_RGB8, 0)


@pytest.mark.parametrize("order", ["rgb", "bgr"])
def test_tensor_three_bytes_host(enc1, order):
    w, h = 333, 211
    fmt = J.JPGE_FMT_RGB8 if order == "rgb" else J.JPGE_FMT_BGR8
    t = torch.from_numpy(F.to_format(_frame(8, w, h), fmt))
    assert enc1.encode_tensor(t, quality=90, order=order) == _want(8, w, h, 90)
    wide = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (h, w + 9, 3), dtype=np.uint8))
    wide[:, :w] = t
    assert enc1.encode_tensor(wide[:, :w], quality=90, order=order) == _want(8, w, h, 90)  # a padded row stride


def test_tensor_rejects_strided_inner_dimension(enc1):
    t = torch.zeros((3, 32, 64), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        enc1.encode_tensor(t[:, :, ::2])
    hwc = torch.zeros((32, 64, 4), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        enc1.encode_tensor(hwc[:, ::2])  # pixels not packed
    with pytest.raises(ValueError):
        enc1.encode_tensor(t.permute(1, 2, 0))  # (H, W, 3) view of planar memory
    with pytest.raises(ValueError):
        enc1.encode_tensor(t, order="bgr")
    assert enc1.input_format() == (J.JPGE_FMT_RGB8, 0)


# ---- 10. state ----
def test_rgb8_setting_is_todays_path(enc):
    rgb = _frame(8, 333, 211)
    before = enc.encode(rgb, quality=90)
    enc.set_input_format(J.JPGE_FMT_BGRA8)
    enc.set_input_format(J.JPGE_FMT_RGB8)
    assert enc.encode(rgb, quality=90) == before == _want(8, 333, 211, 90)


def test_bad_settings(enc):
    for fmt in (-1, 5, 99):
        with pytest.raises(J.JpgeError):
            enc.set_input_format(fmt)
    for fmt in (J.JPGE_FMT_RGB8,) + INTERLEAVED:
        with pytest.raises(J.JpgeError):
            enc.set_input_format(fmt, 4096)
    assert enc.input_format() == (J.JPGE_FMT_RGB8, 0)  # a refused call changes nothing


@FMT
def test_short_stride_is_refused(enc, fmt):
    w, h = 64, 16
    a = F.to_format(_frame(1, w, h), fmt)
    enc.set_input_format(fmt)
    dev = torch.from_numpy(a).cuda()
    out = torch.zeros(J.max_jpeg_bytes(w, h), dtype=torch.uint8, device="cuda")
    with pytest.raises(J.JpgeError):
        enc.encode_ptr(dev.data_ptr(), w, h, _row(fmt, w) - 1, out.data_ptr(), out.numel(), 90)
    n = enc.encode_ptr(dev.data_ptr(), w, h, 0, out.data_ptr(), out.numel(), 90)  # 0: the layout's row
    torch.cuda.synchronize()
    assert out[:n].cpu().numpy().tobytes() == _want(1, w, h, 90)


@FMT
def test_ppm_entry_ignores_the_setting(enc, fmt, golden_dir, tmp_path):
    path = os.path.join(golden_dir, "ppm", "tester_RGB_26x19.ppm")
    img = J.load_ppm(path)
    enc.set_input_format(fmt)
    out = str(tmp_path / "o.jpg")
    enc.encode_file(path, out, quality=90)
    with open(out, "rb") as f:
        assert f.read() == _oracle.encode(img.rgb, 90, maxval=img.maxval)


@pytest.mark.parametrize("fmt", [J.JPGE_FMT_RGBA8, J.JPGE_FMT_BGRA8], ids=["rgba8", "bgra8"])
def test_alpha_is_ignored(enc, fmt):
    rgb = _frame(8, 333, 211)
    enc.set_input_format(fmt)
    zero = enc.encode(F.to_format(rgb, fmt, alpha=0), quality=90)
    rand = enc.encode(F.to_format(rgb, fmt), quality=90)
    assert zero == rand == _want(8, 333, 211, 90)


def test_tensor_ambiguous_shape_needs_layout(enc1):
    rgb = _frame(3, 4, 32)  # 4 px wide, 32 rows: planar it is (3, 32, 4)
    t = torch.from_numpy(F.to_format(rgb, J.JPGE_FMT_RGB8_PLANAR)).cuda()
    with pytest.raises(ValueError):
        enc1.encode_tensor(t, quality=90)
    assert enc1.encode_tensor(t, quality=90, layout="chw") == _want(3, 4, 32, 90)
    col = torch.from_numpy(F.to_format(_frame(3, 1, 32), J.JPGE_FMT_RGBA8)).cuda()  # W == 1
    assert enc1.encode_tensor(col, quality=90) == _want(3, 1, 32, 90)
