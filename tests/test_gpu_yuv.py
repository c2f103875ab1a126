"""Y, Cb, Cr input layouts (JPGE_FMT_NV12, _I420, _YUV444_PLANAR): K1 reads a decoder's
samples in place, with no colour conversion.  A sample v is the fp64 value v - 128 of the
reference Image's plane after convertToColorSpace(YCbCr); the 4:2:0 layouts' chroma planes
are the output of applySubsampling.  Expectations (_yuv.py, checked by test_yuv_cpu.py):
coefficients from the oracle's primitives, whole files from Encoder.encode_planes (pinned to
the oracle by test_gpu_planes.py) on a separate context.  Every comparison is exact."""
import functools

import numpy as np
import pytest

import _oracle
import _yuv as Y
import jpgenc_amd as J

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FMT = pytest.mark.parametrize("fmt", Y.FORMATS, ids=[Y.NAMES[f] for f in Y.FORMATS])
HALF = pytest.mark.parametrize("fmt", Y.HALF, ids=[Y.NAMES[f] for f in Y.HALF])
# a tile is 64x16 px: one pixel, one MCU, one full tile, full + partial tile on two MCU rows, odd, several tiles
SIZES = [(1, 1), (16, 16), (64, 16), (80, 32), (33, 17), (130, 50)]
KINDS = ["random", "photo", "zeros", "ones"]
MODES = [444, 422, 411, 4200, 4201]
# the row-8 kernels' tile is 128x8 px: one partial block, and a full tile + a partial one on three block rows
MODE_SIZES = [(9, 9), (136, 24)]


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


@pytest.fixture(scope="module")
def ref():
    """The context of the expectations (encode_planes, color_convert)."""
    e = J.Encoder(0, lanes=1)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def _defaults(enc, enc1, ref):
    yield
    for e in (enc, enc1, ref):
        e.set_input_format(J.JPGE_FMT_RGB8)
        e.set_subsampling(420)
        e.set_restart(0)


_photo = {}


def _samples(ref, half, w, h, kind, seed=None):
    """(y, cb, cr) uint8 planes, chroma at half size or full; photo: synth_rgb8 through
    color_convert, + 128, rounded and clipped (half size: the top-left sample of each cell)."""
    fmt = Y.I420 if half else Y.YUV444
    if kind != "photo":
        return Y.samples(fmt, 1000 * w + h if seed is None else seed, w, h, kind)
    if (w, h) not in _photo:
        rgb = J.synth_rgb8(w + h, w, h, kind=0).astype(np.float64)
        ycc = ref.color_convert(rgb[:, :, 0], rgb[:, :, 1], rgb[:, :, 2], J.JPGE_TO_YCBCR)
        _photo[(w, h)] = tuple(np.clip(np.rint(p + 128.0), 0, 255).astype(np.uint8) for p in ycc)
    y, cb, cr = _photo[(w, h)]
    return (y, cb[::2, ::2].copy(), cr[::2, ::2].copy()) if half else (y, cb, cr)


@functools.lru_cache(maxsize=None)
def _want_cached(key, mode, quality):
    fmt, planes = _want_cached.planes[key]
    return Y.want_coeffs(Y.pad_planes(fmt, *planes, mcu=Y.mcu_size(mode)), mode, quality)


_want_cached.planes = {}


def _want(fmt, planes, mode, quality, key):
    """want_coeffs, computed once per (input, mode, quality): NV12 and I420 share it."""
    half = fmt in Y.HALF
    _want_cached.planes.setdefault((half, key), (Y.I420 if half else Y.YUV444, planes))
    return _want_cached((half, key), mode, quality)


def _same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


# ---- 1. coefficients ----
@FMT
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w,h", SIZES)
def test_coefficients(enc, ref, fmt, w, h, kind):
    p = _samples(ref, fmt in Y.HALF, w, h, kind)
    enc.set_input_format(fmt)
    got = enc.fdct_quant(Y.build(fmt, *p), quality=90)
    assert _same(got, _want(fmt, p, 420, 90, (w, h, kind)))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["random", "photo"])
@pytest.mark.parametrize("w,h", MODE_SIZES)
def test_coefficients_modes(enc, ref, mode, w, h, kind):
    p = _samples(ref, False, w, h, kind)
    enc.set_input_format(Y.YUV444)
    enc.set_subsampling(mode)
    got = enc.fdct_quant(Y.build(Y.YUV444, *p), quality=90)
    assert _same(got, _want(Y.YUV444, p, mode, 90, (w, h, kind)))


# ---- 2. whole files ----
def _planes_jpg(ref, fmt, p, w, h, quality, restart=0):
    ref.set_restart(restart)
    return ref.encode_planes(*Y.pad_planes(fmt, *p), w, h, J.JPGE_TO_YCBCR, quality)


@FMT
@pytest.mark.parametrize("quality", [50, 90, 100])
@pytest.mark.parametrize("w,h", SIZES)
def test_whole_file(enc, ref, fmt, w, h, quality):
    kind = "photo" if quality == 90 else "random"
    p = _samples(ref, fmt in Y.HALF, w, h, kind)
    enc.set_input_format(fmt)
    assert enc.encode(Y.build(fmt, *p), quality=quality) == _planes_jpg(ref, fmt, p, w, h, quality)


@FMT
def test_whole_file_restart(enc, ref, fmt):
    w, h = 130, 50
    p = _samples(ref, fmt in Y.HALF, w, h, "random")
    enc.set_input_format(fmt)
    enc.set_restart(3)
    got = enc.encode(Y.build(fmt, *p), quality=90)
    assert got == _planes_jpg(ref, fmt, p, w, h, 90, restart=3)
    assert got.count(b"\xff\xdd") >= 1  # DRI


# ---- 3. the other modes, whole file ----
def _sof0_sampling(jpg):
    i = jpg.index(b"\xff\xc0")
    assert jpg[i + 9] == 3
    return [(jpg[i + 11 + 3 * c] >> 4, jpg[i + 11 + 3 * c] & 15) for c in range(3)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("w,h", MODE_SIZES)
def test_modes_whole_file(enc, ref, mode, w, h):
    p = _samples(ref, False, w, h, "random")
    enc.set_input_format(Y.YUV444)
    enc.set_subsampling(mode)
    jpg = enc.encode(Y.build(Y.YUV444, *p), quality=90)
    info, y, cb, cr = J.decode_coeffs(jpg)
    assert (info.width, info.height) == (w, h)
    assert _same((y, cb, cr), _want(Y.YUV444, p, mode, 90, (w, h, "random")))
    assert _sof0_sampling(jpg) == [_oracle.SHAPES[mode], (1, 1), (1, 1)]


# ---- 4. invariants ----
@pytest.mark.parametrize("w,h", [(33, 17), (130, 50)])
def test_layouts_agree(enc, ref, w, h):
    y, cb, cr = _samples(ref, True, w, h, "random")
    out = []
    for fmt in Y.HALF:
        enc.set_input_format(fmt)
        out.append(enc.encode(Y.build(fmt, y, cb, cr), quality=90))
    enc.set_input_format(Y.YUV444)
    out.append(enc.encode(Y.build(Y.YUV444, y, Y.upsample(cb, w, h), Y.upsample(cr, w, h)), quality=90))
    assert out[0] == out[1] == out[2] == _planes_jpg(ref, Y.I420, (y, cb, cr), w, h, 90)


# ---- 5. addressing: device frames inside random bytes ----
def _encode_dev(e, buf, off, w, h, stride, quality=90):
    dev = torch.from_numpy(buf).cuda()
    assert dev.data_ptr() % 16 == 0
    out = torch.zeros(J.max_jpeg_bytes(w, h), dtype=torch.uint8, device="cuda")
    n = e.encode_ptr(dev.data_ptr() + off, w, h, stride, out.data_ptr(), out.numel(), quality)
    torch.cuda.synchronize()
    return out[:n].cpu().numpy().tobytes()


@FMT
@pytest.mark.parametrize("w,h", [(80, 32), (33, 17)])
@pytest.mark.parametrize("case", ["unaligned", "aligned"])
def test_addressing(enc, ref, fmt, w, h, case):
    p = _samples(ref, fmt in Y.HALF, w, h, "random")
    if case == "unaligned":  # a padded stride, a plane stride that is no multiple of 16, the base 1 byte in
        stride, off = w + 24, 1
        ps = stride * h + 37
    else:  # every base and pitch 16-byte aligned, a 64-byte pitch where the frame fits one: the fast path
        stride, off = (64 if w <= 64 else 128), 32
        ps = stride * h + 48
    want = _planes_jpg(ref, fmt, p, w, h, 90)
    enc.set_input_format(fmt, ps)
    assert enc.input_format() == (fmt, ps)
    outs = [_encode_dev(enc, Y.raw(fmt, *p, stride=stride, plane_stride=ps, offset=off, seed=s)[0], off, w, h, stride)
            for s in (9, 10)]  # other bytes around the frame
    assert outs[0] == outs[1] == want


# ---- 6. pipeline shapes ----
BATCH = [(160, 96) if i % 2 == 0 else (48 + 16 * i, 40 + i) for i in range(9)]  # 5 of one size: sets form


@HALF
@pytest.mark.parametrize("lanes", [4, 1])
def test_batch(enc, enc1, ref, fmt, lanes):
    e = enc if lanes == 4 else enc1
    assert e.lanes() == lanes
    ps = [_samples(ref, True, w, h, "random", seed=100 + i) for i, (w, h) in enumerate(BATCH)]
    e.set_input_format(fmt)
    outs = e.encode_batch([Y.build(fmt, *p) for p in ps], quality=90)
    for i, (w, h) in enumerate(BATCH):
        assert outs[i] == _planes_jpg(ref, fmt, ps[i], w, h, 90), i


@FMT
def test_frame_sets(enc, ref, fmt):
    w, h = 136, 72
    ps = [_samples(ref, fmt in Y.HALF, w, h, "random", seed=200 + i) for i in range(9)]
    enc.set_input_format(fmt)
    outs = enc.encode_batch([Y.build(fmt, *p) for p in ps], quality=75)
    assert outs == [_planes_jpg(ref, fmt, p, w, h, 75) for p in ps]


@FMT
def test_one_lane_stages(enc1, ref, fmt):
    w, h = 130, 50
    p = _samples(ref, fmt in Y.HALF, w, h, "photo")
    enc1.set_input_format(fmt)
    f = Y.build(fmt, *p)
    assert enc1.encode(f, quality=90) == _planes_jpg(ref, fmt, p, w, h, 90)
    assert _same(enc1.fdct_quant(f, quality=90), _want(fmt, p, 420, 90, (w, h, "photo")))
    # the symbol statistics are those of the same samples in another layout
    counts, first = enc1.symbol_stats(f, quality=90)
    enc1.set_input_format(Y.YUV444)
    full = p if fmt == Y.YUV444 else (p[0], Y.upsample(p[1], w, h), Y.upsample(p[2], w, h))
    c2, f2 = enc1.symbol_stats(Y.build(Y.YUV444, *full), quality=90)
    assert counts.sum() > 0 and np.array_equal(counts, c2) and np.array_equal(first, f2)


@HALF
def test_group_batch(ref, fmt):
    ps = [_samples(ref, True, w, h, "random", seed=100 + i) for i, (w, h) in enumerate(BATCH[:5])]
    with J.Group([0, 0]) as g:
        g.set_input_format(fmt)
        outs = g.encode_batch([Y.build(fmt, *p) for p in ps], quality=90)
    for i, (w, h) in enumerate(BATCH[:5]):
        assert outs[i] == _planes_jpg(ref, fmt, ps[i], w, h, 90), i


def test_tensor_nv12_device(enc1, ref):
    w, h = 130, 50
    y, cb, cr = _samples(ref, True, w, h, "random")
    want = _planes_jpg(ref, Y.NV12, (y, cb, cr), w, h, 90)
    pitch = 144
    surf = torch.randint(0, 256, (h + 25 + 3, pitch), dtype=torch.uint8, device="cuda")  # Y rows, then Cb,Cr rows
    ty, tc = surf[:h, :w], surf[h:h + 25, :2 * 65].view(25, 65, 2)
    ty.copy_(torch.from_numpy(y).cuda())
    tc.copy_(torch.from_numpy(np.stack([cb, cr], axis=2)).cuda())
    enc1.set_input_format(J.JPGE_FMT_BGR8)
    assert enc1.encode_tensor_yuv(ty, tc, quality=90) == want
    out = torch.zeros(J.max_jpeg_bytes(w, h), dtype=torch.uint8, device="cuda")
    n = enc1.encode_tensor_yuv(ty, tc, quality=90, out=out)
    torch.cuda.synchronize()
    assert out[:n].cpu().numpy().tobytes() == want
    assert enc1.input_format() == (J.JPGE_FMT_BGR8, 0)  # as before


def test_tensor_i420_and_444_host(enc1, ref):
    w, h = 33, 17
    y, cb, cr = _samples(ref, True, w, h, "random")
    f = torch.from_numpy(np.asarray(Y.build(Y.I420, y, cb, cr)))
    n, c = w * h, 17 * 9
    planes = (f[:n].view(h, w), f[n:n + c].view(9, 17), f[n + c:].view(9, 17))
    assert enc1.encode_tensor_yuv(*planes, quality=90) == _planes_jpg(ref, Y.I420, (y, cb, cr), w, h, 90)
    p = _samples(ref, False, w, h, "random")
    t = torch.from_numpy(Y.build(Y.YUV444, *p))
    assert enc1.encode_tensor_yuv(t[0], t[1], t[2], quality=90) == _planes_jpg(ref, Y.YUV444, p, w, h, 90)
    assert enc1.input_format() == (J.JPGE_FMT_RGB8, 0)


# ---- 7. refusals: each raises and leaves the context as it was ----
def _rgb_still_works(e):
    rgb = J.synth_rgb8(4, 80, 32, kind=1)
    assert e.input_format() == (J.JPGE_FMT_RGB8, 0)
    assert e.encode(rgb, quality=90) == _oracle.encode(rgb, 90)


@HALF
def test_refuses_other_modes(enc, ref, fmt):
    f = Y.build(fmt, *_samples(ref, True, 80, 32, "random"))
    enc.set_input_format(fmt)
    for mode in MODES:
        enc.set_subsampling(mode)
        with pytest.raises(J.JpgeError) as ei:
            enc.encode(f, quality=90)
        assert ei.value.status == 1  # JPGE_E_ARG
        with pytest.raises(J.JpgeError):
            enc.fdct_quant(f, quality=90)
    enc.set_subsampling(420)
    assert enc.input_format() == (fmt, 0)
    enc.set_input_format(J.JPGE_FMT_RGB8)
    _rgb_still_works(enc)


@FMT
def test_refuses_maxval(enc, ref, fmt):
    p = _samples(ref, fmt in Y.HALF, 80, 32, "random")
    f = Y.build(fmt, *p)
    enc.set_input_format(fmt)
    with pytest.raises(J.JpgeError) as ei:
        enc.encode(f, quality=90, maxval=254)
    assert ei.value.status == 1
    # in a batch it is the frame's status: the call reports it
    with pytest.raises(J.JpgeError):
        enc.encode_batch([f, f], quality=90, maxval=254)
    assert enc.encode(f, quality=90) == _planes_jpg(ref, fmt, p, 80, 32, 90)
    enc.set_input_format(J.JPGE_FMT_RGB8)
    _rgb_still_works(enc)


@FMT
def test_refuses_short_stride(enc, ref, fmt):
    w, h = 33, 17
    p = _samples(ref, fmt in Y.HALF, w, h, "random")
    buf, stride, _ = Y.raw(fmt, *p)
    assert stride == (34 if fmt == Y.NV12 else 33)
    enc.set_input_format(fmt)
    dev = torch.from_numpy(buf).cuda()
    out = torch.zeros(J.max_jpeg_bytes(w, h), dtype=torch.uint8, device="cuda")
    with pytest.raises(J.JpgeError) as ei:
        enc.encode_ptr(dev.data_ptr(), w, h, stride - 1, out.data_ptr(), out.numel(), 90)
    assert ei.value.status == 1
    n = enc.encode_ptr(dev.data_ptr(), w, h, 0, out.data_ptr(), out.numel(), 90)  # 0: the layout's least stride
    torch.cuda.synchronize()
    assert out[:n].cpu().numpy().tobytes() == _planes_jpg(ref, fmt, p, w, h, 90)
    enc.set_input_format(J.JPGE_FMT_RGB8)
    _rgb_still_works(enc)


@FMT
def test_refuses_stripes(enc1, fmt):
    enc1.set_input_format(fmt)
    dev = torch.zeros(3 * 256 * 128, dtype=torch.uint8, device="cuda")
    with pytest.raises(J.JpgeError) as ei:
        enc1.stripe_transform(dev.data_ptr(), 256, 256, 128, 0, 2, 90)
    assert ei.value.status == 1 and enc1.input_format() == (fmt, 0)
    enc1.set_input_format(J.JPGE_FMT_RGB8)
    _rgb_still_works(enc1)


def test_refuses_bad_settings(enc):
    for fmt in (-1, 5, 15, 19, 99, 1000):
        with pytest.raises(J.JpgeError):
            enc.set_input_format(fmt)
    _rgb_still_works(enc)


def test_tensor_refusals(enc1):
    w, h = 64, 16
    a = torch.zeros((h + 8, 64), dtype=torch.uint8, device="cuda")
    b = torch.zeros((8, 64), dtype=torch.uint8, device="cuda")
    wide = torch.zeros((h + 8, 96), dtype=torch.uint8, device="cuda")
    ty = a[:h]
    bad = [
        (ty, b.view(8, 32, 2)),                                        # two allocations
        (wide[:h, :w], wide.view(-1)[96 * h:96 * h + 512].view(8, 32, 2)),  # NV12: Cb,Cr pitch 64 under Y pitch 96
        (ty, a[h:, :32], a[h:, 32:]),                                  # I420: Cb, Cr side by side, pitch 64 for 32
        (a[8:], a[:8].view(8, 32, 2)),                                 # the chroma before the Y plane
        (ty, a[h:, ::2].unsqueeze(2).expand(8, 32, 2)),                # Cb,Cr pairs not packed
        (ty, a[h:].view(8, 32, 2), a[h:]),                             # shapes of no layout
    ]
    for args in bad:
        with pytest.raises(ValueError):
            enc1.encode_tensor_yuv(*args, quality=90)
    # the same planes laid out as the layouts say do encode
    assert enc1.encode_tensor_yuv(ty, a[h:].view(8, 32, 2), quality=90)[:2] == b"\xff\xd8"
    assert enc1.encode_tensor_yuv(wide[:h, :w], wide[h:, :64].view(8, 32, 2), quality=90)[:2] == b"\xff\xd8"
    _rgb_still_works(enc1)
