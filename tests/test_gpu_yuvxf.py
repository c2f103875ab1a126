"""The sample transform of Y, Cb, Cr and gray input (jpge_set_yuv_transform): limited-range and
BT.709 samples converted inside K1, by its !kExact instances of the Y, Cb, Cr builds.
Expectations (_yuvxf.py, checked by test_yuvxf_cpu.py): the three lines of jpge.h in numpy with
the coefficients the library returned or was given, then the oracle's primitives for the
coefficients (_yuv.want_coeffs), Encoder.encode_planes on a separate context for whole files
(as test_gpu_yuv.py does), _gray's builder for the one-component stream and _fixedhuff's coder
for fixed tables.  Every comparison is exact."""
import functools

import numpy as np
import pytest

import _fixedhuff as F
import _gray as G
import _oracle
import _yuv as Y
import _yuvxf as X
import jpgenc_amd as J

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GRAY = X.GRAY
LAYOUTS = (Y.NV12, Y.I420, Y.YUV444, GRAY)
NAMES = {**Y.NAMES, GRAY: "gray"}
FMT = pytest.mark.parametrize("fmt", LAYOUTS, ids=[NAMES[f] for f in LAYOUTS])
XF = pytest.mark.parametrize("xf", ["limited601", "limited709", "full709", "custom"])
# the set that reaches every branch of a tile in test_gpu_yuv.py
SIZES = [(1, 1), (16, 16), (64, 16), (80, 32), (33, 17), (130, 50)]
KINDS = ["random", "zeros", "ones"]
MODES = [444, 422, 411, 4200, 4201]
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
    """The context of the expectations (encode_planes): never given a transform."""
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
        e.set_huffman(J.JPGE_HUFF_OPTIMAL)
        e.set_yuv_transform(J.JPGE_YUV_FULL_601)
    assert ref.yuv_transform() == (J.JPGE_YUV_FULL_601, X.IDENTITY)


@functools.lru_cache(maxsize=None)
def _samples(half, w, h, kind, seed=None):
    """(y, cb, cr) uint8 planes, chroma at half size or full: random bytes over 0..255 (both
    clamps fire), or every sample 0 / 255.  The gray layout takes the Y plane."""
    return Y.samples(Y.I420 if half else Y.YUV444, 1000 * w + h if seed is None else seed, w, h, kind)


def _p(fmt, w, h, kind="random", seed=None):
    return _samples(fmt in Y.HALF, w, h, kind, seed)


def _frame(fmt, p):
    return np.ascontiguousarray(p[0]) if fmt == GRAY else Y.build(fmt, *p)


def _set(e, fmt, xf, plane_stride=0):
    """The layout and the transform on a context; returns the coefficients in force."""
    preset, given, t = X.coeffs(xf)
    e.set_input_format(fmt, plane_stride)
    e.set_yuv_transform(preset, given)
    assert e.yuv_transform() == (preset, tuple(t))
    return t


@functools.lru_cache(maxsize=None)
def _planes(half, gray, w, h, kind, seed, t, mcu):
    p = _samples(half, w, h, kind, seed)
    if gray:
        return X.planes(GRAY, p[0], None, None, t)
    return X.planes(Y.I420 if half else Y.YUV444, *p, t, mcu=mcu)


def _xplanes(fmt, w, h, kind, t, mode=420, seed=None):
    return _planes(fmt in Y.HALF, fmt == GRAY, w, h, kind, seed, tuple(t), Y.mcu_size(mode))


@functools.lru_cache(maxsize=None)
def _want_coeffs(half, gray, w, h, kind, seed, t, mode, quality):
    pl = _planes(half, gray, w, h, kind, seed, t, Y.mcu_size(mode))
    if gray:
        return (Y._blocks(pl[0], _oracle.quality_tables(quality)[0]),)
    return Y.want_coeffs(pl, mode, quality)


def _want(fmt, w, h, kind, t, mode=420, quality=90, seed=None):
    return _want_coeffs(fmt in Y.HALF, fmt == GRAY, w, h, kind, seed, tuple(t), mode, quality)


def _same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


@functools.lru_cache(maxsize=None)
def _gray_jpg(w, h, kind, seed, t, quality, restart):
    return X.gray_file(_samples(False, w, h, kind, seed)[0], t, _oracle.quality_tables(quality)[0], restart).jpg


def _want_jpg(ref, fmt, w, h, kind, t, quality=90, restart=0, seed=None):
    """The expected file: encode_planes of the transformed planes on the separate context
    (FULL_601: it applies nothing of its own), or _gray's builder."""
    if fmt == GRAY:
        return _gray_jpg(w, h, kind, seed, tuple(t), quality, restart)
    ref.set_restart(restart)
    return ref.encode_planes(*_xplanes(fmt, w, h, kind, t, seed=seed), w, h, J.JPGE_TO_YCBCR, quality)


# ---- 1. coefficients ----
@FMT
@XF
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w,h", SIZES)
def test_coefficients(enc, fmt, xf, w, h, kind):
    t = _set(enc, fmt, xf)
    got = enc.fdct_quant(_frame(fmt, _p(fmt, w, h, kind)), quality=90)
    assert _same(got, _want(fmt, w, h, kind, t))


@XF
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("w,h", MODE_SIZES)
def test_coefficients_modes(enc, xf, mode, w, h):
    # YUV444_PLANAR: the transform per pixel, then the mode's filter in the reference's op order
    t = _set(enc, Y.YUV444, xf)
    enc.set_subsampling(mode)
    got = enc.fdct_quant(_frame(Y.YUV444, _p(Y.YUV444, w, h)), quality=90)
    assert _same(got, _want(Y.YUV444, w, h, "random", t, mode=mode))


@pytest.mark.parametrize("mode", MODES + [420])
def test_gray_ignores_the_mode(enc, mode):
    t = _set(enc, GRAY, "custom")
    enc.set_subsampling(mode)
    got = enc.fdct_quant(_frame(GRAY, _p(GRAY, 136, 24)), quality=90)
    assert _same(got, _want(GRAY, 136, 24, "random", t))


# ---- 2. whole files ----
@FMT
@pytest.mark.parametrize("quality", [50, 90, 100])
@pytest.mark.parametrize("w,h", SIZES)
def test_whole_file(enc, ref, fmt, w, h, quality):
    xf = {50: "limited601", 90: "limited709", 100: "custom"}[quality]
    t = _set(enc, fmt, xf)
    assert enc.encode(_frame(fmt, _p(fmt, w, h)), quality=quality) == _want_jpg(ref, fmt, w, h, "random", t, quality)


@FMT
def test_whole_file_restart(enc, ref, fmt):
    w, h = 130, 50
    t = _set(enc, fmt, "limited709")
    enc.set_restart(3)
    got = enc.encode(_frame(fmt, _p(fmt, w, h)), quality=90)
    assert got == _want_jpg(ref, fmt, w, h, "random", t, 90, restart=3)
    assert got.count(b"\xff\xdd") >= 1  # DRI


@pytest.mark.parametrize("mode", MODES)
def test_modes_whole_file(enc, mode):
    w, h = 136, 24
    t = _set(enc, Y.YUV444, "limited709")
    enc.set_subsampling(mode)
    info, y, cb, cr = J.decode_coeffs(enc.encode(_frame(Y.YUV444, _p(Y.YUV444, w, h)), quality=90))
    assert (info.width, info.height) == (w, h)
    assert _same((y, cb, cr), _want(Y.YUV444, w, h, "random", t, mode=mode))


# ---- 3. the two instances agree; the default is unchanged ----
@FMT
@pytest.mark.parametrize("w,h", [(33, 17), (130, 50)])
def test_identity_custom_equals_full601(enc, fmt, w, h):
    f = _frame(fmt, _p(fmt, w, h))
    enc.set_input_format(fmt)
    base = enc.encode(f, quality=90)  # the kExact instances
    base_c = enc.fdct_quant(f, quality=90)
    _set(enc, fmt, "identity")        # CUSTOM with the identity: the !kExact instances
    assert enc.encode(f, quality=90) == base
    assert _same(enc.fdct_quant(f, quality=90), base_c)
    enc.set_yuv_transform(J.JPGE_YUV_FULL_601)
    assert enc.yuv_transform() == (J.JPGE_YUV_FULL_601, X.IDENTITY)


@FMT
def test_back_to_the_default(enc, ref, fmt):
    w, h = 130, 50
    p = _p(fmt, w, h)
    t = _set(enc, fmt, "limited709")
    assert enc.encode(_frame(fmt, p), quality=90) == _want_jpg(ref, fmt, w, h, "random", t)
    enc.set_yuv_transform(J.JPGE_YUV_FULL_601)
    got = enc.encode(_frame(fmt, p), quality=90)
    if fmt == GRAY:
        assert got == G.build(p[0], _oracle.quality_tables(90)[0]).jpg
    else:
        assert got == ref.encode_planes(*Y.pad_planes(fmt, *p), w, h, J.JPGE_TO_YCBCR, 90)
        assert _same(enc.fdct_quant(_frame(fmt, p), quality=90), Y.want_coeffs(Y.pad_planes(fmt, *p), 420, 90))


def test_rgb_ignores_the_setting(enc, enc1):
    rgb = J.synth_rgb8(4, 80, 32, kind=1)
    for e in (enc, enc1):
        e.set_yuv_transform(J.JPGE_YUV_LIMITED_709)
        assert e.encode(rgb, quality=90) == _oracle.encode(rgb, 90)
        assert e.encode(rgb, quality=90, maxval=200) == _oracle.encode(rgb, 90, maxval=200)
        e.set_input_format(J.JPGE_FMT_RGB8_PLANAR)
        assert e.encode(np.ascontiguousarray(rgb.transpose(2, 0, 1)), quality=90) == _oracle.encode(rgb, 90)


# ---- 4. addressing: device frames inside random bytes ----
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
    p = _p(fmt, w, h)
    if case == "unaligned":  # the clamped path: a padded stride, an odd plane stride, the base 1 byte in
        stride, off = w + 24, 1
        ps = stride * h + 37
    else:  # every base and pitch 16-byte aligned: the fast path
        stride, off = (64 if w <= 64 else 128), 32
        ps = stride * h + 48
    t = _set(enc, fmt, "limited709", 0 if fmt == GRAY else ps)
    want = _want_jpg(ref, fmt, w, h, "random", t)
    src = (p[0], p[0], p[0]) if fmt == GRAY else p  # (gray: the Y plane of a 4:4:4 buffer)
    outs = [_encode_dev(enc, Y.raw(Y.YUV444 if fmt == GRAY else fmt, *src, stride=stride, plane_stride=ps, offset=off, seed=s)[0],
                        off, w, h, stride) for s in (9, 10)]  # other bytes around the frame
    assert outs[0] == outs[1] == want


@FMT
def test_host_input_padded_stride(enc1, ref, fmt):
    # host frames go through the upload's repitch: the transform sees the same samples
    w, h = 33, 17
    t = _set(enc1, fmt, "custom")
    assert enc1.encode(_frame(fmt, _p(fmt, w, h)), quality=90) == _want_jpg(ref, fmt, w, h, "random", t)


# ---- 5. pipeline shapes ----
BATCH = [(160, 96) if i % 2 == 0 else (48 + 16 * i, 40 + i) for i in range(9)]  # 5 of one size: sets form


@pytest.mark.parametrize("fmt", [Y.NV12, Y.I420, GRAY], ids=["nv12", "i420", "gray"])
@pytest.mark.parametrize("lanes", [4, 1])
def test_batch(enc, enc1, ref, fmt, lanes):
    e = enc if lanes == 4 else enc1
    assert e.lanes() == lanes
    t = _set(e, fmt, "limited709")
    outs = e.encode_batch([_frame(fmt, _p(fmt, w, h, seed=100 + i)) for i, (w, h) in enumerate(BATCH)], quality=90)
    for i, (w, h) in enumerate(BATCH):
        assert outs[i] == _want_jpg(ref, fmt, w, h, "random", t, seed=100 + i), i


@FMT
def test_frame_sets_short_last_set(enc, ref, fmt):
    w, h = 136, 72
    t = _set(enc, fmt, "custom")
    outs = enc.encode_batch([_frame(fmt, _p(fmt, w, h, seed=200 + i)) for i in range(9)], quality=75)  # 4 + 4 + 1
    assert outs == [_want_jpg(ref, fmt, w, h, "random", t, 75, seed=200 + i) for i in range(9)]


def test_preset_change_between_batches(enc, ref):
    w, h = 136, 72
    frames = [_frame(Y.NV12, _p(Y.NV12, w, h, seed=200 + i)) for i in range(5)]
    for xf in ("limited709", "limited601"):
        t = _set(enc, Y.NV12, xf)
        assert enc.encode_batch(frames, quality=75) == [
            _want_jpg(ref, Y.NV12, w, h, "random", t, 75, seed=200 + i) for i in range(5)], xf
    enc.set_yuv_transform(J.JPGE_YUV_FULL_601)
    assert enc.encode_batch(frames[:2], quality=75) == [
        ref.encode_planes(*Y.pad_planes(Y.NV12, *_p(Y.NV12, w, h, seed=200 + i)), w, h, J.JPGE_TO_YCBCR, 75) for i in range(2)]


def test_one_lane_stages(enc1, ref):
    w, h = 130, 50
    t = _set(enc1, Y.NV12, "limited709")
    f = _frame(Y.NV12, _p(Y.NV12, w, h))
    assert _same(enc1.fdct_quant(f, quality=90), _want(Y.NV12, w, h, "random", t))
    # the symbol statistics are those of the same samples in another layout
    counts, first = enc1.symbol_stats(f, quality=90)
    p = _p(Y.NV12, w, h)
    enc1.set_input_format(Y.YUV444)
    c2, f2 = enc1.symbol_stats(Y.build(Y.YUV444, p[0], Y.upsample(p[1], w, h), Y.upsample(p[2], w, h)), quality=90)
    assert counts.sum() > 0 and np.array_equal(counts, c2) and np.array_equal(first, f2)


@pytest.mark.parametrize("fmt", [Y.NV12, Y.I420], ids=["nv12", "i420"])
def test_group_batch(ref, fmt):
    preset, given, t = X.coeffs("limited709")
    with J.Group([0, 0]) as g:
        g.set_input_format(fmt)
        g.set_yuv_transform(preset, given)
        outs = g.encode_batch([_frame(fmt, _p(fmt, w, h, seed=100 + i)) for i, (w, h) in enumerate(BATCH[:5])], quality=90)
    for i, (w, h) in enumerate(BATCH[:5]):
        assert outs[i] == _want_jpg(ref, fmt, w, h, "random", t, seed=100 + i), i


# ---- 6. fixed Huffman tables: the case the clamps protect ----
@pytest.mark.parametrize("fmt", [Y.NV12, Y.YUV444, GRAY], ids=["nv12", "yuv444", "gray"])
@pytest.mark.parametrize("kind", KINDS)
def test_fixed_tables(enc, fmt, kind):
    # random bytes reach far outside studio swing: unclamped, LIMITED_709 would carry them past
    # the 8-bit interval and the coefficients past DC category 11 / AC size 10, for which a
    # fixed table has no code
    w, h = 130, 50
    t = _set(enc, fmt, "limited709")
    enc.set_huffman(J.JPGE_HUFF_STANDARD)
    specs = [J.standard_huffman(i) for i in range(4)]
    qy, qc = _oracle.quality_tables(100)
    got = enc.encode(_frame(fmt, _p(fmt, w, h, kind)), quality=100)
    c = _want(fmt, w, h, kind, t, quality=100)
    if fmt == GRAY:
        want = F.header_gray(w, h, qy, specs) + F.scan(F.mcu_blocks(c[0], None, None, w, h, 444), specs) + b"\xff\xd9"
    else:
        want = F.expected_coeffs(*c, w, h, qy, qc, specs)
    assert got == want
    assert all(np.abs(x[:, 0]).max() < 2048 and np.abs(x[:, 1:]).max() < 1024 for x in c)  # the bound itself


# ---- 7. the tensor entries follow the context ----
def test_tensor_nv12_device(enc1, ref):
    w, h = 130, 50
    y, cb, cr = _p(Y.NV12, w, h)
    t = _set(enc1, J.JPGE_FMT_BGR8, "limited709")
    want = _want_jpg(ref, Y.NV12, w, h, "random", t)
    pitch = 144
    surf = torch.randint(0, 256, (h + 25 + 3, pitch), dtype=torch.uint8, device="cuda")  # Y rows, then Cb,Cr rows
    ty, tc = surf[:h, :w], surf[h:h + 25, :2 * 65].view(25, 65, 2)
    ty.copy_(torch.from_numpy(y).cuda())
    tc.copy_(torch.from_numpy(np.stack([cb, cr], axis=2)).cuda())
    assert enc1.encode_tensor_yuv(ty, tc, quality=90) == want
    assert enc1.input_format() == (J.JPGE_FMT_BGR8, 0)  # as before
    # a 2-D tensor is a gray frame: y_off and m0
    assert enc1.encode_tensor(ty, quality=90) == _want_jpg(ref, GRAY, w, h, "random", t)


# ---- 8. refusals: each raises and leaves the context encoding as it was ----
def test_refusals(enc, ref):
    w, h = 80, 32
    t = _set(enc, Y.NV12, "limited601")
    f = _frame(Y.NV12, _p(Y.NV12, w, h))
    want = _want_jpg(ref, Y.NV12, w, h, "random", t)
    nan, inf = float("nan"), float("inf")
    bad = [(-1, None), (5, None), (J.JPGE_YUV_CUSTOM, None),
           (J.JPGE_YUV_CUSTOM, (nan,) + X.IDENTITY[1:]), (J.JPGE_YUV_CUSTOM, (-0.5,) + X.IDENTITY[1:]),
           (J.JPGE_YUV_CUSTOM, (255.5,) + X.IDENTITY[1:])]
    for i in range(1, 8):
        for v in (4.5, -4.5, inf, nan):
            c = list(X.IDENTITY)
            c[i] = v
            bad.append((J.JPGE_YUV_CUSTOM, tuple(c)))
    for preset, c in bad:
        with pytest.raises(J.JpgeError) as ei:
            enc.set_yuv_transform(preset, c)
        assert ei.value.status == 1, (preset, c)
    assert enc.yuv_transform() == (J.JPGE_YUV_LIMITED_601, tuple(t))
    assert enc.encode(f, quality=90) == want
    # maxval must still be 255; in a batch it is the frame's status
    with pytest.raises(J.JpgeError) as ei:
        enc.encode(f, quality=90, maxval=254)
    assert ei.value.status == 1
    with pytest.raises(J.JpgeError):
        enc.encode_batch([f, f], quality=90, maxval=254)
    # NV12 outside S420_M stays refused
    enc.set_subsampling(444)
    with pytest.raises(J.JpgeError):
        enc.encode(f, quality=90)
    enc.set_subsampling(420)
    assert enc.encode(f, quality=90) == want


def test_refuses_stripes(enc1):
    _set(enc1, Y.NV12, "limited709")
    dev = torch.zeros(3 * 256 * 128, dtype=torch.uint8, device="cuda")
    with pytest.raises(J.JpgeError) as ei:
        enc1.stripe_transform(dev.data_ptr(), 256, 256, 128, 0, 2, 90)
    assert ei.value.status == 1
