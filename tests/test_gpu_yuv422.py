"""The 4:2:2 input layouts (JPGE_FMT_YUYV, _UYVY, _NV16, _I422): K1 reads a capture buffer's
or a 4:2:2 decoder's samples in place.  A frame is, byte for byte of the .jpg, the
JPGE_FMT_YUV444_PLANAR frame whose chroma planes hold c[y][x >> 1] at pixel (y, x), in every
subsampling mode.  Expectations (_yuv422.py and _yuv.py, checked by test_yuv422_cpu.py and
test_yuv_cpu.py): coefficients from the oracle's primitives on those repeated planes, whole
files from _fixedhuff's coder or from the YUV444_PLANAR encode of the repeated planes on a
separate context (pinned to the oracle by test_gpu_yuv.py).  Every comparison is exact."""
import functools

import numpy as np
import pytest

import _fixedhuff as F
import _oracle
import _yuv as Y
import _yuv422 as Z
import _yuvxf as X
import jpgenc_amd as J

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FMT = pytest.mark.parametrize("fmt", Z.FORMATS, ids=[Z.NAMES[f] for f in Z.FORMATS])
# the row-8 tile is 128x8 px, the 4:2:0 tile 64x16: a lone and a half-filled group, the clamped
# path only, one MCU, odd width, exactly one fast row-8 tile, fast + clamped tiles, larger mixes
SIZES = [(1, 1), (2, 1), (9, 9), (16, 8), (33, 17), (128, 8), (136, 24), (130, 50), (160, 96)]
KINDS = ["random", "photo", "zeros", "ones"]
MODES = [444, 420, 411, 4200, 4201]  # the five modes beside the native 422
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
    """The context of the expectations (YUV444_PLANAR encodes, color_convert)."""
    e = J.Encoder(0, lanes=1)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def _defaults(enc, enc1, ref):
    for e in (enc, enc1, ref):
        e.set_subsampling(422)
    yield
    for e in (enc, enc1, ref):
        e.set_input_format(J.JPGE_FMT_RGB8)
        e.set_subsampling(420)
        e.set_restart(0)
        e.set_huffman(J.JPGE_HUFF_OPTIMAL)
        e.set_yuv_transform(J.JPGE_YUV_FULL_601)


_photo = {}


def _samples(ref, w, h, kind="random", seed=None):
    """(y, cb, cr) uint8 planes, chroma (h, cw); photo: synth_rgb8 through color_convert, + 128,
    rounded and clipped, the even column's chroma sample of each pair."""
    if kind != "photo":
        return Z.samples(1000 * w + h if seed is None else seed, w, h, kind)
    if (w, h) not in _photo:
        rgb = J.synth_rgb8(w + h, w, h, kind=0).astype(np.float64)
        ycc = ref.color_convert(rgb[:, :, 0], rgb[:, :, 1], rgb[:, :, 2], J.JPGE_TO_YCBCR)
        y, cb, cr = (np.clip(np.rint(p + 128.0), 0, 255).astype(np.uint8) for p in ycc)
        _photo[(w, h)] = (y, cb[:, ::2].copy(), cr[:, ::2].copy())
    return _photo[(w, h)]


@functools.lru_cache(maxsize=None)
def _want_cached(key, mode, quality):
    planes = _want_cached.planes[key]
    return Y.want_coeffs(Y.pad_planes(Y.YUV444, *Z.repeated(*planes), mcu=Y.mcu_size(mode)), mode, quality)


_want_cached.planes = {}


def _want(planes, mode, quality, key):
    """want_coeffs of the repeated planes, computed once per (input, mode, quality): the four
    layouts share it."""
    _want_cached.planes.setdefault(key, planes)
    return _want_cached(key, mode, quality)


def _same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


def _ref_jpg(ref, p, quality, mode=422, restart=0, xf=None):
    """The encode of the repeated-chroma YUV444_PLANAR frame on the separate context."""
    ref.set_input_format(Y.YUV444)
    ref.set_subsampling(mode)
    ref.set_restart(restart)
    if xf is not None:
        preset, given, _ = X.coeffs(xf)
        ref.set_yuv_transform(preset, given)
    try:
        return ref.encode(Z.yuv444(*p), quality=quality)
    finally:
        ref.set_yuv_transform(J.JPGE_YUV_FULL_601)


# ---- 1. coefficients ----
@FMT
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w,h", SIZES)
def test_coefficients(enc, ref, fmt, w, h, kind):
    p = _samples(ref, w, h, kind)
    enc.set_input_format(fmt)
    got = enc.fdct_quant(Z.build(fmt, *p), quality=90)
    assert _same(got, _want(p, 422, 90, (w, h, kind)))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w,h", [(96, 16), (80, 16)])
def test_coefficients_i422_chroma_load_at_the_row_end(enc, ref, w, h, kind):
    # an I422 lane loads the aligned 16 chroma bytes that hold its 8.  96 px: the lanes at
    # x = 64 and x = 80 share bytes 32..47, the last of a 48-byte row.  80 px: the lane at
    # x = 64 lies inside the Y row, but its load, bytes 32..47, would pass the end of the
    # 40-byte chroma row (on the last row, the end of the plane): it takes the clamped path
    p = _samples(ref, w, h, kind)
    enc.set_input_format(Z.I422)
    assert _same(enc.fdct_quant(Z.build(Z.I422, *p), quality=90), _want(p, 422, 90, (w, h, kind)))


@FMT
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["random", "photo"])
@pytest.mark.parametrize("w,h", MODE_SIZES)
def test_coefficients_modes(enc, ref, fmt, mode, w, h, kind):
    p = _samples(ref, w, h, kind)
    enc.set_input_format(fmt)
    enc.set_subsampling(mode)
    got = enc.fdct_quant(Z.build(fmt, *p), quality=90)
    assert _same(got, _want(p, mode, 90, (w, h, kind)))


# ---- 2. whole files with fixed tables ----
@pytest.fixture(scope="module")
def std():
    return F.golden_specs()


@FMT
@pytest.mark.parametrize("quality", [50, 90, 100])
@pytest.mark.parametrize("w,h", [(33, 17), (136, 24)])
def test_fixed_tables_whole_file(enc, ref, std, fmt, w, h, quality):
    kind = "photo" if quality == 90 else "random"
    p = _samples(ref, w, h, kind)
    qy, qc = _oracle.quality_tables(quality)
    enc.set_input_format(fmt)
    enc.set_huffman(J.JPGE_HUFF_STANDARD)
    got = enc.encode(Z.build(fmt, *p), quality=quality)
    assert got == F.expected_coeffs(*_want(p, 422, quality, (w, h, kind)), w, h, qy, qc, std, mode=422)


@FMT
def test_fixed_tables_restart(enc, ref, std, fmt):
    w, h = 130, 50
    p = _samples(ref, w, h, "random")
    qy, qc = _oracle.quality_tables(90)
    enc.set_input_format(fmt)
    enc.set_huffman(J.JPGE_HUFF_STANDARD)
    enc.set_restart(7)
    got = enc.encode(Z.build(fmt, *p), quality=90)
    assert got == F.expected_coeffs(*_want(p, 422, 90, (w, h, "random")), w, h, qy, qc, std, mode=422, restart=7)
    assert got.count(b"\xff\xdd") >= 1  # DRI


# ---- 3. whole files with per-image tables ----
@pytest.mark.parametrize("restart", [0, 3])
@pytest.mark.parametrize("mode", [422, 420])
@pytest.mark.parametrize("w,h", [(33, 17), (130, 50)])
def test_whole_file_equals_repeated_444(enc, ref, mode, w, h, restart):
    p = _samples(ref, w, h, "photo" if restart else "random")
    want = _ref_jpg(ref, p, 90, mode, restart)
    outs = []
    for fmt in Z.FORMATS:
        enc.set_input_format(fmt)
        enc.set_subsampling(mode)
        enc.set_restart(restart)
        outs.append(enc.encode(Z.build(fmt, *p), quality=90))
    assert outs[0] == outs[1] == outs[2] == outs[3] == want
    if mode == 422:  # and the file holds the expected coefficients
        info, y, cb, cr = J.decode_coeffs(want)
        assert (info.width, info.height) == (w, h)
        assert _same((y, cb, cr), _want(p, mode, 90, (w, h, "photo" if restart else "random")))


# ---- 4. sample transform ----
@FMT
@pytest.mark.parametrize("xf", ["limited709", "custom"])
@pytest.mark.parametrize("mode", [422, 420])
def test_sample_transform(enc, ref, fmt, xf, mode):
    w, h = 136, 24
    p = _samples(ref, w, h, "random")
    preset, given, t = X.coeffs(xf)
    enc.set_input_format(fmt)
    enc.set_subsampling(mode)
    enc.set_yuv_transform(preset, given)
    f = Z.build(fmt, *p)
    assert enc.encode(f, quality=90) == _ref_jpg(ref, p, 90, mode, xf=xf)
    # the transform per pixel of the repeated planes, then the mode's filter
    planes = X.planes(Y.YUV444, *Z.repeated(*p), t, mcu=Y.mcu_size(mode))
    assert _same(enc.fdct_quant(f, quality=90), Y.want_coeffs(planes, mode, 90))


@FMT
def test_sample_transform_clamped_path(enc, ref, fmt):
    w, h = 33, 17
    p = _samples(ref, w, h, "random")
    preset, given, t = X.coeffs("limited709")
    enc.set_input_format(fmt)
    enc.set_yuv_transform(preset, given)
    planes = X.planes(Y.YUV444, *Z.repeated(*p), t, mcu=(16, 8))
    assert _same(enc.fdct_quant(Z.build(fmt, *p), quality=90), Y.want_coeffs(planes, 422, 90))


# ---- 5. addressing: device frames inside random bytes ----
def _encode_dev(e, buf, off, w, h, stride, quality=90):
    dev = torch.from_numpy(buf).cuda()
    assert dev.data_ptr() % 16 == 0
    out = torch.zeros(J.max_jpeg_bytes(w, h), dtype=torch.uint8, device="cuda")
    n = e.encode_ptr(dev.data_ptr() + off, w, h, stride, out.data_ptr(), out.numel(), quality)
    torch.cuda.synchronize()
    return out[:n].cpu().numpy().tobytes()


@FMT
@pytest.mark.parametrize("w,h", [(136, 24), (33, 17), (96, 16), (80, 16)])
@pytest.mark.parametrize("case", ["unaligned", "aligned"])
def test_addressing(enc, ref, fmt, w, h, case):
    p = _samples(ref, w, h, "random")
    least = Z.least_stride(fmt, w)
    if case == "unaligned":  # an odd stride, a plane stride that is no multiple of 16, the base 1 byte in
        stride, off = least + 25 + (least % 2), 1
        ps = stride * h + 37
    else:  # every base and pitch a multiple of 32, the plane stride of 16: the fast path
        stride, off = -(-least // 32) * 32 + 32, 32
        ps = stride * h + 48
    assert (stride % 2 == 1) == (case == "unaligned")
    ps = 0 if fmt in Z.PACKED else ps
    want = _ref_jpg(ref, p, 90)
    enc.set_input_format(fmt, ps)
    assert enc.input_format() == (fmt, ps)
    outs = [_encode_dev(enc, Z.raw(fmt, *p, stride=stride, plane_stride=ps, offset=off, seed=s)[0], off, w, h, stride)
            for s in (9, 10)]  # other bytes around the frame
    assert outs[0] == outs[1] == want


@pytest.mark.parametrize("fmt", Z.PACKED, ids=[Z.NAMES[f] for f in Z.PACKED])
@pytest.mark.parametrize("case", ["unaligned", "aligned"])
def test_spare_y_byte_is_storage_only(enc, ref, fmt, case):
    w, h = 33, 17
    p = _samples(ref, w, h, "random")
    stride, off = (95, 1) if case == "unaligned" else (96, 32)
    enc.set_input_format(fmt)
    outs = []
    for spare in (0, 255):
        buf = Z.raw(fmt, *p, stride=stride, offset=off, spare=spare)[0]
        outs.append(_encode_dev(enc, buf, off, w, h, stride))
    assert outs[0] == outs[1] == _ref_jpg(ref, p, 90)


# ---- 6. plumbing ----
BATCH = [(160, 96) if i % 2 == 0 else (48 + 16 * i, 40 + i) for i in range(9)]  # 5 of one size: sets form


@FMT
@pytest.mark.parametrize("lanes", [4, 1])
def test_batch_host(enc, enc1, ref, fmt, lanes):
    e = enc if lanes == 4 else enc1
    assert e.lanes() == lanes
    ps = [_samples(ref, w, h, "random", seed=100 + i) for i, (w, h) in enumerate(BATCH)]
    e.set_input_format(fmt)
    outs = e.encode_batch([Z.build(fmt, *p) for p in ps], quality=90)
    for i, p in enumerate(ps):
        assert outs[i] == _ref_jpg(ref, p, 90), i


@FMT
@pytest.mark.parametrize("lanes", [4, 1])
def test_batch_device(enc, enc1, ref, fmt, lanes):
    e = enc if lanes == 4 else enc1
    ps = [_samples(ref, w, h, "random", seed=100 + i) for i, (w, h) in enumerate(BATCH)]
    devs = [torch.from_numpy(np.asarray(Z.build(fmt, *p))).cuda() for p in ps]
    outs = [torch.zeros(J.max_jpeg_bytes(w, h), dtype=torch.uint8, device="cuda") for w, h in BATCH]
    e.set_input_format(fmt)
    lens = e.encode_batch_dev([(d.data_ptr(), w, h, 0) for d, (w, h) in zip(devs, BATCH)],
                              [(o.data_ptr(), o.numel()) for o in outs], quality=90)
    torch.cuda.synchronize()
    for i, p in enumerate(ps):
        assert outs[i][:lens[i]].cpu().numpy().tobytes() == _ref_jpg(ref, p, 90), i


@FMT
def test_frame_sets(enc, ref, fmt):
    w, h = 136, 72
    ps = [_samples(ref, w, h, "random", seed=200 + i) for i in range(9)]
    enc.set_input_format(fmt)
    outs = enc.encode_batch([Z.build(fmt, *p) for p in ps], quality=75)
    assert outs == [_ref_jpg(ref, p, 75) for p in ps]


@FMT
def test_group_batch(ref, fmt):
    ps = [_samples(ref, w, h, "random", seed=100 + i) for i, (w, h) in enumerate(BATCH[:5])]
    with J.Group([0, 0]) as g:  # (a group's members keep the default mode, 4:2:0)
        g.set_input_format(fmt)
        outs = g.encode_batch([Z.build(fmt, *p) for p in ps], quality=90)
    for i, p in enumerate(ps):
        assert outs[i] == _ref_jpg(ref, p, 90, mode=420), i


@FMT
def test_symbol_stats(enc1, ref, fmt):
    w, h = 130, 50
    p = _samples(ref, w, h, "photo")
    enc1.set_input_format(fmt)
    counts, first = enc1.symbol_stats(Z.build(fmt, *p), quality=90)
    enc1.set_input_format(Y.YUV444)
    c2, f2 = enc1.symbol_stats(Z.yuv444(*p), quality=90)
    assert counts.sum() > 0 and np.array_equal(counts, c2) and np.array_equal(first, f2)


def test_tensor_packed_device(enc1, ref):
    w, h = 130, 50
    p = _samples(ref, w, h, "random")
    want = _ref_jpg(ref, p, 90)
    for fmt, name in ((Z.YUYV, "yuyv"), (Z.UYVY, "uyvy")):
        pitch = 288  # a pitched surface: rows of 260 bytes at pitch 288
        surf = torch.randint(0, 256, (h + 2, pitch), dtype=torch.uint8, device="cuda")
        t = surf[:h, :2 * w].view(h, w, 2)
        t.copy_(torch.from_numpy(np.asarray(Z.build(fmt, *p)).reshape(h, w, 2)).cuda())
        enc1.set_input_format(J.JPGE_FMT_BGR8)
        assert enc1.encode_tensor_yuv422(t, quality=90, layout=name) == want
        out = torch.zeros(J.max_jpeg_bytes(w, h), dtype=torch.uint8, device="cuda")
        n = enc1.encode_tensor_yuv422(t, quality=90, out=out, layout=name)
        torch.cuda.synchronize()
        assert out[:n].cpu().numpy().tobytes() == want
        assert enc1.input_format() == (J.JPGE_FMT_BGR8, 0)  # as before


def test_tensor_nv16_and_i422_device(enc1, ref):
    w, h = 130, 50
    y, cb, cr = p = _samples(ref, w, h, "random")
    want = _ref_jpg(ref, p, 90)
    pitch = 160
    surf = torch.randint(0, 256, (2 * h + 3, pitch), dtype=torch.uint8, device="cuda")  # Y rows, then Cb,Cr rows
    ty, tc = surf[:h, :w], surf[h:2 * h, :2 * 65].view(h, 65, 2)
    ty.copy_(torch.from_numpy(y).cuda())
    tc.copy_(torch.from_numpy(np.stack([cb, cr], axis=2)).cuda())
    assert enc1.encode_tensor_yuv422(ty, tc, quality=90) == want
    # I422: Y rows at pitch 160, then Cb and Cr rows at pitch 80
    flat = torch.randint(0, 256, (pitch * h + 2 * 80 * h + 16,), dtype=torch.uint8, device="cuda")
    iy = flat[:pitch * h].view(h, pitch)[:, :w]
    ib = flat[pitch * h:pitch * h + 80 * h].view(h, 80)[:, :65]
    ir = flat[pitch * h + 80 * h:pitch * h + 160 * h].view(h, 80)[:, :65]
    for t, a in ((iy, y), (ib, cb), (ir, cr)):
        t.copy_(torch.from_numpy(a).cuda())
    out = torch.zeros(J.max_jpeg_bytes(w, h), dtype=torch.uint8, device="cuda")
    n = enc1.encode_tensor_yuv422(iy, ib, ir, quality=90, out=out)
    torch.cuda.synchronize()
    assert out[:n].cpu().numpy().tobytes() == want
    assert enc1.input_format() == (J.JPGE_FMT_RGB8, 0)


def test_tensor_host(enc1, ref):
    w, h = 33, 17
    y, cb, cr = p = _samples(ref, w, h, "random")
    want = _ref_jpg(ref, p, 90)
    f = torch.from_numpy(np.asarray(Z.build(Z.I422, *p)))
    n, c = w * h, 17 * h
    assert enc1.encode_tensor_yuv422(f[:n].view(h, w), f[n:n + c].view(h, 17), f[n + c:].view(h, 17), quality=90) == want
    f = torch.from_numpy(np.asarray(Z.build(Z.NV16, *p)))
    assert enc1.encode_tensor_yuv422(f[:34 * h].view(h, 34)[:, :w], f[34 * h:].view(h, 17, 2), quality=90) == want
    w = 32  # (a packed tensor has an even width)
    p = _samples(ref, w, h, "random")
    f = torch.from_numpy(np.asarray(Z.build(Z.UYVY, *p)))
    assert enc1.encode_tensor_yuv422(f.view(h, w, 2), quality=90, layout="uyvy") == _ref_jpg(ref, p, 90)
    assert enc1.input_format() == (J.JPGE_FMT_RGB8, 0)


def test_tensor_refusals(enc1):
    w, h = 64, 16
    a = torch.zeros((2 * h, 64), dtype=torch.uint8, device="cuda")
    b = torch.zeros((h, 64), dtype=torch.uint8, device="cuda")
    wide = torch.zeros((2 * h, 96), dtype=torch.uint8, device="cuda")
    ty = a[:h]
    pk = torch.zeros((h, w, 2), dtype=torch.uint8, device="cuda")
    bad = [
        ((ty, b.view(h, 32, 2)), {}),                                          # two allocations
        ((wide[:h, :w], wide.view(-1)[96 * h:96 * h + 64 * h].view(h, 32, 2)), {}),  # NV16: Cb,Cr pitch 64 under Y pitch 96
        ((ty, a[h:, :32], a[h:, 32:]), {}),                                    # I422: Cb, Cr side by side, pitch 64 for 32
        ((a[h:], a[:h].view(h, 32, 2)), {}),                                   # the chroma before the Y plane
        ((ty, a[h:, ::2].unsqueeze(2).expand(h, 32, 2)), {}),                  # Cb,Cr pairs not packed
        ((ty, a[h:].view(h, 32, 2), a[h:]), {}),                               # shapes of no layout
        ((ty,), {}),                                                           # no chroma
        ((pk,), {}),                                                           # a packed frame without its order
        ((pk,), {"layout": "nv16"}),
        ((pk[:, :63],), {"layout": "yuyv"}),                                   # odd width
        ((pk[:, ::2],), {"layout": "yuyv"}),                                   # pixels not packed
        ((pk, b.view(h, 32, 2)), {"layout": "yuyv"}),                          # a packed frame is one tensor
        ((ty, a[h:].view(h, 32, 2)), {"layout": "yuyv"}),                      # an order for planes
        ((pk.float(),), {"layout": "yuyv"}),
    ]
    for args, kw in bad:
        with pytest.raises(ValueError):
            enc1.encode_tensor_yuv422(*args, quality=90, **kw)
    # the same tensors laid out as the layouts say do encode
    assert enc1.encode_tensor_yuv422(ty, a[h:].view(h, 32, 2), quality=90)[:2] == b"\xff\xd8"
    assert enc1.encode_tensor_yuv422(wide[:h, :w], wide[h:, :64].view(h, 32, 2), quality=90)[:2] == b"\xff\xd8"
    assert enc1.encode_tensor_yuv422(pk, quality=90, layout="yuyv")[:2] == b"\xff\xd8"
    _rgb_still_works(enc1)


# ---- 7. refusals: each raises and leaves the context as it was ----
def _rgb_still_works(e):
    rgb = J.synth_rgb8(4, 80, 32, kind=1)
    e.set_subsampling(420)
    assert e.input_format() == (J.JPGE_FMT_RGB8, 0)
    assert e.encode(rgb, quality=90) == _oracle.encode(rgb, 90)


@FMT
def test_refuses_maxval(enc, ref, fmt):
    p = _samples(ref, 80, 32, "random")
    f = Z.build(fmt, *p)
    enc.set_input_format(fmt)
    with pytest.raises(J.JpgeError) as ei:
        enc.encode(f, quality=90, maxval=254)
    assert ei.value.status == 1  # JPGE_E_ARG
    with pytest.raises(J.JpgeError):  # in a batch it is the frame's status: the call reports it
        enc.encode_batch([f, f], quality=90, maxval=254)
    assert enc.input_format() == (fmt, 0)
    assert enc.encode(f, quality=90) == _ref_jpg(ref, p, 90)
    enc.set_input_format(J.JPGE_FMT_RGB8)
    _rgb_still_works(enc)


@FMT
def test_refuses_short_stride(enc, ref, fmt):
    w, h = 33, 17
    p = _samples(ref, w, h, "random")
    buf, stride, _ = Z.raw(fmt, *p)
    assert stride == {Z.YUYV: 68, Z.UYVY: 68, Z.NV16: 34, Z.I422: 33}[fmt]
    enc.set_input_format(fmt)
    dev = torch.from_numpy(buf).cuda()
    out = torch.zeros(J.max_jpeg_bytes(w, h), dtype=torch.uint8, device="cuda")
    with pytest.raises(J.JpgeError) as ei:
        enc.encode_ptr(dev.data_ptr(), w, h, stride - 1, out.data_ptr(), out.numel(), 90)
    assert ei.value.status == 1
    n = enc.encode_ptr(dev.data_ptr(), w, h, 0, out.data_ptr(), out.numel(), 90)  # 0: the layout's least stride
    torch.cuda.synchronize()
    assert out[:n].cpu().numpy().tobytes() == _ref_jpg(ref, p, 90)
    enc.set_input_format(J.JPGE_FMT_RGB8)
    _rgb_still_works(enc)


@pytest.mark.parametrize("fmt", Z.PACKED, ids=[Z.NAMES[f] for f in Z.PACKED])
def test_refuses_plane_stride_on_packed(enc, fmt):
    enc.set_input_format(J.JPGE_FMT_RGB8)
    with pytest.raises(J.JpgeError) as ei:
        enc.set_input_format(fmt, 4096)
    assert ei.value.status == 1
    _rgb_still_works(enc)


@FMT
def test_refuses_stripes(enc1, fmt):
    enc1.set_subsampling(420)
    enc1.set_input_format(fmt)
    dev = torch.zeros(3 * 256 * 128, dtype=torch.uint8, device="cuda")
    with pytest.raises(J.JpgeError) as ei:
        enc1.stripe_transform(dev.data_ptr(), 256 * 3, 256, 128, 0, 2, 90)
    assert ei.value.status == 1 and enc1.input_format() == (fmt, 0)
    enc1.set_input_format(J.JPGE_FMT_RGB8)
    _rgb_still_works(enc1)


@FMT
def test_group_refuses_striped(fmt):
    rgb = J.synth_rgb8(2, 640, 480)
    with J.Group([0, 0]) as g:
        g.set_input_format(fmt)
        with pytest.raises(J.JpgeError):
            g.encode_striped(rgb, quality=90)
        g.set_input_format(J.JPGE_FMT_RGB8)
        assert g.encode_striped(rgb, quality=90) == _oracle.encode(rgb, 90)
