"""Frames at the 65535-pixel limit, extreme aspect ratios, large pitches and the 32-bit extent
bound, on the GPU.  Shapes (_limits.LIMIT_SHAPES) are the smallest at which these paths can go
wrong: a row of 8192 MCUs three rows high, a column of 8192 one-MCU rows (every K1 tile
three-quarters invalid), a padded width of 2^16 (chroma width 2^15), 24 576 restart
segments, pitches of 64 MiB and a frame whose stride * height is just below the transform
kernel's offset bound (fdct.hip kOob, kernels.hpp kK1OffsetBound).  Expected bytes and
coefficients come from the C oracle's whole-frame entries, pinned at these shapes by
test_limits_cpu.py; the other layouts from the chain pinned at small sizes by their own
tests.  Every comparison is exact.  Pillow cannot decode above 65500 pixels (_limits.py):
the decode-side check here is decode_coeffs."""
import functools
import os

import numpy as np
import pytest

import _fixedhuff as FH
import _formats as F
import _limits as L
import _oracle
import _yuv as Y
import _yuv422 as Z
import _yuvxf as X
import jpgenc_amd as J

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SHAPES = pytest.mark.parametrize("w,h", L.LIMIT_SHAPES, ids=L.ids(L.LIMIT_SHAPES))
LONG = pytest.mark.parametrize("w,h", L.LONG, ids=L.ids(L.LONG))
K1_SHAPES = [(65535, 17), (17, 65535), (65535, 1)]
K1 = pytest.mark.parametrize("w,h", K1_SHAPES, ids=L.ids(K1_SHAPES))
CASE = pytest.mark.parametrize("case", ["fast", "clamped"])
MODE = pytest.mark.parametrize("mode", L.MODES)
BIG_PITCH = 64 * 1024 * 1024
GRAY = J.JPGE_FMT_GRAY8


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
    """The context of the expectations (encode_planes, the YUV444_PLANAR encodes)."""
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


def _encoder(lanes=0, **env):
    # (a context reads its switches when it opens: a fresh one under the setting)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return J.Encoder(0, lanes=lanes) if lanes else J.Encoder(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


# ---- 2. RGB8 against the oracle ----
@MODE
@SHAPES
def test_whole_file(enc, enc1, w, h, mode):
    rgb = L.frame("photo", w, h)
    for e in (enc, enc1):
        e.set_subsampling(mode)
        assert e.encode(rgb, quality=90) == L.want("photo", w, h, 90, mode), e.lanes()


@MODE
@LONG
@pytest.mark.parametrize("quality", [50, 100])
def test_whole_file_random_bytes(enc, enc1, w, h, mode, quality):
    rgb = L.frame("random", w, h)
    for e in (enc, enc1):
        e.set_subsampling(mode)
        assert e.encode(rgb, quality=quality) == L.want("random", w, h, quality, mode), e.lanes()


@pytest.mark.parametrize("wgs", [1, 65536], ids=["least", "most"])
def test_entropy_workgroups_forced(wgs):
    e = _encoder(lanes=1, JPGE_ENTROPY_WGS=wgs)
    try:
        for w, h in L.LONG:
            for mode in (420, 444, 411):
                e.set_subsampling(mode)
                e.set_restart(0)
                assert e.encode(L.frame("photo", w, h), quality=90) == L.want("photo", w, h, 90, mode), (w, h, mode)
                e.set_restart(1)
                assert e.encode(L.frame("photo", w, h), quality=90) == L.want("photo", w, h, 90, mode, 1), (w, h, mode)
    finally:
        e.close()


@MODE
@SHAPES
def test_fdct_quant(enc, w, h, mode):
    enc.set_subsampling(mode)
    for kind in ("photo", "random"):
        assert L.same(enc.fdct_quant(L.frame(kind, w, h), quality=90), L.want_coeffs(kind, w, h, 90, mode)), kind


@SHAPES
def test_symbol_stats(enc1, w, h):
    rgb = L.frame("photo", w, h)
    counts, first = enc1.symbol_stats(rgb, quality=90)
    ocounts, ofirst = _oracle.stage_hist(rgb, 90)
    assert np.array_equal(counts, ocounts)
    none = np.uint64(0xFFFFFFFFFFFFFFFF)
    for t in range(4):
        present = np.nonzero(ocounts[t])[0]
        # the first-occurrence order of the present symbols is what the table build consumes: the
        # Y text key is the block's raster index from (MCU, slot), here on a wide and a tall grid
        assert list(present[np.argsort(first[t][present], kind="stable")]) == \
            list(present[np.argsort(ofirst[t][present], kind="stable")]), t
        assert len(set(first[t][present].tolist())) == len(present), t  # (no two symbols share a key)
        assert np.all(first[t][ocounts[t] == 0] == none), t


@MODE
@LONG
@pytest.mark.parametrize("lanes", [4, 1])
def test_restart_intervals(enc, enc1, lanes, w, h, mode):
    rgb = L.frame("photo", w, h)
    e = enc if lanes == 4 else enc1
    assert e.lanes() == lanes
    e.set_subsampling(mode)
    for r in L.restarts(w, h, mode):
        e.set_restart(r)
        assert e.encode(rgb, quality=90) == L.want("photo", w, h, 90, mode, r), r


def test_restart_more_than_65535_segments(enc, enc1):
    # 8192 x 9 MCUs at R = 1: 73 728 segments, past what a 16-bit segment count or index holds
    # (the shapes above stay below 2^15 segments)
    w, h = L.MANY_SEGMENTS
    assert np.prod(L.mcus(w, h, 444)) > 65535
    for e in (enc, enc1):
        e.set_subsampling(444)
        e.set_restart(1)
        assert e.encode(L.frame("photo", w, h), quality=90) == L.want("photo", w, h, 90, 444, 1), e.lanes()


def test_restart_65536_is_refused(enc):
    w, h = 65535, 17
    enc.set_restart(65535)
    with pytest.raises(J.JpgeError) as e:
        enc.set_restart(65536)
    assert e.value.status == L.E_ARG
    assert enc.encode(L.frame("photo", w, h), quality=90) == L.want("photo", w, h, 90, 420, 65535)  # (the setting stays)


@MODE
@LONG
def test_decode_round_trip(enc, w, h, mode):
    rgb = L.frame("random", w, h)
    enc.set_subsampling(mode)
    coef = enc.fdct_quant(rgb, quality=90)
    for r in (0, L.restarts(w, h, mode)[-1]):
        enc.set_restart(r)
        info, y, cb, cr = J.decode_coeffs(enc.encode(rgb, quality=90))
        assert (info.width, info.height, info.restart) == (w, h, r)
        assert L.same((y, cb, cr), coef), r


@pytest.mark.parametrize("mode", [420, 411])
@LONG
def test_maxval_100(enc, w, h, mode):
    rgb = L.scaled(L.frame("photo", w, h), 100)
    enc.set_subsampling(mode)
    assert enc.encode(rgb, quality=90, maxval=100) == L.want("photo", w, h, 90, mode, 0, 100)
    assert L.same(enc.fdct_quant(rgb, quality=90, maxval=100), L.want_coeffs("photo", w, h, 90, mode, 100))


# ---- 3. every other K1 build ----
def _encode_dev(e, buf, off, w, h, stride, quality=90):
    dev = torch.from_numpy(buf).cuda()
    assert dev.data_ptr() % 16 == 0
    out = torch.zeros(J.max_jpeg_bytes(w, h), dtype=torch.uint8, device="cuda")
    n = e.encode_ptr(dev.data_ptr() + off, w, h, stride, out.data_ptr(), out.numel(), quality)
    torch.cuda.synchronize()
    return out[:n].cpu().numpy().tobytes()


def _pitch(case, least):
    """(stride, offset, extra plane-stride bytes): every base and pitch a multiple of 32 (of 16
    for the plane stride), or an odd pitch with the base one byte in."""
    if case == "fast":
        return -(-least // 32) * 32 + 32, 32, 48
    return least + 25 + least % 2, 1, 37


@K1
@CASE
@pytest.mark.parametrize("fmt", F.NEW_FORMATS, ids=[F.NAMES[f] for f in F.NEW_FORMATS])
def test_rgb_layouts(enc, fmt, w, h, case):
    a = F.to_format(L.frame("random", w, h), fmt)
    stride, off, extra = _pitch(case, w * J.input_format_info(fmt)[0])
    planar = fmt == J.JPGE_FMT_RGB8_PLANAR
    buf, off, ps = L.padded(a, fmt, stride, plane_stride=stride * h + extra if planar else 0, offset=off)
    enc.set_input_format(fmt, ps)
    assert _encode_dev(enc, buf, off, w, h, stride) == L.want("random", w, h, 90)


def _yuv_samples(w, h):
    """Random (y, cb, cr) planes of full size; [::2, ::2] and [:, ::2] of the chroma are the 4:2:0
    and 4:2:2 layouts' planes."""
    return Y.samples(Y.YUV444, 7 * w + h, w, h)


def _ref_444(ref, planes, mode, quality=90):
    """The YUV444_PLANAR encode on the separate context (pinned by test_yuv444_planar below)."""
    ref.set_input_format(Y.YUV444)
    ref.set_subsampling(mode)
    try:
        return ref.encode(Y.build(Y.YUV444, *planes), quality=quality)
    finally:
        ref.set_input_format(J.JPGE_FMT_RGB8)
        ref.set_subsampling(420)


@K1
def test_encode_planes_rgb(ref, w, h):
    # the fp64 plane kernels at this shape: what test_yuv444_planar's expectation rests on
    rgb = L.frame("random", w, h)
    assert ref.encode_planes(*L.rgb_planes(rgb), w, h, J.JPGE_TO_RGB, 90) == L.want("random", w, h, 90)


@functools.lru_cache(maxsize=None)
def _yuv_coeffs(w, h, mode):
    return Y.want_coeffs(Y.pad_planes(Y.YUV444, *_yuv_samples(w, h), mcu=Y.mcu_size(mode)), mode, 90)


@K1
@CASE
@pytest.mark.parametrize("mode", [420, 422, 444])
def test_yuv444_planar(enc, ref, w, h, case, mode):
    # 420: the file equals encode_planes' (writeJPEG on planes is S420_m); 422 and 444, the modes
    # the 4:2:2 layouts' and the gray expectations use: the file holds the oracle primitives'
    # coefficients
    p = _yuv_samples(w, h)
    stride, off, extra = _pitch(case, w)
    buf, stride, ps = L.yuv_raw(Y.YUV444, *p, stride, stride * h + extra, off)
    enc.set_input_format(Y.YUV444, ps)
    enc.set_subsampling(mode)
    got = _encode_dev(enc, buf, off, w, h, stride)
    if mode == 420:
        assert got == ref.encode_planes(*Y.pad_planes(Y.YUV444, *p), w, h, J.JPGE_TO_YCBCR, 90)
    else:
        info, y, cb, cr = J.decode_coeffs(got)
        assert (info.width, info.height) == (w, h) and (info.yh, info.yv) == _oracle.SHAPES[mode]
        assert L.same((y, cb, cr), _yuv_coeffs(w, h, mode))
        assert got == _ref_444(ref, p, mode)  # (the contiguous host frame on the other context)


@K1
@CASE
@pytest.mark.parametrize("fmt", Y.HALF, ids=[Y.NAMES[f] for f in Y.HALF])
def test_yuv420_layouts(enc, ref, fmt, w, h, case):
    y, cb, cr = _yuv_samples(w, h)
    cb, cr = cb[::2, ::2].copy(), cr[::2, ::2].copy()
    want = _ref_444(ref, (y, Y.upsample(cb, w, h), Y.upsample(cr, w, h)), 420)
    stride, off, extra = _pitch(case, 2 * ((w + 1) // 2) if fmt == Y.NV12 else w)
    buf, stride, ps = L.yuv_raw(fmt, y, cb, cr, stride, stride * h + extra, off)
    enc.set_input_format(fmt, ps)
    assert _encode_dev(enc, buf, off, w, h, stride) == want


@K1
@CASE
@pytest.mark.parametrize("fmt", Z.FORMATS, ids=[Z.NAMES[f] for f in Z.FORMATS])
def test_yuv422_layouts(enc, ref, fmt, w, h, case):
    y, cb, cr = _yuv_samples(w, h)
    cb, cr = cb[:, ::2].copy(), cr[:, ::2].copy()
    want = _ref_444(ref, Z.repeated(y, cb, cr), 422)
    stride, off, extra = _pitch(case, Z.least_stride(fmt, w))
    buf, stride, ps = L.yuv422_raw(fmt, y, cb, cr, stride, 0 if fmt in Z.PACKED else stride * h + extra, off)
    enc.set_input_format(fmt, ps)
    enc.set_subsampling(422)
    assert _encode_dev(enc, buf, off, w, h, stride) == want


@K1
@CASE
def test_gray(enc, ref, w, h, case):
    p = _yuv_samples(w, h)[0]
    c = np.full_like(p, 128)
    info3, y3, cb3, cr3 = J.decode_coeffs(_ref_444(ref, (p, c, c), 444))
    stride, off, _ = _pitch(case, w)
    buf, off, _ = L.padded(p[:, :, None], GRAY, stride, offset=off)
    enc.set_input_format(GRAY)
    info, y, cb, cr = J.decode_coeffs(_encode_dev(enc, buf, off, w, h, stride))
    assert cb is None and cr is None and info.c_blocks == 0 and (info.width, info.height) == (w, h)
    assert np.array_equal(y, y3) and not cb3.any() and not cr3.any() and bytes(info.qy) == bytes(info3.qy)
    assert np.array_equal(enc.fdct_quant(p, quality=90)[0], y3)


@K1
def test_nv12_limited_709(enc, ref, w, h):
    y, cb, cr = _yuv_samples(w, h)
    cb, cr = cb[::2, ::2].copy(), cr[::2, ::2].copy()
    preset, given, t = X.coeffs("limited709")
    want = ref.encode_planes(*X.planes(Y.NV12, y, cb, cr, t), w, h, J.JPGE_TO_YCBCR, 90)
    enc.set_input_format(Y.NV12)
    enc.set_yuv_transform(preset, given)
    assert enc.encode(Y.build(Y.NV12, y, cb, cr), quality=90) == want


# (_fixedhuff's coder loops per block in Python: one row and one column of blocks only)
@pytest.mark.parametrize("w,h", [(65535, 1), (1, 65535)], ids=["65535x1", "1x65535"])
def test_standard_huffman_nv12_and_gray(enc, w, h):
    std = [J.standard_huffman(t) for t in range(4)]
    qy, qc = _oracle.quality_tables(90)
    y, cb, cr = Y.samples(Y.NV12, 11, w, h)
    enc.set_huffman(J.JPGE_HUFF_STANDARD)
    enc.set_input_format(Y.NV12)
    coef = Y.want_coeffs(Y.pad_planes(Y.NV12, y, cb, cr), 420, 90)
    assert enc.encode(Y.build(Y.NV12, y, cb, cr), quality=90) == FH.expected_coeffs(*coef, w, h, qy, qc, std)
    enc.set_input_format(GRAY)
    assert enc.encode(y, quality=90) == FH.expected_gray(y, qy, std)


# ---- 4. large pitches and the 32-bit extent bound (device input) ----
def _alloc(nbytes):
    try:
        return torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    except getattr(torch, "OutOfMemoryError", torch.cuda.OutOfMemoryError):
        pytest.skip(f"no {nbytes / 1e9:.1f} GB of device memory for this frame's extent")


def _place(dev, off, plane, stride):
    """Write an (h, n) byte plane into the device allocation at rows of pitch stride; nothing
    else of the allocation is touched."""
    h, n = plane.shape
    assert off + (h - 1) * stride + n <= dev.numel()
    dev.as_strided((h, n), (stride, 1), off).copy_(torch.from_numpy(np.array(plane)).cuda())


def _batch_dev(e, ptr, w, h, stride, quality=90):
    """One frame through encode_batch_dev -> (status of the call, the frame's status, its bytes, the
    whole zero-filled output buffer)."""
    out = torch.zeros(J.max_jpeg_bytes(w, h), dtype=torch.uint8, device="cuda")
    try:
        n = e.encode_batch_dev([(ptr, w, h, stride)], [(out.data_ptr(), out.numel())], quality=quality)[0]
        st = 0
    except J.JpgeError as err:
        n, st = 0, err.status
    torch.cuda.synchronize()
    return st, e.batch_status()[0], out[:n].cpu().numpy().tobytes(), out


@pytest.mark.parametrize("w,h", [(48, 40), (33, 17)], ids=["48x40", "33x17"])
@pytest.mark.parametrize("pitch,off", [(BIG_PITCH + 16, 0), (BIG_PITCH + 3, 1)], ids=["fast", "clamped"])
def test_large_pitch_rgb8(enc, w, h, pitch, off):
    rgb = L.frame("random", w, h)
    dev = _alloc(off + pitch * h)
    _place(dev, off, rgb.reshape(h, 3 * w), pitch)
    st, fst, got, _ = _batch_dev(enc, dev.data_ptr() + off, w, h, pitch)
    assert (st, fst) == (0, 0) and got == enc.encode(rgb, quality=90) == L.want("random", w, h, 90)


def test_large_pitch_other_layouts(enc):
    w, h, pitch = 33, 17, BIG_PITCH + 16
    rgb = L.frame("random", w, h)
    # planar RGB with a plane stride of its own
    ps = pitch * h + 48
    dev = _alloc(3 * ps)
    for c in range(3):
        _place(dev, c * ps, rgb[:, :, c], pitch)
    enc.set_input_format(J.JPGE_FMT_RGB8_PLANAR, ps)
    assert _batch_dev(enc, dev.data_ptr(), w, h, pitch)[:3] == (0, 0, L.want("random", w, h, 90))
    # one 4-byte layout
    _place(dev, 0, F.to_format(rgb, J.JPGE_FMT_BGRA8).reshape(h, 4 * w), pitch)
    enc.set_input_format(J.JPGE_FMT_BGRA8)
    assert _batch_dev(enc, dev.data_ptr(), w, h, pitch)[:3] == (0, 0, L.want("random", w, h, 90))
    # NV12 with its chroma descriptor
    y, cb, cr = Y.samples(Y.NV12, 3, w, h)
    enc.set_input_format(Y.NV12)
    want = enc.encode(Y.build(Y.NV12, y, cb, cr), quality=90)
    _place(dev, 0, y, pitch)
    _place(dev, ps, np.stack([cb, cr], axis=2).reshape(cb.shape[0], -1), pitch)
    enc.set_input_format(Y.NV12, ps)
    assert _batch_dev(enc, dev.data_ptr(), w, h, pitch)[:3] == (0, 0, want)


def test_extent_just_under_and_at_the_bound(enc):
    """stride * height of a frame read in place stays below the transform kernel's 32-bit offset
    bound, 0xFFFFFF00 (fdct.hip kOob; kernels.hpp kK1OffsetBound, k1_offsets_fit): the largest
    16-byte-aligned pitch below it encodes exactly, the next one is refused with the argument
    error on the host, before the slot grows or anything is queued (Encoder::prep1; slot sizes
    come from the geometry alone for a device frame).  The allocation has the full extent of
    the larger pitch, so no address outside it is formed whatever the check does."""
    w, h = 48, 40
    under = (L.K_OOB - 1) // h // 16 * 16
    at = under + 16
    assert under * h < L.K_OOB <= at * h
    rgb = L.frame("random", w, h)
    want = L.want("random", w, h, 90)
    dev = _alloc(at * h)  # (4.29 GB; only the frame's rows are written)
    _place(dev, 0, rgb.reshape(h, 3 * w), under)
    st, fst, got, _ = _batch_dev(enc, dev.data_ptr(), w, h, under)
    assert (st, fst) == (0, 0) and got == want
    _place(dev, 0, rgb.reshape(h, 3 * w), at)
    st, fst, got, out = _batch_dev(enc, dev.data_ptr(), w, h, at)
    assert (st, fst) == (L.E_ARG, L.E_ARG) and got == b""
    assert not bool(out.any())  # no output written
    assert enc.encode(rgb, quality=90) == want
    _place(dev, 0, rgb.reshape(h, 3 * w), under)  # (the rows at the larger pitch overlap these)
    assert _batch_dev(enc, dev.data_ptr(), w, h, under)[:3] == (0, 0, want)


def test_stripe_extent_at_the_bound(enc1):
    """stripe_transform refuses a stripe whose pitch * rows reaches the bound, on the host
    (k1_offsets_fit on the stripe's own geometry), and takes the largest pitch below it: the last
    MCU's DCs equal those of the contiguous stripe.  The allocation has the larger pitch's extent."""
    w, h = 48, 40
    under = (L.K_OOB - 1) // h // 16 * 16
    at = under + 16
    rgb = L.frame("random", w, h)
    dev = _alloc(at * h)
    small = torch.from_numpy(np.array(rgb)).cuda()
    want = enc1.stripe_transform(small.data_ptr(), 3 * w, w, h, 0, 3, 90)
    _place(dev, 0, rgb.reshape(h, 3 * w), at)
    with pytest.raises(J.JpgeError) as e:
        enc1.stripe_transform(dev.data_ptr(), at, w, h, 0, 3, 90)
    assert e.value.status == L.E_ARG
    _place(dev, 0, rgb.reshape(h, 3 * w), under)
    assert np.array_equal(enc1.stripe_transform(dev.data_ptr(), under, w, h, 0, 3, 90), want)
    # one MCU row of the frame at the refused pitch fits (16 rows): the stripe's geometry decides
    _place(dev, 0, rgb.reshape(h, 3 * w), at)
    first = enc1.stripe_transform(dev.data_ptr(), at, w, h, 0, 1, 90)
    assert np.array_equal(first, enc1.stripe_transform(small.data_ptr(), 3 * w, w, h, 0, 1, 90))
    assert enc1.encode(rgb, quality=90) == L.want("random", w, h, 90)


# ---- 5. the other entries ----
def _batch(i):
    kind = "photo" if i % 2 else "random"
    return kind, L.frame(kind, 65535, 17)


MIXED = [("photo", 65535, 17), ("photo", 17, 65535), ("photo", 64, 48), ("random", 65535, 17), ("random", 17, 65535)]


@pytest.mark.parametrize("set_size", [1, 2, 3, 4])
def test_batches_forced_set_sizes(set_size):
    e = _encoder(JPGE_LANES=4, JPGE_SET=set_size)
    try:
        assert e.lanes() == 4
        outs = e.encode_batch([_batch(i)[1] for i in range(5)], quality=90)
        assert outs == [L.want(_batch(i)[0], 65535, 17, 90) for i in range(5)]
        outs = e.encode_batch([L.frame(*m) for m in MIXED], quality=90)
        assert outs == [L.want(*m, 90) for m in MIXED]
    finally:
        e.close()


def test_group_batches():
    with J.Group([0, 0]) as g:
        outs = g.encode_batch([_batch(i)[1] for i in range(5)], quality=90)
        assert outs == [L.want(_batch(i)[0], 65535, 17, 90) for i in range(5)]
        outs = g.encode_batch([L.frame(*m) for m in MIXED], quality=90)
        assert outs == [L.want(*m, 90) for m in MIXED]


@pytest.mark.parametrize("w,h,n", [(65535, 64, 4), (17, 4096, 8)], ids=["65535x64/4", "17x4096/8"])
@pytest.mark.parametrize("aligned_restart", [False, True])
def test_stripes(w, h, n, aligned_restart):
    from test_gpu_stripes import _encode_striped
    r = L.mcus(w, h, 420)[0] if aligned_restart else 0  # one MCU row: every stripe starts an interval
    assert _encode_striped(L.frame("photo", w, h), n, 90, restart=r) == L.want("photo", w, h, 90, 420, r)


def test_encode_file(enc, tmp_path):
    w, h = 65535, 17
    src, dst = str(tmp_path / "in.ppm"), str(tmp_path / "out.jpg")
    with open(src, "wb") as f:
        f.write(f"P6\n{w} {h}\n255\n".encode() + L.frame("photo", w, h).tobytes())
    enc.encode_file(src, dst, quality=90)
    with open(dst, "rb") as f:
        assert f.read() == L.want("photo", w, h, 90)


@pytest.mark.parametrize("w,h,short", [(65536, 1, 0), (1, 65536, 0), (65535, 17, 1)], ids=["w65536", "h65536", "pitch"])
def test_refusals_at_the_limit(enc, w, h, short):
    # (the whole frame the arguments describe is there: the refusal is not needed for safety)
    buf = np.zeros((h, w, 3), np.uint8)
    out = np.zeros(1 << 20, np.uint8)
    with pytest.raises(J.JpgeError) as e:
        enc.encode_ptr(buf.ctypes.data, w, h, 3 * w - short, out.ctypes.data, out.size, 90, flags=0)
    assert e.value.status == L.E_ARG and not out.any()
    if not short:
        with pytest.raises(ValueError):
            enc.encode(buf, quality=90)
    assert enc.encode(L.frame("photo", 65535, 17), quality=90) == L.want("photo", 65535, 17, 90)
