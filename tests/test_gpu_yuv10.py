"""The 10-bit 4:2:0 layouts (JPGE_FMT_P010, _I010) on the GPU: K1's P010 and I010 builds, which
stage 10-bit fields and always run the sample transform.  Expectations (_yuv10.py, checked by
test_yuv10_cpu.py): every sample s the exact value s / 4, the three lines of jpge.h in numpy
with the coefficients the library returned (the identity for FULL_601), then the oracle's
primitives for the coefficients (_yuv.want_coeffs) and Encoder.encode_planes on a separate
context for whole files; for samples 4 b, the NV12 / I420 encode of the bytes b.  Every
comparison is exact."""
import functools
import os

import numpy as np
import pytest

import _oracle
import _yuv as Y
import _yuv10 as T
import _yuvxf as X
import jpgenc_amd as J

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FMT = pytest.mark.parametrize("fmt", T.FORMATS, ids=[T.NAMES[f] for f in T.FORMATS])
# the set that reaches every branch of a tile in test_gpu_yuv.py
SIZES = [(1, 1), (16, 16), (64, 16), (80, 32), (33, 17), (130, 50)]
KINDS = ["random", "zeros", "ones"]
SETTINGS = ["full601", "limited601", "limited709", "custom"]
E_ARG = 1


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


def _set(e, fmt, xf, plane_stride=0):
    """The layout and the transform on a context; returns the coefficients in force."""
    e.set_input_format(fmt, plane_stride)
    if xf == "full601":
        e.set_yuv_transform(J.JPGE_YUV_FULL_601)
        t = X.IDENTITY
    else:
        preset, given, t = X.coeffs(xf)
        e.set_yuv_transform(preset, given)
    assert e.yuv_transform()[1] == tuple(t)
    return tuple(t)


@functools.lru_cache(maxsize=None)
def _p(w, h, kind="random", seed=None):
    return T.samples(1000 * w + h if seed is None else seed, w, h, kind)


@functools.lru_cache(maxsize=None)
def _planes(w, h, kind, seed, t):
    return T.planes(*_p(w, h, kind, seed), t)


@functools.lru_cache(maxsize=None)
def _want(w, h, kind, t, quality=90, seed=None):
    return Y.want_coeffs(_planes(w, h, kind, seed, t), 420, quality)


def _want_jpg(ref, w, h, kind, t, quality=90, restart=0, seed=None):
    ref.set_restart(restart)
    return ref.encode_planes(*_planes(w, h, kind, seed, tuple(t)), w, h, J.JPGE_TO_YCBCR, quality)


def _same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


def _encode_dev(e, buf, off, w, h, stride, quality=90):
    dev = torch.from_numpy(buf).cuda()
    assert dev.data_ptr() % 16 == 0
    out = torch.zeros(J.max_jpeg_bytes(w, h), dtype=torch.uint8, device="cuda")
    n = e.encode_ptr(dev.data_ptr() + off, w, h, stride, out.data_ptr(), out.numel(), quality)
    torch.cuda.synchronize()
    return out[:n].cpu().numpy().tobytes()


def _encode_host(e, buf, off, w, h, stride, quality=90):
    out = np.empty(J.max_jpeg_bytes(w, h), np.uint8)
    n = e.encode_ptr(buf.ctypes.data + off, w, h, stride, out.ctypes.data, out.size, quality, 255, 0)
    return out[:n].tobytes()


# ---- 1. coefficients ----
@FMT
@pytest.mark.parametrize("xf", SETTINGS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w,h", SIZES)
def test_coefficients(enc, fmt, xf, w, h, kind):
    t = _set(enc, fmt, xf)
    got = enc.fdct_quant(T.build(fmt, *_p(w, h, kind)), quality=90)
    assert _same(got, _want(w, h, kind, t))


# ---- 2. whole files ----
@FMT
@pytest.mark.parametrize("quality", [50, 90, 100])
@pytest.mark.parametrize("w,h", SIZES)
def test_whole_file(enc, ref, fmt, w, h, quality):
    xf = {50: "full601", 90: "limited709", 100: "custom"}[quality]
    t = _set(enc, fmt, xf)
    assert enc.encode(T.build(fmt, *_p(w, h)), quality=quality) == _want_jpg(ref, w, h, "random", t, quality)


@FMT
@pytest.mark.parametrize("xf", ["full601", "limited709"])
def test_whole_file_restart(enc, ref, fmt, xf):
    w, h = 130, 50
    t = _set(enc, fmt, xf)
    enc.set_restart(3)
    got = enc.encode(T.build(fmt, *_p(w, h)), quality=90)
    assert got == _want_jpg(ref, w, h, "random", t, 90, restart=3)
    assert got.count(b"\xff\xdd") >= 1  # DRI


# ---- 3. samples 4 b are the 8-bit frame of b ----
@functools.lru_cache(maxsize=None)
def _bytes(w, h):
    return Y.samples(Y.I420, 7000 + w + h, w, h)


@FMT
@pytest.mark.parametrize("xf", ["full601", "limited709"])
@pytest.mark.parametrize("huff", ["optimal", "standard"])
@pytest.mark.parametrize("w,h", [(33, 17), (130, 50)])
def test_multiples_of_four_equal_8bit(enc, fmt, xf, huff, w, h):
    # (FULL_601: the new instance against the 8-bit build's kExact one)
    b = _bytes(w, h)
    enc.set_huffman(J.JPGE_HUFF_STANDARD if huff == "standard" else J.JPGE_HUFF_OPTIMAL)
    enc.set_restart(5 if huff == "standard" else 0)
    _set(enc, T.EIGHT[fmt], xf)
    want = enc.encode(Y.build(T.EIGHT[fmt], *b), quality=90)
    want_c = enc.fdct_quant(Y.build(T.EIGHT[fmt], *b), quality=90)
    _set(enc, fmt, xf)
    f = T.build(fmt, *(4 * p.astype(np.uint16) for p in b))
    assert enc.encode(f, quality=90) == want
    assert _same(enc.fdct_quant(f, quality=90), want_c)


_WANT8 = {}


@FMT
@pytest.mark.parametrize("xf", ["full601", "limited709"])
@pytest.mark.parametrize("case", ["aligned", "clamped"])
@pytest.mark.parametrize("w,h", [(65535, 17), (17, 65535)], ids=["65535x17", "17x65535"])
def test_limit_frames_equal_8bit(enc1, fmt, xf, case, w, h):
    b = _bytes(w, h)
    key = (T.EIGHT[fmt], xf, w, h)
    if key not in _WANT8:  # the 8-bit frame's file, once for both cases
        s8, o8 = -(-w // 32) * 32, 32
        _set(enc1, T.EIGHT[fmt], xf, s8 * h + 64)
        _WANT8[key] = _encode_dev(enc1, Y.raw(T.EIGHT[fmt], *b, stride=s8, plane_stride=s8 * h + 64, offset=o8)[0], o8, w, h, s8)
    want = _WANT8[key]
    if case == "aligned":
        stride, off = -(-T.least_stride(fmt, w) // 32) * 32, 32
        ps = stride * h + 64
    else:
        stride, off = T.least_stride(fmt, w) + 6, 2
        ps = stride * h + 10
    _set(enc1, fmt, xf, ps)
    p = [4 * q.astype(np.uint16) for q in b]
    assert _encode_dev(enc1, T.raw(fmt, *p, stride=stride, plane_stride=ps, offset=off)[0], off, w, h, stride) == want


# ---- 4. the bits the layouts never read ----
@FMT
@pytest.mark.parametrize("case", ["aligned", "clamped"])
def test_ignored_bits(enc, ref, fmt, case):
    w, h = 130, 50
    t = _set(enc, fmt, "limited709")
    want = _want_jpg(ref, w, h, "random", t)
    stride, off = (T.least_stride(fmt, w) + 28, 0) if case == "aligned" else (T.least_stride(fmt, w) + 6, 2)
    if case == "aligned":
        stride = -(-stride // 32) * 32
    outs = [_encode_dev(enc, T.raw(fmt, *_p(w, h), stride=stride, offset=off, junk_seed=js)[0], off, w, h, stride)
            for js in (None, 21, 22)]
    assert outs[0] == outs[1] == outs[2] == want


# ---- 5. the case the clamps protect ----
@FMT
def test_all_ones_words_fixed_tables(enc, fmt):
    # 0xFFFF (P010) and 0x03FF (I010) are the sample 1023 = 255.75: unclamped, the coefficients of
    # such data could pass what a fixed table has a code for
    w, h = 130, 50
    ch, cw = T.chroma_shape(w, h)
    enc.set_huffman(J.JPGE_HUFF_STANDARD)
    _set(enc, Y.NV12, "full601")
    want = enc.encode(Y.build(Y.NV12, *Y.samples(Y.NV12, 0, w, h, "ones")), quality=100)
    _set(enc, fmt, "full601")
    word = 0xFFFF if fmt == T.P010 else 0x03FF
    n = J.yuv420p10_bytes(fmt, w, h) // 2
    f = np.full(n, word, "<u2").view(np.uint8).view(J.Yuv420Frame)
    f.fmt, f.width, f.height, f.stride = fmt, w, h, T.least_stride(fmt, w)
    assert enc.encode(f, quality=100) == want


# ---- 6. addressing ----
@FMT
@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("w,h", [(80, 32), (33, 17), (130, 51)])
@pytest.mark.parametrize("case", ["clamped", "aligned"])
def test_addressing(enc, ref, fmt, where, w, h, case):
    p = _p(w, h)
    if case == "clamped":  # base 2 bytes in, a stride that is no multiple of 16, a plane stride of its own
        stride, off = T.least_stride(fmt, w) + 6, 2
        ps = stride * h + 10
    else:  # every base and pitch 16-byte aligned (I010: the stride a multiple of 32): the fast path
        stride, off = -(-(T.least_stride(fmt, w) + 20) // 32) * 32, 32
        ps = stride * h + 48
    t = _set(enc, fmt, "limited709", ps)
    want = _want_jpg(ref, w, h, "random", t)
    run = _encode_dev if where == "device" else _encode_host
    outs = [run(enc, T.raw(fmt, *p, stride=stride, plane_stride=ps, offset=off, seed=s)[0], off, w, h, stride)
            for s in (9, 10)]  # other bytes around the frame
    assert outs[0] == outs[1] == want


@FMT
def test_host_frame_least_stride(enc1, ref, fmt):
    # host frames go through the upload's repitch (odd sizes: every plane by a 2-D copy)
    w, h = 33, 17
    t = _set(enc1, fmt, "custom")
    assert enc1.encode(T.build(fmt, *_p(w, h)), quality=90) == _want_jpg(ref, w, h, "random", t)


# ---- 7. the pipeline and the other entries ----
BATCH = [(160, 96) if i % 2 == 0 else (48 + 16 * i, 40 + i) for i in range(9)]  # 5 of one size: sets form


@FMT
@pytest.mark.parametrize("lanes", [4, 1])
def test_batch(enc, enc1, ref, fmt, lanes):
    e = enc if lanes == 4 else enc1
    assert e.lanes() == lanes
    t = _set(e, fmt, "limited709")
    outs = e.encode_batch([T.build(fmt, *_p(w, h, seed=100 + i)) for i, (w, h) in enumerate(BATCH)], quality=90)
    for i, (w, h) in enumerate(BATCH):
        assert outs[i] == _want_jpg(ref, w, h, "random", t, seed=100 + i), i


def _encoder(**env):
    # (a context reads its switches when it opens: a fresh one under the setting)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return J.Encoder(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.mark.parametrize("set_size", [1, 3, 4])
def test_forced_set_sizes_short_last_set(ref, set_size):
    w, h = 136, 72
    e = _encoder(JPGE_LANES=4, JPGE_SET=set_size)
    try:
        for fmt in T.FORMATS:
            t = _set(e, fmt, "full601")
            outs = e.encode_batch([T.build(fmt, *_p(w, h, seed=200 + i)) for i in range(9)], quality=75)
            assert outs == [_want_jpg(ref, w, h, "random", t, 75, seed=200 + i) for i in range(9)], fmt
    finally:
        e.close()


def test_layout_change_between_batches(enc, ref):
    w, h = 136, 72
    p = [_p(w, h, seed=200 + i) for i in range(5)]
    for fmt in (T.P010, T.I010, T.P010):
        t = _set(enc, fmt, "limited601")
        assert enc.encode_batch([T.build(fmt, *q) for q in p], quality=75) == [
            _want_jpg(ref, w, h, "random", t, 75, seed=200 + i) for i in range(5)], fmt
    # and to an 8-bit layout and back to RGB8
    b = _bytes(w, h)
    _set(enc, Y.NV12, "full601")
    assert enc.encode_batch([Y.build(Y.NV12, *b)] * 2, quality=75) == [
        ref.encode_planes(*Y.pad_planes(Y.NV12, *b), w, h, J.JPGE_TO_YCBCR, 75)] * 2
    enc.set_input_format(J.JPGE_FMT_RGB8)
    rgb = J.synth_rgb8(4, 80, 32, kind=1)
    assert enc.encode_batch([rgb, rgb], quality=90) == [_oracle.encode(rgb, 90)] * 2


@FMT
def test_group_batch(ref, fmt):
    preset, given, t = X.coeffs("limited709")
    with J.Group([0, 0]) as g:
        g.set_input_format(fmt)
        g.set_yuv_transform(preset, given)
        outs = g.encode_batch([T.build(fmt, *_p(w, h, seed=100 + i)) for i, (w, h) in enumerate(BATCH[:5])], quality=90)
    for i, (w, h) in enumerate(BATCH[:5]):
        assert outs[i] == _want_jpg(ref, w, h, "random", tuple(t), seed=100 + i), i


@FMT
def test_symbol_stats(enc1, fmt):
    # the symbol statistics of samples 4 b are those of the 8-bit frame of b
    w, h = 130, 50
    b = _bytes(w, h)
    _set(enc1, T.EIGHT[fmt], "limited709")
    c2, f2 = enc1.symbol_stats(Y.build(T.EIGHT[fmt], *b), quality=90)
    _set(enc1, fmt, "limited709")
    counts, first = enc1.symbol_stats(T.build(fmt, *(4 * q.astype(np.uint16) for q in b)), quality=90)
    assert counts.sum() > 0 and np.array_equal(counts, c2) and np.array_equal(first, f2)


@FMT
def test_tensor_entry(enc1, ref, fmt):
    w, h = 130, 51
    ch, cw = T.chroma_shape(w, h)
    y, cb, cr = _p(w, h)
    t = _set(enc1, J.JPGE_FMT_BGR8, "limited709")
    want = _want_jpg(ref, w, h, "random", t)
    to = lambda a: torch.from_numpy(T.words(fmt, a).astype(np.int16)).cuda()  # (16-bit words, whatever the sign)
    pitch = 144  # words: 288 bytes, a multiple of 32
    surf = torch.randint(-32768, 32767, (h + 2 * ch + 3, pitch), dtype=torch.int16, device="cuda")
    ty = surf[:h, :w]
    ty.copy_(to(y))
    if fmt == T.P010:
        tc = surf[h:h + ch, :2 * cw]
        tc.copy_(to(np.stack([cb, cr], axis=2).reshape(ch, 2 * cw)))
        assert enc1.encode_tensor_yuv10(ty, tc, quality=90) == want
    else:
        half = surf[h:h + ch].reshape(-1)[:2 * ch * (pitch // 2)].view(2 * ch, pitch // 2)  # rows of pitch / 2 words
        tb, tr = half[:ch, :cw], half[ch:2 * ch, :cw]
        tb.copy_(to(cb))
        tr.copy_(to(cr))
        assert enc1.encode_tensor_yuv10(ty, tb, tr, quality=90) == want
        out = torch.zeros(J.max_jpeg_bytes(w, h), dtype=torch.uint8, device="cuda")
        n = enc1.encode_tensor_yuv10(ty, tb, tr, quality=90, out=out)
        assert out[:n].cpu().numpy().tobytes() == want
    assert enc1.input_format() == (J.JPGE_FMT_BGR8, 0)  # as before
    with pytest.raises(ValueError):
        enc1.encode_tensor_yuv10(ty.view(torch.uint8), ty.view(torch.uint8))


# ---- 8. refusals: each raises and leaves the context encoding as it was ----
@FMT
def test_refusals(enc, ref, fmt):
    w, h = 80, 32
    t = _set(enc, fmt, "limited601")
    f = T.build(fmt, *_p(w, h))
    want = _want_jpg(ref, w, h, "random", t)
    assert enc.encode(f, quality=90) == want
    for mode in (444, 422, 411, 4200, 4201):
        enc.set_subsampling(mode)
        with pytest.raises(J.JpgeError) as ei:
            enc.encode(f, quality=90)
        assert ei.value.status == E_ARG, mode
        enc.set_subsampling(420)
        assert enc.encode(f, quality=90) == want
    with pytest.raises(J.JpgeError) as ei:
        enc.encode(f, quality=90, maxval=100)
    assert ei.value.status == E_ARG
    with pytest.raises(J.JpgeError):
        enc.encode_batch([f, f], quality=90, maxval=100)
    assert enc.encode(f, quality=90) == want
    # odd stride, odd plane stride, odd base, a stride below the least
    least = T.least_stride(fmt, w)
    buf, _, _ = T.raw(fmt, *_p(w, h), stride=least + 16, plane_stride=(least + 16) * h + 16, offset=16)
    dev = torch.from_numpy(buf).cuda()
    out = torch.zeros(J.max_jpeg_bytes(w, h), dtype=torch.uint8, device="cuda")
    good = (dev.data_ptr() + 16, least + 16, (least + 16) * h + 16)
    for ptr, stride, ps in [(good[0], least + 17, good[2]), (good[0], good[1], good[2] + 1), (good[0] + 1, good[1], good[2]),
                            (good[0], least - 2, good[2])]:
        enc.set_input_format(fmt, ps)
        with pytest.raises(J.JpgeError) as ei:
            enc.encode_ptr(ptr, w, h, stride, out.data_ptr(), out.numel(), 90)
        assert ei.value.status == E_ARG, (ptr - good[0], stride, ps)
        enc.set_input_format(fmt, good[2])
        n = enc.encode_ptr(good[0], w, h, good[1], out.data_ptr(), out.numel(), 90)
        torch.cuda.synchronize()
        assert out[:n].cpu().numpy().tobytes() == want


@FMT
def test_refuses_stripes(enc1, ref, fmt):
    t = _set(enc1, fmt, "full601")
    dev = torch.zeros(3 * 256 * 128, dtype=torch.uint8, device="cuda")
    with pytest.raises(J.JpgeError) as ei:
        enc1.stripe_transform(dev.data_ptr(), 512, 256, 128, 0, 2, 90)
    assert ei.value.status == E_ARG
    w, h = 33, 17
    assert enc1.encode(T.build(fmt, *_p(w, h)), quality=90) == _want_jpg(ref, w, h, "random", t)


@FMT
def test_group_refuses_striped(fmt):
    rgb = J.synth_rgb8(2, 640, 480)
    with J.Group([0, 0]) as g:
        g.set_input_format(fmt)
        with pytest.raises(J.JpgeError):
            g.encode_striped(rgb, quality=90)
        g.set_input_format(J.JPGE_FMT_RGB8)
        assert g.encode_striped(rgb, quality=90) == _oracle.encode(rgb, 90)
