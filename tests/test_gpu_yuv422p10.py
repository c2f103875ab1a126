"""The 10-bit 4:2:2 layouts (JPGE_FMT_Y210, _P210, _I210) on the GPU: K1's three builds that
stage ten-bit words with one chroma pair per two pixels and always run the sample transform, in
all six subsampling modes.  Expectations (_yuv422p10.py, checked by test_yuv422p10_cpu.py):
every sample s the exact value s / 4, a cell's chroma in both of its pixels, the three lines of
jpge.h in numpy with the coefficients the library returned (the identity for FULL_601), then the
oracle's primitives for the coefficients (_yuv.want_coeffs) and the CPU-built stream
(_stream3.build3) for whole files: no GPU code runs in an expectation.  Where the header states
an equality of two encodes (the three layouts of the same samples; samples 4 b and the 8-bit
frame of b), the two encodes are compared.  Every comparison is exact."""
import functools
import os

import numpy as np
import pytest

import _fixedhuff as F
import _oracle
import _stream3 as S
import _yuv as Y
import _yuv10 as T10
import _yuv422 as Z
import _yuv422p10 as T
import _yuvxf as X
import jpgenc_amd as J

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FMT = pytest.mark.parametrize("fmt", T.FORMATS, ids=[T.NAMES[f] for f in T.FORMATS])
# fdct_kernel's modes (a 64x16 tile): one pixel, one MCU, one full tile, full + partial tile on
# two MCU rows, odd, several tiles
SIZES_420 = [(1, 1), (16, 16), (64, 16), (80, 32), (33, 17), (130, 50)]
# the row-8 kernel's modes (a 128x8 tile): less than one block each way, a ragged last tile
SIZES_ROW8 = [(9, 9), (136, 24), (141, 27)]
MODES_420, MODES_ROW8 = [420, 4200, 4201], [444, 422, 411]
MODE_SIZES = [(m, w, h) for m in MODES_420 for w, h in SIZES_420] + [(m, w, h) for m in MODES_ROW8 for w, h in SIZES_ROW8]
KINDS = ["random", "zeros", "ones"]
SETTINGS = ["full601", "limited709", "custom"]
E_ARG = 1


def _ids(cases):
    return ["-".join(str(x) for x in c) for c in cases]


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
def enc8():
    """The second context: the 8-bit frames of item 3."""
    e = J.Encoder(0, lanes=1)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def _defaults(enc, enc1, enc8):
    yield
    for e in (enc, enc1, enc8):
        e.set_downscale(1)
        e.set_input_format(J.JPGE_FMT_RGB8)
        e.set_subsampling(420)
        e.set_restart(0)
        e.set_huffman(J.JPGE_HUFF_OPTIMAL)
        e.set_yuv_transform(J.JPGE_YUV_FULL_601)


def _set(e, fmt, xf, plane_stride=0, mode=None):
    """The layout, the transform (and the mode) on a context; returns the coefficients in force."""
    e.set_input_format(fmt, plane_stride)
    if mode is not None:
        e.set_subsampling(mode)
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
def _planes(w, h, kind, seed, t, mode):
    return T.planes(*_p(w, h, kind, seed), t, Y.mcu_size(mode))


@functools.lru_cache(maxsize=None)
def _want(w, h, kind, t, mode, quality=90, seed=None):
    return Y.want_coeffs(_planes(w, h, kind, seed, t, mode), mode, quality)


@functools.lru_cache(maxsize=None)
def _jpg(w, h, t, mode, quality=90, restart=0, huff="optimal", kind="random", seed=None):
    """The CPU-built file (_stream3.build3) of the samples _p(w, h, kind, seed)."""
    qy, qc = _oracle.quality_tables(quality)
    specs = F.golden_specs() if huff == "standard" else None
    return S.build3(_planes(w, h, kind, seed, tuple(t), mode), w, h, qy, qc, mode, restart, specs).jpg


def _huff(e, huff):
    e.set_huffman(J.JPGE_HUFF_STANDARD if huff == "standard" else J.JPGE_HUFF_OPTIMAL)


def _same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


def _equal(got: bytes, want: bytes, what=""):
    d = S.difference(got, want)
    assert not d, f"{what}: {d}"


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
@pytest.mark.parametrize("mode,w,h", MODE_SIZES, ids=_ids(MODE_SIZES))
def test_coefficients(enc, fmt, xf, kind, mode, w, h):
    t = _set(enc, fmt, xf, mode=mode)
    got = enc.fdct_quant(T.build(fmt, *_p(w, h, kind)), quality=90)
    assert _same(got, _want(w, h, kind, t, mode))


# ---- 2. whole files ----
FILE_CASES = [(m, w, h) for m in (422, 420) for w, h in SIZES_420 + SIZES_ROW8] + \
             [(m, w, h) for m in (444, 411, 4200, 4201) for w, h in ((9, 9), (141, 27))]


@FMT
@pytest.mark.parametrize("huff", ["optimal", "standard"])
@pytest.mark.parametrize("quality", [50, 90, 100])
@pytest.mark.parametrize("mode,w,h", FILE_CASES, ids=_ids(FILE_CASES))
def test_whole_file(enc, fmt, huff, quality, mode, w, h):
    xf = {50: "full601", 90: "limited709", 100: "custom"}[quality]
    t = _set(enc, fmt, xf, mode=mode)
    _huff(enc, huff)
    _equal(enc.encode(T.build(fmt, *_p(w, h)), quality=quality), _jpg(w, h, t, mode, quality, 0, huff))


@FMT
@pytest.mark.parametrize("huff", ["optimal", "standard"])
@pytest.mark.parametrize("mode", T.MODES)
def test_whole_file_restart(enc, fmt, huff, mode):
    w, h = 130, 50
    t = _set(enc, fmt, "limited709", mode=mode)
    _huff(enc, huff)
    enc.set_restart(3)
    got = enc.encode(T.build(fmt, *_p(w, h)), quality=90)
    _equal(got, _jpg(w, h, t, mode, 90, 3, huff))
    assert got.count(b"\xff\xdd") >= 1  # DRI


# ---- 3. the three layouts equal one another; samples 4 b are the 8-bit frame of b ----
@functools.lru_cache(maxsize=None)
def _bytes(w, h):
    return Z.samples(7000 + w + h, w, h)


@pytest.mark.parametrize("xf", ["full601", "limited709"])
@pytest.mark.parametrize("huff", ["optimal", "standard"])
@pytest.mark.parametrize("mode", [422, 420, 444])
@pytest.mark.parametrize("w,h", [(33, 17), (141, 27)])
def test_layouts_equal_one_another(enc, xf, huff, mode, w, h):
    outs, coefs = [], []
    for fmt in T.FORMATS:
        t = _set(enc, fmt, xf, mode=mode)
        _huff(enc, huff)
        f = T.build(fmt, *_p(w, h))
        outs.append(enc.encode(f, quality=90))
        coefs.append(enc.fdct_quant(f, quality=90))
    assert outs[0] == outs[1] == outs[2]
    assert _same(coefs[0], coefs[1]) and _same(coefs[0], coefs[2])
    _equal(outs[0], _jpg(w, h, t, mode, 90, 0, huff))


@FMT
@pytest.mark.parametrize("xf", ["full601", "limited709"])
@pytest.mark.parametrize("huff", ["optimal", "standard"])
@pytest.mark.parametrize("mode", [422, 420, 444])
@pytest.mark.parametrize("w,h", [(33, 17), (141, 27)])
def test_multiples_of_four_equal_8bit(enc, enc8, fmt, xf, huff, mode, w, h):
    # (FULL_601: the new instance against the 8-bit build's kExact one)
    b = _bytes(w, h)
    for e in (enc, enc8):
        _huff(e, huff)
        e.set_restart(5 if huff == "standard" else 0)
    _set(enc8, T.EIGHT[fmt], xf, mode=mode)
    want = enc8.encode(Z.build(T.EIGHT[fmt], *b), quality=90)
    want_c = enc8.fdct_quant(Z.build(T.EIGHT[fmt], *b), quality=90)
    _set(enc, fmt, xf, mode=mode)
    f = T.build(fmt, *(4 * p.astype(np.uint16) for p in b))
    assert enc.encode(f, quality=90) == want
    assert _same(enc.fdct_quant(f, quality=90), want_c)


# ---- 4. the bits the layouts never read, and addressing ----
def _place(fmt, w, h, case):
    """(stride, offset, plane stride) of a frame inside random bytes: every base and pitch 16-byte
    aligned (I210: the stride a multiple of 32), the fast path; or base 2 bytes in, a stride that
    is no multiple of 16 and a plane stride of its own, the clamped path."""
    if case == "aligned":
        stride, off = -(-(T.least_stride(fmt, w) + 20) // 32) * 32, 32
        ps = 0 if fmt == T.Y210 else stride * h + 48
    else:
        stride, off = T.least_stride(fmt, w) + 6, 2
        ps = 0 if fmt == T.Y210 else stride * h + 10
    return stride, off, ps


@FMT
@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("w,h", [(80, 32), (33, 17), (130, 51)])
@pytest.mark.parametrize("case", ["clamped", "aligned"])
def test_addressing_and_unread_bits(enc, fmt, where, w, h, case):
    stride, off, ps = _place(fmt, w, h, case)
    mode = 422 if h != 51 else 420
    t = _set(enc, fmt, "limited709", ps, mode=mode)
    want = _jpg(w, h, t, mode)
    run = _encode_dev if where == "device" else _encode_host
    # other bytes around the frame; junk in the six unread bits; the spare Y1 word flipped
    variants = [dict(seed=9), dict(seed=10), dict(seed=9, junk_seed=21, spare=0x0000), dict(seed=9, junk_seed=22, spare=0xFFFF)]
    for v in variants:
        buf = T.raw(fmt, *_p(w, h), stride=stride, plane_stride=ps, offset=off, **v)[0]
        _equal(run(enc, buf, off, w, h, stride), want, str(v))


@FMT
@pytest.mark.parametrize("mode", [422, 420])
def test_host_frame_least_stride(enc1, fmt, mode):
    # host frames go through the upload's repitch (odd sizes: every plane by a 2-D copy)
    w, h = 33, 17
    t = _set(enc1, fmt, "custom", mode=mode)
    _equal(enc1.encode(T.build(fmt, *_p(w, h)), quality=90), _jpg(w, h, t, mode))
    # and at an aligned size, where the pitches match: one linear copy
    w, h = 64, 16
    _equal(enc1.encode(T.build(fmt, *_p(w, h)), quality=90), _jpg(w, h, t, mode))


# ---- 5. limits ----
_WANT8 = {}


@functools.lru_cache(maxsize=2)
def _limit_frame(fmt, case, w, h):
    stride, off, ps = _place(fmt, w, h, case)
    p = [4 * q.astype(np.uint16) for q in _bytes(w, h)]
    return T.raw(fmt, *p, stride=stride, plane_stride=ps, offset=off)[0], stride, off, ps


@FMT
@pytest.mark.parametrize("case", ["aligned", "clamped"])
@pytest.mark.parametrize("w,h", [(65535, 17), (17, 65535)], ids=["65535x17", "17x65535"])
def test_limit_frames_equal_8bit(enc1, fmt, case, w, h):
    buf, stride, off, ps = _limit_frame(fmt, case, w, h)
    for mode in (422, 420):
        key = (T.EIGHT[fmt], mode, w, h)
        if key not in _WANT8:  # the 8-bit frame's file, once for both cases
            _set(enc1, T.EIGHT[fmt], "limited709", mode=mode)
            _WANT8[key] = enc1.encode(Z.build(T.EIGHT[fmt], *_bytes(w, h)), quality=90)
        _set(enc1, fmt, "limited709", ps, mode=mode)
        assert _encode_dev(enc1, buf, off, w, h, stride) == _WANT8[key], mode


# ---- 6. the pipeline and the other entries ----
BATCH = [(160, 96) if i % 2 == 0 else (72, 40) for i in range(9)]  # two sizes, 5 of one: sets form


@FMT
@pytest.mark.parametrize("lanes", [4, 1])
def test_batch(enc, enc1, fmt, lanes):
    e = enc if lanes == 4 else enc1
    assert e.lanes() == lanes
    t = _set(e, fmt, "limited709", mode=422)
    outs = e.encode_batch([T.build(fmt, *_p(w, h, seed=100 + i)) for i, (w, h) in enumerate(BATCH)], quality=90)
    for i, (w, h) in enumerate(BATCH):
        _equal(outs[i], _jpg(w, h, t, 422, seed=100 + i), f"frame {i}")


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
def test_forced_set_sizes_short_last_set(set_size):
    w, h = 136, 72
    e = _encoder(JPGE_LANES=4, JPGE_SET=set_size)
    try:
        for fmt, mode in zip(T.FORMATS, (422, 420, 444)):
            t = _set(e, fmt, "full601", mode=mode)
            outs = e.encode_batch([T.build(fmt, *_p(w, h, seed=200 + i)) for i in range(9)], quality=75)
            for i in range(9):
                _equal(outs[i], _jpg(w, h, t, mode, 75, seed=200 + i), f"{T.NAMES[fmt]} frame {i}")
    finally:
        e.close()


def test_layout_change_between_batches(enc):
    # P010, then P210, then NV16 (and back to RGB8)
    w, h = 136, 72
    qy, qc = _oracle.quality_tables(75)
    preset, given, t = X.coeffs("limited709")
    enc.set_yuv_transform(preset, given)
    p10 = [T10.samples(300 + i, w, h) for i in range(5)]
    enc.set_input_format(T10.P010)
    outs = enc.encode_batch([T10.build(T10.P010, *q) for q in p10], quality=75)
    for i, q in enumerate(p10):
        _equal(outs[i], S.build3(T10.planes(*q, tuple(t)), w, h, qy, qc, 420).jpg, f"P010 frame {i}")
    enc.set_input_format(T.P210)
    outs = enc.encode_batch([T.build(T.P210, *_p(w, h, seed=200 + i)) for i in range(5)], quality=75)
    for i in range(5):
        _equal(outs[i], _jpg(w, h, tuple(t), 420, 75, seed=200 + i), f"P210 frame {i}")
    b = _bytes(w, h)
    enc.set_input_format(Z.NV16)
    want = S.build3(X.planes(Y.YUV444, *Z.repeated(*b), tuple(t)), w, h, qy, qc, 420).jpg
    for i, o in enumerate(enc.encode_batch([Z.build(Z.NV16, *b)] * 2, quality=75)):
        _equal(o, want, f"NV16 frame {i}")
    enc.set_input_format(J.JPGE_FMT_RGB8)
    rgb = J.synth_rgb8(4, 80, 32, kind=1)
    assert enc.encode_batch([rgb, rgb], quality=90) == [_oracle.encode(rgb, 90)] * 2


@FMT
def test_group_batch(fmt):
    preset, given, t = X.coeffs("limited709")
    with J.Group([0, 0]) as g:
        g.set_input_format(fmt)  # (a group's members stay in the default mode, 420)
        g.set_yuv_transform(preset, given)
        outs = g.encode_batch([T.build(fmt, *_p(w, h, seed=100 + i)) for i, (w, h) in enumerate(BATCH[:5])], quality=90)
    for i, (w, h) in enumerate(BATCH[:5]):
        _equal(outs[i], _jpg(w, h, tuple(t), 420, seed=100 + i), f"frame {i}")


@FMT
@pytest.mark.parametrize("mode", [422, 420])
def test_symbol_stats(enc1, enc8, fmt, mode):
    # the symbol statistics of samples 4 b are those of the 8-bit frame of b, and hold symbols
    w, h = 130, 50
    b = _bytes(w, h)
    _set(enc8, T.EIGHT[fmt], "limited709", mode=mode)
    c2, f2 = enc8.symbol_stats(Z.build(T.EIGHT[fmt], *b), quality=90)
    _set(enc1, fmt, "limited709", mode=mode)
    counts, first = enc1.symbol_stats(T.build(fmt, *(4 * q.astype(np.uint16) for q in b)), quality=90)
    assert counts.sum() > 0 and np.array_equal(counts, c2) and np.array_equal(first, f2)


@FMT
@pytest.mark.parametrize("where", ["device", "host"])
def test_tensor_entry(enc1, fmt, where):
    w, h = 130, 51
    cw = T.cw_of(w)
    y, cb, cr = _p(w, h)
    t = _set(enc1, J.JPGE_FMT_BGR8, "limited709", mode=422)
    want = _jpg(w, h, t, 422)
    dev = (lambda a: a.cuda()) if where == "device" else (lambda a: a)
    to = lambda a: torch.from_numpy(T.words(fmt, a).astype(np.int16))  # (16-bit words, whatever the sign)
    pitch = 304  # words: 608 bytes, a multiple of 32
    surf = dev(torch.randint(-32768, 32767, (3 * h + 3, pitch), dtype=torch.int16))
    if fmt == T.Y210:
        tp = surf[:h, :4 * cw]
        g = np.zeros((h, cw, 4), np.uint16)
        g[:, :, 0], g[:, :, 2], g[:, :, 1], g[:, :, 3] = y[:, 0::2], y[:, 1::2], cb, cr
        tp.copy_(to(g.reshape(h, 4 * cw)))
        args = (tp,)
    else:
        ty = surf[:h, :w]
        ty.copy_(to(y))
        if fmt == T.P210:
            tc = surf[h:2 * h, :2 * cw]
            tc.copy_(to(np.stack([cb, cr], axis=2).reshape(h, 2 * cw)))
            args = (ty, tc)
        else:
            half = surf[h:2 * h].reshape(-1).view(2 * h, pitch // 2)  # rows of pitch / 2 words
            tb, tr = half[:h, :cw], half[h:2 * h, :cw]
            tb.copy_(to(cb))
            tr.copy_(to(cr))
            args = (ty, tb, tr)
    _equal(enc1.encode_tensor_yuv422p10(*args, quality=90), want)
    if where == "device":
        out = torch.zeros(J.max_jpeg_bytes(w, h), dtype=torch.uint8, device="cuda")
        n = enc1.encode_tensor_yuv422p10(*args, quality=90, out=out)
        _equal(out[:n].cpu().numpy().tobytes(), want, "out=")
    assert enc1.input_format() == (J.JPGE_FMT_BGR8, 0)  # as before
    # geometry the layouts cannot express
    a = args[0]
    with pytest.raises(ValueError):
        enc1.encode_tensor_yuv422p10(a.view(torch.uint8))  # bytes
    with pytest.raises(ValueError):
        enc1.encode_tensor_yuv422p10(surf[:h, :4 * cw + 2])  # no whole groups
    with pytest.raises(ValueError):
        enc1.encode_tensor_yuv422p10(surf[:h, :w], surf[h:h + (h + 1) // 2, :2 * cw])  # 4:2:0's chroma
    with pytest.raises(ValueError):
        enc1.encode_tensor_yuv422p10(surf[h:2 * h, :w], surf[:h, :2 * cw])  # chroma before Y
    with pytest.raises(ValueError):
        enc1.encode_tensor_yuv422p10(surf[:h, :w], surf[h:2 * h, :2 * cw].clone())  # another allocation
    with pytest.raises(ValueError):
        enc1.encode_tensor_yuv422p10(surf[:h, :w], surf[h:2 * h, :cw], surf[2 * h:3 * h, :cw])  # I210's chroma at the Y pitch
    with pytest.raises(ValueError):
        enc1.encode_tensor_yuv422p10(surf[:h, :2 * w:2], surf[h:2 * h, :2 * cw])  # inner stride 2
    assert enc1.input_format() == (J.JPGE_FMT_BGR8, 0)


# ---- 7. refusals: each is the argument error, queues nothing, and leaves the context encoding ----
@FMT
def test_refusals(enc, fmt):
    w, h = 80, 32
    t = _set(enc, fmt, "limited709", mode=422)
    f = T.build(fmt, *_p(w, h))
    want = _jpg(w, h, t, 422)
    _equal(enc.encode(f, quality=90), want)
    with pytest.raises(J.JpgeError) as ei:
        enc.encode(f, quality=90, maxval=100)
    assert ei.value.status == E_ARG
    with pytest.raises(J.JpgeError):
        enc.encode_batch([f, f], quality=90, maxval=100)
    _equal(enc.encode(f, quality=90), want)
    # downscale 2
    enc.set_downscale(2)
    with pytest.raises(J.JpgeError) as ei:
        enc.encode(f, quality=90)
    assert ei.value.status == E_ARG
    enc.set_downscale(1)
    _equal(enc.encode(f, quality=90), want)
    # odd stride, odd plane stride, odd base, a stride below the least
    least = T.least_stride(fmt, w)
    gps = 0 if fmt == T.Y210 else (least + 16) * h + 16
    buf = T.raw(fmt, *_p(w, h), stride=least + 16, plane_stride=gps, offset=16)[0]
    dev = torch.from_numpy(buf).cuda()
    out = torch.zeros(J.max_jpeg_bytes(w, h), dtype=torch.uint8, device="cuda")
    good = (dev.data_ptr() + 16, least + 16, gps)
    bad = [(good[0], least + 17, good[2]), (good[0] + 1, good[1], good[2]), (good[0], least - 2, good[2])]
    if fmt != T.Y210:
        bad.append((good[0], good[1], good[2] + 1))
    for ptr, stride, ps in bad:
        enc.set_input_format(fmt, ps)
        with pytest.raises(J.JpgeError) as ei:
            enc.encode_ptr(ptr, w, h, stride, out.data_ptr(), out.numel(), 90)
        assert ei.value.status == E_ARG, (ptr - good[0], stride, ps)
        enc.set_input_format(fmt, good[2])
        n = enc.encode_ptr(good[0], w, h, good[1], out.data_ptr(), out.numel(), 90)
        torch.cuda.synchronize()
        _equal(out[:n].cpu().numpy().tobytes(), want)
    if fmt == T.Y210:  # one plane: no plane stride
        with pytest.raises(J.JpgeError) as ei:
            enc.set_input_format(fmt, 4096)
        assert ei.value.status == E_ARG
        assert enc.input_format() == (fmt, 0)
        _equal(enc.encode(f, quality=90), want)


@FMT
def test_refuses_stripes(enc1, fmt):
    t = _set(enc1, fmt, "full601", mode=420)
    dev = torch.zeros(3 * 256 * 128, dtype=torch.uint8, device="cuda")
    with pytest.raises(J.JpgeError) as ei:
        enc1.stripe_transform(dev.data_ptr(), 512, 256, 128, 0, 2, 90)
    assert ei.value.status == E_ARG
    w, h = 33, 17
    _equal(enc1.encode(T.build(fmt, *_p(w, h)), quality=90), _jpg(w, h, t, 420))


@FMT
def test_group_refuses_striped(fmt):
    rgb = J.synth_rgb8(2, 640, 480)
    with J.Group([0, 0]) as g:
        g.set_input_format(fmt)
        with pytest.raises(J.JpgeError):
            g.encode_striped(rgb, quality=90)
        g.set_input_format(J.JPGE_FMT_RGB8)
        assert g.encode_striped(rgb, quality=90) == _oracle.encode(rgb, 90)
