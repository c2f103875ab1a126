"""The v210 layout (JPGE_FMT_V210) on the GPU: K1's build that loads the three or four 16-byte
groups holding a lane's 16-pixel run and unpacks them by the lane's phase (run n starts 0, 4 or 2
pixels into its first group for n % 3 = 0, 1, 2), in all six subsampling modes.  Expectations
(_v210.py and _yuv422p10.py, checked by test_v210_cpu.py and test_yuv422p10_cpu.py): the samples
by the stream rule in numpy, every sample s the exact value s / 4, a cell's chroma in both of its
pixels, the three lines of jpge.h with the coefficients the library returned, then the oracle's
primitives for the coefficients (_yuv.want_coeffs) and the CPU-built stream (_stream3.build3) for
whole files: no GPU code under test runs in an expectation.  Where the header states an equality
of two encodes (v210 and Y210 / I210 of the same samples; samples 4 b and the 8-bit YUYV frame of
b), the two encodes are compared, the other one on a second context.  Every comparison is exact.

Sizes: every lane position must meet all three phases on the fast path, which takes three full
tile columns: 192 pixels in the 4:2:0 modes (64-pixel tiles), 384 in the row-8 modes (128)."""
import functools
import os

import numpy as np
import pytest

import _fixedhuff as F
import _oracle
import _stream3 as S
import _v210 as V
import _yuv as Y
import _yuv422 as Z
import _yuv422p10 as T
import _yuvxf as X
import jpgenc_amd as J

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FMT = J.JPGE_FMT_V210
SIZES_420 = [(1, 1), (6, 2), (16, 16), (64, 16), (33, 17), (200, 20), (262, 34)]
SIZES_ROW8 = [(9, 9), (136, 24), (400, 9), (391, 27)]
MODES_420, MODES_ROW8 = [420, 4200, 4201], [444, 422, 411]
MODE_SIZES = [(m, w, h) for m in MODES_420 for w, h in SIZES_420] + [(m, w, h) for m in MODES_ROW8 for w, h in SIZES_ROW8]
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
def enc2():
    """The second context: the other layouts' frames of the equalities."""
    e = J.Encoder(0, lanes=1)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def _defaults(enc, enc1, enc2):
    yield
    for e in (enc, enc1, enc2):
        e.set_downscale(1)
        e.set_input_format(J.JPGE_FMT_RGB8)
        e.set_subsampling(420)
        e.set_restart(0)
        e.set_huffman(J.JPGE_HUFF_OPTIMAL)
        e.set_yuv_transform(J.JPGE_YUV_FULL_601)


def _set(e, fmt, xf, mode=None, plane_stride=0):
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
def _p(w, h, seed=None):
    return V.samples(1000 * w + h if seed is None else seed, w, h)


@functools.lru_cache(maxsize=None)
def _planes(w, h, seed, t, mode):
    return V.planes(*_p(w, h, seed), t, Y.mcu_size(mode))


@functools.lru_cache(maxsize=None)
def _want(w, h, t, mode, quality=90, seed=None):
    return Y.want_coeffs(_planes(w, h, seed, t, mode), mode, quality)


@functools.lru_cache(maxsize=None)
def _jpg(w, h, t, mode, quality=90, restart=0, huff="optimal", seed=None):
    """The CPU-built file (_stream3.build3) of the samples _p(w, h, seed)."""
    qy, qc = _oracle.quality_tables(quality)
    specs = F.golden_specs() if huff == "standard" else None
    return S.build3(_planes(w, h, seed, tuple(t), mode), w, h, qy, qc, mode, restart, specs).jpg


def _huff(e, huff):
    e.set_huffman(J.JPGE_HUFF_STANDARD if huff == "standard" else J.JPGE_HUFF_OPTIMAL)


def _same(got, want):
    return all(np.asarray(g).size == w.size and np.array_equal(np.asarray(g).reshape(w.shape), w) for g, w in zip(got, want))


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


def _place(w, case):
    """(stride, offset) of a frame inside random bytes: base and pitch 16-byte aligned, the fast
    path (with the clamped edge lanes); or base 4 bytes in and a pitch that is a multiple of 4 but
    not of 16, every lane clamped."""
    if case == "aligned":
        return V.row_bytes(w) + 32, 32
    return V.row_bytes(w) + 12, 4


# ---- 1. coefficients ----
@pytest.mark.parametrize("xf", SETTINGS)
@pytest.mark.parametrize("mode,w,h", MODE_SIZES, ids=_ids(MODE_SIZES))
def test_coefficients(enc, xf, mode, w, h):
    # a host frame: uploaded at the conventional pitch, so the fast path with its clamped edge lanes
    t = _set(enc, FMT, xf, mode=mode)
    got = enc.fdct_quant(V.build(*_p(w, h)), quality=90)
    assert _same(got, _want(w, h, t, mode))


@pytest.mark.parametrize("case", ["aligned", "clamped"])
@pytest.mark.parametrize("mode,w,h", MODE_SIZES, ids=_ids(MODE_SIZES))
def test_coefficients_in_place(enc, case, mode, w, h):
    # a device frame read in place; the file's coefficients, decoded on the host
    stride, off = _place(w, case)
    t = _set(enc, FMT, "limited709", mode=mode)
    buf = V.raw(*_p(w, h), stride=stride, offset=off, junk_seed=3)[0]
    info, y, cb, cr = J.decode_coeffs(_encode_dev(enc, buf, off, w, h, stride))
    assert _same((y, cb, cr), _want(w, h, t, mode))


# ---- 2. whole files ----
FILE_CASES = [(420, 262, 34), (422, 391, 27), (444, 136, 24), (411, 400, 9), (4200, 200, 20), (4201, 33, 17),
              (422, 6, 2), (420, 1, 1)]


@pytest.mark.parametrize("huff", ["optimal", "standard"])
@pytest.mark.parametrize("quality", [50, 90, 100])
@pytest.mark.parametrize("mode,w,h", FILE_CASES, ids=_ids(FILE_CASES))
def test_whole_file(enc, huff, quality, mode, w, h):
    xf = {50: "full601", 90: "limited709", 100: "custom"}[quality]
    t = _set(enc, FMT, xf, mode=mode)
    _huff(enc, huff)
    _equal(enc.encode(V.build(*_p(w, h)), quality=quality), _jpg(w, h, t, mode, quality, 0, huff))


@pytest.mark.parametrize("huff", ["optimal", "standard"])
@pytest.mark.parametrize("mode", V.MODES)
def test_whole_file_restart(enc, huff, mode):
    w, h = 200, 20
    t = _set(enc, FMT, "limited709", mode=mode)
    _huff(enc, huff)
    enc.set_restart(3)
    got = enc.encode(V.build(*_p(w, h)), quality=90)
    _equal(got, _jpg(w, h, t, mode, 90, 3, huff))
    assert got.count(b"\xff\xdd") >= 1  # DRI


# ---- 3. the layouts of the same samples equal one another; samples 4 b are the 8-bit frame of b ----
@functools.lru_cache(maxsize=None)
def _bytes(w, h):
    return Z.samples(7000 + w + h, w, h)


@pytest.mark.parametrize("xf", ["full601", "limited709"])
@pytest.mark.parametrize("huff", ["optimal", "standard"])
@pytest.mark.parametrize("mode,w,h", [(420, 262, 34), (422, 391, 27)])
def test_equals_y210_and_i210(enc, enc2, xf, huff, mode, w, h):
    p = _p(w, h)
    _huff(enc, huff)
    _huff(enc2, huff)
    t = _set(enc, FMT, xf, mode=mode)
    got = enc.encode(V.build(*p), quality=90)
    got_c = enc.fdct_quant(V.build(*p), quality=90)
    for other in (T.Y210, T.I210):
        _set(enc2, other, xf, mode=mode)
        f = T.build(other, *p)
        assert enc2.encode(f, quality=90) == got, T.NAMES[other]
        assert _same(enc2.fdct_quant(f, quality=90), got_c)
    _equal(got, _jpg(w, h, t, mode, 90, 0, huff))


@pytest.mark.parametrize("xf", ["full601", "limited709"])
@pytest.mark.parametrize("huff", ["optimal", "standard"])
@pytest.mark.parametrize("mode,w,h", [(420, 262, 34), (422, 391, 27), (444, 136, 24)])
def test_multiples_of_four_equal_yuyv(enc, enc2, xf, huff, mode, w, h):
    b = _bytes(w, h)
    for e in (enc, enc2):
        _huff(e, huff)
        e.set_restart(5 if huff == "standard" else 0)
    _set(enc2, Z.YUYV, xf, mode=mode)
    want = enc2.encode(Z.build(Z.YUYV, *b), quality=90)
    want_c = enc2.fdct_quant(Z.build(Z.YUYV, *b), quality=90)
    _set(enc, FMT, xf, mode=mode)
    f = V.build(*(4 * p.astype(np.uint16) for p in b))
    assert enc.encode(f, quality=90) == want
    assert _same(enc.fdct_quant(f, quality=90), want_c)


# ---- 4. robustness: what the layout never reads, and addressing ----
@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("w,h", [(262, 34), (391, 27), (33, 17)])
@pytest.mark.parametrize("case", ["clamped", "aligned"])
def test_addressing_and_unread_bits(enc, where, w, h, case):
    stride, off = _place(w, case)
    mode = 420 if h == 34 else 422
    t = _set(enc, FMT, "limited709", mode=mode)
    want = _jpg(w, h, t, mode)
    run = _encode_dev if where == "device" else _encode_host
    # other bytes before, between and after the rows; junk in bits 30-31 and the unused samples
    for v in (dict(seed=9), dict(seed=10), dict(seed=9, junk_seed=21), dict(seed=11, junk_seed=22)):
        buf = V.raw(*_p(w, h), stride=stride, offset=off, **v)[0]
        _equal(run(enc, buf, off, w, h, stride), want, str(v))


@pytest.mark.parametrize("mode,w,h", [(420, 192, 16), (422, 384, 8)])
def test_neighbour_groups_of_three_group_lanes(enc, mode, w, h):
    # a lane whose run needs three groups issues a fourth load that must move nothing.  Three full
    # tile columns end with such a run (n % 3 = 2): the group after its third is the row's
    # padding, which changes between the two encodes (as do bits 30-31) while the bytes do not
    assert V.row_bytes(w) == 16 * (w // 6) and (w // 16 - 1) % 3 == 2
    stride, off = V.conventional_stride(w) + 64, 64
    t = _set(enc, FMT, "full601", mode=mode)
    want = _jpg(w, h, t, mode)
    for seed in (1, 2):
        buf = V.raw(*_p(w, h), stride=stride, offset=off, seed=seed, junk_seed=seed)[0]
        _equal(_encode_dev(enc, buf, off, w, h, stride), want, f"padding {seed}")


def test_host_frame_pitches(enc1):
    # the least stride goes through the upload's repitch (one 2-D copy), the conventional pitch is
    # the device copy's own (one linear copy, up to the last row's last group)
    for mode, (w, h) in ((422, (33, 17)), (420, (262, 34)), (422, (48, 8))):
        t = _set(enc1, FMT, "custom", mode=mode)
        want = _jpg(w, h, t, mode)
        _equal(enc1.encode(V.build(*_p(w, h)), quality=90), want, "least")
        f = V.build(*_p(w, h), stride=V.conventional_stride(w))
        assert f.stride == V.conventional_stride(w)
        _equal(enc1.encode(f, quality=90), want, "conventional")
        # a capture buffer that ends with the last row's last group
        n = f.stride * (h - 1) + V.row_bytes(w)
        buf = np.ascontiguousarray(np.asarray(f)[:n])
        _equal(_encode_host(enc1, buf, 0, w, h, f.stride), want, "short last row")


# ---- 5. limits ----
@pytest.mark.parametrize("w,h", [(65535, 7), (7, 65535)], ids=["65535x7", "7x65535"])
def test_limit_frames_equal_yuyv(enc1, enc2, w, h):
    b = _bytes(w, h)
    f = V.build(*(4 * p.astype(np.uint16) for p in b), stride=V.conventional_stride(w))
    buf = np.ascontiguousarray(np.asarray(f))
    for mode in (422, 420):
        _set(enc2, Z.YUYV, "limited709", mode=mode)
        want = enc2.encode(Z.build(Z.YUYV, *b), quality=90)
        _set(enc1, FMT, "limited709", mode=mode)
        assert _encode_dev(enc1, buf, 0, w, h, f.stride) == want, mode


# ---- 6. the pipeline and the other entries ----
BATCH = [(208, 96) if i % 2 == 0 else (72, 40) for i in range(9)]  # two sizes, 5 of one: sets form


@pytest.mark.parametrize("lanes", [4, 1])
def test_batch(enc, enc1, lanes):
    e = enc if lanes == 4 else enc1
    assert e.lanes() == lanes
    t = _set(e, FMT, "limited709", mode=422)
    outs = e.encode_batch([V.build(*_p(w, h, seed=100 + i)) for i, (w, h) in enumerate(BATCH)], quality=90)
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


@pytest.mark.parametrize("set_size", [1, 2, 3, 4])
def test_forced_set_sizes(set_size):
    w, h = 200, 40
    e = _encoder(JPGE_LANES=4, JPGE_SET=set_size)
    try:
        for mode in (422, 420):
            t = _set(e, FMT, "full601", mode=mode)
            outs = e.encode_batch([V.build(*_p(w, h, seed=200 + i)) for i in range(9)], quality=75)
            for i in range(9):
                _equal(outs[i], _jpg(w, h, t, mode, 75, seed=200 + i), f"mode {mode} frame {i}")
    finally:
        e.close()


def test_layout_change_between_batches(enc):
    # Y210, then v210, then NV16 (and back to RGB8) on one context
    w, h = 200, 40
    qy, qc = _oracle.quality_tables(75)
    preset, given, t = X.coeffs("limited709")
    enc.set_yuv_transform(preset, given)
    enc.set_input_format(T.Y210)
    outs = enc.encode_batch([T.build(T.Y210, *_p(w, h, seed=300 + i)) for i in range(5)], quality=75)
    for i in range(5):
        _equal(outs[i], _jpg(w, h, tuple(t), 420, 75, seed=300 + i), f"Y210 frame {i}")
    enc.set_input_format(FMT)
    outs = enc.encode_batch([V.build(*_p(w, h, seed=200 + i)) for i in range(5)], quality=75)
    for i in range(5):
        _equal(outs[i], _jpg(w, h, tuple(t), 420, 75, seed=200 + i), f"v210 frame {i}")
    b = _bytes(w, h)
    enc.set_input_format(Z.NV16)
    want = S.build3(X.planes(Y.YUV444, *Z.repeated(*b), tuple(t)), w, h, qy, qc, 420).jpg
    for i, o in enumerate(enc.encode_batch([Z.build(Z.NV16, *b)] * 2, quality=75)):
        _equal(o, want, f"NV16 frame {i}")
    enc.set_input_format(J.JPGE_FMT_RGB8)
    rgb = J.synth_rgb8(4, 80, 32, kind=1)
    assert enc.encode_batch([rgb, rgb], quality=90) == [_oracle.encode(rgb, 90)] * 2


def test_group_batch():
    preset, given, t = X.coeffs("limited709")
    with J.Group([0, 0]) as g:
        g.set_input_format(FMT)  # (a group's members stay in the default mode, 420)
        g.set_yuv_transform(preset, given)
        outs = g.encode_batch([V.build(*_p(w, h, seed=100 + i)) for i, (w, h) in enumerate(BATCH[:5])], quality=90)
    for i, (w, h) in enumerate(BATCH[:5]):
        _equal(outs[i], _jpg(w, h, tuple(t), 420, seed=100 + i), f"frame {i}")


@pytest.mark.parametrize("mode", [422, 420])
def test_symbol_stats(enc1, enc2, mode):
    # the symbol statistics of samples 4 b are those of the 8-bit frame of b, and hold symbols
    w, h = 200, 40
    b = _bytes(w, h)
    _set(enc2, Z.YUYV, "limited709", mode=mode)
    c2, f2 = enc2.symbol_stats(Z.build(Z.YUYV, *b), quality=90)
    _set(enc1, FMT, "limited709", mode=mode)
    counts, first = enc1.symbol_stats(V.build(*(4 * q.astype(np.uint16) for q in b)), quality=90)
    assert counts.sum() > 0 and np.array_equal(counts, c2) and np.array_equal(first, f2)


@pytest.mark.parametrize("dtype", ["uint8", "int32"])
@pytest.mark.parametrize("where", ["device", "host"])
def test_tensor_entry(enc1, where, dtype):
    w, h = 262, 35
    t = _set(enc1, J.JPGE_FMT_BGR8, "limited709", mode=422)
    want = _jpg(w, h, t, 422)
    row = V.row_bytes(w)
    pitch = V.conventional_stride(w) + 128
    buf = V.raw(*_p(w, h), stride=pitch, offset=0, junk_seed=4, tail=pitch - row)[0]
    surf = torch.from_numpy(buf.reshape(h, pitch).copy())
    if dtype == "int32":
        surf = surf.view(torch.int32)
    if where == "device":
        surf = surf.cuda()
    es = surf.element_size()
    tp = surf[:, :row // es]
    _equal(enc1.encode_tensor_v210(tp, w, quality=90), want)
    _equal(enc1.encode_tensor_v210(surf, w, quality=90), want, "longer rows")
    if where == "device":
        out = torch.zeros(J.max_jpeg_bytes(w, h), dtype=torch.uint8, device="cuda")
        n = enc1.encode_tensor_v210(tp, w, quality=90, out=out)
        _equal(out[:n].cpu().numpy().tobytes(), want, "out=")
    assert enc1.input_format() == (J.JPGE_FMT_BGR8, 0)  # as before
    # what prep1 would refuse, and what is no frame of rows
    bad = [
        lambda: enc1.encode_tensor_v210(tp.to(torch.int16) if dtype == "int32" else tp.view(torch.int16), w),  # 16-bit words
        lambda: enc1.encode_tensor_v210(tp.reshape(-1)[:row // es], w),  # 1-D
        lambda: enc1.encode_tensor_v210(surf[:, :row // es - 1], w),  # a row too short for the width
        lambda: enc1.encode_tensor_v210(tp, 0),
        lambda: enc1.encode_tensor_v210(tp, 65536),
        lambda: enc1.encode_tensor_v210(surf[:, ::2], 6),  # inner stride 2
    ]
    if dtype == "uint8":
        bad.append(lambda: enc1.encode_tensor_v210(surf[:, 2:2 + row], w))  # base 2 bytes in
        odd = surf.reshape(-1)[:(pitch - 2) * h].view(h, pitch - 2)         # pitch no multiple of 4
        bad.append(lambda: enc1.encode_tensor_v210(odd[:, :row], w))
    for f in bad:
        with pytest.raises(ValueError):
            f()
    assert enc1.input_format() == (J.JPGE_FMT_BGR8, 0)
    _equal(enc1.encode_tensor_v210(tp, w, quality=90), want, "after the refusals")


# ---- 7. refusals: each is the argument error, queues nothing, and leaves the context encoding ----
def test_refusals(enc):
    w, h = 200, 20
    t = _set(enc, FMT, "limited709", mode=422)
    f = V.build(*_p(w, h))
    want = _jpg(w, h, t, 422)
    _equal(enc.encode(f, quality=90), want)
    with pytest.raises(J.JpgeError) as ei:
        enc.encode(f, quality=90, maxval=100)
    assert ei.value.status == E_ARG
    with pytest.raises(J.JpgeError):
        enc.encode_batch([f, f], quality=90, maxval=100)
    _equal(enc.encode(f, quality=90), want)
    # downscale 2 and 4
    for s in (2, 4):
        enc.set_downscale(s)
        with pytest.raises(J.JpgeError) as ei:
            enc.encode(f, quality=90)
        assert ei.value.status == E_ARG
        enc.set_downscale(1)
        _equal(enc.encode(f, quality=90), want)
    # a non-zero plane stride: one plane
    with pytest.raises(J.JpgeError) as ei:
        enc.set_input_format(FMT, 4096)
    assert ei.value.status == E_ARG
    assert enc.input_format() == (FMT, 0)
    _equal(enc.encode(f, quality=90), want)
    # base or stride no multiple of 4 (even ones too), a stride below the least
    least = V.row_bytes(w)
    buf = V.raw(*_p(w, h), stride=least + 16, offset=16)[0]
    dev = torch.from_numpy(buf).cuda()
    out = torch.zeros(J.max_jpeg_bytes(w, h), dtype=torch.uint8, device="cuda")
    good = (dev.data_ptr() + 16, least + 16)
    bad = [(good[0], least + 17), (good[0], least + 18), (good[0] + 1, good[1]), (good[0] + 2, good[1]),
           (good[0], least - 4), (good[0], least - 16)]
    for ptr, stride in bad:
        with pytest.raises(J.JpgeError) as ei:
            enc.encode_ptr(ptr, w, h, stride, out.data_ptr(), out.numel(), 90)
        assert ei.value.status == E_ARG, (ptr - good[0], stride)
        n = enc.encode_ptr(good[0], w, h, good[1], out.data_ptr(), out.numel(), 90)
        torch.cuda.synchronize()
        _equal(out[:n].cpu().numpy().tobytes(), want)
    # the same from host memory
    for off, stride in ((0, least + 18), (2, least + 16), (0, least - 4)):
        with pytest.raises(J.JpgeError) as ei:
            _encode_host(enc, buf, 16 + off, w, h, stride)
        assert ei.value.status == E_ARG, (off, stride)
        _equal(_encode_host(enc, buf, 16, w, h, least + 16), want)


def test_refuses_stripes(enc1):
    t = _set(enc1, FMT, "full601", mode=420)
    dev = torch.zeros(3 * 256 * 128, dtype=torch.uint8, device="cuda")
    with pytest.raises(J.JpgeError) as ei:
        enc1.stripe_transform(dev.data_ptr(), 512, 256, 128, 0, 2, 90)
    assert ei.value.status == E_ARG
    w, h = 33, 17
    _equal(enc1.encode(V.build(*_p(w, h)), quality=90), _jpg(w, h, t, 420))


def test_group_refuses_striped():
    rgb = J.synth_rgb8(2, 640, 480)
    with J.Group([0, 0]) as g:
        g.set_input_format(FMT)
        with pytest.raises(J.JpgeError):
            g.encode_striped(rgb, quality=90)
        g.set_input_format(J.JPGE_FMT_RGB8)
        assert g.encode_striped(rgb, quality=90) == _oracle.encode(rgb, 90)
