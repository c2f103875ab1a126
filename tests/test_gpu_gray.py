"""One-component (JPGE_FMT_GRAY8) encodes on the GPU: K1's gray load shape, the statistics
and entropy kernels at one block per MCU, the two-table host build and the one-component
headers.  Expected bytes come from _gray.py (the oracle's primitives; checked on the host by
test_gray_cpu.py); every comparison is exact.  Shapes are the smallest at which each
mechanism can go wrong: edge replication, one block against two, K1's 128-px tile plus a
partial one, the 128-block statistics / entropy tiles, several entropy workgroups."""
import os

import numpy as np
import pytest

import _gray as G
import _oracle
import jpgenc_amd as J

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GRAY = J.JPGE_FMT_GRAY8
E_ARG = 1
SMALL = [(1, 1), (7, 5), (8, 8), (9, 9), (17, 8), (136, 16), (1032, 24)]
BIG = (1024, 512)  # 8192 blocks, 64 tiles


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
def _defaults(enc, enc1):
    for e in (enc, enc1):
        e.set_input_format(GRAY)
    yield
    for e in (enc, enc1):
        e.set_input_format(J.JPGE_FMT_RGB8)
        e.set_subsampling(420)
        e.set_restart(0)


def _one_component(jpg):
    i = jpg.index(b"\xff\xc0")
    return jpg[i + 9] == 1


# ---- 1. whole files ----
@pytest.mark.parametrize("quality", [50, 90, 100])
@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("w,h", SMALL)
def test_whole_file(enc, w, h, kind, quality):
    got = enc.encode(G.plane(kind, w, h), quality=quality)
    assert _one_component(got)
    assert got == G.built(kind, w, h, quality).jpg


@pytest.mark.parametrize("kind,quality", [("random", 100), ("photo", 90), ("photo", 50), ("zeros", 90), ("ones", 50)])
@pytest.mark.parametrize("lanes", [4, 1])
def test_whole_file_many_tiles(enc, enc1, lanes, kind, quality):
    e = enc if lanes == 4 else enc1
    assert e.encode(G.plane(kind, *BIG), quality=quality) == G.built(kind, *BIG, quality).jpg


def _encoder(lanes=0, **env):
    # (a context reads its switches when it opens, Encoder::open: a fresh context under the
    # setting, as test_gpu_env_modes.py does)
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


@pytest.mark.parametrize("wgs", [1, 65536], ids=["least", "most"])
@pytest.mark.parametrize("lanes", [4, 1])
def test_entropy_workgroups_forced(lanes, wgs):
    # 64 tiles: the fewest workgroups (4 tiles each) and the most (one tile each)
    e = _encoder(lanes=lanes, JPGE_ENTROPY_WGS=wgs)
    try:
        e.set_input_format(GRAY)
        assert e.encode(G.plane("photo", *BIG), quality=90) == G.built("photo", *BIG, 90).jpg
        e.set_restart(1000)
        assert e.encode(G.plane("photo", *BIG), quality=90) == G.built("photo", *BIG, 90, 1000).jpg
    finally:
        e.close()


# ---- 2. large symbols: continuation records ----
def _blocks_0_255():
    p = np.zeros((16, 64), np.uint8)
    for by in range(2):
        for bx in range(8):
            if (bx + by) % 2:
                p[8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = 255
    return p


def _checkerboard():
    yy, xx = np.mgrid[0:16, 0:64]
    return (((xx + yy) & 1) * 255).astype(np.uint8)


@pytest.mark.parametrize("lanes", [4, 1])
def test_large_symbols(enc, enc1, lanes):
    e = enc if lanes == 4 else enc1
    ones = np.ones(64, np.uint8)
    a, b = G.build(_blocks_0_255(), ones), G.build(_checkerboard(), ones)
    assert 11 in a.dc_text  # a DC difference of category 11
    assert max(s & 15 for s in b.ac_text) >= 7  # AC sizes past the 6 extra bits a record holds
    assert e.encode(_blocks_0_255(), qy=ones) == a.jpg
    assert e.encode(_checkerboard(), qy=ones) == b.jpg
    # and a chroma table given beside it is not read
    assert e.encode(_checkerboard(), qy=ones, qc=np.full(64, 200, np.uint8)) == b.jpg


# ---- 3. restart intervals (in blocks) ----
@pytest.mark.parametrize("restart", [1, 3, 7, 5000])
@pytest.mark.parametrize("w,h", [(136, 16), (1032, 24)])
@pytest.mark.parametrize("lanes", [4, 1])
def test_restart(enc, enc1, lanes, w, h, restart):
    e = enc if lanes == 4 else enc1
    e.set_restart(restart)
    got = e.encode(G.plane("photo", w, h), quality=90)
    assert got == G.built("photo", w, h, 90, restart).jpg
    assert J.decode_coeffs(got)[0].restart == restart


# ---- 4. the clamped per-pixel path ----
@pytest.mark.parametrize("w,h", [(136, 16), (33, 9)])
def test_slow_path(enc, w, h):
    p = G.plane("random", w, h, seed=5)
    want = G.built("random", w, h, 90, 0, 5).jpg
    assert enc.encode(p, quality=90) == want  # the aligned frame
    stride, off = w + 3, 1
    buf = np.random.default_rng(6).integers(0, 256, off + stride * h + 16, dtype=np.uint8)
    buf[off:off + stride * h].reshape(h, stride)[:, :w] = p
    cap = J.max_jpeg_bytes(w, h)
    # a device buffer
    dev = torch.from_numpy(buf).cuda()
    assert dev.data_ptr() % 16 == 0
    out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    n = enc.encode_ptr(dev.data_ptr() + off, w, h, stride, out.data_ptr(), cap, 90)
    torch.cuda.synchronize()
    assert out[:n].cpu().numpy().tobytes() == want
    # the same bytes from the host
    hout = np.zeros(cap, np.uint8)
    n = enc.encode_ptr(buf.ctypes.data + off, w, h, stride, hout.ctypes.data, cap, 90, flags=0)
    assert hout[:n].tobytes() == want


def test_fast_path_in_place(enc):
    # base and pitch 16-byte aligned, a pitch wider than the row: K1's b128 loads, in place
    w, h, stride, off = 136, 16, 160, 32
    p = G.plane("random", w, h, seed=7)
    buf = np.random.default_rng(8).integers(0, 256, off + stride * h, dtype=np.uint8)
    buf[off:].reshape(h, stride)[:, :w] = p
    dev = torch.from_numpy(buf).cuda()
    out = torch.zeros(J.max_jpeg_bytes(w, h), dtype=torch.uint8, device="cuda")
    n = enc.encode_ptr(dev.data_ptr() + off, w, h, stride, out.data_ptr(), out.numel(), 90)
    torch.cuda.synchronize()
    assert out[:n].cpu().numpy().tobytes() == G.built("random", w, h, 90, 0, 7).jpg


# ---- 5. the subsampling mode does not enter ----
def test_subsampling_modes_agree(enc):
    p = G.plane("photo", 136, 16)
    want = G.built("photo", 136, 16, 90).jpg
    for mode in (420, 444, 422, 411, 4200, 4201):
        enc.set_subsampling(mode)
        assert enc.encode(p, quality=90) == want, mode
        assert np.array_equal(enc.fdct_quant(p, quality=90)[0], G.built("photo", 136, 16, 90).coef), mode


# ---- 6. batches ----
def test_frame_sets(enc):
    assert enc.lanes() == 4
    ps = [G.plane("random", 136, 72, seed=300 + i) for i in range(9)]
    outs = enc.encode_batch(ps, quality=75)
    assert outs == [G.built("random", 136, 72, 75, 0, 300 + i).jpg for i in range(9)]
    assert outs == [enc.encode(p, quality=75) for p in ps]


MIXED = [(136, 16), (9, 9), (1032, 24), (1, 1), (200, 120)]


@pytest.mark.parametrize("lanes", [4, 1])
def test_batch_mixed(enc, enc1, lanes):
    e = enc if lanes == 4 else enc1
    ps = [G.plane("photo", w, h, seed=20 + i) for i, (w, h) in enumerate(MIXED)]
    outs = e.encode_batch(ps, quality=90)
    for i, (w, h) in enumerate(MIXED):
        assert outs[i] == G.built("photo", w, h, 90, 0, 20 + i).jpg, i
        assert outs[i] == e.encode(ps[i], quality=90), i


def test_group_batch():
    ps = [G.plane("photo", w, h, seed=20 + i) for i, (w, h) in enumerate(MIXED)]
    with J.Group([0, 0]) as g:
        g.set_input_format(GRAY)
        outs = g.encode_batch(ps, quality=90)
    assert outs == [G.built("photo", w, h, 90, 0, 20 + i).jpg for i, (w, h) in enumerate(MIXED)]


def test_batch_with_a_refused_frame(enc):
    # frame 2's maxval is 100: its status is JPGE_E_ARG, the others are encoded
    ps = [G.plane("random", 136, 16, seed=40 + i) for i in range(5)]
    qy, qc = J.quality_tables(90)
    outs = [np.zeros(J.max_jpeg_bytes(136, 16), np.uint8) for _ in ps]
    arr = (J.Frame * len(ps))()
    for i, (p, o) in enumerate(zip(ps, outs)):
        arr[i].rgb, arr[i].width, arr[i].height, arr[i].stride = p.ctypes.data, 136, 16, 136
        arr[i].maxval, arr[i].out, arr[i].cap = (100 if i == 2 else 255), o.ctypes.data, o.size
    # (the chroma table may be NULL for this layout)
    st = J.lib().jpge_encode_batch(enc.ctx, arr, len(ps), qy.ctypes.data, None, 0)
    assert st == E_ARG  # the first failing frame's status
    for i in range(5):
        if i == 2:
            assert arr[i].status == E_ARG
        else:
            assert arr[i].status == 0 and outs[i][:arr[i].len].tobytes() == G.built("random", 136, 16, 90, 0, 40 + i).jpg


# ---- 7. stage entries ----
@pytest.mark.parametrize("w,h", [(9, 9), (136, 16), (1032, 24)])
@pytest.mark.parametrize("kind", ["random", "photo"])
def test_fdct_quant(enc, w, h, kind):
    y, cb, cr = enc.fdct_quant(G.plane(kind, w, h), quality=90)
    assert cb is None and cr is None
    assert np.array_equal(y, G.built(kind, w, h, 90).coef)


@pytest.mark.parametrize("w,h", [(9, 9), (136, 16), (1032, 24)])
def test_symbol_stats(enc1, w, h):
    b = G.built("photo", w, h, 90)
    counts, first = enc1.symbol_stats(G.plane("photo", w, h), quality=90)
    want, order = G.hist(b)
    assert np.array_equal(counts[:2], want)
    none = np.uint64(0xFFFFFFFFFFFFFFFF)
    for t in range(2):
        present = np.nonzero(want[t])[0]
        # the symbols in order of first occurrence in the text: what the table build consumes
        assert list(present[np.argsort(first[t][present], kind="stable")]) == order[t]
        assert np.all(first[t][want[t] == 0] == none)
    # a DC symbol's key is the block (= text) index of its first occurrence
    for s in set(b.dc_text):
        assert int(first[0][s]) == b.dc_text.index(s)
    # no chroma tables
    assert not counts[2:].any() and np.all(first[2:] == none)


# ---- 8. independent of _gray: the Y plane of the three-component workaround ----
@pytest.mark.parametrize("w,h", [(17, 8), (136, 16), (1032, 24)])
def test_against_yuv444_with_flat_chroma(enc, w, h):
    p = G.plane("photo", w, h)
    info, y, cb, cr = J.decode_coeffs(enc.encode(p, quality=90))
    assert cb is None and cr is None and info.c_blocks == 0 and (info.width, info.height) == (w, h)
    enc.set_input_format(J.JPGE_FMT_YUV444_PLANAR)
    enc.set_subsampling(444)
    c = np.full_like(p, 128)
    info3, y3, cb3, cr3 = J.decode_coeffs(enc.encode(np.stack([p, c, c]), quality=90))
    assert np.array_equal(y, y3) and not cb3.any() and not cr3.any()
    assert bytes(info.qy) == bytes(info3.qy)


# ---- 9. encode_tensor ----
@pytest.mark.parametrize("where", ["device", "host"])
def test_encode_tensor(enc, where):
    w, h = 136, 16
    p = G.plane("photo", w, h)
    want = G.built("photo", w, h, 90).jpg
    enc.set_input_format(J.JPGE_FMT_RGB8_PLANAR, 4096)  # (restored after each call)
    t = torch.from_numpy(p)
    wide = torch.from_numpy(np.ascontiguousarray(np.pad(p, ((0, 0), (0, 21)), constant_values=77)))
    if where == "device":
        t, wide = t.cuda(), wide.cuda()
    view = wide[:, :w]  # a row-strided view
    assert view.stride() == (w + 21, 1)
    for x in (t, view):
        assert enc.encode_tensor(x, quality=90) == want
        assert enc.input_format() == (J.JPGE_FMT_RGB8_PLANAR, 4096)
        out = torch.zeros(J.max_jpeg_bytes(w, h), dtype=torch.uint8, device="cuda")
        n = enc.encode_tensor(x, quality=90, out=out)
        torch.cuda.synchronize()
        assert out[:n].cpu().numpy().tobytes() == want
        assert enc.input_format() == (J.JPGE_FMT_RGB8_PLANAR, 4096)
    with pytest.raises(ValueError):
        enc.encode_tensor(wide[:, ::2], quality=90)  # an inner stride of 2
    with pytest.raises(ValueError):
        enc.encode_tensor(t.to(torch.float32))
    assert enc.input_format() == (J.JPGE_FMT_RGB8_PLANAR, 4096)


# ---- 10. refusals ----
def test_refusals(enc):
    p = G.plane("random", 136, 16)
    with pytest.raises(J.JpgeError) as e:
        enc.set_input_format(GRAY, 4096)  # a plane stride
    assert e.value.status == E_ARG
    assert enc.input_format() == (GRAY, 0)
    out = np.zeros(J.max_jpeg_bytes(136, 16), np.uint8)
    with pytest.raises(J.JpgeError) as e:  # stride < width
        enc.encode_ptr(p.ctypes.data, 136, 16, 135, out.ctypes.data, out.size, 90, flags=0)
    assert e.value.status == E_ARG
    for maxval in (100, 254, 1):
        with pytest.raises(J.JpgeError) as e:
            enc.encode(p, quality=90, maxval=maxval)
        assert e.value.status == E_ARG
        with pytest.raises(J.JpgeError) as e:
            enc.fdct_quant(p, quality=90, maxval=maxval)
        assert e.value.status == E_ARG
    dev = torch.from_numpy(p).cuda()
    with pytest.raises(J.JpgeError) as e:
        enc.stripe_transform(dev.data_ptr(), 136, 136, 16, 0, 1)
    assert e.value.status == E_ARG
    with J.Group([0, 0], lanes=1) as g:
        g.set_input_format(GRAY)
        with pytest.raises(J.JpgeError) as e:
            g.encode_striped(np.zeros((128, 256, 3), np.uint8), quality=90)
        assert e.value.status == E_ARG
    # and the context still encodes
    assert enc.encode(p, quality=90) == G.built("random", 136, 16, 90).jpg


# ---- 11. the other layouts after a gray encode ----
@pytest.mark.parametrize("lanes", [4, 1])
def test_rgb_after_gray(enc, enc1, lanes):
    e = enc if lanes == 4 else enc1
    assert e.encode(G.plane("photo", 136, 16), quality=90) == G.built("photo", 136, 16, 90).jpg
    e.set_input_format(J.JPGE_FMT_RGB8)
    rgb = J.synth_rgb8(77, 96, 64)
    assert e.encode(rgb, quality=90) == _oracle.encode(rgb, 90)
    e.set_subsampling(444)
    assert e.encode(rgb, quality=90) == _oracle.encode(rgb, 90, subsampling=444)
