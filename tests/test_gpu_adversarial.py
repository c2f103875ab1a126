"""The engineered frames of _adversarial.py through the GPU: the statistics kernel's record
writer and the code kernel on four long records side by side (the per-record path of a
group over 64 bits), blocks of 128 records, every zero run across the parts of a block,
and long codes and continuations in the chroma tables.  test_adversarial_cpu.py shows that
the frames hold those streams.  Expected bytes come from _gray.build and _oracle.encode,
expected coefficients and tables from the oracle's primitives, read back through the host
decoder; every comparison is exact."""
import ctypes
import functools
import os

import numpy as np
import pytest

import _adversarial as A
import _gray as G
import _oracle
import _yuv as Y
import jpgenc_amd as J

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GRAY = J.JPGE_FMT_GRAY8
NAMES = list(A.GRAY_FRAMES)          # F1, F1', F2a, F2b, F3
LONG_AND_FULL = ["F1", "F2a", "F2b"]


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


def _where(want: bytes, i: int, b) -> str:
    """The block that byte i of a one-interval gray file belongs to (b: its _gray.Built)."""
    start = want.index(G.SOS) + len(G.SOS)
    if b is None or i < start:
        return "a header byte" if b is not None and i < start else ""
    bit = 8 * (i - start - want[start:i].count(b"\xff\x00"))
    dc, ac = A.lengths(b.dc_text), A.lengths(b.ac_text)
    ends = np.cumsum([sum((dc if k == 0 else ac)[s] + n for k, (s, n, _) in enumerate(blk)) for blk in b.blocks])
    g = int(np.searchsorted(ends, bit, side="right"))
    return f"in block {g} of {len(b.blocks)} (stream bit {bit}; the block starts at bit {int(ends[g - 1]) if g else 0})"


def _check(got: bytes, want: bytes, size, b=None, what=""):
    """got == want, naming the first differing byte (and, for a gray file without restart
    intervals, its block); and the file within max_jpeg_bytes."""
    assert len(got) <= J.max_jpeg_bytes(*size)
    if got != want:
        n = min(len(got), len(want))
        i = next((k for k in range(n) if got[k] != want[k]), n)
        pytest.fail(f"{what}: {len(got)} bytes for {len(want)}, first difference at byte {i} "
                    f"({got[i:i + 4].hex()} for {want[i:i + 4].hex()}) {_where(want, i, b)}")


def _frame(name):
    return A.GRAY_FRAMES[name]()


# ---- 1. whole files ----
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("lanes", [4, 1])
def test_whole_file(enc, enc1, lanes, name):
    e, f, b = (enc if lanes == 4 else enc1), _frame(name), A.built(name)
    _check(e.encode(f.plane, qy=f.qy), b.jpg, f.size, b, name)


def _encoder(lanes=0, **env):
    # (a context reads its switches when it opens: a fresh context under the setting, as
    # test_gpu_gray.py's _encoder)
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
def test_entropy_workgroups_forced(wgs):
    e = _encoder(JPGE_ENTROPY_WGS=wgs)
    try:
        e.set_input_format(GRAY)
        for name in LONG_AND_FULL:
            f, b = _frame(name), A.built(name)
            _check(e.encode(f.plane, qy=f.qy), b.jpg, f.size, b, name)
    finally:
        e.close()


# ---- 2. restart intervals (in blocks) ----
@pytest.mark.parametrize("restart", [1, 7, 5000])
@pytest.mark.parametrize("name", LONG_AND_FULL)
@pytest.mark.parametrize("lanes", [4, 1])
def test_restart(enc, enc1, lanes, name, restart):
    e, f = (enc if lanes == 4 else enc1), _frame(name)
    e.set_restart(restart)
    _check(e.encode(f.plane, qy=f.qy), A.built(name, restart).jpg, f.size, None, f"{name} restart {restart}")


# ---- 3. batches: 5 frames of one size (frame sets form) and one of another ----
def _batch(e, planes, qy):
    outs = [np.zeros(J.max_jpeg_bytes(p.shape[1], p.shape[0]), np.uint8) for p in planes]
    arr = (J.Frame * len(planes))()
    for i, (p, o) in enumerate(zip(planes, outs)):
        arr[i].rgb, arr[i].width, arr[i].height, arr[i].stride = p.ctypes.data, p.shape[1], p.shape[0], p.shape[1]
        arr[i].maxval, arr[i].out, arr[i].cap = 255, o.ctypes.data, o.size
    assert J.lib().jpge_encode_batch(e.ctx, arr, len(planes), qy.ctypes.data, None, 0) == 0
    return [o[:arr[i].len].tobytes() for i, o in enumerate(outs)]


@pytest.mark.parametrize("kind", ["long", "full"])
@pytest.mark.parametrize("lanes", [4, 1])
def test_batch(enc, enc1, lanes, kind):
    e = enc if lanes == 4 else enc1
    if kind == "long":  # step 2: F1 and F1' in turn, F3 between them
        items = [(_frame(n), A.built(n)) for n in ("F1", "F1'", "F1", "F3", "F1'", "F1")]
    else:               # step 1: two F2a frames of other blocks in turn, F2b between them
        items = [(A.f2a(s), A.built("F2a", 0, 0 if s == 21 else s)) for s in (21, 22, 21, 22, 21)]
        items.insert(3, (_frame("F2b"), A.built("F2b")))
    planes = [np.ascontiguousarray(f.plane) for f, _ in items]
    outs = _batch(e, planes, items[0][0].qy)
    for i, (f, b) in enumerate(items):
        _check(outs[i], b.jpg, f.size, b, f"frame {i} ({f.name})")


# ---- 4. stage entries ----
@pytest.mark.parametrize("name", NAMES)
def test_fdct_quant(enc, name):
    f = _frame(name)
    y, cb, cr = enc.fdct_quant(f.plane, qy=f.qy)
    assert cb is None and cr is None
    want = A.built(name).coef
    bad = np.argwhere(y != want)
    assert not len(bad), f"{len(bad)} values differ, the first in block {bad[0][0]} at natural index {bad[0][1]}"


@pytest.mark.parametrize("name", NAMES)
def test_symbol_stats(enc1, name):
    f, b = _frame(name), A.built(name)
    p = np.ascontiguousarray(f.plane)
    counts, first = np.zeros(1024, np.uint32), np.zeros(1024, np.uint64)
    st = J.lib().jpge_symbol_stats(enc1.ctx, p.ctypes.data, p.shape[1], p.shape[0], p.shape[1], 255, f.qy.ctypes.data,
                                   None, counts.ctypes.data, first.ctypes.data, 0)
    assert st == 0
    counts, first = counts.reshape(4, 256), first.reshape(4, 256)
    want, order = G.hist(b)
    assert np.array_equal(counts[:2], want)
    none = np.uint64(0xFFFFFFFFFFFFFFFF)
    for t in range(2):
        present = np.nonzero(want[t])[0]
        assert list(present[np.argsort(first[t][present], kind="stable")]) == order[t]
        assert np.all(first[t][want[t] == 0] == none)
    assert not counts[2:].any() and np.all(first[2:] == none)


# ---- 5. the same planes as R = G = B frames: the 6-block and the 1-block MCU ----
# (test_adversarial_cpu.py: the oracle's table 1 still holds the F1 and F2 properties)
@functools.lru_cache(maxsize=None)
def _rgb_want(name, mode):
    f = _frame(name)
    return _oracle.encode(A.rgb(f.plane), qy=f.qy, qc=f.qy, subsampling=mode)


@pytest.mark.parametrize("mode", [420, 444])
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("lanes", [4, 1])
def test_rgb(enc, enc1, lanes, name, mode):
    e, f = (enc if lanes == 4 else enc1), _frame(name)
    rgb = A.rgb(f.plane)
    e.set_input_format(J.JPGE_FMT_RGB8)
    e.set_subsampling(mode)
    _check(e.encode(rgb, qy=f.qy, qc=f.qy), _rgb_want(name, mode), f.size, None, f"{name} as RGB at {mode}")


# ---- 6. the chroma tables ----
def _dht_tables(jpg: bytes) -> dict:
    """info byte -> (the 16 counts, the symbols) of every table of the file's DHT segments"""
    out, i = {}, 2
    while jpg[i + 1] != 0xDA:
        assert jpg[i] == 0xFF
        n = (jpg[i + 2] << 8) | jpg[i + 3]
        if jpg[i + 1] == 0xC4:
            k = i + 4
            while k < i + 2 + n:
                cnt = jpg[k + 1:k + 17]
                out[jpg[k]] = (bytes(cnt), bytes(jpg[k + 17:k + 17 + sum(cnt)]))
                k += 17 + sum(cnt)
        i += 2 + n
    return out


def _dht_of(text):
    seg = G._dht(0, _oracle.huffman(text))
    return bytes(seg[5:21]), bytes(seg[21:])


def _planes_jpg(e, planes, w, h, qy, qc):
    """jpge_encode_planes (4:2:0) of three fp64 planes with tables given"""
    ins = [np.ascontiguousarray(p, np.float64) for p in planes]
    rows, cols = ins[0].shape
    out = np.empty(J.max_jpeg_bytes(cols, rows), np.uint8)
    n = ctypes.c_size_t()
    st = J.lib().jpge_encode_planes(e.ctx, *[p.ctypes.data for p in ins], rows, cols, J.JPGE_TO_YCBCR, w, h,
                                    qy.ctypes.data, qc.ctypes.data, out.ctypes.data, out.size, ctypes.byref(n), 0)
    assert st == 0
    return out[:n.value].tobytes()


@pytest.mark.parametrize("name", ["F4", "F4full"])
@pytest.mark.parametrize("lanes", [4, 1])
def test_chroma_444(enc, enc1, lanes, name):
    e = enc if lanes == 4 else enc1
    f, c = {"F4": A.f4, "F4full": A.f4full}[name](), A.chroma(name)
    w, h = f.size
    e.set_input_format(J.JPGE_FMT_YUV444_PLANAR)
    e.set_subsampling(444)
    jpg = e.encode(f.frame, qy=f.qy, qc=f.qc)
    assert len(jpg) <= J.max_jpeg_bytes(w, h)
    # the host decoder (independent of the code kernel) reads the oracle's coefficients back
    info, y, cb, cr = J.decode_coeffs(jpg)
    assert (info.width, info.height, info.yh, info.yv) == (w, h, 1, 1)
    assert not y.any() and np.array_equal(cb, c.cb.coef) and np.array_equal(cr, c.cr.coef)
    # tables 2 and 3 are the oracle's tables of the chroma texts
    dht = _dht_tables(jpg)
    assert dht[0x01] == _dht_of(c.dc_text) and dht[0x11] == _dht_of(c.ac_text)
    assert dht[0x00] == _dht_of([0] * (w // 8 * (h // 8))) and dht[0x10] == _dht_of([0] * (w // 8 * (h // 8)))
    # and the stage entry's coefficients
    got = e.fdct_quant(f.frame, qy=f.qy, qc=f.qc)
    assert not got[0].any() and np.array_equal(got[1], c.cb.coef) and np.array_equal(got[2], c.cr.coef)


@pytest.mark.parametrize("name", ["F4", "F4full"])
def test_chroma_420_against_encode_planes(enc, enc1, name):
    """jpge_encode_planes codes 4:2:0 only: each chroma sample repeated 2x2 under a flat
    192x128 Y plane, so the 4:2:0 chroma planes are the frame's own (test_adversarial_cpu.py)
    and tables 2 and 3 hold the same texts, now in 6-block MCUs."""
    f, c = {"F4": A.f4, "F4full": A.f4full}[name](), A.chroma(name)
    up = [np.full((128, 192), 128, np.uint8)] + [np.repeat(np.repeat(p, 2, 0), 2, 1) for p in f.planes[1:]]
    enc.set_input_format(J.JPGE_FMT_YUV444_PLANAR)
    jpg = enc.encode(np.ascontiguousarray(np.stack(up)), qy=f.qy, qc=f.qc)
    want = _planes_jpg(enc1, Y.pad_planes(Y.YUV444, *up), 192, 128, f.qy, f.qc)
    _check(jpg, want, (192, 128), None, f"{name} at 4:2:0")
    info, y, cb, cr = J.decode_coeffs(jpg)
    assert np.array_equal(cb, c.cb.coef) and np.array_equal(cr, c.cr.coef)
    dht = _dht_tables(jpg)
    assert dht[0x01] == _dht_of(c.dc_text) and dht[0x11] == _dht_of(c.ac_text)


# ---- 7. the output bound ----
def test_device_buffer_of_exactly_the_bound(enc):
    f, b = A.f2a(), A.built("F2a")
    w, h = f.size
    cap = J.max_jpeg_bytes(w, h)
    assert len(b.jpg) <= cap
    dev = torch.from_numpy(np.ascontiguousarray(f.plane)).cuda()
    out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    n = ctypes.c_size_t()
    st = J.lib().jpge_encode_rgb8(enc.ctx, dev.data_ptr(), w, h, w, 255, f.qy.ctypes.data, None, out.data_ptr(), cap,
                                  ctypes.byref(n), J.JPGE_DEVICE_INPUT | J.JPGE_DEVICE_OUTPUT)
    assert st == 0
    torch.cuda.synchronize()
    _check(out[:n.value].cpu().numpy().tobytes(), b.jpg, f.size, b, "F2a into a device buffer")
