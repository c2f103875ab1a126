"""Box downscale inside K1 (jpge_set_downscale): the .jpg of a frame coded with factor s is,
byte for byte, the .jpg of D = downscale_frame(frame) coded with factor 1 in the same layout
(the same context type), and the oracle's bytes of D (the RGB layouts: _oracle.encode of D's
R, G, B; NV12: Encoder.encode_planes on a separate context, pinned to the oracle by
test_gpu_planes.py).  D comes from jpge_downscale_frame, which test_downscale_cpu.py pins to
the numpy rule.  Every comparison is exact."""
import functools
import os
import subprocess

import numpy as np
import pytest

import _downscale as D
import _oracle
import _yuv as Y
import jpgenc_amd as J

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FMT = pytest.mark.parametrize("fmt", D.FORMATS, ids=[D.NAMES[f] for f in D.FORMATS])
S = pytest.mark.parametrize("s", D.FACTORS)
VARIANTS = ("host", "aligned", "unaligned", "padded")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sizes(s):
    """Source sizes: a tile is 64 x 16 output pixels, 64s x 16s source pixels."""
    out = [(1, 1), (16 * s, 16 * s), (64 * s, 16 * s), (64 * s + 16 * s + 3, 16 * s + 5), (517, 131)]
    out += [(80 * s - r, 32 * s - r) for r in range(1, s)]  # dw * s exceeds W by 1 .. s - 1, both ways
    return out


CASES = [(s, w, h) for s in D.FACTORS for (w, h) in sizes(s)]


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
    """The context of NV12's expectations (encode_planes)."""
    e = J.Encoder(0, lanes=1)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def _defaults(enc, enc1):
    yield
    for e in (enc, enc1):
        e.set_downscale(1)
        e.set_input_format(J.JPGE_FMT_RGB8)
        e.set_subsampling(420)
        e.set_restart(0)
        e.set_huffman(J.JPGE_HUFF_OPTIMAL)
        e.set_yuv_transform(J.JPGE_YUV_FULL_601)


POISON = 0xC3


def _device_view(frame, fmt, variant):
    """The frame in device memory: tensors for encode_tensor (RGB layouts) or encode_tensor_yuv
    (NV12).  aligned: a 16-byte aligned base and pitch; unaligned: base + 1 and an odd pitch;
    padded: an aligned pitch a row's bytes + 16 and more.  The bytes around the rows are poison."""
    if fmt == D.NV12:
        w, h = frame.width, frame.height
        y, c = D.split_nv12(frame)
        ch, cw = (h + 1) // 2, (w + 1) // 2
        row = 2 * cw
    else:
        h, w, bpp = frame.shape
        row = w * bpp
    al = -(-row // 16) * 16
    off, st = {"aligned": (0, al), "unaligned": (1, al + 17), "padded": (0, al + 48)}[variant]
    rows = h + (ch + 3 if fmt == D.NV12 else 0)
    host = np.full(off + st * rows + 64, POISON, np.uint8)
    body = host[off:off + st * rows].reshape(rows, st)
    if fmt == D.NV12:
        body[:h, :w] = y
        body[h + 3:h + 3 + ch, :row] = c.reshape(ch, row)  # (the Cb,Cr plane 3 rows of poison after the Y plane)
    else:
        body[:h, :row] = np.asarray(frame).reshape(h, row)
    dev = torch.from_numpy(host).cuda()
    if fmt == D.NV12:
        ty = torch.as_strided(dev, (h, w), (st, 1), off)
        tc = torch.as_strided(dev, (ch, cw, 2), (st, 2, 1), off + st * (h + 3))
        return ty, tc
    return (torch.as_strided(dev, (h, w, bpp), (st, bpp, 1), off),)


def _encode(e, frame, fmt, variant, quality=90, maxval=255):
    """One frame through context e with its current settings (the layout set here)."""
    if variant == "host":
        e.set_input_format(fmt)
        return e.encode(frame, quality, maxval)
    t = _device_view(frame, fmt, variant)
    if fmt == D.NV12:
        return e.encode_tensor_yuv(t[0], t[1], quality=quality)
    return e.encode_tensor(t[0], quality, order="bgr" if fmt in (D.BGR8, D.BGRA8) else "rgb", maxval=maxval)


def _oracle_bytes(ref, d, fmt, quality=90, **kw):
    if fmt == D.NV12:
        assert not kw
        f, y, cb, cr = D.nv12_planes(d)
        return ref.encode_planes(*Y.pad_planes(f, y, cb, cr), d.width, d.height, J.JPGE_TO_YCBCR, quality)
    return _oracle.encode(D.to_rgb(d, fmt), quality, **kw)


def _check(e, ref, frame, fmt, s, variant, quality=90):
    d = J.downscale_frame(frame, fmt, s)
    e.set_downscale(s)
    got = _encode(e, frame, fmt, variant, quality)
    e.set_downscale(1)
    assert got == _encode(e, d, fmt, "host", quality), "differs from the factor-1 encode of D"
    assert got == _oracle_bytes(ref, d, fmt, quality), "differs from the oracle's bytes of D"


# ---- 1. sizes x layouts x paths, random bytes ----
@FMT
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("s,w,h", CASES)
def test_sizes(enc, ref, fmt, s, w, h, variant):
    _check(enc, ref, D.make(fmt, w, h, "random", 1), fmt, s, variant)


# ---- 2. values at the bounds of the packed sums ----
@FMT
@S
@pytest.mark.parametrize("kind", ["tie", "below", "ones"])
@pytest.mark.parametrize("variant", ["aligned", "unaligned"])
def test_values(enc, ref, fmt, s, kind, variant):
    _check(enc, ref, D.make(fmt, 64 * s + 16 * s + 3, 16 * s + 5, kind, 2, s), fmt, s, variant)


# ---- 3. settings ----
@pytest.mark.parametrize("mode", [420, 4200, 4201, 444, 422, 411])
@pytest.mark.parametrize("variant", ["aligned", "unaligned"])
def test_subsampling_modes(enc, mode, variant):
    src = D.make(D.RGB8, 2 * 136 + 5, 2 * 24 + 3, "random", 3)
    d = J.downscale_frame(src, D.RGB8, 2)
    enc.set_subsampling(mode)
    enc.set_downscale(2)
    got = _encode(enc, src, D.RGB8, variant)
    enc.set_downscale(1)
    assert got == _encode(enc, d, D.RGB8, "host")
    assert got == _oracle.encode(d, 90, subsampling=mode)


@S
@pytest.mark.parametrize("fmt", [D.RGB8, D.BGRA8], ids=["rgb8", "bgra8"])
@pytest.mark.parametrize("mode", [444, 411])
def test_row8_kernels_other_layouts(enc, fmt, s, mode):
    src = D.make(fmt, 136 * s + 3, 24 * s + 1, "random", 4)
    d = J.downscale_frame(src, fmt, s)
    enc.set_subsampling(mode)
    enc.set_downscale(s)
    got = _encode(enc, src, fmt, "aligned")
    assert got == _oracle.encode(D.to_rgb(d, fmt), 90, subsampling=mode)


@S
def test_maxval(enc, s):
    """maxval 100: the RGB scaling applies to D's samples."""
    src = (D.make(D.RGB8, 80 * s + 3, 16 * s + 5, "random", 5).astype(np.uint32) * 100 // 255).astype(np.uint8)
    d = J.downscale_frame(src, D.RGB8, s)
    enc.set_downscale(s)
    got = _encode(enc, src, D.RGB8, "aligned", maxval=100)
    enc.set_downscale(1)
    assert got == _encode(enc, d, D.RGB8, "host", maxval=100)
    assert got == _oracle.encode(d, 90, maxval=100)


@S
def test_restart_interval(enc, s):
    src = D.make(D.RGB8, 80 * s + 3, 32 * s + 5, "random", 6)
    d = J.downscale_frame(src, D.RGB8, s)
    enc.set_restart(3)
    enc.set_downscale(s)
    got = _encode(enc, src, D.RGB8, "aligned")
    assert got == _oracle.encode(d, 90, restart=3)


@S
@pytest.mark.parametrize("fmt", [D.RGB8, D.NV12], ids=["rgb8", "nv12"])
def test_standard_huffman(enc, fmt, s):
    src = D.make(fmt, 80 * s + 3, 32 * s + 5, "random", 7)
    d = J.downscale_frame(src, fmt, s)
    enc.set_huffman(J.JPGE_HUFF_STANDARD)
    enc.set_downscale(s)
    got = _encode(enc, src, fmt, "aligned")
    enc.set_downscale(1)
    assert got == _encode(enc, d, fmt, "host")


@S
def test_nv12_limited_709(enc, s):
    """The sample transform applies to D's samples."""
    src = D.make(D.NV12, 80 * s + 3, 32 * s + 5, "random", 8)
    d = J.downscale_frame(src, D.NV12, s)
    enc.set_yuv_transform(J.JPGE_YUV_LIMITED_709)
    enc.set_downscale(s)
    got = {v: _encode(enc, src, D.NV12, v) for v in ("host", "unaligned")}
    enc.set_downscale(1)
    want = _encode(enc, d, D.NV12, "host")
    assert got["host"] == want and got["unaligned"] == want


@FMT
@S
def test_one_lane(enc1, ref, fmt, s):
    _check(enc1, ref, D.make(fmt, 64 * s + 16 * s + 3, 16 * s + 5, "random", 9), fmt, s, "aligned")
    _check(enc1, ref, D.make(fmt, 64 * s + 16 * s + 3, 16 * s + 5, "random", 9), fmt, s, "host")


# ---- 4. batches ----
@functools.lru_cache(maxsize=None)
def _batch_frames(fmt, w, h, n):
    return tuple(D.make(fmt, w, h, "random", 100 + i) for i in range(n))


@pytest.mark.parametrize("fmt", [D.RGB8, D.NV12], ids=["rgb8", "nv12"])
def test_batch_sets_and_factor_changes(enc, ref, fmt):
    """9 frames of one geometry (sets of 4, 4 and 1), the factor changed between batches on one
    context, 2 -> 4 -> 1: each batch is that of its own factor, and factor 1 afterwards gives
    the bytes of a fresh context."""
    frames = list(_batch_frames(fmt, 333, 77, 9))
    enc.set_input_format(fmt)
    for s in (2, 4, 1):
        enc.set_downscale(s)
        got = enc.encode_batch(frames, 90)
        for i, f in enumerate(frames):
            assert got[i] == _oracle_bytes(ref, J.downscale_frame(f, fmt, s), fmt), (s, i)
    with J.Encoder(0) as fresh:
        fresh.set_input_format(fmt)
        assert enc.encode_batch(frames, 90) == fresh.encode_batch(frames, 90)


def test_device_input_and_output(enc1):
    src = D.make(D.RGB8, 517, 131, "random", 10)
    d = J.downscale_frame(src, D.RGB8, 2)
    t = torch.from_numpy(src).cuda()
    out = torch.zeros(J.max_jpeg_bytes(*J.downscaled_size(517, 131, 2)), dtype=torch.uint8, device="cuda")
    enc1.set_downscale(2)
    n = enc1.encode_tensor(t, 90, out=out)
    assert out[:n].cpu().numpy().tobytes() == _oracle.encode(d, 90)


# ---- 5. stage entries ----
@FMT
@S
def test_stage_entries(enc, fmt, s):
    """fdct_quant and symbol_stats return D's planes and histograms."""
    src = D.make(fmt, 80 * s + 3, 16 * s + 5, "random", 11)
    d = J.downscale_frame(src, fmt, s)
    enc.set_input_format(fmt)
    enc.set_downscale(s)
    coef, hist = enc.fdct_quant(src, 90), enc.symbol_stats(src, 90)
    enc.set_downscale(1)
    wcoef, whist = enc.fdct_quant(d, 90), enc.symbol_stats(d, 90)
    assert all(np.array_equal(a, b) for a, b in zip(coef, wcoef))
    assert all(np.array_equal(a, b) for a, b in zip(hist, whist))
    if fmt == D.RGB8:
        assert all(np.array_equal(a, b) for a, b in zip(coef, _oracle.stage_coeffs(d, 90)))


# ---- 6. groups ----
def test_group_batch_on_a_repeated_device(ref):
    frames = [D.make(D.RGB8, 200, 90, "random", 20 + i) for i in range(5)]
    with J.Group([0, 0], lanes=1) as g:
        g.set_downscale(2)
        got = g.encode_batch(frames, 90)
        for f, b in zip(frames, got):
            assert b == _oracle.encode(J.downscale_frame(f, D.RGB8, 2), 90)
        with pytest.raises(J.JpgeError) as e:
            g.encode_striped(frames[0], 90)
        assert e.value.status == 1
        g.set_downscale(1)
        assert g.encode_striped(frames[0], 90) == _oracle.encode(frames[0], 90)


# ---- 7. refusals ----
@pytest.mark.parametrize("fmt", [J.JPGE_FMT_RGB8_PLANAR, J.JPGE_FMT_GRAY8, J.JPGE_FMT_I420, J.JPGE_FMT_YUV444_PLANAR,
                                 J.JPGE_FMT_YUYV, J.JPGE_FMT_UYVY, J.JPGE_FMT_NV16, J.JPGE_FMT_I422, J.JPGE_FMT_P010,
                                 J.JPGE_FMT_I010])
def test_unsupported_layouts_refuse(enc, fmt):
    """Each layout without a downscaling kernel: the argument error, for the single call, the
    stage entries and as a batch frame's status; the same call passes at factor 1."""
    buf = torch.zeros(64 * 64 * 4, dtype=torch.uint8, device="cuda")
    qy, qc = J.quality_tables(90)
    out = torch.zeros(J.max_jpeg_bytes(32, 32), dtype=torch.uint8, device="cuda")
    enc.set_input_format(fmt)
    stride = {J.JPGE_FMT_YUYV: 64, J.JPGE_FMT_UYVY: 64, J.JPGE_FMT_P010: 64, J.JPGE_FMT_I010: 64}.get(fmt, 32)
    if fmt in (J.JPGE_FMT_P010, J.JPGE_FMT_I010):
        enc.set_yuv_transform(J.JPGE_YUV_FULL_601)
    enc.set_downscale(2)
    with pytest.raises(J.JpgeError) as e:
        enc.encode_ptr(buf.data_ptr(), 32, 32, stride, out.data_ptr(), out.numel(), 90)
    assert e.value.status == 1
    with pytest.raises(J.JpgeError):
        enc.encode_batch_dev([(buf.data_ptr(), 32, 32, stride)] * 2, [(out.data_ptr(), out.numel())] * 2, 90)
    assert enc.batch_status() == [1, 1]
    enc.set_downscale(1)
    assert enc.encode_ptr(buf.data_ptr(), 32, 32, stride, out.data_ptr(), out.numel(), 90) > 0


def test_nv12_outside_s420m_refuses(enc):
    src = D.make(D.NV12, 64, 32, "random", 30)
    enc.set_input_format(D.NV12)
    enc.set_downscale(2)
    for mode in (444, 422, 411, 4200, 4201):
        enc.set_subsampling(mode)
        with pytest.raises(J.JpgeError) as e:
            enc.encode(src, 90)
        assert e.value.status == 1
    enc.set_subsampling(420)
    assert len(enc.encode(src, 90)) > 0


def test_stripes_refuse(enc1):
    t = torch.zeros((64, 64, 3), dtype=torch.uint8, device="cuda")
    enc1.set_downscale(2)
    with pytest.raises(J.JpgeError) as e:
        enc1.stripe_transform(t.data_ptr(), 64 * 3, 64, 64, 0, 4, 90)
    assert e.value.status == 1
    enc1.set_downscale(1)
    assert len(enc1.stripe_transform(t.data_ptr(), 64 * 3, 64, 64, 0, 4, 90)) == 3


def test_setter_refuses_other_factors(enc):
    enc.set_downscale(4)
    for bad in (0, 3, 8, -1):
        with pytest.raises(J.JpgeError) as e:
            enc.set_downscale(bad)
        assert e.value.status == 1
        assert enc.downscale == 4
    enc.set_input_format(J.JPGE_FMT_I420)  # (the setter takes a factor whatever the layout)
    enc.set_downscale(2)
    assert enc.downscale == 2


# ---- 8. the limit ----
def test_widest_source(enc1):
    """A source row of 65535 pixels, 16s + 1 rows, s = 2: the source's limits hold, SOF0 has D's size."""
    w, h = 65535, 33
    rng = np.random.default_rng(40)
    src = np.repeat(rng.integers(0, 256, (h, w // 16 + 1, 3), dtype=np.uint8), 16, axis=1)[:, :w].copy()
    d = J.downscale_frame(src, D.RGB8, 2)
    assert d.shape == (17, 32768, 3)
    enc1.set_downscale(2)
    got = enc1.encode(src, 90)
    enc1.set_downscale(1)
    assert got == enc1.encode(d, 90)


# ---- 9. the command line ----
def test_cli_downscale(enc1, tmp_path):
    src = D.make(D.RGB8, 203, 77, "random", 50)
    ppm, jpg = tmp_path / "in.ppm", tmp_path / "out.jpg"
    ppm.write_bytes(b"P6\n203 77\n255\n" + src.tobytes())
    exe = os.path.join(ROOT, "jpgenc_amd", "bin", "jpgenc")
    r = subprocess.run([exe, "--downscale", "2", "-q", "90", str(ppm), str(jpg)], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert jpg.read_bytes() == enc1.encode(J.downscale_frame(src, D.RGB8, 2), 90)
    r = subprocess.run([exe, "--downscale", "2", "--gpus", "1", str(ppm), str(jpg)], capture_output=True, timeout=120)
    assert r.returncode == 1
    r = subprocess.run([exe, "--downscale", "3", str(ppm), str(jpg)], capture_output=True, timeout=120)
    assert r.returncode == 1
    enc1.set_downscale(4)  # the PPM entries honour the context's factor
    out = tmp_path / "f.jpg"
    enc1.encode_file(str(ppm), str(out), 90)
    enc1.set_downscale(1)
    assert out.read_bytes() == enc1.encode(J.downscale_frame(src, D.RGB8, 4), 90)
