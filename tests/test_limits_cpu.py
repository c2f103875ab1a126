"""The reference side of the limit tests, without a GPU: the oracle's whole-frame entries, the
host decoder, the PPM reader and the Python layout helpers at the 65535-pixel limit
(_limits.LIMIT_SHAPES), and _limits' strided builders against the row-by-row ones they
replace.  test_gpu_limits.py compares the GPU with what is pinned here."""
import io

import numpy as np
import pytest

import _formats as F
import _limits as L
import _oracle
import _yuv as Y
import _yuv422 as Z
import jpgenc_amd as J

SHAPES = pytest.mark.parametrize("w,h", L.LIMIT_SHAPES, ids=L.ids(L.LIMIT_SHAPES))
LONG = pytest.mark.parametrize("w,h", L.LONG, ids=L.ids(L.LONG))
MODE = pytest.mark.parametrize("mode", L.MODES)


# ---- 1. the oracle's generic path equals its pinned 4:2:0 and 4:4:4 paths ----
@SHAPES
@pytest.mark.parametrize("kind", ["photo", "random"])
def test_generic_path_equals_the_pinned_paths(w, h, kind):
    rgb = L.frame(kind, w, h)
    assert _oracle.encode(rgb, 90, generic=True) == _oracle.encode(rgb, 90)
    assert _oracle.encode(rgb, 90, subsampling=444, generic=True) == L.want(kind, w, h, 90, 444)
    for got, wanted in zip(_oracle.stage_coeffs_mode(rgb, 420, 90), _oracle.stage_coeffs(rgb, 90)):
        assert np.array_equal(got, wanted)
    for got, wanted in zip(_oracle.stage_coeffs_mode(rgb, 444, 90), _oracle.stage_coeffs444(rgb, 90)):
        assert np.array_equal(got, wanted)


def test_restart_variant_equals_the_generic_path():
    for w, h in L.LONG:
        rgb = L.frame("photo", w, h)
        for r in L.restarts(w, h, 420):
            assert _oracle.encode(rgb, 90, restart=r, generic=True) == L.want("photo", w, h, 90, 420, r), (w, h, r)


# ---- 2. the host decoder returns every stream's coefficients ----
def _decodes_to(jpg, w, h, mode, restart, coeffs):
    info, y, cb, cr = J.decode_coeffs(jpg)
    assert (info.width, info.height, info.restart) == (w, h, restart)
    assert (info.yh, info.yv) == _oracle.SHAPES[mode]
    assert L.same((y, cb, cr), coeffs)


@MODE
@SHAPES
def test_decode_coeffs_of_the_oracle_stream(w, h, mode):
    kind = "random" if (w, h) in L.LONG else "photo"
    _decodes_to(L.want(kind, w, h, 90, mode), w, h, mode, 0, L.want_coeffs(kind, w, h, 90, mode))


@MODE
@LONG
def test_decode_coeffs_with_restart_intervals(w, h, mode):
    rs = L.restarts(w, h, mode)
    assert {1, L.mcus(w, h, mode)[0], 65535} <= set(rs)
    for r in rs:
        jpg = L.want("photo", w, h, 90, mode, r)
        _decodes_to(jpg, w, h, mode, r, L.want_coeffs("photo", w, h, 90, mode))
    # R = 1: one segment per MCU, RSTn cycling mod 8 (markers cannot occur inside stuffed data)
    mw, mh = L.mcus(w, h, mode)
    one = L.want("photo", w, h, 90, mode, 1)
    sos = one.index(b"\xff\xda")
    marks = [one[i + 1] for i in range(sos + 2, len(one) - 2) if one[i] == 0xFF and 0xD0 <= one[i + 1] <= 0xD7]
    assert marks == [0xD0 + (k & 7) for k in range(mw * mh - 1)]


def test_decode_coeffs_with_more_than_65535_segments():
    w, h = L.MANY_SEGMENTS
    assert np.prod(L.mcus(w, h, 444)) == 73728
    _decodes_to(L.want("photo", w, h, 90, 444, 1), w, h, 444, 1, L.want_coeffs("photo", w, h, 90, 444))


def test_restart_helper():
    for w, h in L.LONG:
        for mode in L.MODES:
            mw, mh = L.mcus(w, h, mode)
            rs = L.restarts(w, h, mode)
            assert 1 in rs and mw in rs and 65535 in rs
            assert any((mw % r if mw > 1 else (mw * mh) % r) for r in rs)
    assert L.mcus(65535, 17, 444) == (8192, 3) and L.mcus(17, 65535, 444) == (3, 8192)
    assert L.mcus(65535, 17, 411) == (2048, 3) and L.mcus(17, 65535, 420) == (2, 4096)


# ---- 3. Pillow: up to its own limit ----
@MODE
@pytest.mark.parametrize("w,h", [(65500, 33), (33, 65500)], ids=["65500x33", "33x65500"])
def test_pillow_decodes_its_largest_frame(w, h, mode):
    Image = pytest.importorskip("PIL.Image")
    assert max(w, h) == L.PILLOW_MAX
    im = Image.open(io.BytesIO(L.want("photo", w, h, 90, mode)))
    im.load()
    assert im.size == (w, h) and im.mode == "RGB"
    got = np.asarray(im).astype(np.int32)
    assert got.shape == (h, w, 3)
    # (a decode of the right picture, not a measure of quality: Q90 chroma-subsampled)
    assert np.abs(got - L.frame("photo", w, h).astype(np.int32)).mean() < 8


@pytest.mark.parametrize("w,h", [(65520, 1), (1, 65520), (65535, 1), (1, 65535)])
def test_pillow_refuses_above_its_limit(w, h):
    """Pillow 12.2.0 (libjpeg's 65500-pixel dimension limit) answers "broken data stream" to a
    frame of 65520 pixels or more in either dimension.  That is Pillow's limit, not a property
    of these bytes: the streams decode with decode_coeffs (above), which is the decode-side
    check past 65500.  A Pillow that decodes them passes too."""
    Image = pytest.importorskip("PIL.Image")
    jpg = L.want("photo", w, h, 90, 444)
    try:
        im = Image.open(io.BytesIO(jpg))
        im.load()
    except OSError:
        return
    assert im.size == (w, h)


# ---- 4. the PPM reader ----
@pytest.mark.parametrize("w,h", [(65535, 1), (1, 65535)])
@pytest.mark.parametrize("magic", ["P6", "P3"])
def test_ppm_at_the_limit(w, h, magic):
    rgb = L.frame("random", w, h)
    head = f"{magic}\n{w} {h}\n255\n".encode()
    data = head + (rgb.tobytes() if magic == "P6" else " ".join(map(str, rgb.reshape(-1).tolist())).encode() + b"\n")
    buf = np.frombuffer(data, np.uint8)
    import ctypes
    gw, gh, mv = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_int()
    assert J.lib().jpge_ppm_info(buf.ctypes.data, buf.size, ctypes.byref(gw), ctypes.byref(gh), ctypes.byref(mv)) == 0
    assert (gw.value, gh.value, mv.value) == (w, h, 255)
    img = J.parse_ppm(data)
    assert (img.width, img.height, img.maxval) == (w, h, 255) and np.array_equal(img.rgb, rgb)
    st, samples, maxval = _oracle.parse_ppm(data)  # and the oracle's reader agrees
    assert st == 0 and maxval == 255 and np.array_equal(samples, rgb)


@pytest.mark.parametrize("w,h", [(65536, 1), (1, 65536), (0, 1), (1, 0)])
def test_ppm_past_the_limit_is_refused(w, h):
    with pytest.raises(J.JpgeError) as e:
        J.parse_ppm(f"P6\n{w} {h}\n255\n".encode() + bytes(3 * min(w * h, 65536)))
    assert J.STATUS[e.value.status] == "JPGE_E_FORMAT"


# ---- 5. the Python layout helpers ----
@pytest.mark.parametrize("w,h", [(0, 4), (4, 0), (65536, 1), (1, 65536)])
def test_frame_geom_refuses_sizes_outside_1_to_65535(w, h):
    for fmt, shape in ((J.JPGE_FMT_RGB8, (h, w, 3)), (J.JPGE_FMT_BGRA8, (h, w, 4)), (J.JPGE_FMT_RGB8_PLANAR, (3, h, w)),
                       (J.JPGE_FMT_YUV444_PLANAR, (3, h, w)), (J.JPGE_FMT_GRAY8, (h, w))):
        with pytest.raises(ValueError):
            J._frame_geom(np.zeros(shape, np.uint8), fmt)
        with pytest.raises(ValueError):
            J._as_frame(np.zeros(shape, np.uint8), fmt)
    if w * h:  # (the packers refuse an empty Y plane themselves, with the same error type)
        y = np.zeros((h, w), np.uint8)
        for fmt in Y.HALF:
            c = np.zeros(Y.chroma_shape(fmt, w, h), np.uint8)
            with pytest.raises(ValueError):
                J._frame_geom(J.pack_yuv420(fmt, y, c, c)[0], fmt)
        for fmt in Z.FORMATS:
            c = np.zeros((h, Z.cw_of(w)), np.uint8)
            with pytest.raises(ValueError):
                J._frame_geom(J.pack_yuv422(fmt, y, c, c)[0], fmt)
    else:
        for pack, fmt in ((J.pack_yuv420, Y.NV12), (J.pack_yuv422, Z.YUYV)):
            with pytest.raises(ValueError):
                pack(fmt, np.zeros((h, w), np.uint8), np.zeros((0, 0), np.uint8), np.zeros((0, 0), np.uint8))


@pytest.mark.parametrize("w,h", [(65535, 1), (1, 65535)])
def test_frame_geom_at_the_limit(w, h):
    assert J._frame_geom(np.zeros((h, w, 3), np.uint8), J.JPGE_FMT_RGB8) == (w, h, 3 * w)
    assert J._frame_geom(np.zeros((h, w, 4), np.uint8), J.JPGE_FMT_RGBA8) == (w, h, 4 * w)
    assert J._frame_geom(np.zeros((3, h, w), np.uint8), J.JPGE_FMT_RGB8_PLANAR) == (w, h, w)
    assert J._frame_geom(np.zeros((h, w), np.uint8), J.JPGE_FMT_GRAY8) == (w, h, w)
    y, cb, cr = Y.samples(Y.NV12, 1, w, h)
    cw = (w + 1) // 2
    for fmt, stride in ((Y.NV12, 2 * cw), (Y.I420, w)):
        f = J.pack_yuv420(fmt, y, cb, cr)[0]
        assert J._frame_geom(f, fmt) == (w, h, stride)
        assert L.same(Y.split(fmt, f, w, h), (y, cb, cr))
    y, cb, cr = Z.samples(1, w, h)
    for fmt in Z.FORMATS:
        f = J.pack_yuv422(fmt, y, cb, cr)[0]
        assert J._frame_geom(f, fmt) == (w, h, Z.least_stride(fmt, w))
    assert J.max_jpeg_bytes(w, h) >= len(L.want("random", w, h, 100, 444))


# ---- 6. _limits' strided builders equal the row-by-row ones ----
@pytest.mark.parametrize("w,h", [(33, 17), (48, 40), (1, 9)])
def test_strided_builders(w, h):
    rgb = L.frame("random", w, h, seed=3)
    for fmt in F.ALL_FORMATS:
        a = F.to_format(rgb, fmt)
        row = w * J.input_format_info(fmt)[0]
        for stride, ps, off in ((row + 5, 0, 3), ((row + 15) // 16 * 16 + 16, 0, 32)):
            ps = (stride * h + 7) if fmt == J.JPGE_FMT_RGB8_PLANAR and off == 3 else ps
            got, wanted = L.padded(a, fmt, stride, ps, off), F.padded(a, fmt, stride, ps, off)
            assert np.array_equal(got[0], wanted[0]) and got[1:] == wanted[1:]
    for fmt in Y.FORMATS:
        p = Y.samples(fmt, 5, w, h)
        for stride, ps, off in ((w + 25, (w + 25) * h + 37, 1), (64, 64 * h + 48, 32), (0, 0, 0)):
            got, wanted = L.yuv_raw(fmt, *p, stride, ps, off), Y.raw(fmt, *p, stride, ps, off)
            assert np.array_equal(got[0], wanted[0]) and got[1:] == wanted[1:]
    p = Z.samples(6, w, h)
    for fmt in Z.FORMATS:
        least = Z.least_stride(fmt, w)
        for stride, off in ((least + 25 + least % 2, 1), (-(-least // 32) * 32 + 32, 32), (0, 0)):
            ps = 0 if fmt in Z.PACKED or not stride else stride * h + 37
            got, wanted = L.yuv422_raw(fmt, *p, stride, ps, off), Z.raw(fmt, *p, stride, ps, off)
            assert np.array_equal(got[0], wanted[0]) and got[1:] == wanted[1:]
            s = got[1]
            assert L.same(Z.split(fmt, got[0], w, h, s, got[2], off), p)


def test_rgb_planes_are_the_loaders():
    rgb = L.frame("random", 33, 17, seed=4)
    p = L.rgb_planes(rgb)
    assert all(q.shape == (32, 48) and q.dtype == np.float64 for q in p)
    for c in range(3):
        assert np.array_equal(p[c][:17, :33], rgb[:, :, c])
        assert np.all(p[c][17:, :33] == rgb[16, :, c]) and np.all(p[c][:17, 33:] == rgb[:, 32:33, c])
        assert np.all(p[c][17:, 33:] == rgb[16, 32, c])
