"""The 10-bit 4:2:0 layouts (JPGE_FMT_P010, _I010) without a GPU: the constants and the layout
table, the packers, and tests/_yuv10.py itself (the GPU tests' expectations): its planes of
samples 4 b are _yuvxf.planes of the bytes b, bit for bit, and its clamps are jpge.h's."""
import numpy as np
import pytest

import _yuv as Y
import _yuv10 as T
import _yuvxf as X
import jpgenc_amd as J

FMT = pytest.mark.parametrize("fmt", T.FORMATS, ids=[T.NAMES[f] for f in T.FORMATS])
SIZES = [(1, 1), (2, 1), (9, 9), (33, 17)]


def test_constants_and_version():
    assert (J.JPGE_FMT_P010, J.JPGE_FMT_I010) == (32, 33)
    assert J.lib().jpge_version() >= 104
    assert J.input_format_info(J.JPGE_FMT_P010) == (2, 2)
    assert J.input_format_info(J.JPGE_FMT_I010) == (2, 3)


@pytest.mark.parametrize("fmt", [-1, 5, 15, 19, 24, 31, 34, 99, 1000])
def test_other_values_stay_refused(fmt):
    with pytest.raises(J.JpgeError) as e:
        J.input_format_info(fmt)
    assert e.value.status == 1


@FMT
@pytest.mark.parametrize("w,h", SIZES)
def test_pack_round_trip(fmt, w, h):
    p = T.samples(7, w, h)
    f, fw, fh, stride = J.pack_yuv420p10(fmt, *p)
    assert (fw, fh, stride) == (w, h, T.least_stride(fmt, w))
    assert f.dtype == np.uint8 and f.ndim == 1 and f.size == J.yuv420p10_bytes(fmt, w, h)
    assert (f.fmt, f.width, f.height, f.stride) == (fmt, w, h, stride)
    assert J._frame_geom(f, fmt) == (w, h, stride)
    assert all(np.array_equal(a, b) for a, b in zip(T.split(fmt, f, w, h), p))
    # the unread six bits of a packed frame are zero
    wd = np.asarray(f).view("<u2")
    assert not np.any(wd & (0x3F if fmt == T.P010 else 0xFC00))


@FMT
@pytest.mark.parametrize("w,h", SIZES)
def test_raw_round_trip(fmt, w, h):
    # raw() with the least stride at offset 0 holds the packed frame's bytes; a padded one holds
    # the same samples at jpge.h's addresses, whatever the unread bits
    p = T.samples(8, w, h)
    packed = np.asarray(T.build(fmt, *p))
    buf, stride, ps = T.raw(fmt, *p)
    ch, cw = T.chroma_shape(w, h)
    if fmt == T.P010 and w % 2:  # (a pad word per Y row: random in raw(), zero in the packed frame)
        assert all(np.array_equal(a, b) for a, b in zip(T.split(fmt, buf[:packed.size], w, h), p))
    else:
        assert np.array_equal(buf[:packed.size], packed)
    assert (stride, ps) == (T.least_stride(fmt, w), T.least_stride(fmt, w) * h)
    stride, off = T.least_stride(fmt, w) + 6, 2
    ps = stride * h + 10
    buf, s2, ps2 = T.raw(fmt, *p, stride=stride, plane_stride=ps, offset=off, junk_seed=3)
    assert (s2, ps2) == (stride, ps)
    wd = lambda o: int(buf[o]) | (int(buf[o + 1]) << 8)
    smp = (lambda o: wd(o) >> 6) if fmt == T.P010 else (lambda o: wd(o) & 0x3FF)
    cs = T.chroma_pitch(fmt, stride)
    for (r, c) in [(0, 0), (h - 1, w - 1), (h // 2, w // 2)]:
        assert smp(off + r * stride + 2 * c) == p[0][r, c]
        cr_, cc_ = r // 2, c // 2
        if fmt == T.P010:
            assert smp(off + ps + cr_ * cs + 4 * cc_) == p[1][cr_, cc_]
            assert smp(off + ps + cr_ * cs + 4 * cc_ + 2) == p[2][cr_, cc_]
        else:
            assert smp(off + ps + cr_ * cs + 2 * cc_) == p[1][cr_, cc_]
            assert smp(off + ps + cs * ch + cr_ * cs + 2 * cc_) == p[2][cr_, cc_]


def test_bytes_and_pitches():
    assert J.yuv420p10_bytes(T.P010, 33, 17) == 68 * (17 + 9)
    assert J.yuv420p10_bytes(T.I010, 33, 17) == 66 * 17 + 2 * 34 * 9  # cs = 2 * ceil(66 / 4)
    assert J.yuv420p10_bytes(T.I010, 33, 17, 96) == 96 * 17 + 2 * 48 * 9
    assert T.chroma_pitch(T.I010, 70) == 36 and T.chroma_pitch(T.P010, 70) == 70
    with pytest.raises(ValueError):
        J.yuv420p10_bytes(J.JPGE_FMT_NV12, 4, 4)
    with pytest.raises(ValueError):
        J.pack_yuv420p10(T.P010, np.full((2, 2), 1024, np.uint16), np.zeros((1, 1), np.uint16), np.zeros((1, 1), np.uint16))
    with pytest.raises(ValueError):
        J.pack_yuv420p10(T.I010, np.zeros((2, 2), np.uint16), np.zeros((2, 2), np.uint16), np.zeros((1, 1), np.uint16))


@pytest.mark.parametrize("xf", ["identity", "limited709", "custom"])
@pytest.mark.parametrize("w,h", SIZES)
def test_multiples_of_four_are_the_8bit_planes(xf, w, h):
    t = X.IDENTITY if xf == "identity" else X.CUSTOM if xf == "custom" else J.yuv_preset(J.JPGE_YUV_LIMITED_709)
    b = Y.samples(Y.I420, 5, w, h)
    got = T.planes(*(4 * np.asarray(p, np.uint16) for p in b), t)
    want = X.planes(Y.I420, *b, t)
    assert all(g.dtype == np.float64 and g.shape == x.shape and np.array_equal(g, x) for g, x in zip(got, want))


def test_clamps():
    s = np.array([[0, 63, 64, 940, 941, 1020, 1021, 1023]], np.uint16)
    c = np.full((1, 4), 512, np.uint16)  # centred chroma: u = v = 0
    # identity: Y' = min(s / 4, 255) - 128
    y = T.planes(s, c, c)[0][0, :8]
    assert np.array_equal(y, np.array([0, 15.75, 16, 235, 235.25, 255, 255, 255]) - 128.0)
    # LIMITED_601: Y' = clamp(fl(255/219) * (s / 4 - 16), 0, 255) - 128
    t = J.yuv_preset(J.JPGE_YUV_LIMITED_601)
    m0 = float(t[1])
    y = T.planes(s, c, c, t)[0][0, :8]
    want = [min(max(m0 * (int(v) / 4.0 - 16.0), 0.0), 255.0) - 128.0 for v in s[0]]
    assert np.array_equal(y, np.array(want))
    # (below black, black, white to within a rounding, above white)
    assert y[0] == y[1] == y[2] == -128.0 and abs(y[3] - 127.0) < 1e-12 and y[4] == y[5] == y[7] == 127.0
    # chroma as the sample: identity Cb' = min(s / 4 - 128, 127); LIMITED_601 clamps both ends
    cs = np.array([[0, 63, 64, 960, 961, 1020, 1021, 1023]], np.uint16)
    yy = np.full((2, 16), 512, np.uint16)
    cb = T.planes(yy, cs, cs)[1][0, 0:16:2]
    assert np.array_equal(cb, np.array([-128, -112.25, -112, 112, 112.25, 127, 127, 127], np.float64))
    cb = T.planes(yy, cs, cs, t)[1][0, 0:16:2]
    m3 = float(t[4])
    assert np.array_equal(cb, np.array([min(max(m3 * (int(v) / 4.0 - 128.0), -128.0), 127.0) for v in cs[0]]))
    assert cb[0] == -128.0 and cb[-1] == 127.0
