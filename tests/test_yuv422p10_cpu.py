"""The 10-bit 4:2:2 layouts (JPGE_FMT_Y210, _P210, _I210) without a GPU: the constants and the
layout table, the packers, and tests/_yuv422p10.py itself (the GPU tests' expectations): its
builders against the header's address rules, its planes of samples 4 b against the 8-bit 4:2:2
expectation of the bytes b in every mode's MCU shape, the edge rule, and the CPU-built file of a
frame per mode decoded back to the expected coefficients."""
import numpy as np
import pytest

import _oracle
import _stream3 as S
import _yuv as Y
import _yuv422 as Z
import _yuv422p10 as T
import _yuvxf as X
import jpgenc_amd as J

FMT = pytest.mark.parametrize("fmt", T.FORMATS, ids=[T.NAMES[f] for f in T.FORMATS])
SIZES = [(1, 1), (2, 1), (9, 9), (33, 17)]


def test_constants_and_version():
    assert (J.JPGE_FMT_Y210, J.JPGE_FMT_P210, J.JPGE_FMT_I210) == (40, 41, 42)
    assert J.lib().jpge_version() >= 105
    assert J.input_format_info(J.JPGE_FMT_Y210) == (2, 1)
    assert J.input_format_info(J.JPGE_FMT_P210) == (2, 2)
    assert J.input_format_info(J.JPGE_FMT_I210) == (2, 3)


@pytest.mark.parametrize("fmt", [-1, 5, 15, 19, 24, 31, 34, 39, 43, 99, 1000])
def test_other_values_stay_refused(fmt):
    with pytest.raises(J.JpgeError) as e:
        J.input_format_info(fmt)
    assert e.value.status == 1


@FMT
@pytest.mark.parametrize("w,h", SIZES)
def test_pack_round_trip(fmt, w, h):
    p = T.samples(7, w, h)
    f, fw, fh, stride = J.pack_yuv422p10(fmt, *p)
    assert (fw, fh, stride) == (w, h, T.least_stride(fmt, w))
    assert f.dtype == np.uint8 and f.ndim == 1 and f.size == J.yuv422p10_bytes(fmt, w, h)
    assert (f.fmt, f.width, f.height, f.stride) == (fmt, w, h, stride)
    assert J._frame_geom(f, fmt) == (w, h, stride)
    assert all(np.array_equal(a, b) for a, b in zip(T.split(fmt, f, w, h), p))
    # the unread six bits of a packed frame are zero, and so is an odd width's spare Y1 word
    wd = np.asarray(f).view("<u2")
    assert not np.any(wd & (0x3F if fmt in T.HIGH else 0xFC00))
    if fmt == T.Y210 and w % 2:
        assert not np.any(wd.reshape(h, -1)[:, -2])


def test_pack_refuses_what_is_no_frame():
    y, cb, cr = T.samples(1, 9, 4)
    with pytest.raises(ValueError):
        J.pack_yuv422p10(T.P210, y, cb[:2], cr[:2])  # (4:2:0's chroma shape)
    with pytest.raises(ValueError):
        J.pack_yuv422p10(T.P210, y + 1024, cb, cr)
    with pytest.raises(ValueError):
        J.pack_yuv422p10(J.JPGE_FMT_P010, y, cb, cr)
    with pytest.raises(ValueError):
        J.yuv422p10_bytes(J.JPGE_FMT_NV16, 9, 4)
    f = T.build(T.P210, y, cb, cr)
    with pytest.raises(ValueError):
        J._frame_geom(f, T.I210)


@FMT
@pytest.mark.parametrize("w,h", SIZES)
def test_raw_round_trip(fmt, w, h):
    # raw() with the least stride at offset 0 holds the packed frame's samples at the packed
    # frame's addresses; a padded one holds them at jpge.h's addresses, whatever the unread bits
    p = T.samples(8, w, h)
    packed = np.asarray(T.build(fmt, *p))
    buf, stride, ps = T.raw(fmt, *p, spare=0)
    if fmt == T.P210 and w % 2:  # (a pad word per Y row: random in raw(), zero in the packed frame)
        assert all(np.array_equal(a, b) for a, b in zip(T.split(fmt, buf[:packed.size], w, h), p))
    else:
        assert np.array_equal(buf[:packed.size], packed)
    assert (stride, ps) == (T.least_stride(fmt, w), 0 if fmt == T.Y210 else T.least_stride(fmt, w) * h)
    stride, off = T.least_stride(fmt, w) + 6, 2
    ps = 0 if fmt == T.Y210 else stride * h + 10
    for junk, spare in ((None, None), (5, 0xFFFF)):
        buf, s2, p2 = T.raw(fmt, *p, stride=stride, plane_stride=ps, offset=off, junk_seed=junk, spare=spare)
        assert (s2, p2) == (stride, ps)
        got = T.split(fmt, buf, w, h, stride, ps, off)
        assert all(np.array_equal(a, b) for a, b in zip(got, p))
    # junk reaches the unread bits
    a = T.raw(fmt, *p, junk_seed=None, seed=3)[0]
    b = T.raw(fmt, *p, junk_seed=5, seed=3)[0]
    assert (w, h) == (1, 1) or not np.array_equal(a, b)


def test_words():
    s = np.array([0, 1, 512, 1023], np.uint16)
    assert T.words(T.P210, s).tolist() == [0, 64, 32768, 0xFFC0] == T.words(T.Y210, s).tolist()
    assert T.words(T.I210, s).tolist() == [0, 1, 512, 1023]
    assert T.words(T.P210, s, [63] * 4).tolist() == [63, 127, 32831, 0xFFFF]
    assert T.words(T.I210, s, [63] * 4).tolist() == [0xFC00, 0xFC01, 0xFE00, 0xFFFF]


@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("xf", ["identity", "limited709", "custom"])
@pytest.mark.parametrize("w,h", SIZES)
def test_planes_of_multiples_of_four_are_the_8bit_planes(mode, xf, w, h):
    t = tuple(X.coeffs(xf)[2])
    mcu = Y.mcu_size(mode)
    b = Z.samples(11 * w + h, w, h)
    got = T.planes(*(4 * q.astype(np.uint16) for q in b), t, mcu)
    want = X.planes(Y.YUV444, *Z.repeated(*b), t, mcu=mcu)
    assert all(g.shape == x.shape and g.shape[0] % mcu[1] == 0 and g.shape[1] % mcu[0] == 0 and np.array_equal(g, x)
               for g, x in zip(got, want))


@pytest.mark.parametrize("w,h", SIZES + [(141, 27)])
def test_chroma_domain_replication_is_pixel_domain_replication(w, h):
    # jpge.h: the clamped pixel's cell is the clamped cell
    y, cb, cr = T.samples(5, w, h)
    for mode in T.MODES:
        mcu = Y.mcu_size(mode)
        if mcu[0] % 2:
            continue
        q = [np.asarray(p, np.float64) / 4.0 for p in (y, cb, cr)]
        want = Z.pad_chroma_domain(*q, mcu=mcu)  # (its - 128 is the planes' own)
        got = T.planes(y, cb, cr, T.IDENTITY, mcu)
        # the identity's clamps: Y' = min(s / 4, 255) - 128, C' = min(s / 4 - 128, 127)
        assert np.array_equal(got[0], np.minimum(want[0] + 128.0, 255.0) - 128.0)
        assert np.array_equal(got[1], np.minimum(want[1], 127.0)) and np.array_equal(got[2], np.minimum(want[2], 127.0))


def test_clamps_at_the_top_of_the_range():
    y, cb, cr = T.samples(0, 9, 9, "ones")
    p = T.planes(y, cb, cr)
    assert all(np.all(a == 127.0) for a in p)
    z = T.planes(*T.samples(0, 9, 9, "zeros"))
    assert all(np.all(a == -128.0) for a in z)


@pytest.mark.parametrize("mode", T.MODES)
def test_built_file_decodes_to_the_expected_coefficients(mode):
    w, h = 33, 17
    t = tuple(X.coeffs("limited709")[2])
    planes = T.planes(*T.samples(3, w, h), t, Y.mcu_size(mode))
    qy, qc = _oracle.quality_tables(90)
    b = S.build3(planes, w, h, qy, qc, mode, 3 if mode == 420 else 0)
    want = Y.want_coeffs(planes, mode, 90)
    info, y, cb, cr = J.decode_coeffs(b.jpg)
    assert all(np.array_equal(np.asarray(g).reshape(x.shape), x) for g, x in zip((y, cb, cr), want))
    assert all(np.array_equal(g, x) for g, x in zip(b.coef, want))
