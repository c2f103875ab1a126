"""The v210 layout (JPGE_FMT_V210) without a GPU: the constant, the version and the layout table,
jpge_v210_row_bytes, jpge_v210_unpack against the stream rule stated on its own in tests/_v210.py
(the GPU tests' expectations rest on that file), pack_v210, the meaning of a frame (the planes of
the I210 frame of the same samples), and what the host refuses."""
import ctypes

import numpy as np
import pytest

import _v210 as V
import _yuv as Y
import _yuv422p10 as T
import jpgenc_amd as J

WIDTHS = [1, 2, 5, 6, 7, 11, 12, 13, 49]


def test_constant_version_and_table():
    assert J.JPGE_FMT_V210 == 48
    assert J.lib().jpge_version() >= 106
    assert J.input_format_info(J.JPGE_FMT_V210) == (0, 1)
    assert "jpge_v210_row_bytes" in J.EXPORTS and "jpge_v210_unpack" in J.EXPORTS


@pytest.mark.parametrize("fmt", [43, 39, 34, 31, 24, 47, 49])
def test_other_values_stay_refused(fmt):
    with pytest.raises(J.JpgeError) as e:
        J.input_format_info(fmt)
    assert e.value.status == 1


@pytest.mark.parametrize("w", list(range(1, 14)) + [47, 48, 49])
def test_row_bytes(w):
    want = 16 * -(-w // 6)
    assert J.v210_row_bytes(w) == want == V.row_bytes(w)
    assert want % 16 == 0 and 6 * (want // 16) >= w > 6 * (want // 16 - 1)
    assert V.conventional_stride(w) >= want and V.conventional_stride(w) % 128 == 0


def test_row_bytes_of_the_largest_width():
    assert J.v210_row_bytes(65535) == 16 * 10923
    assert J.v210_row_bytes(0xFFFFFFFF) == 16 * 715827883  # (no 32-bit overflow)


def test_stream_rule_on_a_hand_made_group():
    # one group of six pixels: Cb0 Y0 Cr0 | Y1 Cb1 Y2 | Cr1 Y3 Cb2 | Y4 Cr2 Y5
    s = [100, 1, 200, 2, 101, 3, 201, 4, 102, 5, 202, 6]
    words = np.array([s[3 * i] | (s[3 * i + 1] << 10) | (s[3 * i + 2] << 20) | (3 << 30) for i in range(4)], "<u4")
    y, cb, cr = V.unpack(words.view(np.uint8), 6, 1)
    assert y.tolist() == [[1, 2, 3, 4, 5, 6]] and cb.tolist() == [[100, 101, 102]] and cr.tolist() == [[200, 201, 202]]
    y, cb, cr = J.v210_unpack(words.view(np.uint8), 6, 1)
    assert y.tolist() == [[1, 2, 3, 4, 5, 6]] and cb.tolist() == [[100, 101, 102]] and cr.tolist() == [[200, 201, 202]]
    # an odd width: the last cell's Cb and Cr are real
    y, cb, cr = J.v210_unpack(words.view(np.uint8), 3, 1)
    assert y.tolist() == [[1, 2, 3]] and cb.tolist() == [[100, 101]] and cr.tolist() == [[200, 201]]


@pytest.mark.parametrize("junk", [None, 31])
@pytest.mark.parametrize("pad", [0, 4, 16, 100])
@pytest.mark.parametrize("w", WIDTHS)
def test_unpack_against_the_stream_rule(w, pad, junk):
    # strides above the least, random bytes in the padding, junk in bits 30-31 and unused samples
    h = 3
    p = T.samples(40 + w, w, h)
    stride = V.row_bytes(w) + pad
    buf, s2 = V.raw(*p, stride=stride, offset=8, seed=w + pad, junk_seed=junk)
    assert s2 == stride
    want = V.unpack(buf, w, h, stride, 8)
    assert all(np.array_equal(a, b) for a, b in zip(want, p))
    got = J.v210_unpack(buf[8:], w, h, stride)
    assert all(g.dtype == np.uint16 and np.array_equal(g, x) for g, x in zip(got, p))
    if pad == 0:
        got = J.v210_unpack(buf[8:], w, h)  # stride 0: the least
        assert all(np.array_equal(g, x) for g, x in zip(got, p))


@pytest.mark.parametrize("w", WIDTHS)
def test_junk_reaches_only_what_is_never_read(w):
    h = 2
    p = T.samples(3, w, h)
    a = V.raw(*p, seed=5)[0]
    b = V.raw(*p, seed=5, junk_seed=77)[0]
    assert not np.array_equal(a, b)
    n = 3 * (V.row_bytes(w) // 4)
    sa, sb = V.stream(a, w, h), V.stream(b, w, h)
    u = V.used(w)
    assert sa.shape == (h, n) and np.array_equal(sa[:, u], sb[:, u])
    assert u.sum() == w + 2 * V.cw_of(w)
    assert not np.any(sa[:, ~u])  # without junk the unused samples are zero


@pytest.mark.parametrize("w,h", [(1, 1), (2, 1), (5, 3), (6, 2), (7, 2), (13, 3), (49, 2), (33, 17)])
def test_pack_round_trip(w, h):
    p = T.samples(7, w, h)
    f, fw, fh, stride = J.pack_v210(*p)
    assert (fw, fh, stride) == (w, h, V.row_bytes(w))
    assert f.dtype == np.uint8 and f.ndim == 1 and f.size == stride * h
    assert (f.fmt, f.width, f.height, f.stride) == (J.JPGE_FMT_V210, w, h, stride)
    assert J._frame_geom(f, J.JPGE_FMT_V210) == (w, h, stride)
    assert all(np.array_equal(a, b) for a, b in zip(J.v210_unpack(f, w, h), p))
    assert all(np.array_equal(a, b) for a, b in zip(V.unpack(f, w, h), p))
    # the packed frame is raw() without junk: unused samples and bits 30-31 zero
    assert np.array_equal(np.asarray(f), V.raw(*p, tail=0)[0])
    assert not np.any(np.asarray(f).view("<u4") >> 30)
    # a larger stride: the same samples, zero padding
    s2 = V.conventional_stride(w)
    g, _, _, gs = J.pack_v210(*p, stride=s2)
    assert gs == s2 and g.size == s2 * h and J._frame_geom(g, J.JPGE_FMT_V210) == (w, h, s2)
    assert all(np.array_equal(a, b) for a, b in zip(J.v210_unpack(g, w, h, s2), p))
    assert not np.any(np.asarray(g).reshape(h, s2)[:, stride:])


@pytest.mark.parametrize("mode", V.MODES)
@pytest.mark.parametrize("w,h", [(1, 1), (7, 3), (33, 17)])
def test_unpacked_planes_are_the_i210_frames(mode, w, h):
    # the frame means what the I210 frame of the same samples means
    p = T.samples(11, w, h)
    mcu = Y.mcu_size(mode)
    i210 = T.build(T.I210, *p)
    want = T.planes(*T.split(T.I210, i210, w, h), T.IDENTITY, mcu)
    buf, stride = V.raw(*p, stride=V.row_bytes(w) + 12, offset=4, junk_seed=2)
    got = V.planes(*J.v210_unpack(buf[4:], w, h, stride), V.IDENTITY, mcu)
    assert all(g.shape == x.shape and np.array_equal(g, x) for g, x in zip(got, want))


def test_refusals():
    y, cb, cr = T.samples(1, 9, 4)
    with pytest.raises(ValueError):
        J.pack_v210(y, cb[:2], cr[:2])  # (4:2:0's chroma shape)
    with pytest.raises(ValueError):
        J.pack_v210(y + 1024, cb, cr)
    with pytest.raises(ValueError):
        J.pack_v210(y.astype(np.float64), cb, cr)
    with pytest.raises(ValueError):
        J.pack_v210(y, cb, cr, stride=V.row_bytes(9) - 4)  # below a row
    with pytest.raises(ValueError):
        J.pack_v210(y, cb, cr, stride=V.row_bytes(9) + 2)  # no multiple of 4
    f = V.build(y, cb, cr)
    with pytest.raises(ValueError):
        J._frame_geom(f, T.I210)
    with pytest.raises(ValueError):
        J._frame_geom(T.build(T.Y210, y, cb, cr), J.JPGE_FMT_V210)
    with pytest.raises(ValueError):
        J.v210_unpack(np.asarray(f)[:-1], 9, 4)  # too few bytes
    with pytest.raises(ValueError):
        J.v210_unpack(f, 9, 4, stride=16)  # below a row
    with pytest.raises(ValueError):
        J.v210_unpack(f, 0, 4)
    # the C entry itself
    L = J.lib()
    a = np.asarray(f)
    o = [np.zeros((4, 9), np.uint16), np.zeros((4, 5), np.uint16), np.zeros((4, 5), np.uint16)]
    ptr = lambda x: ctypes.c_void_p(x.ctypes.data)
    assert L.jpge_v210_unpack(ptr(a), 9, 4, 0, *(ptr(x) for x in o)) == 0
    assert all(np.array_equal(g, x) for g, x in zip(o, (y, cb, cr)))
    assert L.jpge_v210_unpack(ptr(a), 9, 4, 16, *(ptr(x) for x in o)) == 1
    assert L.jpge_v210_unpack(ptr(a), 0, 4, 0, *(ptr(x) for x in o)) == 1
    assert L.jpge_v210_unpack(ptr(a), 9, 0, 0, *(ptr(x) for x in o)) == 1
    assert L.jpge_v210_unpack(None, 9, 4, 0, *(ptr(x) for x in o)) == 1
    assert L.jpge_v210_unpack(ptr(a), 9, 4, 0, ptr(o[0]), None, ptr(o[2])) == 1
