"""Per-channel lookup tables, host side (no GPU): jpge_lut_frame against the numpy statement
lut[c][a[..., c]] of the rule in include/jpge.h, its refusals, and the Python argument shapes."""
import numpy as np
import pytest

import _lut as L
import jpgenc_amd as J

E_ARG = 1
SIZES = [(1, 1), (2, 3), (3, 2), (16, 16), (65, 17), (157, 37)]  # (W, H)


def _lut_frame(fmt, src, w, h, stride, lut, dst, dst_stride):
    return J.lib().jpge_lut_frame(int(fmt), J._p(src) if src is not None else None, w, h, stride,
                                  J._p(lut) if lut is not None else None, J._p(dst) if dst is not None else None, dst_stride)


def test_version_and_tables():
    assert J.lib().jpge_version() >= 108
    # the three permutations differ, so a swapped channel shows
    p = L.TABLES["perm"]
    assert not np.array_equal(p[0], p[1]) and not np.array_equal(p[1], p[2]) and not np.array_equal(p[0], p[2])
    assert all(sorted(p[c].tolist()) == list(range(256)) for c in range(3))


def test_equals_the_numpy_rule():
    for name, lut in L.TABLES.items():
        for fmt in L.INTERLEAVED:
            for w, h in SIZES:
                a = L.noise(fmt, w, h, 3)
                want = L.rule(a, fmt, lut)
                got = J.lut_frame(a, fmt, lut)
                assert got.shape == a.shape and np.array_equal(got, want), (name, L.NAMES[fmt], w, h)
                if L.CHANNELS[fmt] == 4:
                    assert np.array_equal(got[..., 3], a[..., 3]), (name, L.NAMES[fmt], w, h, "alpha")


def test_the_table_goes_by_colour():
    """BGR8's byte 0 goes through the B table: a frame and its channel-reversed twin map to
    channel-reversed results."""
    lut = L.TABLES["perm"]
    a = L.noise(L.RGB8, 33, 9, 5)
    assert np.array_equal(J.lut_frame(a[..., ::-1], L.BGR8, lut)[..., ::-1], J.lut_frame(a, L.RGB8, lut))
    assert np.array_equal(J.lut_frame(a, L.RGB8, lut)[..., 0], lut[0][a[..., 0]])
    assert np.array_equal(J.lut_frame(a, L.BGR8, lut)[..., 0], lut[2][a[..., 0]])
    # identity and constant tables
    assert np.array_equal(J.lut_frame(a, L.RGB8, L.TABLES["identity"]), a)
    assert np.array_equal(J.lut_frame(a, L.RGB8, L.TABLES["const"]), np.broadcast_to(np.array([17, 200, 99], np.uint8), a.shape))
    # one (256,) table serves all three channels
    assert np.array_equal(J.lut_frame(a, L.RGB8, L.TABLES["gamma"][0]), L.TABLES["gamma"][0][a])


def test_padded_strides():
    lut = L.TABLES["perm"]
    for fmt in L.INTERLEAVED:
        c = L.CHANNELS[fmt]
        for w, h in ((3, 2), (65, 17)):
            a = L.noise(fmt, w, h, 9)
            want = L.rule(a, fmt, lut).reshape(h, w * c)
            for stride, dst_stride in ((0, 0), (w * c + 5, 0), (0, w * c + 7), (w * c + 16, w * c + 16)):
                src = np.full((h, stride or w * c), 0xC3, np.uint8)
                src[:, :w * c] = a.reshape(h, w * c)
                dst = np.full((h, dst_stride or w * c), 0x5A, np.uint8)
                assert _lut_frame(fmt, src, w, h, stride, lut, dst, dst_stride) == 0
                case = (L.NAMES[fmt], w, h, stride, dst_stride)
                assert np.array_equal(dst[:, :w * c], want), case
                assert (dst[:, w * c:] == 0x5A).all(), (case, "the padding was written")


def test_refusals_write_nothing():
    lut = L.TABLES["perm"]
    w, h = 8, 4
    src = np.zeros((h, w * 4), np.uint8)

    def refused(fmt, s, ww, hh, stride, t, d, dst_stride):
        dst = np.full((h, w * 4), 0x5A, np.uint8)
        st = _lut_frame(fmt, s, ww, hh, stride, t, dst if d else None, dst_stride)
        return st == E_ARG and (dst == 0x5A).all()

    # another layout: planar RGB, gray, the Bayer ones, NV12, an unknown code
    for fmt in (J.JPGE_FMT_RGB8_PLANAR, J.JPGE_FMT_GRAY8, J.JPGE_FMT_BAYER_RGGB8, J.JPGE_FMT_BAYER_BGGR8, J.JPGE_FMT_NV12, 99, -1):
        assert refused(fmt, src, w, h, 0, lut, True, 0), fmt
    for fmt in L.INTERLEAVED:
        c = L.CHANNELS[fmt]
        assert refused(fmt, src, 0, h, 0, lut, True, 0), "zero width"
        assert refused(fmt, src, w, 0, 0, lut, True, 0), "zero height"
        assert refused(fmt, None, w, h, 0, lut, True, 0), "NULL source"
        assert refused(fmt, src, w, h, 0, None, True, 0), "NULL tables"
        assert refused(fmt, src, w, h, 0, lut, False, 0), "NULL destination"
        assert refused(fmt, src, w, h, w * c - 1, lut, True, 0), "source stride below a row"
        assert refused(fmt, src, w, h, 0, lut, True, w * c - 1), "destination stride below a row"
        assert _lut_frame(fmt, src, w, h, 0, lut, np.zeros((h, w * c), np.uint8), 0) == 0


def test_python_argument_shapes():
    a = L.noise(L.RGB8, 5, 4, 1)
    for bad in (np.zeros((3, 255), np.uint8), np.zeros((2, 256), np.uint8), np.zeros(768, np.uint8),
                np.zeros((3, 256), np.int32), np.zeros((3, 256), np.float32), np.zeros((256, 3), np.uint8)):
        with pytest.raises(ValueError):
            J.lut_frame(a, L.RGB8, bad)
    for bad_frame in (np.zeros((4, 5), np.uint8), np.zeros((4, 5, 2), np.uint8), np.zeros((4, 5, 3), np.uint16), np.zeros((0, 5, 3), np.uint8)):
        with pytest.raises(ValueError):
            J.lut_frame(bad_frame, L.RGB8, L.TABLES["perm"])
    # a list of lists is taken as it is when it has the type
    assert np.array_equal(J.lut_frame(a, L.RGB8, np.array(L.TABLES["invert"].tolist(), np.uint8)), 255 - a)
    assert J.lut_frame(L.noise(L.RGBA8, 5, 4, 1), L.RGBA8, L.TABLES["perm"]).shape == (4, 5, 4)
    with pytest.raises(J.JpgeError) as e:
        J.lut_frame(a, J.JPGE_FMT_GRAY8, L.TABLES["perm"])
    assert e.value.status == E_ARG
