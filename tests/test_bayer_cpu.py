"""8-bit Bayer input, host side (no GPU): jpge_demosaic_frame against the numpy statement of the
rule in include/jpge.h, its refusals, and the layouts' entries in jpge_input_format_info."""
import ctypes

import numpy as np

import _bayer as B
import jpgenc_amd as J

E_ARG = 1
SIZES = [(2, 2), (2, 3), (3, 2), (3, 3), (16, 16), (65, 17), (157, 37)]  # (W, H)


def _demosaic(fmt, src, w, h, stride, dst, dst_stride):
    return J.lib().jpge_demosaic_frame(int(fmt), J._p(src), w, h, stride, J._p(dst), dst_stride)


def test_constants_and_version():
    assert (B.RGGB, B.GRBG, B.GBRG, B.BGGR) == (10, 11, 12, 13)
    assert J.BAYER_LAYOUTS == {"bayer_rggb": 10, "bayer_grbg": 11, "bayer_gbrg": 12, "bayer_bggr": 13}
    assert J.lib().jpge_version() >= 107


def test_input_format_info():
    for fmt in B.FORMATS:
        assert J.input_format_info(fmt) == (1, 1), B.NAMES[fmt]


def test_equals_the_numpy_rule():
    for fmt in B.FORMATS:
        for w, h in SIZES:
            a = B.noise(w, h, 7)
            want = B.rule(a, fmt)
            assert np.array_equal(J.demosaic_frame(a, fmt), want), (B.NAMES[fmt], w, h)
            # padded strides on both sides; the padding stays as it was
            for stride, dst_stride in ((0, 0), (w + 5, 0), (0, 3 * w + 7), (w + 16, 3 * w + 16)):
                src = np.full((h, stride or w), 0xC3, np.uint8)
                src[:, :w] = a
                dst = np.full((h, dst_stride or 3 * w), 0x5A, np.uint8)
                assert _demosaic(fmt, src, w, h, stride, dst, dst_stride) == 0
                case = (B.NAMES[fmt], w, h, stride, dst_stride)
                assert np.array_equal(dst[:, :3 * w].reshape(h, w, 3), want), case
                assert (dst[:, 3 * w:] == 0x5A).all(), case


def test_checkers_hit_every_rounding():
    for fmt in B.FORMATS:
        for which in range(8):
            for w, h in ((16, 16), (65, 17)):
                a = B.checker(w, h, which)
                assert np.array_equal(J.demosaic_frame(a, fmt), B.rule(a, fmt)), (B.NAMES[fmt], which, w, h)


def test_pure_colours_stay_constant():
    """All R sites a, G sites b, B sites c: D is (a, b, c) everywhere, the edges included, which a
    reflection that changed a site's parity would break."""
    for fmt in B.FORMATS:
        for w, h in SIZES:
            for abc in ((255, 0, 0), (0, 255, 0), (0, 0, 255), (13, 200, 77)):
                a = np.array(abc, np.uint8)[B.colours(fmt, h, w)]
                d = J.demosaic_frame(a, fmt)
                assert (d == np.array(abc, np.uint8)).all(), (B.NAMES[fmt], w, h, abc)


def test_mosaic_of_a_flat_frame_round_trips():
    rgb = np.broadcast_to(np.array([9, 99, 199], np.uint8), (21, 34, 3))
    for fmt in B.FORMATS:
        assert np.array_equal(J.demosaic_frame(B.mosaic(rgb, fmt), fmt), rgb), B.NAMES[fmt]


def test_refusals_write_nothing():
    w, h = 8, 6
    src = B.noise(w, h, 1)
    null = ctypes.c_void_p(None)

    def refused(call):
        dst = np.full((h, 3 * w), 0x5A, np.uint8)
        st = call(dst)
        return st == E_ARG and (dst == 0x5A).all()

    # another layout (the ones around the four codes, RGB8, GRAY8, NV12)
    for fmt in (0, 8, 9, 14, 16, -1):
        assert refused(lambda d: _demosaic(fmt, src, w, h, 0, d, 0)), fmt
    for fmt in B.FORMATS:
        # a dimension below 2
        for bw, bh in ((1, h), (w, 1), (0, h), (w, 0), (1, 1)):
            assert refused(lambda d: _demosaic(fmt, src, bw, bh, w, d, 0)), (fmt, bw, bh)
        # a stride below a row's bytes, either side
        assert refused(lambda d: _demosaic(fmt, src, w, h, w - 1, d, 0)), fmt
        assert refused(lambda d: _demosaic(fmt, src, w, h, 0, d, 3 * w - 1)), fmt
        # NULL
        assert refused(lambda d: J.lib().jpge_demosaic_frame(fmt, null, w, h, 0, J._p(d), 0)), fmt
        assert J.lib().jpge_demosaic_frame(fmt, J._p(src), w, h, 0, null, 0) == E_ARG
        # (the same call with valid arguments does write)
        dst = np.full((h, 3 * w), 0x5A, np.uint8)
        assert _demosaic(fmt, src, w, h, 0, dst, 0) == 0 and np.array_equal(dst.reshape(h, w, 3), B.rule(src, fmt))


def test_frames_are_2d_uint8():
    import pytest
    for bad in (np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4), np.float32), np.zeros((0, 4), np.uint8)):
        with pytest.raises(ValueError):
            J._as_frame(bad, B.RGGB)
    a, w, h, stride = J._as_frame(B.noise(5, 4), B.BGGR)
    assert (w, h, stride) == (5, 4, 5)
