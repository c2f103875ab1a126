"""The 4:2:2 input layouts (JPGE_FMT_YUYV, _UYVY, _NV16, _I422) without a GPU: the constants,
the Python packers, and the helpers of test_gpu_yuv422.py (_yuv422.py), whose expectations
then rest on checked code."""
import numpy as np
import pytest

import _oracle
import _yuv
import _yuv422 as Z
import jpgenc_amd as J

FMT = pytest.mark.parametrize("fmt", Z.FORMATS, ids=[Z.NAMES[f] for f in Z.FORMATS])
SIZES = [(1, 1), (2, 1), (9, 9), (20, 9), (33, 17)]


def test_constants():
    assert (J.JPGE_FMT_YUYV, J.JPGE_FMT_UYVY, J.JPGE_FMT_NV16, J.JPGE_FMT_I422) == (20, 21, 22, 23)


@pytest.mark.parametrize("fmt,info", [(20, (2, 1)), (21, (2, 1)), (22, (1, 2)), (23, (1, 3))])
def test_input_format_info(fmt, info):
    assert J.input_format_info(fmt) == info


def test_other_values_stay_refused():
    for fmt in (-1, 5, 15, 19, 24, 99, 1000):
        with pytest.raises(J.JpgeError):
            J.input_format_info(fmt)


@FMT
@pytest.mark.parametrize("w,h", SIZES)
def test_pack_round_trips(fmt, w, h):
    p = Z.samples(7 * w + h, w, h)
    f, fw, fh, stride = J.pack_yuv422(fmt, *p)
    assert (fw, fh, stride) == (w, h, Z.least_stride(fmt, w))
    assert f.dtype == np.uint8 and f.ndim == 1 and f.size == J.yuv422_bytes(fmt, w, h)
    assert J._frame_geom(f, fmt) == (w, h, stride)
    a, aw, ah, astride = J._as_frame(f, fmt)
    assert (aw, ah, astride) == (w, h, stride) and np.array_equal(a, np.asarray(f))
    for got, want in zip(Z.split(fmt, f, w, h), p):
        assert np.array_equal(got, want)
    # the builder that writes sample by sample agrees with the packer on every frame byte
    buf, rs, ps = Z.raw(fmt, *p, spare=0)
    n = f.size
    if fmt == Z.NV16 and w % 2:  # (the packer zeroes the pad byte of each Y row)
        buf[w:rs * h:rs] = 0
    assert rs == stride and np.array_equal(buf[:n], np.asarray(f))


@FMT
@pytest.mark.parametrize("w,h", [(9, 9), (33, 17), (20, 9)])
def test_raw_round_trips_with_strides(fmt, w, h):
    p = Z.samples(w + h, w, h)
    stride = Z.least_stride(fmt, w) + 13
    ps = 0 if fmt in Z.PACKED else stride * h + 37
    bufs = [Z.raw(fmt, *p, stride=stride, plane_stride=ps, offset=5, seed=s)[0] for s in (1, 2)]
    assert not np.array_equal(bufs[0], bufs[1])  # other bytes around the same frame
    for b in bufs:
        for got, want in zip(Z.split(fmt, b, w, h, stride=stride, plane_stride=ps, offset=5), p):
            assert np.array_equal(got, want)


def test_yuv422_bytes():
    assert J.yuv422_bytes(Z.YUYV, 5, 3) == 12 * 3 and J.yuv422_bytes(Z.UYVY, 4, 3, 32) == 96
    assert J.yuv422_bytes(Z.NV16, 5, 3) == 6 * 6 and J.yuv422_bytes(Z.NV16, 5, 3, 16) == 96
    assert J.yuv422_bytes(Z.I422, 5, 3) == 15 + 2 * 9 and J.yuv422_bytes(Z.I422, 5, 3, 7) == 21 + 2 * 12
    with pytest.raises(ValueError):
        J.yuv422_bytes(J.JPGE_FMT_NV12, 4, 4)


@FMT
def test_pack_shape_errors(fmt):
    y, cb, cr = Z.samples(1, 9, 4)
    for bad in ((y, cb[:, :4], cr), (y, cb, cr[:3]), (y[0], cb, cr), (y, cb.T, cr.T), (y[:0], cb[:0], cr[:0])):
        with pytest.raises(ValueError):
            J.pack_yuv422(fmt, *bad)
    with pytest.raises(ValueError):
        J.pack_yuv422(J.JPGE_FMT_NV12, y, cb, cr)
    f = J.pack_yuv422(fmt, y, cb, cr)[0]
    other = Z.FORMATS[(Z.FORMATS.index(fmt) + 1) % 4]
    with pytest.raises(ValueError):  # a frame of another layout
        J._frame_geom(f, other)
    with pytest.raises(ValueError):  # a flat buffer without the geometry
        J._frame_geom(np.asarray(f).copy(), fmt)
    with pytest.raises(ValueError):
        J._frame_geom(np.zeros((4, 9, 2), np.uint8), fmt)


# ---- the chroma-repeated 4:4:4 planes ----
@pytest.mark.parametrize("mcu", [(16, 8), (16, 16), (8, 8), (32, 8)])
@pytest.mark.parametrize("w,h", [(20, 9), (33, 17)])
def test_chroma_domain_replication_is_pixel_domain_replication(w, h, mcu):
    p = Z.samples(3 * w + h, w, h)
    a = Z.pad_chroma_domain(*p, mcu=mcu)
    b = _yuv.pad_planes(_yuv.YUV444, *Z.repeated(*p), mcu=mcu)
    assert all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))
    assert a[0].shape[0] % mcu[1] == 0 and a[0].shape[1] % mcu[0] == 0


def test_repeat():
    c = np.arange(6, dtype=np.uint8).reshape(2, 3)
    assert Z.repeat(c, 5).tolist() == [[0, 0, 1, 1, 2], [3, 3, 4, 4, 5]]
    assert Z.repeat(c, 6).tolist() == [[0, 0, 1, 1, 2, 2], [3, 3, 4, 4, 5, 5]]


@pytest.mark.parametrize("w,h", [(20, 9), (33, 17)])
def test_subsampling_the_repeated_planes(w, h):
    p = Z.samples(w * h, w, h)
    for mode, mcu in ((422, (16, 8)), (420, (16, 16))):
        planes = Z.pad_chroma_domain(*p, mcu=mcu)
        H, W = planes[0].shape
        for c, src in zip(planes[1:], p[1:]):
            padded = np.pad(src.astype(np.float64) - 128.0, ((0, H - h), (0, W // 2 - src.shape[1])), mode="edge")
            got = _oracle.subsample_mode(c, mode)
            if mode == 422:  # the kept sample of each pair: the chroma plane itself
                assert np.array_equal(got, padded)
            else:  # ((a + a) + (b + b)) / 4 of a vertical pair a, b: its exact mean
                assert np.array_equal(got, (padded[0::2] + padded[1::2]) / 2)
