"""Y, Cb, Cr input layouts (JPGE_FMT_NV12, _I420, _YUV444_PLANAR), host side: the layout
table, pack_yuv420, and the numpy helpers (_yuv.py) the GPU tests build their inputs and
expectations with."""
import numpy as np
import pytest

import _yuv as Y
import jpgenc_amd as J

FMT = pytest.mark.parametrize("fmt", Y.FORMATS, ids=[Y.NAMES[f] for f in Y.FORMATS])
SIZES = [(33, 17), (1, 1), (16, 16), (2, 3), (130, 50)]


def test_input_format_info():
    assert (J.JPGE_FMT_NV12, J.JPGE_FMT_I420, J.JPGE_FMT_YUV444_PLANAR) == (16, 17, 18)
    assert J.input_format_info(16) == (1, 2)
    assert J.input_format_info(17) == (1, 3)
    assert J.input_format_info(18) == (1, 3)


@pytest.mark.parametrize("fmt", [-1, 5, 99, 1000, 15, 19])
def test_input_format_info_rejects_unknown(fmt):
    with pytest.raises(J.JpgeError):
        J.input_format_info(fmt)
    assert J.lib().jpge_input_format_info(fmt, None, None) == 1  # JPGE_E_ARG


def test_version():
    assert J.lib().jpge_version() >= 102


@pytest.mark.parametrize("fmt", Y.HALF, ids=[Y.NAMES[f] for f in Y.HALF])
@pytest.mark.parametrize("w,h", SIZES)
def test_pack_yuv420(fmt, w, h):
    y, cb, cr = Y.samples(fmt, w + h, w, h)
    f, fw, fh, stride = J.pack_yuv420(fmt, y, cb, cr)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    assert (fw, fh) == (w, h) and f.dtype == np.uint8 and f.ndim == 1 and f.flags.c_contiguous
    # each sample sits where jpge.h says, with plane stride 0 = stride * h
    if fmt == J.JPGE_FMT_NV12:
        assert stride == 2 * cw and f.size == stride * (h + ch) == J.yuv420_bytes(fmt, w, h)
        at_cb = lambda r, c: stride * h + r * stride + 2 * c
        at_cr = lambda r, c: at_cb(r, c) + 1
    else:
        cs = (stride + 1) // 2
        assert stride == w and cs == cw and f.size == w * h + 2 * cw * ch == J.yuv420_bytes(fmt, w, h)
        at_cb = lambda r, c: stride * h + r * cs + c
        at_cr = lambda r, c: at_cb(r, c) + cs * ch
    for r, c in {(0, 0), (h - 1, w - 1), (h // 2, w // 3)}:
        assert f[r * stride + c] == y[r, c]
        assert f[at_cb(r // 2, c // 2)] == cb[r // 2, c // 2] and f[at_cr(r // 2, c // 2)] == cr[r // 2, c // 2]
    # the independent builder writes the same bytes (NV12 with odd W: but for the pad byte of each Y row)
    buf, s2, ps = Y.raw(fmt, y, cb, cr)
    assert (s2, ps) == (stride, stride * h)
    for a, b in zip(Y.split(fmt, f, w, h), Y.split(fmt, buf[:f.size], w, h)):
        assert np.array_equal(a, b)
    for a, b in zip(Y.split(fmt, f, w, h), (y, cb, cr)):
        assert np.array_equal(a, b)


def test_pack_yuv420_rejects():
    y, cb, cr = Y.samples(J.JPGE_FMT_NV12, 1, 33, 17)
    with pytest.raises(ValueError):
        J.pack_yuv420(J.JPGE_FMT_NV12, y, cb[:-1], cr)
    with pytest.raises(ValueError):
        J.pack_yuv420(J.JPGE_FMT_I420, y, cb, cr[:, :-1])
    with pytest.raises(ValueError):
        J.pack_yuv420(J.JPGE_FMT_YUV444_PLANAR, y, cb, cr)


@FMT
@pytest.mark.parametrize("w,h", SIZES)
def test_builders_round_trip(fmt, w, h):
    y, cb, cr = Y.samples(fmt, 7, w, h)
    f = Y.build(fmt, y, cb, cr)
    for a, b in zip(Y.split(fmt, f, w, h), (y, cb, cr)):
        assert np.array_equal(a, b)
    # in a padded buffer: an explicit plane stride, an offset base
    stride = w + 7 + (w & 1)
    buf, s, ps = Y.raw(fmt, y, cb, cr, stride=stride, plane_stride=stride * h + 5, offset=1)
    assert (s, ps) == (stride, stride * h + 5)
    assert np.array_equal(buf[1:1 + stride * h].reshape(h, stride)[:, :w], y)
    ch, cw = Y.chroma_shape(fmt, w, h)
    c0 = 1 + ps
    if fmt == J.JPGE_FMT_NV12:
        c = buf[c0:c0 + stride * ch].reshape(ch, stride)[:, :2 * cw]
        assert np.array_equal(c[:, 0::2], cb) and np.array_equal(c[:, 1::2], cr)
    elif fmt == J.JPGE_FMT_I420:
        cs = (stride + 1) // 2
        assert np.array_equal(buf[c0:c0 + cs * ch].reshape(ch, cs)[:, :cw], cb)
        assert np.array_equal(buf[c0 + cs * ch:c0 + 2 * cs * ch].reshape(ch, cs)[:, :cw], cr)
    else:
        assert np.array_equal(buf[c0:c0 + stride * h].reshape(h, stride)[:, :w], cb)
        assert np.array_equal(buf[c0 + ps:c0 + ps + stride * h].reshape(h, stride)[:, :w], cr)


def test_pad_planes_3x3():
    y = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 255]], np.uint8)
    cb = np.array([[10, 20], [30, 40]], np.uint8)
    cr = np.array([[200, 210], [220, 230]], np.uint8)
    wy = np.empty((16, 16))
    wy[:3, :3] = y.astype(np.float64) - 128
    wy[:3, 3:] = wy[:3, 2:3]      # the last column, to the right
    wy[3:, :] = wy[2:3, :]        # the last row, downwards
    assert wy[0, 15] == -126 and wy[15, 0] == -122 and wy[15, 15] == 127 and wy[1, 1] == -124
    wcb = np.empty((16, 16))
    wcb[:2, :2] = -118            # sample (0, 0) covers pixels (0..1, 0..1)
    wcb[:2, 2:] = -108            # sample (0, 1), and its replicas to the right
    wcb[2:, :2] = -98             # sample (1, 0), and its replicas downwards
    wcb[2:, 2:] = -88             # sample (1, 1)
    for fmt in Y.HALF:
        got = Y.pad_planes(fmt, y, cb, cr)
        assert all(p.dtype == np.float64 and p.shape == (16, 16) for p in got)
        assert np.array_equal(got[0], wy) and np.array_equal(got[1], wcb) and np.array_equal(got[2], wcb + 190)
    # full-size chroma: replicated like Y; other MCU sizes
    got = Y.pad_planes(J.JPGE_FMT_YUV444_PLANAR, y, y, y)
    assert all(np.array_equal(p, wy) for p in got)
    got = Y.pad_planes(J.JPGE_FMT_YUV444_PLANAR, y, y, y, mcu=(32, 8))
    assert all(p.shape == (8, 32) and np.array_equal(p, np.pad(wy[:3, :3], ((0, 5), (0, 29)), mode="edge")) for p in got)


def test_want_coeffs_flat_planes():
    # a constant plane of value v has DC 8 v and no AC: round(8 v / q[0]) in every block
    import _oracle
    planes = Y.pad_planes(J.JPGE_FMT_I420, *Y.samples(J.JPGE_FMT_I420, 0, 20, 9, "ones"))
    qy, qc = _oracle.quality_tables(90)
    for mode in (420, 444, 411):
        wy, wcb, wcr = Y.want_coeffs(planes, mode, 90)
        yh, yv = _oracle.SHAPES[mode]
        assert wy.shape == (2 * 4, 64) and wcb.shape == wcr.shape == ((16 // (8 * yv)) * (32 // (8 * yh)), 64)
        assert np.all(wy[:, 0] == round(8 * 127 / int(qy[0]))) and not wy[:, 1:].any()
        assert np.all(wcb[:, 0] == round(8 * 127 / int(qc[0]))) and not wcr[:, 1:].any()


@FMT
def test_frame_geom(fmt):
    w, h = 33, 17
    f = Y.build(fmt, *Y.samples(fmt, 3, w, h))
    stride = {J.JPGE_FMT_NV12: 34, J.JPGE_FMT_I420: 33, J.JPGE_FMT_YUV444_PLANAR: 33}[fmt]
    assert J._frame_geom(f, fmt) == (w, h, stride)
    a, gw, gh, gs = J._as_frame(f, fmt)
    assert (gw, gh, gs) == (w, h, stride) and a.dtype == np.uint8 and a.flags.c_contiguous and a.size == f.size
    with pytest.raises(ValueError):
        J._frame_geom(np.zeros((h, w, 3), np.uint8), fmt)
    if fmt in Y.HALF:
        other = J.JPGE_FMT_I420 if fmt == J.JPGE_FMT_NV12 else J.JPGE_FMT_NV12
        with pytest.raises(ValueError):
            J._frame_geom(f, other)  # a frame packed for the other layout
        with pytest.raises(ValueError):
            J._frame_geom(np.asarray(f), fmt)  # a flat buffer does not show its geometry
