"""Orientation, host side (no GPU): jpge_oriented_size, and jpge_orient_frame (the table of
jpge.h in plain C++, which defines the frame an oriented encode codes) against the table's
numpy expressions (_orient.py), exactly."""
import ctypes

import numpy as np
import pytest

import _orient as O
import jpgenc_amd as J

FMT = pytest.mark.parametrize("fmt", O.FORMATS, ids=[O.NAMES[f] for f in O.FORMATS])
ORI = pytest.mark.parametrize("o", O.ORIENTS, ids=O.ONAMES)
SIZES = [(1, 1), (1, 200), (200, 1), (16, 16), (157, 37)]
E_ARG = 1
POISON = 0x5A


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_constants():
    assert (J.JPGE_ORIENT_NONE, J.JPGE_ORIENT_FLIP_H, J.JPGE_ORIENT_ROT180, J.JPGE_ORIENT_FLIP_V, J.JPGE_ORIENT_TRANSPOSE,
            J.JPGE_ORIENT_ROT90, J.JPGE_ORIENT_TRANSVERSE, J.JPGE_ORIENT_ROT270) == O.ORIENTS


@ORI
@pytest.mark.parametrize("w,h", SIZES + [(65535, 1), (3840, 2160)])
def test_oriented_size(o, w, h):
    assert J.oriented_size(w, h, o) == ((h, w) if o in O.TRANSPOSED else (w, h))


def test_oriented_size_refusals():
    ow, oh = ctypes.c_uint32(7), ctypes.c_uint32(7)
    call = J.lib().jpge_oriented_size
    for o in (-1, 8, 9, 100):
        assert call(16, 16, o, ctypes.byref(ow), ctypes.byref(oh)) == E_ARG
    assert call(0, 16, 1, ctypes.byref(ow), ctypes.byref(oh)) == E_ARG
    assert call(16, 0, 1, ctypes.byref(ow), ctypes.byref(oh)) == E_ARG
    assert call(16, 16, 1, None, ctypes.byref(oh)) == E_ARG
    assert call(16, 16, 1, ctypes.byref(ow), None) == E_ARG
    assert (ow.value, oh.value) == (7, 7)


@FMT
@ORI
@pytest.mark.parametrize("w,h", SIZES)
def test_frame_equals_table(fmt, o, w, h):
    """Dense pitches, through the binding: the numpy column of the table."""
    src = O.make(fmt, w, h, seed=o)
    got = J.orient_frame(src, fmt, o)
    assert got.shape == O.rule(src, o).shape and np.array_equal(got, O.rule(src, o))
    assert got.shape[:2] == J.oriented_size(w, h, o)[::-1]


@ORI
def test_numpy_column_equals_formula_column(o):
    """The table's two right-hand columns say the same thing."""
    for w, h in ((5, 3), (1, 4), (6, 1)):
        src = O.make(O.RGB8, w, h, seed=20 + o)
        assert np.array_equal(O.rule(src, o), O.formula(src, o))


@FMT
@ORI
@pytest.mark.parametrize("w,h", SIZES)
def test_padded_pitches_and_poison(fmt, o, w, h):
    """Rows at a pitch above their bytes on both sides: the source's padding is not read (it holds
    other bytes than the frame and the result is the table's), the destination's bytes outside
    its rows' pixels are untouched."""
    bpp = O.BPP[fmt]
    src = O.make(fmt, w, h, seed=40 + o)
    ow, oh = J.oriented_size(w, h, o)
    sst, dst_st = w * bpp + 13, ow * bpp + 7
    sbuf = np.full((h, sst), 0xEE, np.uint8)
    sbuf[:, :w * bpp] = src.reshape(h, -1)
    head, tail = 32, 32
    dbuf = np.full(head + oh * dst_st + tail, POISON, np.uint8)
    body = dbuf[head:head + oh * dst_st].reshape(oh, dst_st)
    assert J.lib().jpge_orient_frame(fmt, _p(sbuf), w, h, sst, o, _p(body), dst_st) == 0
    assert np.array_equal(body[:, :ow * bpp].reshape(oh, ow, bpp), O.rule(src, o))
    assert (body[:, ow * bpp:] == POISON).all()
    assert (dbuf[:head] == POISON).all() and (dbuf[head + oh * dst_st:] == POISON).all()


@FMT
@ORI
@pytest.mark.parametrize("w,h", SIZES)
def test_inverse_returns_the_source(fmt, o, w, h):
    src = O.make(fmt, w, h, seed=60 + o)
    back = J.orient_frame(J.orient_frame(src, fmt, o), fmt, O.INVERSE[o])
    assert back.shape == src.shape and np.array_equal(back, src)


def test_frame_refusals():
    src = np.zeros((8, 8, 4), np.uint8)
    dst = np.full((8, 8, 4), POISON, np.uint8)
    call = J.lib().jpge_orient_frame
    assert call(O.RGB8, _p(src), 8, 8, 0, 5, _p(dst), 0) == 0
    dst[:] = POISON
    for fmt in (J.JPGE_FMT_RGB8_PLANAR, J.JPGE_FMT_GRAY8, J.JPGE_FMT_NV12, J.JPGE_FMT_I420, J.JPGE_FMT_YUV444_PLANAR,
                J.JPGE_FMT_YUYV, J.JPGE_FMT_NV16, J.JPGE_FMT_P010, J.JPGE_FMT_V210, 99, -1):
        assert call(fmt, _p(src), 8, 8, 0, 1, _p(dst), 0) == E_ARG
    for o in (-1, 8, 9):
        assert call(O.RGB8, _p(src), 8, 8, 0, o, _p(dst), 0) == E_ARG
    assert call(O.RGB8, _p(src), 8, 8, 23, 1, _p(dst), 0) == E_ARG   # source rows overlap
    assert call(O.RGB8, _p(src), 8, 8, 0, 1, _p(dst), 23) == E_ARG   # destination rows overlap
    assert call(O.RGBA8, _p(src), 8, 4, 0, 4, _p(dst), 15) == E_ARG  # (the destination's rows are 4 pixels: 16 bytes)
    assert call(O.RGB8, None, 8, 8, 0, 1, _p(dst), 0) == E_ARG
    assert call(O.RGB8, _p(src), 8, 8, 0, 1, None, 0) == E_ARG
    assert call(O.RGB8, _p(src), 0, 8, 0, 1, _p(dst), 0) == E_ARG
    assert call(O.RGB8, _p(src), 8, 0, 0, 1, _p(dst), 0) == E_ARG
    assert (dst == POISON).all()  # a refused call writes nothing


def test_null_context():
    """The setting's argument checks that need no device."""
    o = ctypes.c_int32(9)
    assert J.lib().jpge_set_orientation(None, 1) == E_ARG
    assert J.lib().jpge_set_orientation(None, 99) == E_ARG
    assert J.lib().jpge_get_orientation(None, ctypes.byref(o)) == E_ARG
    assert o.value == 9
