"""Box downscale, host side (no GPU): jpge_downscaled_size, and jpge_downscale_frame (the rule
of jpge.h in plain C++, which defines the frame a downscaling encode codes) against the
numpy rule of _downscale.py, exactly."""
import ctypes

import numpy as np
import pytest

import _downscale as D
import jpgenc_amd as J

FMT = pytest.mark.parametrize("fmt", D.FORMATS, ids=[D.NAMES[f] for f in D.FORMATS])
S = pytest.mark.parametrize("s", D.FACTORS)
SIZES = [(1, 1), (2, 1), (9, 9), (33, 17), (130, 50)]
E_ARG = 1


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.mark.parametrize("w,h,s,want", [
    (1, 1, 1, (1, 1)), (1, 1, 2, (1, 1)), (1, 1, 4, (1, 1)),
    (7, 9, 2, (4, 5)), (8, 8, 2, (4, 4)), (9, 7, 2, (5, 4)),     # s*k - 1, s*k, s*k + 1
    (15, 17, 4, (4, 5)), (16, 16, 4, (4, 4)), (17, 15, 4, (5, 4)),
    (65535, 65535, 1, (65535, 65535)), (65535, 65535, 2, (32768, 32768)), (65535, 65534, 4, (16384, 16384)),
    (3840, 2160, 2, (1920, 1080)), (7680, 4320, 4, (1920, 1080)),
])
def test_downscaled_size(w, h, s, want):
    assert J.downscaled_size(w, h, s) == want


@pytest.mark.parametrize("s", [0, 3, 8, -1, 16])
def test_downscaled_size_bad_factor(s):
    dw, dh = ctypes.c_uint32(7), ctypes.c_uint32(7)
    assert J.lib().jpge_downscaled_size(16, 16, s, ctypes.byref(dw), ctypes.byref(dh)) == E_ARG
    assert (dw.value, dh.value) == (7, 7)
    assert J.lib().jpge_downscaled_size(0, 16, 2, ctypes.byref(dw), ctypes.byref(dh)) == E_ARG
    assert J.lib().jpge_downscaled_size(16, 16, 2, None, ctypes.byref(dh)) == E_ARG


@FMT
@S
@pytest.mark.parametrize("w,h", SIZES + [(131, 51)])  # (NV12: odd x odd too)
@pytest.mark.parametrize("kind", D.KINDS)
def test_frame_equals_rule(fmt, s, w, h, kind):
    src = D.make(fmt, w, h, kind, seed=s, s=s)
    got, want = J.downscale_frame(src, fmt, s), D.rule(src, fmt, s)
    assert D.same(got, want)
    if fmt == D.NV12:
        assert (got.width, got.height) == J.downscaled_size(w, h, s)


@S
def test_tie_rounds_up_and_below_rounds_down(s):
    """The tie frame's whole cells are exact halves: they round up, and one below rounds down."""
    tie, below = D.make(D.RGB8, 8 * s, 4 * s, "tie", 5, s), D.make(D.RGB8, 8 * s, 4 * s, "below", 5, s)
    k = tie[::s, ::s].astype(np.int64) - 1  # (a cell's first sample is k + 1)
    assert np.array_equal(J.downscale_frame(tie, D.RGB8, s), k + 1)
    assert np.array_equal(J.downscale_frame(below, D.RGB8, s), below[s - 1::s, s - 1::s])  # (its last sample is k)


@FMT
@pytest.mark.parametrize("w,h", [(9, 9), (33, 17)])
def test_factor_one_copies(fmt, w, h):
    src = D.make(fmt, w, h, "random", 3)
    assert D.same(J.downscale_frame(src, fmt, 1), src)


@S
@pytest.mark.parametrize("fmt", [D.RGB8, D.BGRA8], ids=["rgb8", "bgra8"])
def test_padded_strides(fmt, s):
    """Rows at a pitch above their bytes, on both sides: the padding is neither read nor written."""
    w, h, bpp = 33, 17, D.BPP[fmt]
    src = D.make(fmt, w, h, "random", 11)
    dw, dh = J.downscaled_size(w, h, s)
    sst, dst_st = w * bpp + 13, dw * bpp + 7
    sbuf = np.full((h, sst), 0xEE, np.uint8)
    sbuf[:, :w * bpp] = src.reshape(h, -1)
    dbuf = np.full((dh, dst_st), 0x5A, np.uint8)
    assert J.lib().jpge_downscale_frame(fmt, _p(sbuf), w, h, sst, 0, s, _p(dbuf), dst_st, 0) == 0
    assert np.array_equal(dbuf[:, :dw * bpp].reshape(dh, dw, bpp), D.rule(src, fmt, s))
    assert (dbuf[:, dw * bpp:] == 0x5A).all()


@S
def test_padded_strides_nv12(s):
    w, h = 33, 17
    src = D.make(D.NV12, w, h, "random", 12)
    y, c = D.split_nv12(src)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    sst, gap = 2 * cw + 10, 5
    sbuf = np.full(sst * h + gap * sst + sst * ch, 0xEE, np.uint8)
    sbuf[:sst * h].reshape(h, sst)[:, :w] = y
    ps = sst * (h + gap)
    sbuf[ps:].reshape(ch, sst)[:, :2 * cw] = c.reshape(ch, -1)
    dw, dh = J.downscaled_size(w, h, s)
    dch, dcw = (dh + 1) // 2, (dw + 1) // 2
    dst_st = 2 * dcw + 6
    dps = dst_st * (dh + 3)
    dbuf = np.full(dps + dst_st * dch, 0x5A, np.uint8)
    assert J.lib().jpge_downscale_frame(D.NV12, _p(sbuf), w, h, sst, ps, s, _p(dbuf), dst_st, dps) == 0
    wy, wc = D.split_nv12(D.rule(src, D.NV12, s))
    assert np.array_equal(dbuf[:dst_st * dh].reshape(dh, dst_st)[:, :dw], wy)
    assert np.array_equal(dbuf[dps:].reshape(dch, dst_st)[:, :2 * dcw].reshape(dch, dcw, 2), wc)
    assert (dbuf[:dst_st * dh].reshape(dh, dst_st)[:, 2 * dcw:] == 0x5A).all()


def test_null_context():
    f = ctypes.c_int32(9)
    assert J.lib().jpge_set_downscale(None, 2) == E_ARG
    assert J.lib().jpge_get_downscale(None, ctypes.byref(f)) == E_ARG
    assert f.value == 9


def test_frame_refusals():
    src = np.zeros((8, 8, 4), np.uint8)
    dst = np.zeros((8, 8, 4), np.uint8)
    call = J.lib().jpge_downscale_frame
    assert call(D.RGB8, _p(src), 8, 8, 0, 0, 2, _p(dst), 0, 0) == 0
    for fmt in (J.JPGE_FMT_RGB8_PLANAR, J.JPGE_FMT_GRAY8, J.JPGE_FMT_I420, J.JPGE_FMT_YUV444_PLANAR, J.JPGE_FMT_YUYV,
                J.JPGE_FMT_NV16, J.JPGE_FMT_P010, 99, -1):
        assert call(fmt, _p(src), 8, 8, 0, 0, 2, _p(dst), 0, 0) == E_ARG
    for s in (0, 3, 8, -1):
        assert call(D.RGB8, _p(src), 8, 8, 0, 0, s, _p(dst), 0, 0) == E_ARG
    assert call(D.RGB8, _p(src), 8, 8, 23, 0, 2, _p(dst), 0, 0) == E_ARG    # source rows overlap
    assert call(D.RGB8, _p(src), 8, 8, 0, 0, 2, _p(dst), 11, 0) == E_ARG    # destination rows overlap
    assert call(D.NV12, _p(src), 8, 8, 8, 8 * 7, 2, _p(dst), 0, 0) == E_ARG  # the chroma inside the Y plane
    assert call(D.RGB8, None, 8, 8, 0, 0, 2, _p(dst), 0, 0) == E_ARG
    assert call(D.RGB8, _p(src), 0, 8, 0, 0, 2, _p(dst), 0, 0) == E_ARG
