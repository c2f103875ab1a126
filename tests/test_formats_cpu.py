"""Input layouts (jpge_set_input_format), host side: the layout table, the version, and
the numpy helpers the GPU tests build their inputs with."""
import ctypes

import numpy as np
import pytest

import _formats as F
import jpgenc_amd as J


def test_input_format_info():
    assert J.input_format_info(J.JPGE_FMT_RGB8) == (3, 1)
    assert J.input_format_info(J.JPGE_FMT_BGR8) == (3, 1)
    assert J.input_format_info(J.JPGE_FMT_RGBA8) == (4, 1)
    assert J.input_format_info(J.JPGE_FMT_BGRA8) == (4, 1)
    assert J.input_format_info(J.JPGE_FMT_RGB8_PLANAR) == (1, 3)
    assert (J.JPGE_FMT_RGB8, J.JPGE_FMT_BGR8, J.JPGE_FMT_RGBA8, J.JPGE_FMT_BGRA8, J.JPGE_FMT_RGB8_PLANAR) == (0, 1, 2, 3, 4)


@pytest.mark.parametrize("fmt", [-1, 5, 1000])
def test_input_format_info_rejects_unknown(fmt):
    with pytest.raises(J.JpgeError):
        J.input_format_info(fmt)
    assert J.lib().jpge_input_format_info(fmt, None, None) == 1  # JPGE_E_ARG


def test_input_format_info_null_outputs():
    b = ctypes.c_int32(-1)
    assert J.lib().jpge_input_format_info(J.JPGE_FMT_RGBA8, ctypes.byref(b), None) == 0 and b.value == 4
    assert J.lib().jpge_input_format_info(J.JPGE_FMT_RGB8_PLANAR, None, ctypes.byref(b)) == 0 and b.value == 3


def test_version():
    assert J.lib().jpge_version() >= 101


def test_setter_needs_a_context():
    assert J.lib().jpge_set_input_format(None, 0, 0) == 1
    assert J.lib().jpge_get_input_format(None, None, None) == 1


@pytest.mark.parametrize("fmt", F.ALL_FORMATS, ids=[F.NAMES[f] for f in F.ALL_FORMATS])
def test_helpers_round_trip(fmt):
    rgb = J.synth_rgb8(3, 37, 21, kind=1)
    a = F.to_format(rgb, fmt)
    bpp, planes = J.input_format_info(fmt)
    assert a.shape == ((3, 21, 37) if planes == 3 else (21, 37, bpp)) and a.flags.c_contiguous
    assert np.array_equal(F.from_format(a, fmt), rgb)
    # channel c of pixel (y, x) sits where the layout says
    y, x = 5, 11
    r, g, b = (int(v) for v in rgb[y, x])
    flat = a.reshape(-1)
    if planes == 3:
        assert [int(flat[c * 21 * 37 + y * 37 + x]) for c in range(3)] == [r, g, b]
    else:
        px = [int(v) for v in flat[(y * 37 + x) * bpp:][:3]]
        assert px == ([b, g, r] if fmt in (J.JPGE_FMT_BGR8, J.JPGE_FMT_BGRA8) else [r, g, b])


def test_alpha_is_random_unless_given():
    rgb = J.synth_rgb8(4, 16, 16, kind=1)
    a = F.to_format(rgb, J.JPGE_FMT_RGBA8)
    assert len(np.unique(a[:, :, 3])) > 16
    assert not F.to_format(rgb, J.JPGE_FMT_BGRA8, alpha=0)[:, :, 3].any()


@pytest.mark.parametrize("fmt", F.ALL_FORMATS, ids=[F.NAMES[f] for f in F.ALL_FORMATS])
def test_padded_layout(fmt):
    rgb = J.synth_rgb8(6, 19, 7, kind=1)
    a = F.to_format(rgb, fmt)
    bpp, planes = J.input_format_info(fmt)
    stride = 19 * bpp + 13
    buf, off, ps = F.padded(a, fmt, stride, plane_stride=(stride * 7 + 5 if planes == 3 else 0), offset=1)
    assert off == 1 and ps == (stride * 7 + 5 if planes == 3 else 0)
    rows = a if planes == 3 else a.reshape(1, 7, -1)
    for c in range(planes):
        for y in range(7):
            o = off + c * ps + y * stride
            assert np.array_equal(buf[o:o + 19 * bpp], rows[c, y])


def test_frame_shape_is_checked():
    with pytest.raises(ValueError):
        J._frame_geom(np.zeros((4, 4, 4), np.uint8), J.JPGE_FMT_RGB8)
    with pytest.raises(ValueError):
        J._frame_geom(np.zeros((4, 4, 3), np.uint8), J.JPGE_FMT_RGB8_PLANAR)
    assert J._frame_geom(np.zeros((3, 5, 7), np.uint8), J.JPGE_FMT_RGB8_PLANAR) == (7, 5, 7)
    assert J._frame_geom(np.zeros((5, 7, 4), np.uint8), J.JPGE_FMT_BGRA8) == (7, 5, 28)
