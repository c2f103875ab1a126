"""One-component (JPGE_FMT_GRAY8) streams, host side: the expected-bytes builder (_gray.py)
against the host decoder, the YUV helpers' Y plane and PIL; the layout table; the Python
binding's argument checks; and the three-component streams through the same decoder."""
import glob
import io
import os

import numpy as np
import pytest

import _gray as G
import _oracle
import _yuv as Y
import jpgenc_amd as J

CASES = [(1, 1, 0), (7, 5, 0), (9, 9, 0), (17, 8, 1), (136, 16, 3), (40, 24, 100)]


@pytest.mark.parametrize("w,h,restart", CASES)
@pytest.mark.parametrize("kind", ["random", "photo", "ones"])
def test_decoder_reads_the_builders_file(kind, w, h, restart):
    b = G.built(kind, w, h, 90, restart)
    info, y, cb, cr = J.decode_coeffs(b.jpg)
    assert cb is None and cr is None
    assert (info.width, info.height, info.yh, info.yv, info.restart) == (w, h, 1, 1, restart)
    assert info.c_blocks == 0 and info.y_blocks == b.mw * b.mh == -(-w // 8) * -(-h // 8)
    assert bytes(info.qy) == _oracle.quality_tables(90)[0].tobytes() and bytes(info.qc) == bytes(64)
    assert y.shape == b.coef.shape and np.array_equal(y, b.coef)


def test_decoder_c_abi_one_component():
    # cb / cr may be NULL; a Y buffer that is too small is JPGE_E_NOSPACE; a truncated file a format error
    b = G.built("random", 17, 8, 50)
    buf = np.frombuffer(b.jpg, np.uint8)
    info = J.Decoded()
    y = np.zeros((3, 64), np.int16)
    L = J.lib()
    assert L.jpge_decode_coeffs(buf.ctypes.data, buf.size, info, None, None, None, 0, 0) == 0
    assert (info.y_blocks, info.c_blocks) == (3, 0)
    assert L.jpge_decode_coeffs(buf.ctypes.data, buf.size, info, y.ctypes.data, None, None, 2, 0) == 2
    assert L.jpge_decode_coeffs(buf.ctypes.data, buf.size, info, y.ctypes.data, None, None, 3, 0) == 0
    assert np.array_equal(y, b.coef)
    with pytest.raises(J.JpgeError):
        J.decode_coeffs(b.jpg[:len(b.jpg) - 6])
    bad = bytearray(b.jpg)  # a two-component frame is not a jpge stream
    bad[bad.index(b"\xff\xc0") + 9] = 2
    with pytest.raises(J.JpgeError):
        J.decode_coeffs(bytes(bad))


@pytest.mark.parametrize("w,h", [(1, 1), (7, 5), (17, 8), (136, 16), (50, 33)])
@pytest.mark.parametrize("quality", [50, 100])
def test_builder_coefficients_are_the_yuv_y_plane(w, h, quality):
    y = G.plane("random", w, h, seed=w + h)
    c = np.full((h, w), 128, np.uint8)
    planes = Y.pad_planes(Y.YUV444, y, c, c, mcu=(8, 8))
    assert np.array_equal(G.coefficients(y, _oracle.quality_tables(quality)[0]), Y.want_coeffs(planes, 444, quality)[0])


def test_segments():
    # the header is exactly the listed segments, in order
    b = G.built("photo", 40, 24, 90, 7)
    d = b.jpg
    assert d[:20] == G.SOI_APP0 and d[20:25] == bytes([0xFF, 0xDB, 0x00, 0x43, 0x00])
    assert d[89:102] == bytes([0xFF, 0xC0, 0x00, 0x0B, 0x08, 0, 24, 0, 40, 1, 1, 0x11, 0])
    pos, seen = 102, []
    while d[pos + 1] != 0xDA:
        seen.append((d[pos + 1], d[pos + 4]))
        pos += 2 + (d[pos + 2] << 8 | d[pos + 3])
    assert seen == [(0xC4, 0x00), (0xC4, 0x10), (0xDD, 0x00)]
    assert d[pos:pos + 10] == G.SOS and d[-2:] == b"\xff\xd9"
    # 15 blocks in intervals of 7: RST0 and RST1, and no other marker in the entropy data
    body = d[pos + 10:-2]
    marks = [body[i + 1] for i in range(len(body) - 1) if body[i] == 0xFF and body[i + 1] != 0]
    assert marks == [0xD0, 0xD1]


def test_input_format_info():
    assert J.JPGE_FMT_GRAY8 == 8
    assert J.input_format_info(J.JPGE_FMT_GRAY8) == (1, 1)


def test_frame_geom():
    a = np.zeros((5, 7), np.uint8)
    assert J._frame_geom(a, J.JPGE_FMT_GRAY8) == (7, 5, 7)
    for bad in (np.zeros((5, 7, 1), np.uint8), np.zeros((5, 7, 3), np.uint8), np.zeros(35, np.uint8),
                np.zeros((5, 7), np.float32), np.zeros((5, 7), np.uint16), np.zeros((0, 7), np.uint8)):
        with pytest.raises(ValueError, match="GRAY8"):
            J._frame_geom(bad, J.JPGE_FMT_GRAY8)
        with pytest.raises(ValueError, match="GRAY8"):
            J._as_frame(bad, J.JPGE_FMT_GRAY8)
    with pytest.raises(ValueError):  # and a gray plane is no colour frame
        J._frame_geom(a, J.JPGE_FMT_RGB8)
    # a non-contiguous view is taken as its contiguous copy
    v = np.arange(70, dtype=np.uint8).reshape(5, 14)[:, ::2]
    f, w, h, stride = J._as_frame(v, J.JPGE_FMT_GRAY8)
    assert (w, h, stride) == (7, 5, 7) and f.flags.c_contiguous and np.array_equal(f, v)


@pytest.mark.parametrize("w,h,restart", [(7, 5, 0), (136, 16, 3), (64, 64, 0)])
@pytest.mark.parametrize("kind", ["photo", "zeros"])
def test_pil_opens_the_builders_file(kind, w, h, restart):
    Image = pytest.importorskip("PIL.Image")
    b = G.built(kind, w, h, 90, restart)
    im = Image.open(io.BytesIO(b.jpg))
    assert im.mode == "L" and im.size == (w, h)
    im.load()
    # and its pixels are the plane's, to within the quantiser's error at quality 90
    got = np.asarray(im, np.float64)
    assert np.abs(got - G.plane(kind, w, h).astype(np.float64)).mean() < 8.0


PPMS = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ppm", "*.ppm")))


@pytest.mark.parametrize("path", PPMS, ids=[os.path.basename(p)[:-4] for p in PPMS])
def test_three_component_files_still_decode(path):
    # every golden image as the oracle's three-component file: the decoder returns the
    # oracle's coefficients, three planes, and the chroma table
    ppm = J.load_ppm(path)
    info, y, cb, cr = J.decode_coeffs(_oracle.encode(ppm.rgb, 50, maxval=ppm.maxval))
    qy, qc = _oracle.quality_tables(50)
    assert (info.width, info.height, info.yh, info.yv) == (ppm.width, ppm.height, 2, 2)
    assert info.c_blocks == cb.shape[0] == cr.shape[0] > 0
    assert bytes(info.qy) == qy.tobytes() and bytes(info.qc) == qc.tobytes()
    for got, want in zip((y, cb, cr), _oracle.stage_coeffs(ppm.rgb, 50, maxval=ppm.maxval)):
        assert np.array_equal(got, want)
