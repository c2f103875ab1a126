"""Input-layout helpers of the format tests: an RGB frame rearranged with numpy into each
layout the encoder reads (jpge.h JPGE_FMT_*), and back.  test_formats_cpu.py checks that
they round-trip, so the GPU tests' expectation, _oracle.encode of the RGB frame, does
not rest on an unchecked helper."""
import numpy as np

import jpgenc_amd as J

NEW_FORMATS = (J.JPGE_FMT_BGR8, J.JPGE_FMT_RGBA8, J.JPGE_FMT_BGRA8, J.JPGE_FMT_RGB8_PLANAR)
ALL_FORMATS = (J.JPGE_FMT_RGB8,) + NEW_FORMATS
NAMES = {J.JPGE_FMT_RGB8: "rgb8", J.JPGE_FMT_BGR8: "bgr8", J.JPGE_FMT_RGBA8: "rgba8", J.JPGE_FMT_BGRA8: "bgra8",
         J.JPGE_FMT_RGB8_PLANAR: "planar"}


def to_format(rgb: np.ndarray, fmt: int, alpha=None, seed: int = 5) -> np.ndarray:
    """The (H, W, 3) RGB frame in layout fmt: (H, W, 3), (H, W, 4) or (3, H, W).
    alpha: the 4-byte layouts' alpha plane (default: random bytes)."""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    h, w = rgb.shape[:2]
    if fmt == J.JPGE_FMT_RGB8:
        return rgb.copy()
    if fmt == J.JPGE_FMT_BGR8:
        return np.ascontiguousarray(rgb[:, :, ::-1])
    if fmt in (J.JPGE_FMT_RGBA8, J.JPGE_FMT_BGRA8):
        if alpha is None:
            alpha = np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)
        a = np.broadcast_to(np.asarray(alpha, np.uint8), (h, w))[:, :, None]
        c = rgb if fmt == J.JPGE_FMT_RGBA8 else rgb[:, :, ::-1]
        return np.ascontiguousarray(np.concatenate([c, a], axis=2))
    if fmt == J.JPGE_FMT_RGB8_PLANAR:
        return np.ascontiguousarray(rgb.transpose(2, 0, 1))
    raise ValueError(fmt)


def from_format(a: np.ndarray, fmt: int) -> np.ndarray:
    """Back to (H, W, 3) RGB."""
    if fmt == J.JPGE_FMT_RGB8:
        return np.ascontiguousarray(a)
    if fmt == J.JPGE_FMT_BGR8:
        return np.ascontiguousarray(a[:, :, ::-1])
    if fmt == J.JPGE_FMT_RGBA8:
        return np.ascontiguousarray(a[:, :, :3])
    if fmt == J.JPGE_FMT_BGRA8:
        return np.ascontiguousarray(a[:, :, 2::-1])
    if fmt == J.JPGE_FMT_RGB8_PLANAR:
        return np.ascontiguousarray(a.transpose(1, 2, 0))
    raise ValueError(fmt)


def padded(frame: np.ndarray, fmt: int, stride: int, plane_stride: int = 0, offset: int = 0, seed: int = 9):
    """The frame laid out in a flat buffer of random bytes with the given row stride
    (and, planar, plane stride; 0 = stride * height), starting `offset` bytes in.
    Returns (buffer, offset of the first pixel, plane stride used)."""
    planar = fmt == J.JPGE_FMT_RGB8_PLANAR
    planes = frame if planar else frame[None].reshape(1, frame.shape[0], -1)
    n, h, row = planes.shape
    assert stride >= row
    ps = plane_stride or stride * h
    assert not planar or ps >= stride * (h - 1) + row
    size = offset + (n - 1) * ps + stride * (h - 1) + row + 64
    buf = np.random.default_rng(seed).integers(0, 256, size, dtype=np.uint8)
    for c in range(n):
        for y in range(h):
            o = offset + c * ps + y * stride
            buf[o:o + row] = planes[c, y]
    return buf, offset, (ps if planar else 0)
