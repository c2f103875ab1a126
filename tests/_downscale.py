"""Box downscale (jpge_set_downscale): the rule of jpge.h in numpy integer arithmetic, and the
test frames.  A sample of the downscaled frame D is (sum of its s x s source samples +
s*s/2) // (s*s), the source coordinates clamped to the plane; NV12's Cb,Cr plane in its own
domain.  test_downscale_cpu.py pins jpge_downscale_frame to this file; the GPU tests then use
that function for D."""
import numpy as np

import _yuv as Y
import jpgenc_amd as J

RGB8, BGR8, RGBA8, BGRA8, NV12 = J.JPGE_FMT_RGB8, J.JPGE_FMT_BGR8, J.JPGE_FMT_RGBA8, J.JPGE_FMT_BGRA8, J.JPGE_FMT_NV12
FORMATS = (RGB8, BGR8, RGBA8, BGRA8, NV12)
NAMES = {RGB8: "rgb8", BGR8: "bgr8", RGBA8: "rgba8", BGRA8: "bgra8", NV12: "nv12"}
BPP = {RGB8: 3, BGR8: 3, RGBA8: 4, BGRA8: 4}
FACTORS = (2, 4)
KINDS = ("random", "ones", "tie", "below")


def box(a: np.ndarray, s: int) -> np.ndarray:
    """(H, W, C) uint8 -> (ceil(H/s), ceil(W/s), C): clamping a coordinate is repeating the last row / column."""
    h, w = a.shape[:2]
    dh, dw = -(-h // s), -(-w // s)
    p = np.pad(a.astype(np.int64), ((0, dh * s - h), (0, dw * s - w), (0, 0)), mode="edge")
    t = p.reshape(dh, s, dw, s, -1).sum(axis=(1, 3))
    return ((t + s * s // 2) // (s * s)).astype(np.uint8)


def split_nv12(f):
    """(y, cbcr) of a pack_yuv420 NV12 frame: (H, W) and (ch, cw, 2)."""
    w, h, st = f.width, f.height, f.stride
    ch, cw = (h + 1) // 2, (w + 1) // 2
    a = np.asarray(f).reshape(h + ch, st)
    return a[:h, :w].copy(), a[h:, :2 * cw].reshape(ch, cw, 2).copy()


def rule(frame, fmt: int, s: int):
    """D of `frame` (shaped as Encoder.encode takes it for layout fmt), in the same shape."""
    if fmt == NV12:
        y, c = split_nv12(frame)
        dy, dc = box(y[:, :, None], s)[:, :, 0], box(c, s)
        return J.pack_yuv420(NV12, dy, dc[:, :, 0], dc[:, :, 1])[0]
    if s == 1:
        return np.array(frame, np.uint8)
    d = box(np.asarray(frame)[:, :, :3], s)
    if BPP[fmt] == 4:  # (alpha is ignored: D is opaque)
        d = np.concatenate([d, np.full(d.shape[:2] + (1,), 255, np.uint8)], axis=2)
    return d


def _plane(rng, h: int, w: int, c: int, s: int, kind: str) -> np.ndarray:
    if kind == "random":
        return rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    if kind == "ones":
        return np.full((h, w, c), 255, np.uint8)
    # tie: every whole s x s cell sums to k*s*s + s*s/2 (the first s*s/2 samples of the cell are
    # k + 1, the others k): the mean rounds up to k + 1.  below: one sample fewer, it rounds to k.
    n = s * s // 2 - (kind == "below")
    k = rng.integers(0, 255, (-(-h // s), -(-w // s), c), dtype=np.uint8)
    a = np.repeat(np.repeat(k, s, axis=0), s, axis=1)[:h, :w].copy()
    yy, xx = np.mgrid[0:h, 0:w]
    a[((yy % s) * s + xx % s) < n] += 1
    return a


def make(fmt: int, w: int, h: int, kind: str = "random", seed: int = 0, s: int = 2):
    """A w x h test frame in layout fmt (kinds: KINDS; s: the cell size of the tie frames)."""
    rng = np.random.default_rng(seed * 1000003 + w * 65537 + h)
    if fmt == NV12:
        ch, cw = (h + 1) // 2, (w + 1) // 2
        y, c = _plane(rng, h, w, 1, s, kind)[:, :, 0], _plane(rng, ch, cw, 2, s, kind)
        return J.pack_yuv420(NV12, y, c[:, :, 0], c[:, :, 1])[0]
    a = _plane(rng, h, w, BPP[fmt], s, kind)
    if BPP[fmt] == 4 and kind != "ones":
        a[:, :, 3] = rng.integers(0, 256, (h, w), dtype=np.uint8)  # (alpha: anything)
    return a


def same(a, b) -> bool:
    return np.array_equal(np.asarray(a), np.asarray(b)) and np.asarray(a).shape == np.asarray(b).shape


def to_rgb(frame, fmt: int) -> np.ndarray:
    """The (H, W, 3) R, G, B frame of an interleaved one (the oracle's input)."""
    a = np.asarray(frame)
    return np.ascontiguousarray(a[:, :, 2::-1] if fmt in (BGR8, BGRA8) else a[:, :, :3])


def nv12_planes(frame):
    """(fmt, y, cb, cr) of an NV12 frame, as _yuv.pad_planes takes them."""
    y, c = split_nv12(frame)
    return Y.NV12, y, c[:, :, 0].copy(), c[:, :, 1].copy()
