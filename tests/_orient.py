"""Orientation inside K1 (jpge_set_orientation): the table of include/jpge.h as numpy
expressions, test frames, and the device views of the GPU tests."""
import numpy as np

import jpgenc_amd as J

RGB8, BGR8, RGBA8, BGRA8 = J.JPGE_FMT_RGB8, J.JPGE_FMT_BGR8, J.JPGE_FMT_RGBA8, J.JPGE_FMT_BGRA8
FORMATS = (RGB8, BGR8, RGBA8, BGRA8)
NAMES = {RGB8: "rgb8", BGR8: "bgr8", RGBA8: "rgba8", BGRA8: "bgra8"}
BPP = {RGB8: 3, BGR8: 3, RGBA8: 4, BGRA8: 4}
ORIENTS = tuple(range(8))
ONAMES = ("none", "flip-h", "rot180", "flip-v", "transpose", "rot90", "transverse", "rot270")
INVERSE = (0, 1, 2, 3, 4, 7, 6, 5)  # 5 and 7 undo each other; the others undo themselves
TRANSPOSED = (4, 5, 6, 7)

# the table's numpy column: a is (H, W, C)
RULE = (
    lambda a: a,
    lambda a: a[:, ::-1],
    lambda a: a[::-1, ::-1],
    lambda a: a[::-1],
    lambda a: a.transpose(1, 0, 2),
    lambda a: np.rot90(a, -1),
    lambda a: np.rot90(a, 2).transpose(1, 0, 2),
    lambda a: np.rot90(a, 1),
)


def rule(a: np.ndarray, o: int) -> np.ndarray:
    return np.ascontiguousarray(RULE[o](np.asarray(a)))


def formula(a: np.ndarray, o: int) -> np.ndarray:
    """The table's O(y, x) column, pixel by pixel (small frames)."""
    a = np.asarray(a)
    hs, ws = a.shape[:2]
    ow, oh = (hs, ws) if o >= 4 else (ws, hs)
    src = (
        lambda y, x: (y, x), lambda y, x: (y, ws - 1 - x), lambda y, x: (hs - 1 - y, ws - 1 - x),
        lambda y, x: (hs - 1 - y, x), lambda y, x: (x, y), lambda y, x: (hs - 1 - x, y),
        lambda y, x: (hs - 1 - x, ws - 1 - y), lambda y, x: (x, ws - 1 - y),
    )[o]
    out = np.zeros((oh, ow, a.shape[2]), np.uint8)
    for y in range(oh):
        for x in range(ow):
            out[y, x] = a[src(y, x)]
    return out


def make(fmt: int, w: int, h: int, seed: int = 0) -> np.ndarray:
    """A w x h frame of random bytes in layout fmt (alpha: anything)."""
    rng = np.random.default_rng(seed * 1000003 + w * 65537 + h)
    return rng.integers(0, 256, (h, w, BPP[fmt]), dtype=np.uint8)


def to_rgb(frame, fmt: int) -> np.ndarray:
    """The (H, W, 3) R, G, B frame of an interleaved one (the oracle's input)."""
    a = np.asarray(frame)
    return np.ascontiguousarray(a[:, :, 2::-1] if fmt in (BGR8, BGRA8) else a[:, :, :3])


POISON = 0xC3


def device_view(torch, frame, variant: str):
    """The frame in device memory as a strided tensor for encode_tensor.  aligned: a 16-byte
    aligned base and pitch; unaligned: base + 1 and an odd pitch; padded: an aligned pitch of a
    row's bytes + 48 and more.  The bytes around the rows are poison."""
    h, w, bpp = frame.shape
    row = w * bpp
    al = -(-row // 16) * 16
    off, st = {"aligned": (0, al), "unaligned": (1, al + 17), "padded": (0, al + 48)}[variant]
    host = np.full(off + st * h + 64, POISON, np.uint8)
    host[off:off + st * h].reshape(h, st)[:, :row] = np.asarray(frame).reshape(h, row)
    dev = torch.from_numpy(host).cuda()
    return torch.as_strided(dev, (h, w, bpp), (st, bpp, 1), off)
