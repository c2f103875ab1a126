"""Per-channel lookup tables (jpge_set_channel_lut): the tables the tests use, the rule of
include/jpge.h as a numpy expression, test frames in the eight layouts, and the device views of the
GPU tests."""
import numpy as np

import _bayer as B
import jpgenc_amd as J

RGB8, BGR8, RGBA8, BGRA8 = J.JPGE_FMT_RGB8, J.JPGE_FMT_BGR8, J.JPGE_FMT_RGBA8, J.JPGE_FMT_BGRA8
INTERLEAVED = (RGB8, BGR8, RGBA8, BGRA8)
LAYOUTS = INTERLEAVED + B.FORMATS
NAMES = {RGB8: "rgb8", BGR8: "bgr8", RGBA8: "rgba8", BGRA8: "bgra8", **B.NAMES}
CHANNELS = {RGB8: 3, BGR8: 3, RGBA8: 4, BGRA8: 4}
# the byte offset of R, G, B in a pixel
OFFSETS = {RGB8: (0, 1, 2), RGBA8: (0, 1, 2), BGR8: (2, 1, 0), BGRA8: (2, 1, 0)}


def _tables():
    i = np.arange(256)
    rng = np.random.default_rng(20240917)
    gamma = np.round(255.0 * (i / 255.0) ** (1 / 2.2)).astype(np.uint8)
    return {
        "identity": np.broadcast_to(i.astype(np.uint8), (3, 256)).copy(),
        "invert": np.broadcast_to((255 - i).astype(np.uint8), (3, 256)).copy(),
        # three different permutations: a swapped channel or a BGR mix-up changes the frame
        "perm": np.stack([rng.permutation(256).astype(np.uint8) for _ in range(3)]),
        "perm2": np.stack([rng.permutation(256).astype(np.uint8) for _ in range(3)]),
        "gamma": np.broadcast_to(gamma, (3, 256)).copy(),
        "const": np.stack([np.full(256, v, np.uint8) for v in (17, 200, 99)]),
    }


TABLES = _tables()


def rule(a: np.ndarray, fmt: int, lut: np.ndarray) -> np.ndarray:
    """jpge.h's rule for an interleaved frame, in its own layout: lut[c][a[..., offset of c]]; a
    fourth byte is copied."""
    out = np.array(a)
    for c, k in enumerate(OFFSETS[fmt]):
        out[..., k] = lut[c][a[..., k]]
    return out


def rgb_of(a: np.ndarray, fmt: int) -> np.ndarray:
    """D: the (H, W, 3) RGB8 frame of a frame in any of the eight layouts."""
    if fmt in B.FORMATS:
        return J.demosaic_frame(a, fmt)
    return np.ascontiguousarray(a[..., list(OFFSETS[fmt])])


def mapped(a: np.ndarray, fmt: int, lut: np.ndarray) -> np.ndarray:
    """M: the RGB8 frame an encode of `a` with the tables `lut` codes."""
    d = rgb_of(a, fmt)
    return np.stack([lut[c][d[..., c]] for c in range(3)], axis=-1)


def noise(fmt: int, w: int, h: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(seed * 1000003 + w * 65537 + h * 257 + fmt)
    shape = (h, w) if fmt in B.FORMATS else (h, w, CHANNELS[fmt])
    return rng.integers(0, 256, shape, dtype=np.uint8)


POISON = 0xC3
VARIANTS = ("aligned", "unaligned", "host")


def device_view(torch, frame, variant: str):
    """The (H, W) or (H, W, C) frame in device memory as a strided tensor for encode_tensor.
    aligned: a 16-byte aligned base and pitch; unaligned: base + 1 and an odd pitch, so that every
    tile takes the byte path.  The bytes around the rows are poison."""
    h, w = frame.shape[:2]
    c = frame.shape[2] if frame.ndim == 3 else 1
    row = w * c
    al = -(-row // 16) * 16
    off, st = {"aligned": (0, al), "unaligned": (1, al + 17)}[variant]
    host = np.full(off + st * h + 64, POISON, np.uint8)
    host[off:off + st * h].reshape(h, st)[:, :row] = np.asarray(frame).reshape(h, row)
    dev = torch.from_numpy(host).cuda()
    if frame.ndim == 2:
        return torch.as_strided(dev, (h, w), (st, 1), off)
    return torch.as_strided(dev, (h, w, c), (st, c, 1), off)


def tensor_kwargs(fmt: int) -> dict:
    """encode_tensor's arguments for a device view in layout fmt."""
    if fmt in B.FORMATS:
        return {"layout": B.LAYOUTS[fmt]}
    return {"order": "bgr" if fmt in (BGR8, BGRA8) else "rgb", "layout": "hwc"}
