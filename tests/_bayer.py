"""8-bit Bayer input (JPGE_FMT_BAYER_*): the demosaic rule of include/jpge.h as numpy expressions,
test frames, and the device views of the GPU tests."""
import numpy as np

import jpgenc_amd as J

RGGB, GRBG, GBRG, BGGR = J.JPGE_FMT_BAYER_RGGB8, J.JPGE_FMT_BAYER_GRBG8, J.JPGE_FMT_BAYER_GBRG8, J.JPGE_FMT_BAYER_BGGR8
FORMATS = (RGGB, GRBG, GBRG, BGGR)
NAMES = {RGGB: "rggb", GRBG: "grbg", GBRG: "gbrg", BGGR: "bggr"}
LAYOUTS = {f: "bayer_" + n for f, n in NAMES.items()}
# the colours (0 R, 1 G, 2 B) of the 2x2 cell at rows 0-1, columns 0-1, as the names spell them
CELL = {f: np.array(["rgb".index(c) for c in NAMES[f]]).reshape(2, 2) for f in FORMATS}


def colours(fmt: int, h: int, w: int) -> np.ndarray:
    """(h, w): the colour index of every site, cell[y & 1][x & 1]."""
    return CELL[fmt][np.arange(h)[:, None] & 1, np.arange(w)[None, :] & 1]


def rule(a: np.ndarray, fmt: int) -> np.ndarray:
    """jpge.h's rule, stated with np.pad(mode="reflect") and slices: (H, W) uint8 -> (H, W, 3)."""
    a = np.asarray(a)
    h, w = a.shape
    v = np.pad(a.astype(np.int32), 1, mode="reflect")  # v[y + 1, x + 1] = V(y, x), y, x = -1 .. n
    c = v[1:-1, 1:-1]
    up, down, left, right = v[:-2, 1:-1], v[2:, 1:-1], v[1:-1, :-2], v[1:-1, 2:]
    plus = (up + down + left + right + 2) >> 2
    diag = (v[:-2, :-2] + v[:-2, 2:] + v[2:, :-2] + v[2:, 2:] + 2) >> 2
    rowm, colm = (left + right + 1) >> 1, (up + down + 1) >> 1
    col = colours(fmt, h, w)
    # the colour of a G site's row: that of the site beside it (of the other column parity, same row)
    row_colour = CELL[fmt][np.arange(h)[:, None] & 1, (np.arange(w)[None, :] & 1) ^ 1]
    out = np.zeros((h, w, 3), np.int32)
    for k in (0, 2):  # R, B
        out[..., k] = np.where(col == k, c, np.where(col == 1, np.where(row_colour == k, rowm, colm), diag))
    out[..., 1] = np.where(col == 1, c, plus)
    return out.astype(np.uint8)


def mosaic(rgb: np.ndarray, fmt: int) -> np.ndarray:
    """The (H, W) mosaic that samples an (H, W, 3) frame: each site keeps its own colour."""
    h, w = rgb.shape[:2]
    return np.ascontiguousarray(np.take_along_axis(np.asarray(rgb), colours(fmt, h, w)[..., None], 2)[..., 0])


def noise(w: int, h: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(seed * 1000003 + w * 65537 + h)
    return rng.integers(0, 256, (h, w), dtype=np.uint8)


def checker(w: int, h: int, which: int) -> np.ndarray:
    """0 / 255 by site, which = 0..7: the sites of one of the 2x2 cell's four positions,
    (x & 1) + 2 * (y & 1) == which & 3, are 255 and the others 0; which >= 4 inverts the frame.
    Sums of four reach 0 and 1020, sums of two 0, 255 and 510: every rounding of the rule."""
    y, x = np.arange(h)[:, None] & 1, np.arange(w)[None, :] & 1
    hit = (x + 2 * y) == (which & 3)
    return np.where(hit ^ bool(which & 4), 255, 0).astype(np.uint8)


def single_pixels(w: int, h: int):
    """Frames that are 0 but for one 255 byte, at the columns and rows where the kernels' tiles,
    runs and halos meet (those that exist in a w x h frame)."""
    xs = sorted({x for x in (0, 15, 16, 63, 64, w - 1) if x < w})
    ys = sorted({y for y in (0, 7, 8, 15, 16, h - 1) if y < h})
    for y in ys:
        for x in xs:
            a = np.zeros((h, w), np.uint8)
            a[y, x] = 255
            yield (x, y), a


POISON = 0xC3
VARIANTS = ("host", "aligned", "unaligned", "padded")


def device_view(torch, frame, variant: str):
    """The (H, W) frame in device memory as a strided tensor for encode_tensor.  aligned: a 16-byte
    aligned base and pitch; unaligned: base + 1 and an odd pitch; padded: an aligned pitch of a
    row's bytes + 48 and more.  The bytes around the rows are poison."""
    h, w = frame.shape
    al = -(-w // 16) * 16
    off, st = {"aligned": (0, al), "unaligned": (1, al + 17), "padded": (0, al + 48)}[variant]
    host = np.full(off + st * h + 64, POISON, np.uint8)
    host[off:off + st * h].reshape(h, st)[:, :w] = np.asarray(frame)
    dev = torch.from_numpy(host).cuda()
    return torch.as_strided(dev, (h, w), (st, 1), off)
