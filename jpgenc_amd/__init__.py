"""jpge — MI355X-native JPEG baseline encoder (Python side of the C ABI).

This module is a thin ctypes binding over ``jpgenc_amd/lib/libjpge.so`` (the
HIP kernels + host C++; see ``include/jpge.h``).  It mirrors the reference's
entry points — ``load_ppm`` (Image.hpp:28 ``loadPPM``) and
``Encoder.encode`` / ``write_jpeg`` (Image.hpp:92 ``Image::writeJPEG``) — and
raises ``JpgeError`` (a ``RuntimeError``, the reference's ``std::runtime_error``
convention, Image.cpp:428/450) on failure.  There is no CPU fallback: if the
library or a GPU is missing, calls fail loudly.
"""
from __future__ import annotations

import atexit
import ctypes
import os
import weakref
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("JPGE_LIB") or os.path.join(_HERE, "lib", "libjpge.so")

JPGE_DEVICE_INPUT = 1
JPGE_DEVICE_OUTPUT = 2

#: input layouts (jpge.h JPGE_FMT_*): interleaved (H, W, 3) / (H, W, 4) frames, or planar (3, H, W)
JPGE_FMT_RGB8, JPGE_FMT_BGR8, JPGE_FMT_RGBA8, JPGE_FMT_BGRA8, JPGE_FMT_RGB8_PLANAR = 0, 1, 2, 3, 4
#: full-range 8-bit Y, Cb, Cr frames (no colour conversion): NV12 and I420 (chroma at half size;
#: host frames from pack_yuv420), and planar (3, H, W)
JPGE_FMT_NV12, JPGE_FMT_I420, JPGE_FMT_YUV444_PLANAR = 16, 17, 18
#: 10-bit 4:2:0 frames of little-endian 16-bit words (jpge.h): P010 (NV12's planes, a sample in its
#: word's top 10 bits) and I010 / yuv420p10le (I420's planes, a sample in the low 10 bits); a
#: sample s enters the sample transform as s / 4, unrounded
JPGE_FMT_P010, JPGE_FMT_I010 = 32, 33
#: 10-bit 4:2:2 frames of the same words (one Cb, Cr per horizontal pixel pair of every row): Y210
#: (packed groups Y0 Cb Y1 Cr, top 10 bits), P210 (NV16's planes, top 10 bits) and I210 /
#: yuv422p10le (I422's planes, low 10 bits); host frames from pack_yuv422p10
JPGE_FMT_Y210, JPGE_FMT_P210, JPGE_FMT_I210 = 40, 41, 42
#: v210 (10-bit SDI capture; QuickTime / AVI "uncompressed 10-bit"): the same samples, three to a
#: 32-bit word, six pixels in 16 bytes; host frames from pack_v210
JPGE_FMT_V210 = 48
# orientations (jpge.h JPGE_ORIENT_*): the operation applied to the pixels
JPGE_ORIENT_NONE, JPGE_ORIENT_FLIP_H, JPGE_ORIENT_ROT180, JPGE_ORIENT_FLIP_V = 0, 1, 2, 3
JPGE_ORIENT_TRANSPOSE, JPGE_ORIENT_ROT90, JPGE_ORIENT_TRANSVERSE, JPGE_ORIENT_ROT270 = 4, 5, 6, 7
#: 4:2:2 frames of the same samples (one Cb, Cr per horizontal pixel pair of every row): packed
#: Y0 Cb Y1 Cr / Cb Y0 Cr Y1 groups, NV16 (Y plane + Cb,Cr rows), I422 (three planes); host
#: frames from pack_yuv422
JPGE_FMT_YUYV, JPGE_FMT_UYVY, JPGE_FMT_NV16, JPGE_FMT_I422 = 20, 21, 22, 23
#: one (H, W) plane of 8-bit luminance -> a one-component (grayscale) JPEG; no chroma: the
#: chroma table and the subsampling mode do not enter
JPGE_FMT_GRAY8 = 8
#: 8-bit Bayer mosaics (jpge.h): one (H, W) plane of raw bytes, the name the colours of the 2x2
#: cell at rows 0-1, columns 0-1; coded as the RGB8 frame demosaic_frame returns
JPGE_FMT_BAYER_RGGB8, JPGE_FMT_BAYER_GRBG8, JPGE_FMT_BAYER_GBRG8, JPGE_FMT_BAYER_BGGR8 = 10, 11, 12, 13
#: the Bayer layouts by their encode_tensor(layout=...) names
BAYER_LAYOUTS = {"bayer_rggb": JPGE_FMT_BAYER_RGGB8, "bayer_grbg": JPGE_FMT_BAYER_GRBG8,
                 "bayer_gbrg": JPGE_FMT_BAYER_GBRG8, "bayer_bggr": JPGE_FMT_BAYER_BGGR8}
_BAYER = frozenset(BAYER_LAYOUTS.values())

#: Huffman modes (jpge.h JPGE_HUFF_*): per-image tables (the reference's stream, the default),
#: the ITU T.81 Annex K tables, or the caller's four tables
JPGE_HUFF_OPTIMAL, JPGE_HUFF_STANDARD, JPGE_HUFF_CUSTOM = 0, 1, 2

#: sample transforms of Y, Cb, Cr and gray input (jpge.h JPGE_YUV_*): full-range BT.601 (JFIF's
#: own samples, the default), studio swing with the BT.601 or the BT.709 matrix, full-range
#: BT.709, or the caller's coefficients; converted inside the transform kernel
JPGE_YUV_FULL_601, JPGE_YUV_LIMITED_601, JPGE_YUV_LIMITED_709, JPGE_YUV_FULL_709, JPGE_YUV_CUSTOM = 0, 1, 2, 3, 4

#: subsampling modes (jpge.h JPGE_S*) -> (Y blocks across, Y blocks down) an MCU
SUBSAMPLING = {420: (2, 2), 4200: (2, 2), 4201: (2, 2), 444: (1, 1), 422: (2, 1), 411: (4, 1)}

STATUS = {
    0: "JPGE_OK", 1: "JPGE_E_ARG", 2: "JPGE_E_NOSPACE", 3: "JPGE_E_HIP", 4: "JPGE_E_NODEV",
    5: "JPGE_E_FORMAT", 6: "JPGE_E_IO", 7: "JPGE_E_TRUNC", 8: "JPGE_E_RANGE", 9: "JPGE_E_TIMEOUT",
    10: "JPGE_E_RCCL", 11: "JPGE_E_INTERNAL",
}

# every symbol include/jpge.h declares (checked by tests/test_abi.py)
EXPORTS = (
    "jpge_strerror", "jpge_version", "jpge_device_count", "jpge_open", "jpge_open_ex", "jpge_close", "jpge_set_timing",
    "jpge_get_timing", "jpge_reset_timing", "jpge_get_lanes", "jpge_set_restart_interval", "jpge_set_subsampling",
    "jpge_set_input_format", "jpge_get_input_format", "jpge_input_format_info", "jpge_demosaic_frame",
    "jpge_set_channel_lut", "jpge_get_channel_lut", "jpge_lut_frame",
    "jpge_v210_row_bytes", "jpge_v210_unpack",
    "jpge_set_huffman", "jpge_get_huffman", "jpge_standard_huffman",
    "jpge_set_yuv_transform", "jpge_get_yuv_transform", "jpge_yuv_preset",
    "jpge_set_downscale", "jpge_get_downscale", "jpge_downscaled_size", "jpge_downscale_frame",
    "jpge_set_orientation", "jpge_get_orientation", "jpge_oriented_size", "jpge_orient_frame",
    "jpge_max_jpeg_bytes", "jpge_quality_tables", "jpge_encode_rgb8", "jpge_encode_batch",
    "jpge_fdct_quant", "jpge_symbol_stats", "jpge_huffman_table", "jpge_huffman_text", "jpge_parse_ppm",
    "jpge_ppm_info", "jpge_encode_file", "jpge_encode_files", "jpge_synth_rgb8", "jpge_arai_constants",
    "jpge_stripe_transform", "jpge_stripe_stats", "jpge_stripe_code", "jpge_stripe_place", "jpge_stripe_pack",
    "jpge_huffman_decode", "jpge_idct8x8", "jpge_decode_coeffs",
    "jpge_zigzag_index", "jpge_zigzag_block", "jpge_quantize_block", "jpge_rle_ac", "jpge_category_code",
    "jpge_encode_category", "jpge_dc_difference", "jpge_color_convert", "jpge_subsample_plane", "jpge_dct_plane",
    "jpge_quantize_plane", "jpge_encode_planes",
    "jpge_group_open", "jpge_group_close", "jpge_group_size", "jpge_group_context", "jpge_group_set_restart_interval",
    "jpge_group_encode_batch", "jpge_group_encode_striped", "jpge_concat_segments",
)

JPGE_TO_RGB, JPGE_TO_YCBCR = 0, 1
DCT_SIMPLE, DCT_MATRIX, DCT_ARAI = 0, 1, 2


class JpgeError(RuntimeError):
    def __init__(self, status: int, what: str = ""):
        self.status = status
        msg = lib().jpge_strerror(status).decode() if _LIB is not None else STATUS.get(status, str(status))
        super().__init__(f"{what}: {STATUS.get(status, status)} ({msg})" if what else msg)


class Frame(ctypes.Structure):
    _fields_ = [
        ("rgb", ctypes.c_void_p), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32),
        ("stride", ctypes.c_size_t), ("maxval", ctypes.c_int), ("out", ctypes.c_void_p),
        ("cap", ctypes.c_size_t), ("len", ctypes.c_size_t), ("status", ctypes.c_int),
    ]


class StripeSummary(ctypes.Structure):
    """jpge_stripe_summary: a stripe's bit count, inside-0xFF count per start
    alignment, first and last 8 bits."""
    _fields_ = [("bits", ctypes.c_uint64), ("ff", ctypes.c_uint32 * 8), ("head", ctypes.c_uint32),
                ("tail", ctypes.c_uint32), ("restart", ctypes.c_uint32), ("pad", ctypes.c_uint32)]

    def as_tuple(self):
        return (int(self.bits), tuple(int(x) for x in self.ff), int(self.head), int(self.tail), int(self.restart))

    @classmethod
    def from_tuple(cls, t):
        s = cls()
        s.bits, s.head, s.tail = t[0], t[2], t[3]
        s.restart = t[4] if len(t) > 4 else 0
        for i in range(8):
            s.ff[i] = t[1][i]
        return s


class Decoded(ctypes.Structure):
    """jpge_decoded: the frame header of a decoded jpge stream."""
    _fields_ = [("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("yh", ctypes.c_uint32),
                ("yv", ctypes.c_uint32), ("restart", ctypes.c_uint32), ("y_blocks", ctypes.c_size_t),
                ("c_blocks", ctypes.c_size_t), ("qy", ctypes.c_uint8 * 64), ("qc", ctypes.c_uint8 * 64)]


class HuffSpec(ctypes.Structure):
    """jpge_huff_spec: a Huffman table in DHT form (codes per length 1..16, then the symbols)."""
    _fields_ = [("bits", ctypes.c_uint8 * 16), ("huffval", ctypes.c_uint8 * 256)]

    def as_tuple(self) -> tuple[list[int], list[int]]:
        bits = [int(b) for b in self.bits]
        return bits, [int(v) for v in self.huffval[:min(256, sum(bits))]]

    @classmethod
    def from_tuple(cls, t):
        """(bits, huffval): 16 counts and the symbols (at most 256 are kept; a longer
        list still counts in bits, so the library rejects it)."""
        bits, vals = t
        if len(bits) != 16:
            raise ValueError("a Huffman spec has 16 code-length counts")
        s = cls()
        for i, b in enumerate(bits):
            s.bits[i] = int(b)
        for i, v in enumerate(list(vals)[:256]):
            s.huffval[i] = int(v)
        return s


class YuvTransform(ctypes.Structure):
    """jpge_yuv_transform: y_off and m[0..6] of the sample transform (jpge.h):
    Y' = clamp((m0 (y - y_off) + m1 u) + m2 v, 0, 255) - 128, Cb' = clamp(m3 u + m4 v, -128, 127),
    Cr' = clamp(m5 u + m6 v, -128, 127) with u = cb - 128, v = cr - 128."""
    _fields_ = [("y_off", ctypes.c_double), ("m", ctypes.c_double * 7)]

    def as_tuple(self) -> tuple[float, ...]:
        """(y_off, m0, ..., m6)"""
        return (float(self.y_off),) + tuple(float(x) for x in self.m)

    @classmethod
    def from_tuple(cls, t):
        t = [float(x) for x in t]
        if len(t) != 8:
            raise ValueError("a sample transform has 8 coefficients: y_off, m0..m6")
        s = cls()
        s.y_off = t[0]
        for i in range(7):
            s.m[i] = t[1 + i]
        return s


class Timing(ctypes.Structure):
    _fields_ = [("fdct", ctypes.c_float), ("dc_stats", ctypes.c_float), ("entropy", ctypes.c_float),
                ("total", ctypes.c_float), ("fdct_sum", ctypes.c_double), ("dc_stats_sum", ctypes.c_double),
                ("entropy_sum", ctypes.c_double), ("frames", ctypes.c_uint64),
                ("symbols", ctypes.c_uint64), ("code_sum", ctypes.c_double), ("pack_sum", ctypes.c_double),
                ("launches", ctypes.c_uint64), ("gate_timeouts", ctypes.c_uint64)]


_LIB = None


def lib() -> ctypes.CDLL:
    """Load libjpge.so (raises if it has not been built).  A process that also uses
    torch on the GPU must import torch first: torch ships its own HIP runtime, and
    loaded after libjpge's (ROCm's) it finds no GPU."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: run `make` (or __graft_entry__.build())")
        L = ctypes.CDLL(LIB_PATH)
        vp, u32, sz, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_size_t, ctypes.c_int
        L.jpge_strerror.restype = ctypes.c_char_p
        L.jpge_strerror.argtypes = [i32]
        L.jpge_open.argtypes = [i32, ctypes.POINTER(vp)]
        L.jpge_open_ex.argtypes = [i32, i32, ctypes.POINTER(vp)]
        L.jpge_close.argtypes = [vp]
        L.jpge_set_timing.argtypes = [vp, i32]
        L.jpge_get_timing.argtypes = [vp, ctypes.POINTER(Timing)]
        L.jpge_reset_timing.argtypes = [vp]
        L.jpge_get_lanes.argtypes = [vp, ctypes.POINTER(i32)]
        L.jpge_set_restart_interval.argtypes = [vp, u32]
        L.jpge_set_subsampling.argtypes = [vp, i32]
        L.jpge_set_input_format.argtypes = [vp, i32, sz]
        L.jpge_get_input_format.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(sz)]
        L.jpge_input_format_info.argtypes = [i32, ctypes.POINTER(i32), ctypes.POINTER(i32)]
        L.jpge_v210_row_bytes.restype = sz
        L.jpge_v210_row_bytes.argtypes = [u32]
        L.jpge_v210_unpack.argtypes = [vp, u32, u32, sz, vp, vp, vp]
        L.jpge_set_huffman.argtypes = [vp, i32, ctypes.POINTER(HuffSpec)]
        L.jpge_get_huffman.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(HuffSpec)]
        L.jpge_standard_huffman.argtypes = [i32, ctypes.POINTER(HuffSpec)]
        L.jpge_set_yuv_transform.argtypes = [vp, i32, ctypes.POINTER(YuvTransform)]
        L.jpge_get_yuv_transform.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(YuvTransform)]
        L.jpge_yuv_preset.argtypes = [i32, ctypes.POINTER(YuvTransform)]
        L.jpge_set_downscale.argtypes = [vp, i32]
        L.jpge_get_downscale.argtypes = [vp, ctypes.POINTER(i32)]
        L.jpge_downscaled_size.argtypes = [u32, u32, i32, ctypes.POINTER(u32), ctypes.POINTER(u32)]
        L.jpge_downscale_frame.argtypes = [i32, vp, u32, u32, sz, sz, i32, vp, sz, sz]
        L.jpge_set_orientation.argtypes = [vp, i32]
        L.jpge_get_orientation.argtypes = [vp, ctypes.POINTER(i32)]
        L.jpge_oriented_size.argtypes = [u32, u32, i32, ctypes.POINTER(u32), ctypes.POINTER(u32)]
        L.jpge_orient_frame.argtypes = [i32, vp, u32, u32, sz, i32, vp, sz]
        L.jpge_demosaic_frame.argtypes = [i32, vp, u32, u32, sz, vp, sz]
        L.jpge_set_channel_lut.argtypes = [vp, vp]
        L.jpge_get_channel_lut.argtypes = [vp, ctypes.POINTER(i32), vp]
        L.jpge_lut_frame.argtypes = [i32, vp, u32, u32, sz, vp, vp, sz]
        L.jpge_device_count.argtypes = [ctypes.POINTER(i32)]
        L.jpge_max_jpeg_bytes.restype = sz
        L.jpge_max_jpeg_bytes.argtypes = [u32, u32]
        L.jpge_quality_tables.argtypes = [i32, vp, vp]
        L.jpge_encode_rgb8.argtypes = [vp, vp, u32, u32, sz, i32, vp, vp, vp, sz, ctypes.POINTER(sz), u32]
        L.jpge_encode_batch.argtypes = [vp, ctypes.POINTER(Frame), i32, vp, vp, u32]
        L.jpge_fdct_quant.argtypes = [vp, vp, u32, u32, sz, i32, vp, vp, vp, vp, vp, u32]
        L.jpge_symbol_stats.argtypes = [vp, vp, u32, u32, sz, i32, vp, vp, vp, vp, u32]
        L.jpge_stripe_transform.argtypes = [vp, vp, sz, u32, u32, u32, u32, i32, vp, vp, vp]
        L.jpge_stripe_stats.argtypes = [vp, vp, vp, vp]
        L.jpge_stripe_code.argtypes = [vp, vp, vp, ctypes.POINTER(StripeSummary), ctypes.POINTER(sz)]
        L.jpge_stripe_place.argtypes = [ctypes.POINTER(StripeSummary), i32, i32, sz, ctypes.POINTER(sz),
                                        ctypes.POINTER(sz)]
        L.jpge_stripe_pack.argtypes = [vp, ctypes.POINTER(StripeSummary), i32, i32, vp, sz, ctypes.POINTER(sz),
                                       ctypes.POINTER(sz), ctypes.POINTER(sz)]
        L.jpge_huffman_table.argtypes = [vp, vp, vp, vp, ctypes.POINTER(i32), vp, vp]
        L.jpge_concat_segments.argtypes = [i32, vp, vp, vp, i32, vp, ctypes.POINTER(sz)]
        L.jpge_huffman_text.argtypes = [vp, sz, vp, vp, vp, ctypes.POINTER(i32)]
        L.jpge_parse_ppm.argtypes = [vp, sz, vp, sz, ctypes.POINTER(u32), ctypes.POINTER(u32),
                                     ctypes.POINTER(i32)]
        L.jpge_ppm_info.argtypes = [vp, sz, ctypes.POINTER(u32), ctypes.POINTER(u32), ctypes.POINTER(i32)]
        L.jpge_encode_file.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p, i32]
        L.jpge_encode_files.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_char_p), i32,
                                        i32, vp, vp, i32]
        L.jpge_synth_rgb8.argtypes = [ctypes.c_uint64, u32, u32, i32, vp, sz]
        L.jpge_arai_constants.argtypes = [vp, vp]
        L.jpge_arai_constants.restype = None
        L.jpge_huffman_decode.argtypes = [vp, ctypes.c_uint64, vp, vp, vp, i32, vp, sz, ctypes.POINTER(sz)]
        L.jpge_idct8x8.argtypes = [vp, vp]
        L.jpge_idct8x8.restype = None
        L.jpge_decode_coeffs.argtypes = [vp, sz, ctypes.POINTER(Decoded), vp, vp, vp, sz, sz]
        L.jpge_zigzag_index.argtypes = [i32]
        L.jpge_zigzag_block.argtypes = [vp, vp]
        L.jpge_quantize_block.argtypes = [vp, vp, vp]
        L.jpge_rle_ac.argtypes = [vp, sz, i32, vp, vp, sz, ctypes.POINTER(sz)]
        L.jpge_category_code.argtypes = [ctypes.c_int32, ctypes.POINTER(ctypes.c_uint16), ctypes.POINTER(u32)]
        L.jpge_encode_category.argtypes = [vp, vp, sz, vp, vp, vp]
        L.jpge_dc_difference.argtypes = [vp, u32, u32, vp, vp, u32, u32]
        L.jpge_color_convert.argtypes = [vp, vp, vp, vp, vp, vp, vp, sz, i32, u32]
        L.jpge_subsample_plane.argtypes = [vp, vp, u32, u32, i32, vp, ctypes.POINTER(u32), ctypes.POINTER(u32), u32]
        L.jpge_dct_plane.argtypes = [vp, vp, u32, u32, i32, vp, u32]
        L.jpge_quantize_plane.argtypes = [vp, vp, u32, u32, vp, vp, u32]
        L.jpge_encode_planes.argtypes = [vp, vp, vp, vp, u32, u32, i32, u32, u32, vp, vp, vp, sz, ctypes.POINTER(sz),
                                         u32]
        L.jpge_group_open.argtypes = [i32, vp, i32, ctypes.POINTER(vp)]
        L.jpge_group_close.argtypes = [vp]
        L.jpge_group_size.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i32)]
        L.jpge_group_context.argtypes = [vp, i32, ctypes.POINTER(vp)]
        L.jpge_group_set_restart_interval.argtypes = [vp, u32]
        L.jpge_group_encode_batch.argtypes = [vp, ctypes.POINTER(Frame), i32, vp, vp, u32]
        L.jpge_group_encode_striped.argtypes = [vp, vp, u32, u32, sz, i32, vp, vp, vp, sz, ctypes.POINTER(sz)]
        _LIB = L
    return _LIB


def _p(a: np.ndarray) -> int:
    return a.ctypes.data


def _check(st: int, what: str) -> None:
    if st != 0:
        raise JpgeError(st, what)


def quality_tables(quality: int = 50) -> tuple[np.ndarray, np.ndarray]:
    """Annex-K tables scaled for `quality` (50 = the reference's tables, Image.cpp:850-869)."""
    qy = np.zeros(64, np.uint8)
    qc = np.zeros(64, np.uint8)
    _check(lib().jpge_quality_tables(int(quality), _p(qy), _p(qc)), "quality_tables")
    return qy, qc


def synth_rgb8(seed: int, width: int, height: int, kind: int = 0) -> np.ndarray:
    """Deterministic synthetic frame (H, W, 3) uint8: 0 photo-like, 1 random bytes, 2 flat."""
    out = np.empty((height, width, 3), np.uint8)
    _check(lib().jpge_synth_rgb8(seed, width, height, kind, _p(out), width * 3), "synth_rgb8")
    return out


@dataclass
class PPM:
    rgb: np.ndarray  # (H, W, 3) uint8, unscaled samples
    maxval: int

    @property
    def width(self) -> int:
        return self.rgb.shape[1]

    @property
    def height(self) -> int:
        return self.rgb.shape[0]


def parse_ppm(data: bytes) -> PPM:
    """P3/P6 parser with the reference's tokenizer semantics (Image.cpp:334-474)."""
    buf = np.frombuffer(data, np.uint8)
    w, h, mv = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_int()
    _check(lib().jpge_ppm_info(_p(buf), buf.size, ctypes.byref(w), ctypes.byref(h), ctypes.byref(mv)),
           "parse_ppm")
    rgb = np.empty((h.value, w.value, 3), np.uint8)
    _check(lib().jpge_parse_ppm(_p(buf), buf.size, _p(rgb), rgb.size, ctypes.byref(w), ctypes.byref(h),
                                ctypes.byref(mv)), "parse_ppm")
    return PPM(rgb, mv.value)


def load_ppm(path: str) -> PPM:
    """loadPPM (Image.hpp:28)."""
    with open(path, "rb") as f:
        return parse_ppm(f.read())


def huffman_text(text) -> list[tuple[int, int, int]]:
    """generateHuffmanCode (Huffman.hpp:53) on an int text -> [(symbol, length, code)] in DHT order."""
    t = np.ascontiguousarray(np.asarray(text, dtype=np.int32))
    n = max(1, len(set(t.tolist())))
    syms = np.zeros(n + 1, np.int32)
    lens = np.zeros(n + 1, np.int32)
    codes = np.zeros(n + 1, np.uint32)
    k = ctypes.c_int()
    _check(lib().jpge_huffman_text(_p(t), t.size, _p(syms), _p(lens), _p(codes), ctypes.byref(k)), "huffman_text")
    return list(zip(syms[:k.value].tolist(), lens[:k.value].tolist(), codes[:k.value].tolist()))


def huffman_decode(data: bytes, nbits: int, table) -> list[int]:
    """huffmanDecode (Huffman.cpp:91-146): the symbols coded in the first nbits bits of
    data by table = [(symbol, length, code)] (as huffman_text returns it)."""
    buf = np.frombuffer(bytes(data) + b"\0", np.uint8)
    syms = np.ascontiguousarray([t[0] for t in table], np.uint32)
    lens = np.ascontiguousarray([t[1] for t in table], np.uint8)
    codes = np.ascontiguousarray([t[2] for t in table], np.uint32)
    n = ctypes.c_size_t()
    _check(lib().jpge_huffman_decode(_p(buf), nbits, _p(syms), _p(codes), _p(lens), len(table), None, 0,
                                     ctypes.byref(n)), "huffman_decode")
    out = np.zeros(max(1, n.value), np.int32)
    _check(lib().jpge_huffman_decode(_p(buf), nbits, _p(syms), _p(codes), _p(lens), len(table), _p(out), out.size,
                                     ctypes.byref(n)), "huffman_decode")
    return out[:n.value].tolist()


def idct8x8(block) -> np.ndarray:
    """inverseDctMat (Dct.hpp:278-306) of an 8x8 block."""
    x = np.ascontiguousarray(block, np.float64).reshape(64)
    out = np.zeros(64, np.float64)
    lib().jpge_idct8x8(_p(x), _p(out))
    return out.reshape(8, 8)


def decode_coeffs(data: bytes):
    """Entropy-decode a jpge .jpg -> (Decoded header, Y, Cb, Cr) quantised coefficient
    planes of shape (blocks, 64), raster block order, natural order (jpge_decode_coeffs).
    A one-component (grayscale) file gives (header, Y, None, None); its c_blocks is 0."""
    buf = np.frombuffer(bytes(data), np.uint8)
    info = Decoded()
    _check(lib().jpge_decode_coeffs(_p(buf), buf.size, ctypes.byref(info), None, None, None, 0, 0), "decode_coeffs")
    y = np.zeros((info.y_blocks, 64), np.int16)
    if info.c_blocks == 0:
        _check(lib().jpge_decode_coeffs(_p(buf), buf.size, ctypes.byref(info), _p(y), None, None, y.shape[0], 0),
               "decode_coeffs")
        return info, y, None, None
    cb = np.zeros((info.c_blocks, 64), np.int16)
    cr = np.zeros_like(cb)
    _check(lib().jpge_decode_coeffs(_p(buf), buf.size, ctypes.byref(info), _p(y), _p(cb), _p(cr), y.shape[0],
                                    cb.shape[0]), "decode_coeffs")
    return info, y, cb, cr


def concat_segments(device: int, stream: int, ptrs, lens, dst: int) -> int:
    """jpge_concat_segments: device byte runs (pointers ptrs[k], lens[k] bytes) back to
    back into the device buffer dst, queued on `stream` (a hipStream_t as an int, 0 =
    the null stream).  ptrs/lens may be ctypes arrays (reused) or sequences.  Returns
    the total length."""
    n = len(ptrs)
    if not isinstance(ptrs, ctypes.Array):
        ptrs = (ctypes.c_void_p * n)(*ptrs)
    if not isinstance(lens, ctypes.Array):
        lens = (ctypes.c_size_t * n)(*lens)
    tot = ctypes.c_size_t()
    _check(lib().jpge_concat_segments(int(device), stream or None, ptrs, lens, n, dst, ctypes.byref(tot)),
           "concat_segments")
    return tot.value


def huffman_table(counts, first):
    """Byte-symbol table from counts/first-occurrence keys -> (bits[16], huffval list, code[256], len[256])."""
    c = np.ascontiguousarray(counts, dtype=np.uint32)
    f = np.ascontiguousarray(first, dtype=np.uint64)
    bits = np.zeros(16, np.uint8)
    hv = np.zeros(256, np.uint8)
    code = np.zeros(256, np.uint32)
    ln = np.zeros(256, np.uint8)
    n = ctypes.c_int()
    _check(lib().jpge_huffman_table(_p(c), _p(f), _p(bits), _p(hv), ctypes.byref(n), _p(code), _p(ln)),
           "huffman_table")
    return bits, hv[:n.value].tolist(), code, ln


# ---- Coding.hpp primitives (host, C ABI) ----
def zigzag_index(i: int) -> int:
    """zigzag(int) (Coding.hpp:57-81): natural index of zig-zag position i (-1 outside 0..63)."""
    return int(lib().jpge_zigzag_index(int(i)))


def zigzag_block(block) -> np.ndarray:
    """zigzag(matrix) (Coding.hpp:30-54) of a natural-order 8x8 block."""
    a = np.ascontiguousarray(block, np.int32).reshape(64)
    out = np.zeros(64, np.int32)
    _check(lib().jpge_zigzag_block(_p(a), _p(out)), "zigzag_block")
    return out


def quantize_block(block, table) -> np.ndarray:
    """quantize (Coding.hpp:84-97): round-half-away of block / table, natural order."""
    b = np.ascontiguousarray(block, np.float64).reshape(64)
    t = np.ascontiguousarray(table, np.float64).reshape(64)
    out = np.zeros(64, np.int32)
    _check(lib().jpge_quantize_block(_p(b), _p(t), _p(out)), "quantize_block")
    return out.reshape(8, 8)


def rle_ac(data, zigzag_scan: bool = False) -> list[tuple[int, int]]:
    """RLE_AC (Coding.hpp:112-183): [(run, value)]; zigzag_scan: the 8x8 matrix version."""
    d = np.ascontiguousarray(data, np.int32).reshape(-1)
    runs = np.zeros(d.size + 64, np.uint8)
    vals = np.zeros(d.size + 64, np.int32)
    n = ctypes.c_size_t()
    _check(lib().jpge_rle_ac(_p(d), d.size, int(zigzag_scan), _p(runs), _p(vals), runs.size, ctypes.byref(n)),
           "rle_ac")
    return list(zip(runs[:n.value].tolist(), vals[:n.value].tolist()))


def category_code(value: int) -> tuple[int, int]:
    """getCategoryAndCode (Coding.hpp:197-262): (category, extra bits)."""
    c, b = ctypes.c_uint16(), ctypes.c_uint32()
    _check(lib().jpge_category_code(int(value), ctypes.byref(c), ctypes.byref(b)), "category_code")
    return c.value, b.value


def encode_category(pairs) -> list[tuple[int, int, int]]:
    """encode_category (Coding.hpp:265-283): [(symbol, extra bits, bit count)]."""
    n = len(pairs)
    runs = np.ascontiguousarray([p[0] for p in pairs] or [0], np.uint8)
    vals = np.ascontiguousarray([p[1] for p in pairs] or [0], np.int32)
    syms, lens = np.zeros(max(1, n), np.uint8), np.zeros(max(1, n), np.uint8)
    codes = np.zeros(max(1, n), np.uint32)
    _check(lib().jpge_encode_category(_p(runs), _p(vals), n, _p(syms), _p(codes), _p(lens)), "encode_category")
    return list(zip(syms[:n].tolist(), codes[:n].tolist(), lens[:n].tolist()))


def dc_difference(qy: np.ndarray, qcb: np.ndarray, qcr: np.ndarray) -> None:
    """applyDCdifferenceCoding (Image.cpp:638-678) in place on int32 planes."""
    for a in (qy, qcb, qcr):
        if a.dtype != np.int32 or not a.flags.c_contiguous:
            raise ValueError("int32 C-contiguous planes expected")
    _check(lib().jpge_dc_difference(_p(qy), qy.shape[0], qy.shape[1], _p(qcb), _p(qcr), qcb.shape[0], qcb.shape[1]),
           "dc_difference")


def arai_constants() -> tuple[np.ndarray, np.ndarray]:
    a = np.zeros(5)
    s = np.zeros(8)
    lib().jpge_arai_constants(_p(a), _p(s))
    return a, s


def input_format_info(fmt: int) -> tuple[int, int]:
    """(bytes per pixel along a row, planes) of an input layout (JPGE_FMT_*); host only.
    (JPGE_FMT_V210: 0 bytes per pixel, not a whole number; its rows are v210_row_bytes(w).)"""
    b, n = ctypes.c_int32(), ctypes.c_int32()
    _check(lib().jpge_input_format_info(int(fmt), ctypes.byref(b), ctypes.byref(n)), "input_format_info")
    return b.value, n.value


def standard_huffman(table: int) -> tuple[list[int], list[int]]:
    """ITU T.81 Annex K table 0 Y-DC, 1 Y-AC, 2 C-DC, 3 C-AC as (bits, huffval): the
    number of codes of each length 1..16, and the symbols in DHT order; host only."""
    s = HuffSpec()
    _check(lib().jpge_standard_huffman(int(table), ctypes.byref(s)), "standard_huffman")
    return s.as_tuple()


def yuv_preset(preset: int) -> tuple[float, ...]:
    """(y_off, m0, ..., m6) of a sample-transform preset (JPGE_YUV_*, not CUSTOM); host only."""
    t = YuvTransform()
    _check(lib().jpge_yuv_preset(int(preset), ctypes.byref(t)), "yuv_preset")
    return t.as_tuple()


def _huff_specs(specs):
    if specs is None:
        return None
    if len(specs) != 4:
        raise ValueError("four Huffman specs: Y-DC, Y-AC, C-DC, C-AC")
    return (HuffSpec * 4)(*[HuffSpec.from_tuple(t) for t in specs])


class Yuv420Frame(np.ndarray):
    """A host NV12, I420, P010 or I010 frame (pack_yuv420, pack_yuv420p10): the layout's bytes,
    planes back to back (plane stride 0), with the geometry that a flat buffer does not show."""
    fmt = width = height = stride = None

    def __array_finalize__(self, obj):
        for k in ("fmt", "width", "height", "stride"):
            setattr(self, k, getattr(obj, k, None))


class Yuv422Frame(Yuv420Frame):
    """A host 4:2:2 frame (pack_yuv422, pack_yuv422p10, pack_v210): the layout's bytes, planes back
    to back (plane stride 0), with the geometry that a flat buffer does not show."""


class _Yuv(NamedTuple):
    """A Y, Cb, Cr layout with half-width chroma, as jpge.h states it."""
    family: str  # pack_<family> builds its host frames, <family>_bytes sizes them
    size: int    # bytes per sample: 1, or 2 (a little-endian word)
    shift: int   # the sample's lowest bit inside its word
    vsub: int    # picture rows per chroma row: 2 (ceil(h / 2) chroma rows; a Yuv420Frame) or 1 (a Yuv422Frame)
    order: str   # "planar" Y, Cb, Cr planes; "semi": a Y plane + rows of Cb,Cr pairs; groups "yuyv" or "uyvy"


#: the one statement of these layouts on the Python side: the byte counts, the host packers, the
#: frame check and the plane geometry of the encode_tensor_yuv* methods all read it (v210 keeps
#: its own row rule, v210_row_bytes; the RGB layouts, GRAY8 and YUV444_PLANAR: input_format_info)
_YUV = {
    JPGE_FMT_NV12: _Yuv("yuv420", 1, 0, 2, "semi"), JPGE_FMT_I420: _Yuv("yuv420", 1, 0, 2, "planar"),
    JPGE_FMT_P010: _Yuv("yuv420p10", 2, 6, 2, "semi"), JPGE_FMT_I010: _Yuv("yuv420p10", 2, 0, 2, "planar"),
    JPGE_FMT_YUYV: _Yuv("yuv422", 1, 0, 1, "yuyv"), JPGE_FMT_UYVY: _Yuv("yuv422", 1, 0, 1, "uyvy"),
    JPGE_FMT_NV16: _Yuv("yuv422", 1, 0, 1, "semi"), JPGE_FMT_I422: _Yuv("yuv422", 1, 0, 1, "planar"),
    JPGE_FMT_Y210: _Yuv("yuv422p10", 2, 6, 1, "yuyv"), JPGE_FMT_P210: _Yuv("yuv422p10", 2, 6, 1, "semi"),
    JPGE_FMT_I210: _Yuv("yuv422p10", 2, 0, 1, "planar"),
}


def _yuv_layout(fmt: int, family: str) -> _Yuv:
    L = _YUV.get(fmt)
    if L is None or L.family != family:
        raise ValueError(f"input layout {fmt} is not one of pack_{family}'s")
    return L


def _yuv_least_stride(L: _Yuv, w: int) -> int:
    """Least row pitch in bytes: w samples, or ceil(w / 2) Cb,Cr pairs or four-sample groups."""
    cw = (w + 1) // 2
    return L.size * (w if L.order == "planar" else 2 * cw if L.order == "semi" else 4 * cw)


def _yuv_chroma_stride(L: _Yuv, stride: int) -> int:
    """Chroma row pitch for Y rows at `stride`: Cb,Cr pairs keep it; Cb and Cr planes halve it,
    rounded up to whole samples ((stride + 1) / 2 bytes, or 2 * ceil(stride / 4))."""
    return stride if L.order == "semi" else L.size * -(-stride // (2 * L.size))


def _yuv_bytes(L: _Yuv, w: int, h: int, stride: int = 0) -> int:
    """Bytes of a frame with plane stride 0 (stride 0: the least one)."""
    stride = stride or _yuv_least_stride(L, w)
    if L.order in ("yuyv", "uyvy"):
        return stride * h
    return stride * h + (1 if L.order == "semi" else 2) * _yuv_chroma_stride(L, stride) * -(-h // L.vsub)


def yuv420_bytes(fmt: int, w: int, h: int, stride: int = 0) -> int:
    """Bytes of an NV12 or I420 frame with plane stride 0 (stride 0: the least one)."""
    return _yuv_bytes(_yuv_layout(fmt, "yuv420"), w, h, stride)


def yuv420p10_bytes(fmt: int, w: int, h: int, stride: int = 0) -> int:
    """Bytes of a P010 or I010 frame with plane stride 0 (stride, in bytes, 0: the least one)."""
    return _yuv_bytes(_yuv_layout(fmt, "yuv420p10"), w, h, stride)


def yuv422_bytes(fmt: int, w: int, h: int, stride: int = 0) -> int:
    """Bytes of a YUYV, UYVY, NV16 or I422 frame with plane stride 0 (stride 0: the least one)."""
    return _yuv_bytes(_yuv_layout(fmt, "yuv422"), w, h, stride)


def yuv422p10_bytes(fmt: int, w: int, h: int, stride: int = 0) -> int:
    """Bytes of a Y210, P210 or I210 frame with plane stride 0 (stride, in bytes, 0: the least one)."""
    return _yuv_bytes(_yuv_layout(fmt, "yuv422p10"), w, h, stride)


def _sample_planes(name: str, y, cb, cr, vsub: int, ten_bit: bool):
    """(y, cb, cr, w, h, cw) of a pack_* call's planes, contiguous: an (H, W) Y plane and
    (ceil(H / vsub), ceil(W / 2)) Cb and Cr planes, converted to uint8, or, ten_bit, integers
    0..1023 as they came."""
    y, cb, cr = (np.ascontiguousarray(p, None if ten_bit else np.uint8) for p in (y, cb, cr))
    for p in (y, cb, cr):
        if ten_bit and (p.dtype.kind not in "ui" or (p.size and (int(p.min()) < 0 or int(p.max()) > 1023))):
            raise ValueError(f"{name} takes integer planes of 10-bit samples (0..1023)")
    if y.ndim != 2 or y.size == 0:
        raise ValueError(f"Y plane of shape {y.shape}: (H, W)")
    h, w = y.shape
    cw, ch = (w + 1) // 2, -(-h // vsub)
    if cb.shape != (ch, cw) or cr.shape != (ch, cw):
        raise ValueError(f"chroma planes of shapes {cb.shape}, {cr.shape}: ({ch}, {cw}) for a {w}x{h} frame")
    return y, cb, cr, w, h, cw


def _pack_yuv(family: str, fmt: int, y, cb, cr):
    L = _yuv_layout(fmt, family)
    y, cb, cr, w, h, cw = _sample_planes(f"pack_{family}", y, cb, cr, L.vsub, L.size == 2)
    dt = np.uint8 if L.size == 1 else "<u2"
    y, cb, cr = (p.astype(dt) << L.shift for p in (y, cb, cr))
    if L.order == "planar":
        buf = np.concatenate([y.reshape(-1), cb.reshape(-1), cr.reshape(-1)])
    elif L.order == "semi":
        buf = np.zeros((h + len(cb), 2 * cw), dt)  # (odd width: one pad sample per Y row)
        buf[:h, :w] = y
        buf[h:, 0::2], buf[h:, 1::2] = cb, cr
    else:
        yo, co = (0, 1) if L.order == "yuyv" else (1, 0)
        buf = np.zeros((h, cw, 4), dt)  # (odd width: the last group's second Y sample stays 0)
        buf[:, :, yo], buf[:, :w // 2, yo + 2] = y[:, 0::2], y[:, 1::2]
        buf[:, :, co], buf[:, :, co + 2] = cb, cr
    f = buf.reshape(-1).view(np.uint8).view(Yuv420Frame if L.vsub == 2 else Yuv422Frame)
    f.fmt, f.width, f.height, f.stride = int(fmt), w, h, _yuv_least_stride(L, w)
    return f, w, h, f.stride


def pack_yuv420(fmt: int, y: np.ndarray, cb: np.ndarray, cr: np.ndarray):
    """(frame, w, h, stride): the (H, W) Y plane and the (ceil(H/2), ceil(W/2)) Cb and Cr planes
    as one contiguous host frame in layout JPGE_FMT_NV12 or JPGE_FMT_I420 with the least
    stride and plane stride 0 (jpge.h).  The frame (a Yuv420Frame) is what encode,
    encode_batch, fdct_quant and symbol_stats take when the input layout is `fmt`."""
    return _pack_yuv("yuv420", fmt, y, cb, cr)


def pack_yuv420p10(fmt: int, y: np.ndarray, cb: np.ndarray, cr: np.ndarray):
    """(frame, w, h, stride): the (H, W) Y plane and the (ceil(H/2), ceil(W/2)) Cb and Cr planes of
    10-bit samples (uint16 values 0..1023) as one contiguous host frame of bytes in layout
    JPGE_FMT_P010 (each sample in its word's top 10 bits, the low six zero) or JPGE_FMT_I010 with
    the least stride and plane stride 0 (jpge.h).  The frame (a Yuv420Frame) is what encode,
    encode_batch, fdct_quant and symbol_stats take when the input layout is `fmt`."""
    return _pack_yuv("yuv420p10", fmt, y, cb, cr)


def pack_yuv422(fmt: int, y: np.ndarray, cb: np.ndarray, cr: np.ndarray):
    """(frame, w, h, stride): the (H, W) Y plane and the (H, ceil(W/2)) Cb and Cr planes as one
    contiguous host frame in layout JPGE_FMT_YUYV, _UYVY, _NV16 or _I422 with the least stride
    and plane stride 0 (jpge.h).  The frame (a Yuv422Frame) is what encode, encode_batch,
    fdct_quant and symbol_stats take when the input layout is `fmt`.  (Odd width: the last
    group's second Y byte, and NV16's pad byte per Y row, are 0.)"""
    return _pack_yuv("yuv422", fmt, y, cb, cr)


def pack_yuv422p10(fmt: int, y: np.ndarray, cb: np.ndarray, cr: np.ndarray):
    """(frame, w, h, stride): the (H, W) Y plane and the (H, ceil(W/2)) Cb and Cr planes of 10-bit
    samples (uint16 values 0..1023) as one contiguous host frame of bytes in layout JPGE_FMT_Y210,
    _P210 (each sample in its word's top 10 bits, the low six zero) or _I210 (the high six zero)
    with the least stride and plane stride 0 (jpge.h).  The frame (a Yuv422Frame) is what encode,
    encode_batch, fdct_quant and symbol_stats take when the input layout is `fmt`.  (Odd width:
    the last group's second Y word, and P210's pad word per Y row, are 0.)"""
    return _pack_yuv("yuv422p10", fmt, y, cb, cr)


def v210_row_bytes(w: int) -> int:
    """Bytes of a v210 row of w pixels: 16 * ceil(w / 6) (jpge_v210_row_bytes)."""
    if not 0 <= int(w) <= 0xFFFFFFFF:
        raise ValueError(f"width {w}")
    return int(lib().jpge_v210_row_bytes(int(w)))


def v210_unpack(frame, w: int, h: int, stride: int = 0):
    """(y, cb, cr): the uint16 sample planes (H, W), (H, ceil(W/2)), (H, ceil(W/2)) of a host v210
    frame of bytes, rows of pitch `stride` (0: the least one), by the layout rule of jpge.h on the
    host (jpge_v210_unpack)."""
    a = np.ascontiguousarray(np.asarray(frame)).reshape(-1).view(np.uint8)
    w, h, stride = int(w), int(h), int(stride)
    if w < 1 or h < 1 or stride < 0:
        raise ValueError(f"a {w}x{h} frame of stride {stride}")
    row = v210_row_bytes(w)
    pitch = stride or row
    if pitch < row or a.size < pitch * (h - 1) + row:
        raise ValueError(f"{a.size} bytes do not hold {h} v210 rows of {w} pixels at stride {pitch}")
    cw = (w + 1) // 2
    y, cb, cr = np.empty((h, w), np.uint16), np.empty((h, cw), np.uint16), np.empty((h, cw), np.uint16)
    _check(lib().jpge_v210_unpack(_p(a), w, h, stride, _p(y), _p(cb), _p(cr)), "v210_unpack")
    return y, cb, cr


def pack_v210(y: np.ndarray, cb: np.ndarray, cr: np.ndarray, stride: int = 0):
    """(frame, w, h, stride): the (H, W) Y plane and the (H, ceil(W/2)) Cb and Cr planes of 10-bit
    samples (integers 0..1023) as one contiguous host v210 frame of bytes, rows of pitch `stride`
    (0: the least one, v210_row_bytes(W); else a multiple of 4 not below it).  The samples of the
    last group beyond the frame, bits 30-31 of every word and the rows' padding are zero.  The
    frame (a Yuv422Frame) is what encode, encode_batch, fdct_quant and symbol_stats take when the
    input layout is JPGE_FMT_V210."""
    y, cb, cr, w, h, cw = _sample_planes("pack_v210", y, cb, cr, 1, True)
    row = v210_row_bytes(w)
    stride = int(stride) or row
    if stride < row or stride % 4:
        raise ValueError(f"stride {stride}: a multiple of 4, at least {row}")
    # the row's stream Cb0 Y0 Cr0 Y1 Cb1 Y2 Cr1 Y3 ..., three samples to a word
    n = 3 * (row // 4)
    st = np.zeros((h, n), np.uint32)
    st[:, 1:2 * w:2] = y
    st[:, 0:4 * cw:4] = cb
    st[:, 2:4 * cw:4] = cr
    buf = np.zeros((h, stride // 4), "<u4")
    buf[:, :row // 4] = st[:, 0::3] | (st[:, 1::3] << 10) | (st[:, 2::3] << 20)
    f = buf.reshape(-1).view(np.uint8).view(Yuv422Frame)
    f.fmt, f.width, f.height, f.stride = JPGE_FMT_V210, w, h, stride
    return f, w, h, stride


def _frame_geom(a: np.ndarray, fmt: int) -> tuple[int, int, int]:
    """(width, height, row stride in bytes) of a C-contiguous frame shaped for layout `fmt`:
    (H, W, 3), (H, W, 4) or (3, H, W); GRAY8: (H, W); NV12 and I420: a pack_yuv420 frame of
    that layout; YUYV, UYVY, NV16 and I422: a pack_yuv422 frame of that layout; P010, I010 and
    Y210, P210, I210: a pack_yuv420p10 / pack_yuv422p10 frame of that layout; V210: a pack_v210
    frame.  A width or
    height of 0 or above 65535 (a JPEG frame header's limit) is a ValueError."""
    w, h, stride = _frame_geom_any(a, fmt)
    if not (1 <= w <= 65535 and 1 <= h <= 65535):
        raise ValueError(f"a {w}x{h} frame: width and height are 1..65535")
    return w, h, stride


def _frame_geom_any(a: np.ndarray, fmt: int) -> tuple[int, int, int]:
    bpp, planes = input_format_info(fmt)
    if fmt == JPGE_FMT_GRAY8 or fmt in _BAYER:  # one plane of bytes
        if a.ndim != 2 or a.dtype != np.uint8 or a.size == 0:
            raise ValueError(f"frame of shape {a.shape} and type {a.dtype}: input layout {fmt} "
                             f"({'GRAY8' if fmt == JPGE_FMT_GRAY8 else 'Bayer'}) takes a non-empty (H, W) uint8 array")
        return a.shape[1], a.shape[0], a.shape[1]
    if fmt in _YUV:
        if getattr(a, "fmt", None) != fmt or a.ndim != 1 or a.dtype != np.uint8 or \
                a.size != _yuv_bytes(_YUV[fmt], a.width, a.height, a.stride):
            raise ValueError(f"input layout {fmt} takes a pack_{_YUV[fmt].family}({fmt}, y, cb, cr) frame")
        return a.width, a.height, a.stride
    if fmt == JPGE_FMT_V210:
        if getattr(a, "fmt", None) != fmt or a.ndim != 1 or a.dtype != np.uint8 or a.size != a.stride * a.height:
            raise ValueError(f"input layout {fmt} takes a pack_v210(y, cb, cr) frame")
        return a.width, a.height, a.stride
    want = "(3, H, W)" if planes == 3 else f"(H, W, {bpp})"
    if a.ndim != 3 or (a.shape[0] != 3 if planes == 3 else a.shape[2] != bpp):
        raise ValueError(f"frame of shape {a.shape}: input layout {fmt} takes {want}")
    h, w = (a.shape[1], a.shape[2]) if planes == 3 else (a.shape[0], a.shape[1])
    return w, h, w * bpp


def _as_frame(a, fmt: int):
    """(C-contiguous uint8 array, width, height, stride) of a frame for layout `fmt`."""
    if fmt == JPGE_FMT_GRAY8 or fmt in _BAYER:
        a = np.ascontiguousarray(a)  # (the type is checked, not converted: a float plane is no gray frame)
    elif fmt not in _YUV and fmt != JPGE_FMT_V210:
        a = np.ascontiguousarray(a, np.uint8)
    w, h, stride = _frame_geom(a, fmt)
    return np.ascontiguousarray(a, np.uint8), w, h, stride


def _as_frames(frames, fmt: int):
    fr = [_as_frame(f, fmt) for f in frames]
    return [f[0] for f in fr], [f[1:] for f in fr]


def _row_pitch(p):
    """Row pitch in bytes of a torch tensor (rows, ...) whose rows are packed: every dimension
    after the first at the stride of a contiguous row, unless it has one entry (else ValueError).
    None for a single row: it has no pitch, so any serves."""
    run = 1
    for d in range(p.dim() - 1, 0, -1):
        if p.stride(d) != run and p.shape[d] > 1:
            raise ValueError(f"strides {tuple(p.stride())}: the inner dimension must have unit stride"
                             + (" and the pairs must be packed" if p.dim() > 2 else ""))
        run *= p.shape[d]
    return p.element_size() * p.stride(0) if p.shape[0] > 1 else None


def _chroma_offset(planes) -> int:
    """Bytes from the Y plane to the next of torch planes Y, chroma...: the plane stride."""
    store = planes[0].untyped_storage().data_ptr()
    if any(p.untyped_storage().data_ptr() != store for p in planes):
        raise ValueError("the planes must be views of one allocation")
    plane_stride = planes[1].data_ptr() - planes[0].data_ptr()
    if plane_stride <= 0:
        raise ValueError("the chroma must follow the Y plane in memory")
    return plane_stride


def _plane_geom(L: _Yuv, w: int, h: int, y, c=None, cr=None) -> tuple[int, int]:
    """(row stride, plane stride) in bytes that say where the torch tensors of a w x h frame in
    layout L lie: `y` the Y plane or the packed groups, `c` the Cb,Cr pairs or the Cb plane, `cr`
    the Cr plane.  ValueError where jpge.h's rules cannot express the views: chroma rows at
    _yuv_chroma_stride of the Y pitch, Cr `chroma rows` rows after Cb."""
    least = _yuv_least_stride(L, w)
    stride = _row_pitch(y)
    if stride is None:
        stride = least  # (one Y row, hence one row in every plane: no pitch to agree with)
    if stride < least:
        raise ValueError(f"rows overlap: pitch {stride}, a row takes {least} bytes")
    if c is None:
        return stride, 0
    plane_stride = _chroma_offset([y, c] + ([] if cr is None else [cr]))
    cs, rows = _yuv_chroma_stride(L, stride), -(-h // L.vsub)
    for p in (c, cr):
        cp = None if p is None else _row_pitch(p)
        if cp is not None and cp != cs:
            raise ValueError(f"chroma pitch {cp}: for Y rows at pitch {stride} the layout's " +
                             ("Cb,Cr rows have the same" if L.order == "semi" else f"Cb and Cr rows have {cs}"))
    if cr is not None and cr.data_ptr() - c.data_ptr() != cs * rows:
        raise ValueError(f"the Cr plane must start {cs * rows} bytes ({rows} rows) after the Cb plane")
    return stride, plane_stride


def downscaled_size(w: int, h: int, s: int) -> tuple[int, int]:
    """(ceil(w / s), ceil(h / s)) for s = 1, 2 or 4 (jpge_downscaled_size)."""
    dw, dh = ctypes.c_uint32(), ctypes.c_uint32()
    _check(lib().jpge_downscaled_size(int(w), int(h), int(s), ctypes.byref(dw), ctypes.byref(dh)), "downscaled_size")
    return dw.value, dh.value


def downscale_frame(a, fmt: int, s: int):
    """The frame an encode with Encoder.set_downscale(s) codes (jpge_downscale_frame, on the
    host): `a` shaped for layout `fmt` (RGB8, BGR8, RGBA8, BGRA8: (H, W, C); NV12: a
    pack_yuv420 frame) -> the frame of ceil(W / s) x ceil(H / s) pixels in the same layout,
    every sample the mean, rounded half up, of its s x s source samples."""
    a, w, h, stride = _as_frame(a, fmt)
    dw, dh = downscaled_size(w, h, s)
    if fmt == JPGE_FMT_NV12:
        dstride = 2 * ((dw + 1) // 2)
        out = np.zeros(yuv420_bytes(fmt, dw, dh), np.uint8)
    else:
        bpp = input_format_info(fmt)[0]
        dstride = dw * bpp
        out = np.zeros((dh, dw, bpp), np.uint8)
    _check(lib().jpge_downscale_frame(int(fmt), _p(a), w, h, stride, 0, int(s), _p(out), dstride, 0), "downscale_frame")
    if fmt == JPGE_FMT_NV12:
        out = out.view(Yuv420Frame)
        out.fmt, out.width, out.height, out.stride = int(fmt), dw, dh, dstride
    return out


def oriented_size(w: int, h: int, o: int) -> tuple[int, int]:
    """(ow, oh) of a w x h frame under orientation o (JPGE_ORIENT_*): (h, w) for the transposed
    ones, 4-7 (jpge_oriented_size)."""
    ow, oh = ctypes.c_uint32(), ctypes.c_uint32()
    _check(lib().jpge_oriented_size(int(w), int(h), int(o), ctypes.byref(ow), ctypes.byref(oh)), "oriented_size")
    return ow.value, oh.value


def orient_frame(a, fmt: int, o: int):
    """The frame an encode with Encoder.set_orientation(o) codes (jpge_orient_frame, on the
    host): `a`, (H, W, C) in layout `fmt` (RGB8, BGR8, RGBA8, BGRA8) -> the (oh, ow, C) frame
    in the same layout; a fourth byte is copied."""
    a, w, h, stride = _as_frame(a, fmt)
    ow, oh = oriented_size(w, h, o)
    bpp = input_format_info(fmt)[0]
    out = np.zeros((oh, ow, bpp), np.uint8)
    _check(lib().jpge_orient_frame(int(fmt), _p(a), w, h, stride, int(o), _p(out), ow * bpp), "orient_frame")
    return out


def demosaic_frame(a, fmt: int):
    """The (H, W, 3) RGB8 frame an encode codes for the (H, W) uint8 Bayer mosaic `a` in layout
    `fmt` (JPGE_FMT_BAYER_*): the bilinear rule of jpge.h on the host (jpge_demosaic_frame)."""
    a = np.ascontiguousarray(a)
    if a.ndim != 2 or a.dtype != np.uint8:
        raise ValueError(f"frame of shape {a.shape} and type {a.dtype}: a Bayer mosaic is an (H, W) uint8 array")
    h, w = a.shape
    out = np.zeros((h, w, 3), np.uint8)
    _check(lib().jpge_demosaic_frame(int(fmt), _p(a), w, h, w, _p(out), 3 * w), "demosaic_frame")
    return out


def _channel_lut(lut) -> np.ndarray:
    """The (3, 256) uint8 tables (R, G, B) of a set_channel_lut / lut_frame argument: a (3, 256)
    uint8 array, or a (256,) one used for all three channels."""
    t = np.asarray(lut)
    if t.dtype != np.uint8 or t.shape not in ((3, 256), (256,)):
        raise ValueError(f"lookup tables of shape {t.shape} and type {t.dtype}: a (3, 256) uint8 array "
                         "(the R, G and B tables) or a (256,) one for all three channels")
    return np.ascontiguousarray(np.broadcast_to(t, (3, 256)))


def lut_frame(a, fmt: int, lut):
    """The frame an encode with Encoder.set_channel_lut(lut) codes for the (H, W, 3) or (H, W, 4)
    uint8 frame `a` in layout `fmt` (RGB8, BGR8, RGBA8, BGRA8), in the same layout: every R, G, B
    byte through its colour's table, alpha copied (jpge_lut_frame, on the host).  A Bayer frame:
    lut_frame(demosaic_frame(a, fmt), JPGE_FMT_RGB8, lut)."""
    t = _channel_lut(lut)
    a = np.ascontiguousarray(a)
    if a.ndim != 3 or a.dtype != np.uint8 or a.shape[2] not in (3, 4) or a.size == 0:
        raise ValueError(f"frame of shape {a.shape} and type {a.dtype}: a non-empty (H, W, 3) or (H, W, 4) uint8 array")
    h, w, c = a.shape
    out = np.zeros_like(a)
    _check(lib().jpge_lut_frame(int(fmt), _p(a), w, h, w * c, _p(t), _p(out), w * c), "lut_frame")
    return out


def device_count() -> int:
    n = ctypes.c_int(0)
    lib().jpge_device_count(ctypes.byref(n))
    return n.value


def max_jpeg_bytes(width: int, height: int) -> int:
    return int(lib().jpge_max_jpeg_bytes(width, height))


# Encoders (and device groups) still open at interpreter exit are closed by an atexit hook, ahead of the
# HIP runtime's own teardown in the C++ static destructors (a lane stream destroyed
# after that, e.g. once a profiler's tool library has finalised, can fault the process).
_live_encoders = weakref.WeakSet()


@atexit.register
def _close_live_encoders() -> None:
    for e in list(_live_encoders):
        try:
            e.close()
        except Exception:
            pass


class Encoder:
    """One GPU context (jpge_open).  Host-array methods copy in/out; the `*_dev`
    variants take device pointers (ints) for HBM-resident frames."""

    _orient = JPGE_ORIENT_NONE  # the orientation as set through this object (sizes the output buffers)

    def __init__(self, device: int = 0, lanes: int = 0):
        """lanes: concurrent pipelines on the device (0 = JPGE_LANES or the default 4)."""
        self._ctx = ctypes.c_void_p()
        _check(lib().jpge_open_ex(int(device), int(lanes), ctypes.byref(self._ctx)), f"jpge_open({device})")
        _live_encoders.add(self)
        self.device = device
        self._qcache = {}     # quality -> (qy, qc) byte tables
        self._desc = None     # (key, Frame array) of the last device batch
        self._fmt = JPGE_FMT_RGB8

    def close(self) -> None:
        if self._ctx:
            lib().jpge_close(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def ctx(self) -> ctypes.c_void_p:
        return self._ctx

    def set_timing(self, every: int = 1) -> None:
        """HIP-event kernel timing of every `every`-th frame (0/False = off, True = all)."""
        _check(lib().jpge_set_timing(self._ctx, int(every)), "set_timing")

    def timing(self) -> dict:
        t = Timing()
        _check(lib().jpge_get_timing(self._ctx, ctypes.byref(t)), "get_timing")
        return {"fdct": t.fdct, "dc_stats": t.dc_stats, "entropy": t.entropy, "total": t.total,
                "fdct_sum": t.fdct_sum, "dc_stats_sum": t.dc_stats_sum, "entropy_sum": t.entropy_sum,
                "frames": t.frames, "symbols": t.symbols, "code_sum": t.code_sum, "pack_sum": t.pack_sum,
                "launches": t.launches, "gate_timeouts": t.gate_timeouts}

    def reset_timing(self) -> None:
        _check(lib().jpge_reset_timing(self._ctx), "reset_timing")

    def set_restart(self, mcus: int) -> None:
        """Restart interval in MCUs for the following encodes (0 = none: the reference's stream)."""
        _check(lib().jpge_set_restart_interval(self._ctx, int(mcus)), "set_restart_interval")

    def set_subsampling(self, mode: int) -> None:
        """Chroma subsampling for the following encodes (applySubsampling's modes,
        Image.hpp:44-52): 420 (S420_m, the reference's writeJPEG, the default), 444
        (S444), 422 (S422), 411 (S411), 4200 (S420) or 4201 (S420_lm); see SUBSAMPLING."""
        _check(lib().jpge_set_subsampling(self._ctx, int(mode)), "set_subsampling")
        self._sub = int(mode)

    def set_input_format(self, fmt: int, plane_stride: int = 0) -> None:
        """Input layout of the following encodes (JPGE_FMT_*): frames are then (H, W, 3),
        (H, W, 4) or, planar, (3, H, W); GRAY8: (H, W), written as a one-component JPEG;
        NV12 and I420: pack_yuv420 frames; YUYV, UYVY, NV16 and I422: pack_yuv422 frames; P010 and
        I010: pack_yuv420p10 frames; Y210, P210 and I210: pack_yuv422p10 frames; V210: pack_v210
        frames; BAYER_*: (H, W) mosaics of raw bytes, coded as demosaic_frame's RGB8 frame.  plane_stride:
        bytes between the planes of the raw-pointer entries' planar frames (NV12, I420: from
        the Y plane to the chroma, as for NV16 and I422; 0 = stride * height; the packed 4:2:2
        layouts are one plane and take 0)."""
        _check(lib().jpge_set_input_format(self._ctx, int(fmt), int(plane_stride)), "set_input_format")
        self._fmt = int(fmt)

    def input_format(self) -> tuple[int, int]:
        """(layout, plane stride) as set."""
        f, ps = ctypes.c_int32(), ctypes.c_size_t()
        _check(lib().jpge_get_input_format(self._ctx, ctypes.byref(f), ctypes.byref(ps)), "get_input_format")
        return f.value, ps.value

    def set_huffman(self, mode: int, specs=None) -> None:
        """Huffman tables of the following encodes (encode*, encode_tensor*, encode_file(s)):
        JPGE_HUFF_OPTIMAL (per-image tables, the reference's stream; the default),
        JPGE_HUFF_STANDARD (ITU T.81 Annex K) or JPGE_HUFF_CUSTOM with specs = four
        (bits, huffval) tables, Y-DC, Y-AC, C-DC, C-AC (as standard_huffman returns them).
        A fixed mode has no host work between a frame's kernels; the stripe phases and
        encode_planes refuse it."""
        _check(lib().jpge_set_huffman(self._ctx, int(mode), _huff_specs(specs)), "set_huffman")

    def huffman(self):
        """(mode, specs): the Huffman mode and, in a fixed mode, its four (bits, huffval)
        tables (None with JPGE_HUFF_OPTIMAL)."""
        m = ctypes.c_int32()
        arr = (HuffSpec * 4)()
        _check(lib().jpge_get_huffman(self._ctx, ctypes.byref(m), arr), "get_huffman")
        return m.value, ([a.as_tuple() for a in arr] if m.value else None)

    def set_yuv_transform(self, preset: int, coeffs=None) -> None:
        """Sample transform of the following encodes of Y, Cb, Cr and gray frames (NV12, I420,
        YUV444_PLANAR, YUYV, UYVY, NV16, I422, GRAY8; encode*, encode_tensor_yuv, encode_tensor_yuv422, a 2-D encode_tensor, fdct_quant,
        symbol_stats): JPGE_YUV_FULL_601 (the default: a sample v is v - 128), LIMITED_601,
        LIMITED_709, FULL_709, or JPGE_YUV_CUSTOM with coeffs = (y_off, m0, ..., m6).  The
        conversion runs inside the transform kernel; the RGB layouts ignore the setting."""
        t = None if coeffs is None else YuvTransform.from_tuple(coeffs)
        _check(lib().jpge_set_yuv_transform(self._ctx, int(preset), t), "set_yuv_transform")

    def yuv_transform(self) -> tuple[int, tuple[float, ...]]:
        """(preset, (y_off, m0, ..., m6)) as set."""
        p, t = ctypes.c_int32(), YuvTransform()
        _check(lib().jpge_get_yuv_transform(self._ctx, ctypes.byref(p), ctypes.byref(t)), "get_yuv_transform")
        return p.value, t.as_tuple()

    def set_downscale(self, factor: int) -> None:
        """Box downscale of the following encodes (encode*, encode_tensor, encode_tensor_yuv with
        NV12, encode_batch, encode_file(s), fdct_quant, symbol_stats): 1 (none), 2 or 4.  A W x H
        frame is coded at ceil(W / factor) x ceil(H / factor), each sample the rounded mean of
        factor x factor source samples, averaged inside the transform kernel: the bytes are
        those of encoding downscale_frame(frame, fmt, factor).  RGB8, BGR8, RGBA8, BGRA8 and
        NV12 input; other layouts and the stripe phases fail with JPGE_E_ARG while it is set."""
        _check(lib().jpge_set_downscale(self._ctx, int(factor)), "set_downscale")

    @property
    def downscale(self) -> int:
        f = ctypes.c_int32()
        _check(lib().jpge_get_downscale(self._ctx, ctypes.byref(f)), "get_downscale")
        return f.value

    def set_orientation(self, o: int) -> None:
        """Orientation of the following encodes (the calls set_downscale applies to): one of
        JPGE_ORIENT_*, named by the operation applied to the pixels.  A W x H frame is coded
        flipped, rotated or transposed (4-7: as H x W), turned inside the transform kernel: the
        bytes are those of encoding orient_frame(frame, fmt, o).  RGB8, BGR8, RGBA8 and BGRA8
        input; 4-7 in the 16x16-MCU subsampling modes; other layouts, a downscale factor above
        1 and the stripe phases fail with JPGE_E_ARG while it is set."""
        _check(lib().jpge_set_orientation(self._ctx, int(o)), "set_orientation")
        self._orient = int(o)

    @property
    def orientation(self) -> int:
        o = ctypes.c_int32()
        _check(lib().jpge_get_orientation(self._ctx, ctypes.byref(o)), "get_orientation")
        return o.value

    def set_channel_lut(self, lut) -> None:
        """Per-channel lookup tables of the following encodes (the calls set_downscale applies
        to): None (off, the default), a (3, 256) uint8 array (the R, G and B tables) or a (256,)
        one used for all three channels.  Every pixel is mapped inside the transform kernel: the
        bytes are those of encoding lut_frame(frame, fmt, lut) (a Bayer mosaic: of its
        demosaic_frame) as RGB8.  RGB8, BGR8, RGBA8, BGRA8 and Bayer input of maxval 255; other
        layouts, a downscale factor above 1, an orientation and the stripe phases fail with
        JPGE_E_ARG while tables are set.  encode_tensor honours the setting."""
        t = None if lut is None else _channel_lut(lut)
        _check(lib().jpge_set_channel_lut(self._ctx, None if t is None else _p(t)), "set_channel_lut")

    def channel_lut(self):
        """The tables in force: a (3, 256) uint8 array, or None when they are off."""
        on, t = ctypes.c_int32(), np.zeros((3, 256), np.uint8)
        _check(lib().jpge_get_channel_lut(self._ctx, ctypes.byref(on), _p(t)), "get_channel_lut")
        return t if on.value else None

    def _cap(self, w: int, h: int) -> int:
        # the output bound of a w x h source: the coded frame's (oriented_size)
        return max_jpeg_bytes(h, w) if self._orient >= JPGE_ORIENT_TRANSPOSE else max_jpeg_bytes(w, h)

    def lanes(self) -> int:
        n = ctypes.c_int32()
        _check(lib().jpge_get_lanes(self._ctx, ctypes.byref(n)), "get_lanes")
        return n.value

    def _gray_qc(self, qy, qc):
        # (GRAY8 reads no chroma table: a caller's luma table alone is a whole setting)
        return qy if qc is None and self._fmt == JPGE_FMT_GRAY8 else qc

    @staticmethod
    def _tables(quality, qy, qc):
        if qy is None or qc is None:
            qy, qc = quality_tables(quality)
        return np.ascontiguousarray(qy, np.uint8), np.ascontiguousarray(qc, np.uint8)

    def encode(self, rgb: np.ndarray, quality: int = 50, maxval: int = 255, qy=None, qc=None) -> bytes:
        """Image::writeJPEG (Image.cpp:831-976) on an (H, W, 3) uint8 frame -> .jpg bytes
        (the frame shaped for the input layout, set_input_format)."""
        rgb, w, h, stride = _as_frame(rgb, self._fmt)
        qy, qc = self._tables(quality, qy, self._gray_qc(qy, qc))
        out = np.empty(self._cap(w, h), np.uint8)
        n = ctypes.c_size_t()
        _check(lib().jpge_encode_rgb8(self._ctx, _p(rgb), w, h, stride, int(maxval), _p(qy), _p(qc), _p(out),
                                      out.size, ctypes.byref(n), 0), "encode")
        return out[:n.value].tobytes()

    def encode_ptr(self, rgb_ptr: int, w: int, h: int, stride: int, out_ptr: int, cap: int, quality: int = 50,
                   maxval: int = 255, flags: int = JPGE_DEVICE_INPUT | JPGE_DEVICE_OUTPUT) -> int:
        """One frame through jpge_encode_rgb8 on raw pointers (device or host per `flags`;
        host pointers may be pinned memory); returns the .jpg length."""
        q = self._qcache.get(quality)
        if q is None:
            qy, qc = self._tables(quality, None, None)
            q = self._qcache[quality] = (qy, qc, _p(qy), _p(qc))
        n = ctypes.c_size_t()
        _check(lib().jpge_encode_rgb8(self._ctx, rgb_ptr, w, h, stride, int(maxval), q[2], q[3], out_ptr, cap,
                                      ctypes.byref(n), int(flags)), "encode_rgb8")
        return n.value

    def _encode_view(self, ptr: int, is_cuda: bool, fmt: int, plane_stride: int, w: int, h: int, stride: int,
                     quality: int, maxval: int, out):
        """The end of every encode_tensor* method: one frame at `ptr` (device memory if is_cuda) in
        layout `fmt` through encode_ptr, into a host buffer (-> the .jpg bytes) or into `out`, a
        uint8 tensor on the device (-> their length); the input layout is put back afterwards."""
        flags = JPGE_DEVICE_INPUT if is_cuda else 0
        host_out = None
        if out is None:
            host_out = np.empty(self._cap(w, h), np.uint8)
            out_ptr, cap = _p(host_out), host_out.size
        else:
            if not out.is_cuda or not out.is_contiguous() or out.element_size() != 1:
                raise ValueError("out: a contiguous uint8 device tensor")
            out_ptr, cap, flags = out.data_ptr(), out.numel(), flags | JPGE_DEVICE_OUTPUT
        prev = self.input_format()
        self.set_input_format(fmt, plane_stride)
        try:
            n = self.encode_ptr(ptr, w, h, stride, out_ptr, cap, quality, maxval, flags)
        finally:
            self.set_input_format(*prev)
        return n if host_out is None else host_out[:n].tobytes()

    def encode_tensor(self, t, quality: int = 50, out=None, order: str = "rgb", maxval: int = 255, layout=None):
        """One torch uint8 tensor through jpge_encode_rgb8 without a repack: (3, H, W) is the
        planar layout (plane stride t.stride(0)), (H, W, 3) and (H, W, 4) the interleaved ones
        in channel order `order` ("rgb" or "bgr"; planar tensors are R, G, B); a 2-dimensional
        (H, W) tensor is a gray plane (JPGE_FMT_GRAY8: a one-component JPEG).  Any row stride;
        the inner dimension must have unit stride (else ValueError).  A device tensor is read
        in place (JPGE_DEVICE_INPUT), a host tensor goes the host path.  Returns the .jpg
        bytes, or, with `out` a uint8 tensor on the frame's device, writes them there and
        returns their length.  The encoder's input layout is the same afterwards.
        layout: "chw" or "hwc"; needed only for a (3, H, 3) or (3, H, 4) tensor, which
        could be either (else ValueError).  "bayer_rggb", "bayer_grbg", "bayer_gbrg" or
        "bayer_bggr" (BAYER_LAYOUTS): the (H, W) tensor is a Bayer mosaic of raw bytes
        (JPGE_FMT_BAYER_*), coded as the RGB8 frame demosaic_frame returns."""
        bayer = BAYER_LAYOUTS.get(layout) if isinstance(layout, str) else None
        if layout not in (None, "chw", "hwc") and bayer is None:
            raise ValueError(f"layout {layout!r}: 'chw' or 'hwc'")
        if bayer is not None and t.dim() != 2:
            raise ValueError(f"layout {layout!r} takes a 2-dimensional (H, W) uint8 tensor of raw bytes")
        if order not in ("rgb", "bgr"):
            raise ValueError(f"order {order!r}: 'rgb' or 'bgr'")
        if t.dim() not in (2, 3) or t.element_size() != 1 or t.dtype.is_floating_point:
            raise ValueError("encode_tensor takes a 3-dimensional (colour) or 2-dimensional (gray) uint8 tensor")
        shape, st = tuple(t.shape), tuple(t.stride())
        plane_stride = 0
        gray = t.dim() == 2
        hwc, chw = not gray and shape[2] in (3, 4), not gray and shape[0] == 3
        if hwc and chw and layout is None:
            raise ValueError(f"tensor of shape {shape} is (3, H, W) or (H, W, C): pass layout='chw' or 'hwc'")
        if layout is not None and bayer is None:
            hwc, chw = hwc and layout == "hwc", chw and layout == "chw"
        if gray:  # (H, W)
            if shape[0] == 0 or shape[1] == 0:
                raise ValueError(f"tensor of shape {shape}: an empty frame")
            if st[1] != 1 and shape[1] > 1:
                raise ValueError(f"strides {st}: the inner dimension must have unit stride")
            h, w, stride, fmt = shape[0], shape[1], st[0], JPGE_FMT_GRAY8 if bayer is None else bayer
            if h == 1:
                stride = w  # (one row: any pitch)
        elif hwc:  # (H, W, C)
            if st[2] != 1 or (st[1] != shape[2] and shape[1] > 1):  # (one pixel per row: any pixel stride)
                raise ValueError(f"strides {st}: the inner dimension must have unit stride (pixels packed)")
            h, w, stride = shape[0], shape[1], st[0]
            fmt = {(3, "rgb"): JPGE_FMT_RGB8, (3, "bgr"): JPGE_FMT_BGR8, (4, "rgb"): JPGE_FMT_RGBA8,
                   (4, "bgr"): JPGE_FMT_BGRA8}[(shape[2], order)]
        elif chw:  # (3, H, W)
            if order != "rgb":
                raise ValueError("a planar (3, H, W) tensor is R, G, B")
            if st[2] != 1:
                raise ValueError(f"strides {st}: the inner dimension must have unit stride")
            h, w, stride, plane_stride, fmt = shape[1], shape[2], st[1], st[0], JPGE_FMT_RGB8_PLANAR
        else:
            raise ValueError(f"tensor of shape {shape}: (3, H, W), (H, W, 3), (H, W, 4) or (H, W)")
        if stride < w * input_format_info(fmt)[0] and h > 1:
            raise ValueError("rows overlap")
        return self._encode_view(t.data_ptr(), t.is_cuda, fmt, plane_stride, w, h, stride, quality, maxval, out)

    def encode_tensor_yuv(self, y, cbcr_or_cb, cr=None, quality: int = 50, out=None):
        """One frame of Y, Cb, Cr torch uint8 tensors (a decoder's surface; full-range BT.601
        samples, or what set_yuv_transform says they are) through jpge_encode_rgb8, read in place: (H, W) + (ch, cw, 2) is NV12, (H, W) + two (ch, cw) is
        I420, (H, W) + two (H, W) is YUV444_PLANAR (ch, cw: H, W halved, rounded up).  The
        planes must be views of one allocation, all on one device, at offsets the layout can
        express (jpge.h): unit inner strides, the chroma after the Y plane, NV12's Cb,Cr rows
        at the Y pitch, I420's Cb and Cr rows at pitch (Y pitch + 1) / 2 with Cr ch rows after
        Cb, the 4:4:4 planes at the Y pitch and equally spaced; else ValueError.  A 4:2:0
        layout needs subsampling mode 420.  Result and `out`: as encode_tensor."""
        planes = [y, cbcr_or_cb] + ([] if cr is None else [cr])
        for p in planes:
            if p.element_size() != 1 or p.dtype.is_floating_point or p.device != y.device:
                raise ValueError("encode_tensor_yuv takes uint8 tensors on one device")
        if y.dim() != 2 or y.numel() == 0:
            raise ValueError(f"Y plane of shape {tuple(y.shape)}: (H, W)")
        h, w = y.shape
        ch, cw = (h + 1) // 2, (w + 1) // 2
        c = cbcr_or_cb
        if cr is None and tuple(c.shape) == (ch, cw, 2):
            fmt = JPGE_FMT_NV12
        elif cr is not None and tuple(c.shape) == (ch, cw) == tuple(cr.shape) and (h, w) != (ch, cw):
            fmt = JPGE_FMT_I420
        elif cr is not None and tuple(c.shape) == (h, w) == tuple(cr.shape):
            fmt = JPGE_FMT_YUV444_PLANAR  # (a 1x1 frame's planes fit both: the layouts agree on it)
        else:
            raise ValueError(f"chroma of shape {tuple(c.shape)}" + ("" if cr is None else f", {tuple(cr.shape)}") +
                             f" for a {w}x{h} Y plane: ({ch}, {cw}, 2), two ({ch}, {cw}) or two ({h}, {w})")
        if fmt == JPGE_FMT_YUV444_PLANAR:  # (full-size chroma: not a layout of the table)
            plane_stride = _chroma_offset(planes)
            stride, cp, rp = (_row_pitch(p) for p in planes)
            if stride is None:
                stride = w  # (one row in every plane: any pitch)
            if any(q is not None and q != stride for q in (cp, rp)):
                raise ValueError(f"chroma pitches {cp}, {rp}: the planes share the Y pitch {stride}")
            if cr.data_ptr() - c.data_ptr() != plane_stride:
                raise ValueError("the Y, Cb and Cr planes must be equally spaced")
            if stride < w:
                raise ValueError("rows overlap")
        else:
            stride, plane_stride = _plane_geom(_YUV[fmt], w, h, y, c, cr)
        return self._encode_view(y.data_ptr(), y.is_cuda, fmt, plane_stride, w, h, stride, quality, 255, out)

    def encode_tensor_yuv10(self, y, cbcr_or_cb, cr=None, quality: int = 50, out=None):
        """One 10-bit 4:2:0 frame of 2-D 16-bit torch tensors (a Main10 decoder's surface), read in
        place through jpge_encode_rgb8: (H, W) + (ch, 2 * cw) of interleaved Cb,Cr words is P010
        (samples in the words' top 10 bits), (H, W) + two (ch, cw) is I010 (samples in the low
        10 bits; ch, cw: H, W halved, rounded up).  The planes must be views of one allocation,
        on one device, at offsets the layout can express (jpge.h): unit inner strides, the chroma
        after the Y plane, P010's Cb,Cr rows at the Y pitch, I010's Cb and Cr rows at pitch
        2 * ceil(Y pitch in bytes / 4) with Cr ch rows after Cb; else ValueError.  Needs
        subsampling mode 420.  Result and `out`: as encode_tensor."""
        planes = [y, cbcr_or_cb] + ([] if cr is None else [cr])
        for p in planes:
            if p.element_size() != 2 or p.dtype.is_floating_point or p.dim() != 2 or p.device != y.device:
                raise ValueError("encode_tensor_yuv10 takes 2-D 16-bit integer tensors on one device")
        if y.numel() == 0:
            raise ValueError(f"Y plane of shape {tuple(y.shape)}: (H, W)")
        h, w = y.shape
        ch, cw = (h + 1) // 2, (w + 1) // 2
        c = cbcr_or_cb
        if cr is None and tuple(c.shape) == (ch, 2 * cw):
            fmt = JPGE_FMT_P010
        elif cr is not None and tuple(c.shape) == (ch, cw) == tuple(cr.shape):
            fmt = JPGE_FMT_I010
        else:
            raise ValueError(f"chroma of shape {tuple(c.shape)}" + ("" if cr is None else f", {tuple(cr.shape)}") +
                             f" for a {w}x{h} Y plane: ({ch}, {2 * cw}) or two ({ch}, {cw})")
        stride, plane_stride = _plane_geom(_YUV[fmt], w, h, y, c, cr)
        return self._encode_view(y.data_ptr(), y.is_cuda, fmt, plane_stride, w, h, stride, quality, 255, out)

    def encode_tensor_yuv422p10(self, y_or_packed, cbcr_or_cb=None, cr=None, quality: int = 50, out=None):
        """One 10-bit 4:2:2 frame of 2-D 16-bit torch tensors (an SDI capture buffer, or a ProRes /
        DNxHR / HEVC RExt decoder's surface), read in place through jpge_encode_rgb8: (H, 4 * cw)
        alone is Y210 (groups Y0 Cb Y1 Cr, samples in the words' top 10 bits; the width is
        2 * cw, an odd width goes through encode_ptr), (H, W) + (H, 2 * cw) of interleaved Cb,Cr
        words is P210 (top 10 bits), (H, W) + two (H, cw) is I210 (low 10 bits; cw: W halved,
        rounded up).  The planes must be views of one allocation, on one device, at offsets the
        layout can express (jpge.h): unit inner strides, the chroma after the Y plane, P210's
        Cb,Cr rows at the Y pitch, I210's Cb and Cr rows at pitch 2 * ceil(Y pitch in bytes / 4)
        with Cr H rows after Cb; else ValueError.  Every subsampling mode takes these layouts (422
        is the native one).  Result and `out`: as encode_tensor."""
        y, c = y_or_packed, cbcr_or_cb
        planes = [p for p in (y, c, cr) if p is not None]
        for p in planes:
            if p.element_size() != 2 or p.dtype.is_floating_point or p.dim() != 2 or p.device != y.device:
                raise ValueError("encode_tensor_yuv422p10 takes 2-D 16-bit integer tensors on one device")
        if y.numel() == 0:
            raise ValueError(f"Y plane of shape {tuple(y.shape)}: (H, W)")
        if c is None and cr is not None:
            raise ValueError("a Cr plane goes with a Cb plane")
        h, w = y.shape
        cw = (w + 1) // 2
        if c is None:  # packed
            if w % 4:
                raise ValueError(f"packed frame of shape {tuple(y.shape)}: (H, 4 * cw), whole groups of four words")
            w, fmt = w // 2, JPGE_FMT_Y210
        elif cr is None and tuple(c.shape) == (h, 2 * cw):
            fmt = JPGE_FMT_P210
        elif cr is not None and tuple(c.shape) == (h, cw) == tuple(cr.shape):
            fmt = JPGE_FMT_I210
        else:
            raise ValueError(f"chroma of shapes {[tuple(p.shape) for p in planes[1:]]} for a {w}x{h} Y plane: "
                             f"({h}, {2 * cw}) or two ({h}, {cw})")
        stride, plane_stride = _plane_geom(_YUV[fmt], w, h, y, c, cr)
        return self._encode_view(y.data_ptr(), y.is_cuda, fmt, plane_stride, w, h, stride, quality, 255, out)

    def encode_tensor_v210(self, t, width: int, quality: int = 50, out=None):
        """One v210 frame (JPGE_FMT_V210: a 10-bit SDI capture buffer) of a 2-D device or host torch
        tensor of rows, uint8 (H, bytes) or int32 (H, words), read in place through
        jpge_encode_rgb8.  `width` is explicit: a row's length does not determine it.  ValueError
        for what the library would refuse: another type or rank, an inner stride other than 1, a row
        shorter than v210_row_bytes(width), a base or row pitch that is no multiple of 4, a width
        outside 1..65535.  Every subsampling mode takes the layout (422 is the native one).
        Result and `out`: as encode_tensor."""
        import torch
        if t.dtype not in (torch.uint8, torch.int32) or t.dim() != 2 or t.numel() == 0:
            raise ValueError("encode_tensor_v210 takes a 2-D uint8 or int32 tensor of rows")
        if t.stride(1) != 1 and t.shape[1] > 1:
            raise ValueError(f"strides {tuple(t.stride())}: the inner dimension must have unit stride")
        w, h, es = int(width), int(t.shape[0]), t.element_size()
        if not 1 <= w <= 65535 or h > 65535:
            raise ValueError(f"a {w}x{h} frame: 1..65535 each way")
        row = v210_row_bytes(w)
        if int(t.shape[1]) * es < row:
            raise ValueError(f"rows of {int(t.shape[1]) * es} bytes: {w} pixels take {row}")
        stride = es * t.stride(0) if h > 1 else row
        if stride < row:
            raise ValueError("rows overlap")
        if stride % 4 or t.data_ptr() % 4:
            raise ValueError("the base and the row pitch must be multiples of 4")
        return self._encode_view(t.data_ptr(), t.is_cuda, JPGE_FMT_V210, 0, w, h, stride, quality, 255, out)

    def encode_tensor_yuv422(self, y_or_packed, cbcr_or_cb=None, cr=None, quality: int = 50, out=None,
                             layout=None):
        """One 4:2:2 frame of torch uint8 tensors (a capture buffer or a 4:2:2 decoder's surface;
        full-range BT.601 samples, or what set_yuv_transform says they are) through
        jpge_encode_rgb8, read in place: a packed (H, W, 2) tensor with layout="yuyv" or "uyvy"
        (W even: a pixel's two bytes are its Y and one chroma sample of its pair; an odd width
        goes through encode_ptr); (H, W) + (H, cw, 2) is NV16; (H, W) + two (H, cw) is I422
        (cw: W halved, rounded up).  The planes must be views of one allocation, all on one
        device, at offsets the layout can express (jpge.h): unit inner strides, the chroma
        after the Y plane, NV16's Cb,Cr rows at the Y pitch, I422's Cb and Cr rows at pitch
        (Y pitch + 1) / 2 with Cr H rows after Cb; else ValueError.  Every subsampling mode
        takes these layouts (422 is the native one).  Result and `out`: as encode_tensor."""
        y, c = y_or_packed, cbcr_or_cb
        planes = [p for p in (y, c, cr) if p is not None]
        for p in planes:
            if p.element_size() != 1 or p.dtype.is_floating_point or p.device != y.device:
                raise ValueError("encode_tensor_yuv422 takes uint8 tensors on one device")
        if y.dim() == 3:  # packed
            if layout not in ("yuyv", "uyvy"):
                raise ValueError(f"layout {layout!r}: a packed (H, W, 2) tensor is 'yuyv' or 'uyvy'")
            if c is not None or cr is not None:
                raise ValueError("a packed frame is one tensor")
            if y.shape[2] != 2 or y.numel() == 0:
                raise ValueError(f"packed frame of shape {tuple(y.shape)}: (H, W, 2)")
            h, w = y.shape[:2]
            if w % 2:
                raise ValueError(f"packed frame of odd width {w}: a (H, W, 2) tensor cannot hold the last group")
            fmt = JPGE_FMT_YUYV if layout == "yuyv" else JPGE_FMT_UYVY
        else:
            if layout is not None:
                raise ValueError("layout goes with a packed (H, W, 2) tensor")
            if y.dim() != 2 or y.numel() == 0:
                raise ValueError(f"Y plane of shape {tuple(y.shape)}: (H, W)")
            h, w = y.shape
            cw = (w + 1) // 2
            if c is not None and cr is None and tuple(c.shape) == (h, cw, 2):
                fmt = JPGE_FMT_NV16
            elif c is not None and cr is not None and tuple(c.shape) == (h, cw) == tuple(cr.shape):
                fmt = JPGE_FMT_I422
            else:
                raise ValueError(f"chroma of shapes {[tuple(p.shape) for p in planes[1:]]} for a {w}x{h} Y plane: "
                                 f"({h}, {cw}, 2) or two ({h}, {cw})")
        stride, plane_stride = _plane_geom(_YUV[fmt], w, h, y, c, cr)
        return self._encode_view(y.data_ptr(), y.is_cuda, fmt, plane_stride, w, h, stride, quality, 255, out)

    def encode_batch_dev(self, frames: list[tuple[int, int, int, int]], outs: list[tuple[int, int]],
                         quality: int = 50, maxval: int = 255,
                         flags: int = JPGE_DEVICE_INPUT | JPGE_DEVICE_OUTPUT) -> list[int]:
        """Pipelined batch on device memory: frames = [(ptr, w, h, stride)], outs = [(ptr, cap)].
        Returns the .jpg length of each frame (bytes stay in device memory; without
        JPGE_DEVICE_OUTPUT in `flags` the outs are host pointers, e.g. pinned memory).
        The quality tables and the descriptor array of a repeated batch are reused."""
        q = self._qcache.get(quality)
        if q is None:
            qy, qc = self._tables(quality, None, None)
            q = self._qcache[quality] = (qy, qc, _p(qy), _p(qc))
        key = (tuple(frames), tuple(outs), maxval)
        if self._desc is None or self._desc[0] != key:
            arr = (Frame * len(frames))()
            for i, ((p, w, h, s), (o, cap)) in enumerate(zip(frames, outs)):
                arr[i].rgb, arr[i].width, arr[i].height, arr[i].stride, arr[i].maxval = p, w, h, s, maxval
                arr[i].out, arr[i].cap = o, cap
            self._desc = (key, arr)
        arr = self._desc[1]
        st = lib().jpge_encode_batch(self._ctx, arr, len(frames), q[2], q[3], int(flags))
        _check(st, "encode_batch")
        return [f.len for f in arr]

    def batch_status(self) -> list[int]:
        """The status of each frame of the last encode_batch_dev call (jpge_frame.status): when the
        call raised, the frames that were refused or failed; 0 for the others."""
        return [] if self._desc is None else [int(f.status) for f in self._desc[1]]

    def encode_batch(self, frames: list[np.ndarray], quality: int = 50, maxval: int = 255) -> list[bytes]:
        qy, qc = self._tables(quality, None, None)
        frames, geom = _as_frames(frames, self._fmt)
        outs = [np.empty(self._cap(w, h), np.uint8) for w, h, _ in geom]
        arr = (Frame * len(frames))()
        for i, (f, o, (w, h, stride)) in enumerate(zip(frames, outs, geom)):
            arr[i].rgb, arr[i].width, arr[i].height = _p(f), w, h
            arr[i].stride, arr[i].maxval, arr[i].out, arr[i].cap = stride, maxval, _p(o), o.size
        _check(lib().jpge_encode_batch(self._ctx, arr, len(frames), _p(qy), _p(qc), 0), "encode_batch")
        return [outs[i][:arr[i].len].tobytes() for i in range(len(frames))]

    def fdct_quant(self, rgb: np.ndarray, quality: int = 50, maxval: int = 255, qy=None, qc=None):
        """Stage dump: quantised coefficients (before DC diff) -> (Y, Cb, Cr) arrays of shape
        (nblocks, 64), blocks in raster order, natural order within a block.  GRAY8: (Y, None,
        None), the ceil(W/8) * ceil(H/8) blocks of the one component."""
        rgb, w, h, stride = _as_frame(rgb, self._fmt)
        if self._fmt == JPGE_FMT_GRAY8:
            y = np.zeros((-(-w // 8) * -(-h // 8), 64), np.int16)
            qy, qc = self._tables(quality, qy, self._gray_qc(qy, qc))
            _check(lib().jpge_fdct_quant(self._ctx, _p(rgb), w, h, stride, int(maxval), _p(qy), None, _p(y), None,
                                         None, 0), "fdct_quant")
            return y, None, None
        yh, yv = SUBSAMPLING[getattr(self, "_sub", 420)]
        dw, dh = downscaled_size(w, h, self.downscale)  # (the coded frame's blocks)
        dw, dh = oriented_size(dw, dh, self.orientation)
        mw, mh = -(-dw // (8 * yh)), -(-dh // (8 * yv))  # MCUs across / down
        y = np.zeros((mw * yh * mh * yv, 64), np.int16)
        cb = np.zeros((mw * mh, 64), np.int16)
        cr = np.zeros_like(cb)
        qy, qc = self._tables(quality, qy, qc)
        _check(lib().jpge_fdct_quant(self._ctx, _p(rgb), w, h, stride, int(maxval), _p(qy), _p(qc), _p(y), _p(cb),
                                     _p(cr), 0), "fdct_quant")
        return y, cb, cr

    # ---- row stripes (jpge_stripe_*; orchestration in jpgenc_amd.stripes) ----
    def stripe_transform(self, rgb_ptr: int, stride: int, width: int, height: int, mcu_row0: int, mcu_rows: int,
                         quality: int = 50, maxval: int = 255) -> np.ndarray:
        """K1 on a stripe (device RGB of its rows); returns its last Y/Cb/Cr DC (int32[3])."""
        qy, qc = self._tables(quality, None, None)
        last = np.zeros(3, np.int32)
        _check(lib().jpge_stripe_transform(self._ctx, rgb_ptr, stride, width, height, mcu_row0, mcu_rows,
                                           int(maxval), _p(qy), _p(qc), _p(last)), "stripe_transform")
        return last

    def stripe_stats(self, seed_dc) -> tuple[np.ndarray, np.ndarray]:
        seed = np.ascontiguousarray(seed_dc, np.int32)
        counts = np.zeros(1024, np.uint32)
        first = np.zeros(1024, np.uint64)
        _check(lib().jpge_stripe_stats(self._ctx, _p(seed), _p(counts), _p(first)), "stripe_stats")
        return counts, first

    def stripe_code(self, counts: np.ndarray, first: np.ndarray) -> tuple[tuple, int]:
        counts = np.ascontiguousarray(counts, np.uint32)
        first = np.ascontiguousarray(first, np.uint64)
        sm = StripeSummary()
        hl = ctypes.c_size_t()
        _check(lib().jpge_stripe_code(self._ctx, _p(counts), _p(first), ctypes.byref(sm), ctypes.byref(hl)),
               "stripe_code")
        return sm.as_tuple(), hl.value

    def stripe_pack(self, summaries: list, index: int, out_ptr: int, cap: int) -> tuple[int, int, int]:
        arr = (StripeSummary * len(summaries))(*[StripeSummary.from_tuple(t) for t in summaries])
        off, ln, tot = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
        _check(lib().jpge_stripe_pack(self._ctx, arr, len(summaries), index, out_ptr, cap, ctypes.byref(off),
                                      ctypes.byref(ln), ctypes.byref(tot)), "stripe_pack")
        return off.value, ln.value, tot.value

    # ---- plane stages: the reference's Image stage methods on fp64 planes (GPU) ----
    def color_convert(self, p0, p1, p2, target: int = JPGE_TO_YCBCR):
        """convertToColorSpace (Image.cpp:112-179) of three equal-size planes."""
        ins = [np.ascontiguousarray(p, np.float64) for p in (p0, p1, p2)]
        outs = [np.empty_like(ins[0]) for _ in range(3)]
        _check(lib().jpge_color_convert(self._ctx, *[_p(a) for a in ins], *[_p(a) for a in outs], ins[0].size,
                                        int(target), 0), "color_convert")
        return outs

    def subsample_plane(self, plane, mode: int) -> np.ndarray:
        """Image::subsample with applySubsampling's mask for `mode` (jpge.h JPGE_S*)."""
        a = np.ascontiguousarray(plane, np.float64)
        r, c = ctypes.c_uint32(), ctypes.c_uint32()
        _check(lib().jpge_subsample_plane(self._ctx, _p(a), a.shape[0], a.shape[1], int(mode), None, ctypes.byref(r),
                                          ctypes.byref(c), 0), "subsample_plane")
        out = np.empty((r.value, c.value), np.float64)
        _check(lib().jpge_subsample_plane(self._ctx, _p(a), a.shape[0], a.shape[1], int(mode), _p(out),
                                          ctypes.byref(r), ctypes.byref(c), 0), "subsample_plane")
        return out

    def dct_plane(self, plane, mode: int = DCT_ARAI) -> np.ndarray:
        """applyDCT(mode) (Image.cpp:540-595) on one plane of 8x8 blocks."""
        a = np.ascontiguousarray(plane, np.float64)
        out = np.empty_like(a)
        _check(lib().jpge_dct_plane(self._ctx, _p(a), a.shape[0], a.shape[1], int(mode), _p(out), 0), "dct_plane")
        return out

    def quantize_plane(self, plane, table) -> np.ndarray:
        """applyQuantization's per-block quantize (Coding.hpp:84-97) with one table."""
        a = np.ascontiguousarray(plane, np.float64)
        t = np.ascontiguousarray(table, np.uint8).reshape(64)
        out = np.empty(a.shape, np.int32)
        _check(lib().jpge_quantize_plane(self._ctx, _p(a), a.shape[0], a.shape[1], _p(t), _p(out), 0),
               "quantize_plane")
        return out

    def encode_planes(self, p0, p1, p2, real_width: int, real_height: int, colorspace: int = JPGE_TO_RGB,
                      quality: int = 50) -> bytes:
        """writeJPEG (Image.cpp:831-976) on an Image's three fp64 planes (rows x cols,
        multiples of 16): R,G,B (colorspace JPGE_TO_RGB) or Y,Cb,Cr (JPGE_TO_YCBCR)."""
        ins = [np.ascontiguousarray(p, np.float64) for p in (p0, p1, p2)]
        rows, cols = ins[0].shape
        qy, qc = self._tables(quality, None, None)
        out = np.empty(max_jpeg_bytes(cols, rows), np.uint8)
        n = ctypes.c_size_t()
        _check(lib().jpge_encode_planes(self._ctx, *[_p(a) for a in ins], rows, cols, int(colorspace), real_width,
                                        real_height, _p(qy), _p(qc), _p(out), out.size, ctypes.byref(n), 0),
               "encode_planes")
        return out[:n.value].tobytes()

    def encode_file(self, ppm_path: str, jpg_path: str, quality: int = 50) -> None:
        """main.cpp: loadPPM(ppm_path) + writeJPEG(jpg_path)."""
        _check(lib().jpge_encode_file(self._ctx, ppm_path.encode(), jpg_path.encode(), int(quality)), "encode_file")

    def encode_files(self, ppm_paths: list[str], jpg_paths: list[str], quality: int = 50, group: int = 0):
        """Many PPM files -> .jpg files through the ingest pipeline; returns the .jpg lengths."""
        n = len(ppm_paths)
        if len(jpg_paths) != n:
            raise ValueError("ppm_paths and jpg_paths differ in length")
        ins = (ctypes.c_char_p * n)(*[p.encode() for p in ppm_paths])
        outs = (ctypes.c_char_p * n)(*[p.encode() for p in jpg_paths])
        lens = np.zeros(n, np.uint64)
        sts = np.zeros(n, np.int32)
        st = lib().jpge_encode_files(self._ctx, ins, outs, n, int(quality), _p(lens), _p(sts), int(group))
        _check(st, f"encode_files (statuses {sts.tolist()})" if st else "encode_files")
        return [int(x) for x in lens]

    def symbol_stats(self, rgb: np.ndarray, quality: int = 50, maxval: int = 255):
        rgb, w, h, stride = _as_frame(rgb, self._fmt)
        qy, qc = self._tables(quality, None, None)
        counts = np.zeros(1024, np.uint32)
        first = np.zeros(1024, np.uint64)
        _check(lib().jpge_symbol_stats(self._ctx, _p(rgb), w, h, stride, int(maxval), _p(qy), _p(qc), _p(counts),
                                       _p(first), 0), "symbol_stats")
        return counts.reshape(4, 256), first.reshape(4, 256)


class Group:
    """A device group (jpge_group_open): one process, one context per listed device,
    RCCL over xGMI between distinct devices (a device listed twice: host exchanges)."""

    _orient = JPGE_ORIENT_NONE  # the orientation as set through this object (sizes the output buffers)

    def __init__(self, devices, lanes: int = 0):
        devs = (ctypes.c_int * len(devices))(*devices)
        self._g = ctypes.c_void_p()
        _check(lib().jpge_group_open(len(devices), devs, int(lanes), ctypes.byref(self._g)), "group_open")
        self._fmt = JPGE_FMT_RGB8
        _live_encoders.add(self)

    def close(self) -> None:
        if self._g:
            lib().jpge_group_close(self._g)
            self._g = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def size(self) -> tuple[int, bool]:
        """(members, whether the exchanges ride RCCL)"""
        n, r = ctypes.c_int(), ctypes.c_int()
        _check(lib().jpge_group_size(self._g, ctypes.byref(n), ctypes.byref(r)), "group_size")
        return n.value, bool(r.value)

    def set_restart(self, mcus: int) -> None:
        _check(lib().jpge_group_set_restart_interval(self._g, int(mcus)), "group_set_restart_interval")

    def set_input_format(self, fmt: int, plane_stride: int = 0) -> None:
        """Input layout of every member's context (jpge_set_input_format): for encode_batch;
        encode_striped needs JPGE_FMT_RGB8."""
        for m in range(self.size()[0]):
            c = ctypes.c_void_p()
            _check(lib().jpge_group_context(self._g, m, ctypes.byref(c)), "group_context")
            _check(lib().jpge_set_input_format(c, int(fmt), int(plane_stride)), "set_input_format")
        self._fmt = int(fmt)

    def set_huffman(self, mode: int, specs=None) -> None:
        """Huffman mode of every member's context (Encoder.set_huffman): for encode_batch;
        encode_striped needs JPGE_HUFF_OPTIMAL."""
        arr = _huff_specs(specs)
        for m in range(self.size()[0]):
            c = ctypes.c_void_p()
            _check(lib().jpge_group_context(self._g, m, ctypes.byref(c)), "group_context")
            _check(lib().jpge_set_huffman(c, int(mode), arr), "set_huffman")

    def set_yuv_transform(self, preset: int, coeffs=None) -> None:
        """Sample transform of every member's context (Encoder.set_yuv_transform): for encode_batch."""
        t = None if coeffs is None else YuvTransform.from_tuple(coeffs)
        for m in range(self.size()[0]):
            c = ctypes.c_void_p()
            _check(lib().jpge_group_context(self._g, m, ctypes.byref(c)), "group_context")
            _check(lib().jpge_set_yuv_transform(c, int(preset), t), "set_yuv_transform")

    def set_downscale(self, factor: int) -> None:
        """Box downscale of every member's context (Encoder.set_downscale): for encode_batch;
        encode_striped needs factor 1."""
        for m in range(self.size()[0]):
            c = ctypes.c_void_p()
            _check(lib().jpge_group_context(self._g, m, ctypes.byref(c)), "group_context")
            _check(lib().jpge_set_downscale(c, int(factor)), "set_downscale")

    def set_orientation(self, o: int) -> None:
        """Orientation of every member's context (Encoder.set_orientation): for encode_batch;
        encode_striped needs JPGE_ORIENT_NONE."""
        for m in range(self.size()[0]):
            c = ctypes.c_void_p()
            _check(lib().jpge_group_context(self._g, m, ctypes.byref(c)), "group_context")
            _check(lib().jpge_set_orientation(c, int(o)), "set_orientation")
        self._orient = int(o)

    def set_channel_lut(self, lut) -> None:
        """Per-channel lookup tables of every member's context (Encoder.set_channel_lut): for
        encode_batch; encode_striped needs them off."""
        t = None if lut is None else _channel_lut(lut)
        for m in range(self.size()[0]):
            c = ctypes.c_void_p()
            _check(lib().jpge_group_context(self._g, m, ctypes.byref(c)), "group_context")
            _check(lib().jpge_set_channel_lut(c, None if t is None else _p(t)), "set_channel_lut")

    def encode_batch(self, frames: list[np.ndarray], quality: int = 50, maxval: int = 255) -> list[bytes]:
        """Config 4: frame i on member i mod N."""
        qy, qc = quality_tables(quality)
        frames, geom = _as_frames(frames, self._fmt)
        # (the coded frame's bound: a transposed orientation swaps the sides)
        t = self._orient >= JPGE_ORIENT_TRANSPOSE
        outs = [np.empty(max_jpeg_bytes(h, w) if t else max_jpeg_bytes(w, h), np.uint8) for w, h, _ in geom]
        arr = (Frame * len(frames))()
        for i, (f, o, (w, h, stride)) in enumerate(zip(frames, outs, geom)):
            arr[i].rgb, arr[i].width, arr[i].height = _p(f), w, h
            arr[i].stride, arr[i].maxval, arr[i].out, arr[i].cap = stride, maxval, _p(o), o.size
        _check(lib().jpge_group_encode_batch(self._g, arr, len(frames), _p(qy), _p(qc), 0), "group_encode_batch")
        return [outs[i][:arr[i].len].tobytes() for i in range(len(frames))]

    def encode_striped(self, rgb: np.ndarray, quality: int = 50, maxval: int = 255) -> bytes:
        """Config 5: one image in row stripes over the members."""
        rgb = np.ascontiguousarray(rgb, np.uint8)
        h, w = rgb.shape[:2]
        qy, qc = quality_tables(quality)
        out = np.empty(max_jpeg_bytes(w, h), np.uint8)
        n = ctypes.c_size_t()
        _check(lib().jpge_group_encode_striped(self._g, _p(rgb), w, h, w * 3, int(maxval), _p(qy), _p(qc), _p(out),
                                               out.size, ctypes.byref(n)), "group_encode_striped")
        return out[:n.value].tobytes()


def stripe_place(summaries: list, index: int, header_len: int) -> tuple[int, int]:
    """Host-only placement of stripe `index`: (first output byte, whole file length)."""
    arr = (StripeSummary * len(summaries))(*[StripeSummary.from_tuple(t) for t in summaries])
    off, tot = ctypes.c_size_t(), ctypes.c_size_t()
    _check(lib().jpge_stripe_place(arr, len(summaries), index, header_len, ctypes.byref(off), ctypes.byref(tot)),
           "stripe_place")
    return off.value, tot.value


def write_jpeg(path: str, ppm: PPM, quality: int = 50, device: int = 0) -> int:
    """loadPPM + writeJPEG convenience; returns bytes written."""
    with Encoder(device) as enc:
        data = enc.encode(ppm.rgb, quality=quality, maxval=ppm.maxval)
    with open(path, "wb") as f:
        f.write(data)
    return len(data)
