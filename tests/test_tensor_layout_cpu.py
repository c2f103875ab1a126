"""What the six Encoder.encode_tensor* methods make of their tensors, without a GPU: which views
they accept, and the (layout, plane stride, pointer, width, height, row stride) they hand to
encode_ptr.  A recording subclass of Encoder stands in for the context, so only host arithmetic
runs.  Every expectation is a literal worked out here from the layout rules of include/jpge.h
(in bytes; a row stride of one row is the layout's least one):

  interleaved RGB: rows of `stride` bytes, C bytes per pixel; planar RGB and YUV444_PLANAR: three
    planes `plane stride` apart, rows at `stride`; GRAY8: one plane
  NV12, NV16, P010, P210: Y rows at `stride`, then at `plane stride` from Y rows of Cb,Cr pairs at
    the same stride (ceil(h / 2) rows for the 4:2:0 pair, h for the 4:2:2 pair)
  I420, I422: Cb at `plane stride` from Y, rows at (stride + 1) / 2; Cr that many * rows later
  I010, I210: the same with rows at 2 * ceil(stride / 4)
  YUYV, UYVY: rows of 4-byte groups, least stride 4 * ceil(w / 2); Y210: 8-byte groups
  V210: rows of 16 * ceil(w / 6) bytes, base and stride multiples of 4

A case is (id, method, element type, storage offset, [(offset, shape, strides) per tensor],
keywords, expectation); offsets and strides are in elements as torch counts them, the offsets
relative to the storage offset; "own" as a fourth entry puts a tensor in an allocation of its
own; an expectation of None is a refusal."""
import pytest
import torch

import jpgenc_amd as J

U8, I16, I32, F16, F32 = torch.uint8, torch.int16, torch.int32, torch.float16, torch.float32
F8 = torch.float8_e5m2
IDLE = (J.JPGE_FMT_BGRA8, 123)  # the input format around every call


def test_constants():
    assert (J.JPGE_FMT_RGB8, J.JPGE_FMT_BGR8, J.JPGE_FMT_RGBA8, J.JPGE_FMT_BGRA8, J.JPGE_FMT_RGB8_PLANAR) == (0, 1, 2, 3, 4)
    assert (J.JPGE_FMT_GRAY8, J.JPGE_FMT_NV12, J.JPGE_FMT_I420, J.JPGE_FMT_YUV444_PLANAR) == (8, 16, 17, 18)
    assert (J.JPGE_FMT_YUYV, J.JPGE_FMT_UYVY, J.JPGE_FMT_NV16, J.JPGE_FMT_I422) == (20, 21, 22, 23)
    assert (J.JPGE_FMT_P010, J.JPGE_FMT_I010, J.JPGE_FMT_Y210, J.JPGE_FMT_P210, J.JPGE_FMT_I210) == (32, 33, 40, 41, 42)
    assert J.JPGE_FMT_V210 == 48 and (J.JPGE_DEVICE_INPUT, J.JPGE_DEVICE_OUTPUT) == (1, 2)


class Recorder(J.Encoder):
    """An Encoder without a context: it keeps the input format itself and records every
    encode_ptr call as (fmt, plane stride, ptr - base, w, h, stride, cap, quality, maxval, flags)."""

    def __init__(self, fail=False):
        self._fmt, self._qcache, self.calls = IDLE[0], {}, []
        self.state, self.base, self.fail = IDLE, 0, fail

    def input_format(self):
        return self.state

    def set_input_format(self, fmt, plane_stride=0):
        self.state = (int(fmt), int(plane_stride))
        self._fmt = int(fmt)

    def encode_ptr(self, rgb_ptr, w, h, stride, out_ptr, cap, quality=50, maxval=255, flags=3):
        self.calls.append(self.state + (rgb_ptr - self.base, w, h, stride, cap, quality, maxval, flags))
        if self.fail:
            raise RuntimeError("encode_ptr failed")
        return 7

    def close(self):
        pass

    def __del__(self):
        pass


class DeviceOut:
    """What the methods ask of `out`, answered as a device tensor of 555 bytes would."""
    is_cuda = True

    def is_contiguous(self):
        return True

    def element_size(self):
        return 1

    def data_ptr(self):
        return 4096

    def numel(self):
        return 555


def views(dtype, off, specs):
    """The tensors of a case and the address of their allocation."""
    es = torch.empty(0, dtype=dtype).element_size()

    def span(shape, strides):
        return 0 if 0 in shape else sum((n - 1) * s for n, s in zip(shape, strides)) + 1

    def alloc(n):
        return torch.zeros(max(n, 1) * es, dtype=U8).view(dtype)
    shared = [s for s in specs if s is not None and len(s) == 3]
    buf = alloc(max([off + s[0] + span(s[1], s[2]) for s in shared] + [1]))
    out = []
    for s in specs:
        if s is None:
            out.append(None)
        elif len(s) == 3:
            assert off + s[0] >= 0
            out.append(buf.as_strided(s[1], s[2], off + s[0]))
        else:
            out.append(alloc(span(s[1], s[2])).as_strided(s[1], s[2], 0))
    return out, buf.data_ptr()


def run(enc, method, dtype, off, specs, kw, out=None):
    ts, enc.base = views(dtype, off, specs)
    if method == "rgb":
        return enc.encode_tensor(ts[0], quality=77, maxval=200, out=out, **kw)
    if method == "v210":
        return enc.encode_tensor_v210(ts[0], quality=77, out=out, **kw)
    return getattr(enc, "encode_tensor_" + method)(*ts, quality=77, out=out, **kw)


HWC, CHW = {"layout": "hwc"}, {"layout": "chw"}
BGR = {"order": "bgr"}
YUYV, UYVY = {"layout": "yuyv"}, {"layout": "uyvy"}

# expectation: (layout, plane stride, ptr - base, w, h, stride), all in bytes
ACCEPTED = [
    # ---- interleaved RGB, (H, W, C): any row stride; one row passes its stride as it is
    ("rgb8-1x1", "rgb", U8, 0, [(0, (1, 1, 3), (3, 3, 1))], {}, (0, 0, 0, 1, 1, 3)),
    ("rgb8-row", "rgb", U8, 0, [(0, (1, 4, 3), (12, 3, 1))], {}, (0, 0, 0, 4, 1, 12)),
    ("rgb8-row-short-stride", "rgb", U8, 0, [(0, (1, 4, 3), (5, 3, 1))], {}, (0, 0, 0, 4, 1, 5)),
    ("rgb8-col", "rgb", U8, 0, [(0, (4, 1, 3), (3, 3, 1))], {}, (0, 0, 0, 1, 4, 3)),
    ("rgb8-col-any-pixel-stride", "rgb", U8, 0, [(0, (4, 1, 3), (10, 7, 1))], {}, (0, 0, 0, 1, 4, 10)),
    ("rgb8-5x3", "rgb", U8, 0, [(0, (3, 5, 3), (15, 3, 1))], HWC, (0, 0, 0, 5, 3, 15)),
    ("rgb8-pitched", "rgb", U8, 0, [(0, (3, 5, 3), (32, 3, 1))], HWC, (0, 0, 0, 5, 3, 32)),
    ("rgb8-crop", "rgb", U8, 30, [(0, (2, 5, 3), (24, 3, 1))], {}, (0, 0, 30, 5, 2, 24)),
    ("bgr8-1x1", "rgb", U8, 0, [(0, (1, 1, 3), (3, 3, 1))], BGR, (1, 0, 0, 1, 1, 3)),
    ("bgr8-row", "rgb", U8, 0, [(0, (1, 4, 3), (12, 3, 1))], BGR, (1, 0, 0, 4, 1, 12)),
    ("bgr8-col", "rgb", U8, 0, [(0, (4, 1, 3), (3, 3, 1))], BGR, (1, 0, 0, 1, 4, 3)),
    ("bgr8-5x3", "rgb", U8, 0, [(0, (3, 5, 3), (15, 3, 1))], {"order": "bgr", "layout": "hwc"}, (1, 0, 0, 5, 3, 15)),
    ("bgr8-pitched", "rgb", U8, 0, [(0, (2, 5, 3), (32, 3, 1))], BGR, (1, 0, 0, 5, 2, 32)),
    ("bgr8-crop", "rgb", U8, 30, [(0, (2, 5, 3), (24, 3, 1))], BGR, (1, 0, 30, 5, 2, 24)),
    ("rgba8-1x1", "rgb", U8, 0, [(0, (1, 1, 4), (4, 4, 1))], {}, (2, 0, 0, 1, 1, 4)),
    ("rgba8-row", "rgb", U8, 0, [(0, (1, 4, 4), (16, 4, 1))], {}, (2, 0, 0, 4, 1, 16)),
    ("rgba8-col", "rgb", U8, 0, [(0, (4, 1, 4), (4, 4, 1))], {}, (2, 0, 0, 1, 4, 4)),
    ("rgba8-5x3", "rgb", U8, 0, [(0, (3, 5, 4), (20, 4, 1))], HWC, (2, 0, 0, 5, 3, 20)),
    ("rgba8-pitched", "rgb", U8, 0, [(0, (3, 5, 4), (32, 4, 1))], HWC, (2, 0, 0, 5, 3, 32)),
    ("rgba8-crop", "rgb", U8, 40, [(0, (2, 5, 4), (32, 4, 1))], {}, (2, 0, 40, 5, 2, 32)),
    ("bgra8-1x1", "rgb", U8, 0, [(0, (1, 1, 4), (4, 4, 1))], BGR, (3, 0, 0, 1, 1, 4)),
    ("bgra8-row", "rgb", U8, 0, [(0, (1, 4, 4), (16, 4, 1))], BGR, (3, 0, 0, 4, 1, 16)),
    ("bgra8-col", "rgb", U8, 0, [(0, (4, 1, 4), (4, 4, 1))], BGR, (3, 0, 0, 1, 4, 4)),
    ("bgra8-5x3", "rgb", U8, 0, [(0, (3, 5, 4), (20, 4, 1))], {"order": "bgr", "layout": "hwc"}, (3, 0, 0, 5, 3, 20)),
    ("bgra8-pitched", "rgb", U8, 0, [(0, (2, 5, 4), (32, 4, 1))], BGR, (3, 0, 0, 5, 2, 32)),
    ("bgra8-crop", "rgb", U8, 40, [(0, (2, 5, 4), (32, 4, 1))], BGR, (3, 0, 40, 5, 2, 32)),
    # ---- planar RGB, (3, H, W): plane stride t.stride(0), row stride t.stride(1)
    ("rgbp-1x1", "rgb", U8, 0, [(0, (3, 1, 1), (1, 1, 1))], {}, (4, 1, 0, 1, 1, 1)),
    ("rgbp-row", "rgb", U8, 0, [(0, (3, 1, 5), (5, 5, 1))], {}, (4, 5, 0, 5, 1, 5)),
    ("rgbp-col", "rgb", U8, 0, [(0, (3, 4, 1), (4, 1, 1))], {}, (4, 4, 0, 1, 4, 1)),
    ("rgbp-5x3", "rgb", U8, 0, [(0, (3, 3, 5), (15, 5, 1))], {}, (4, 15, 0, 5, 3, 5)),
    ("rgbp-pitched", "rgb", U8, 0, [(0, (3, 3, 5), (24, 8, 1))], {}, (4, 24, 0, 5, 3, 8)),
    ("rgbp-offset-spare-rows", "rgb", U8, 9, [(0, (3, 3, 5), (40, 8, 1))], {}, (4, 40, 9, 5, 3, 8)),
    ("rgbp-3x2-chw", "rgb", U8, 0, [(0, (3, 2, 3), (6, 3, 1))], CHW, (4, 6, 0, 3, 2, 3)),
    ("rgb8-3x3-hwc", "rgb", U8, 0, [(0, (3, 3, 3), (9, 3, 1))], HWC, (0, 0, 0, 3, 3, 9)),
    # ---- GRAY8, (H, W): one row has the least stride
    ("gray-1x1", "rgb", U8, 0, [(0, (1, 1), (1, 1))], {}, (8, 0, 0, 1, 1, 1)),
    ("gray-row", "rgb", U8, 0, [(0, (1, 4), (9, 1))], {}, (8, 0, 0, 4, 1, 4)),
    ("gray-col", "rgb", U8, 0, [(0, (4, 1), (1, 1))], {}, (8, 0, 0, 1, 4, 1)),
    ("gray-col-any-inner-stride", "rgb", U8, 0, [(0, (4, 1), (3, 5))], {}, (8, 0, 0, 1, 4, 3)),
    ("gray-5x3", "rgb", U8, 0, [(0, (3, 5), (5, 1))], {}, (8, 0, 0, 5, 3, 5)),
    ("gray-pitched", "rgb", U8, 0, [(0, (3, 5), (8, 1))], {}, (8, 0, 0, 5, 3, 8)),
    ("gray-offset", "rgb", U8, 11, [(0, (3, 5), (8, 1))], {}, (8, 0, 11, 5, 3, 8)),
    # ---- NV12: (H, W) + (ch, cw, 2)
    ("nv12-1x1", "yuv", U8, 0, [(0, (1, 1), (1, 1)), (2, (1, 1, 2), (2, 2, 1))], {}, (16, 2, 0, 1, 1, 2)),
    ("nv12-row", "yuv", U8, 0, [(0, (1, 4), (4, 1)), (4, (1, 2, 2), (4, 2, 1))], {}, (16, 4, 0, 4, 1, 4)),
    ("nv12-row-odd", "yuv", U8, 0, [(0, (1, 5), (9, 1)), (6, (1, 3, 2), (9, 2, 1))], {}, (16, 6, 0, 5, 1, 6)),
    ("nv12-col", "yuv", U8, 0, [(0, (4, 1), (2, 1)), (8, (2, 1, 2), (2, 2, 1))], {}, (16, 8, 0, 1, 4, 2)),
    ("nv12-h2", "yuv", U8, 0, [(0, (2, 4), (6, 1)), (12, (1, 2, 2), (100, 2, 1))], {}, (16, 12, 0, 4, 2, 6)),
    ("nv12-5x3", "yuv", U8, 0, [(0, (3, 5), (6, 1)), (18, (2, 3, 2), (6, 2, 1))], {}, (16, 18, 0, 5, 3, 6)),
    ("nv12-pitched", "yuv", U8, 0, [(0, (3, 5), (16, 1)), (48, (2, 3, 2), (16, 2, 1))], {}, (16, 48, 0, 5, 3, 16)),
    ("nv12-offset-spare-rows", "yuv", U8, 5, [(0, (3, 5), (16, 1)), (64, (2, 3, 2), (16, 2, 1))], {}, (16, 64, 5, 5, 3, 16)),
    # ---- I420: (H, W) + two (ch, cw); Cb rows at (stride + 1) / 2, Cr ch rows later
    ("i420-row", "yuv", U8, 0, [(0, (1, 4), (4, 1)), (4, (1, 2), (2, 1)), (6, (1, 2), (2, 1))], {}, (17, 4, 0, 4, 1, 4)),
    ("i420-col", "yuv", U8, 0, [(0, (4, 1), (1, 1)), (4, (2, 1), (1, 1)), (6, (2, 1), (1, 1))], {}, (17, 4, 0, 1, 4, 1)),
    ("i420-h2", "yuv", U8, 0, [(0, (2, 4), (4, 1)), (8, (1, 2), (50, 1)), (10, (1, 2), (60, 1))], {}, (17, 8, 0, 4, 2, 4)),
    ("i420-5x3", "yuv", U8, 0, [(0, (3, 5), (5, 1)), (15, (2, 3), (3, 1)), (21, (2, 3), (3, 1))], {}, (17, 15, 0, 5, 3, 5)),
    ("i420-pitched", "yuv", U8, 0, [(0, (3, 5), (16, 1)), (48, (2, 3), (8, 1)), (64, (2, 3), (8, 1))], {},
     (17, 48, 0, 5, 3, 16)),
    ("i420-odd-pitch", "yuv", U8, 0, [(0, (3, 5), (7, 1)), (21, (2, 3), (4, 1)), (29, (2, 3), (4, 1))], {},
     (17, 21, 0, 5, 3, 7)),
    ("i420-offset-spare-rows", "yuv", U8, 5, [(0, (3, 5), (16, 1)), (64, (2, 3), (8, 1)), (80, (2, 3), (8, 1))], {},
     (17, 64, 5, 5, 3, 16)),
    # ---- YUV444_PLANAR: three (H, W) at equal spacing (two (1, 1) chroma planes of a 1x1 frame are this layout)
    ("yuv444-1x1", "yuv", U8, 0, [(0, (1, 1), (1, 1)), (1, (1, 1), (1, 1)), (2, (1, 1), (1, 1))], {}, (18, 1, 0, 1, 1, 1)),
    ("yuv444-row", "yuv", U8, 0, [(0, (1, 4), (4, 1)), (4, (1, 4), (4, 1)), (8, (1, 4), (4, 1))], {}, (18, 4, 0, 4, 1, 4)),
    ("yuv444-col", "yuv", U8, 0, [(0, (4, 1), (1, 1)), (4, (4, 1), (1, 1)), (8, (4, 1), (1, 1))], {}, (18, 4, 0, 1, 4, 1)),
    ("yuv444-5x3", "yuv", U8, 0, [(0, (3, 5), (5, 1)), (15, (3, 5), (5, 1)), (30, (3, 5), (5, 1))], {}, (18, 15, 0, 5, 3, 5)),
    ("yuv444-pitched", "yuv", U8, 0, [(0, (3, 5), (8, 1)), (24, (3, 5), (8, 1)), (48, (3, 5), (8, 1))], {},
     (18, 24, 0, 5, 3, 8)),
    ("yuv444-offset-spare-rows", "yuv", U8, 3, [(0, (3, 5), (8, 1)), (40, (3, 5), (8, 1)), (80, (3, 5), (8, 1))], {},
     (18, 40, 3, 5, 3, 8)),
    # ---- YUYV, UYVY: one (H, W, 2), W even (a width of 1 is refused below)
    ("yuyv-2x1", "yuv422", U8, 0, [(0, (1, 2, 2), (4, 2, 1))], YUYV, (20, 0, 0, 2, 1, 4)),
    ("yuyv-row", "yuv422", U8, 0, [(0, (1, 4, 2), (99, 2, 1))], YUYV, (20, 0, 0, 4, 1, 8)),
    ("yuyv-one-group-col", "yuv422", U8, 0, [(0, (4, 2, 2), (4, 2, 1))], YUYV, (20, 0, 0, 2, 4, 4)),
    ("yuyv-6x3", "yuv422", U8, 0, [(0, (3, 6, 2), (12, 2, 1))], YUYV, (20, 0, 0, 6, 3, 12)),
    ("yuyv-pitched", "yuv422", U8, 0, [(0, (3, 6, 2), (32, 2, 1))], YUYV, (20, 0, 0, 6, 3, 32)),
    ("yuyv-offset", "yuv422", U8, 6, [(0, (3, 6, 2), (32, 2, 1))], YUYV, (20, 0, 6, 6, 3, 32)),
    ("uyvy-2x1", "yuv422", U8, 0, [(0, (1, 2, 2), (4, 2, 1))], UYVY, (21, 0, 0, 2, 1, 4)),
    ("uyvy-row", "yuv422", U8, 0, [(0, (1, 4, 2), (99, 2, 1))], UYVY, (21, 0, 0, 4, 1, 8)),
    ("uyvy-one-group-col", "yuv422", U8, 0, [(0, (4, 2, 2), (4, 2, 1))], UYVY, (21, 0, 0, 2, 4, 4)),
    ("uyvy-6x3", "yuv422", U8, 0, [(0, (3, 6, 2), (12, 2, 1))], UYVY, (21, 0, 0, 6, 3, 12)),
    ("uyvy-pitched", "yuv422", U8, 0, [(0, (3, 6, 2), (32, 2, 1))], UYVY, (21, 0, 0, 6, 3, 32)),
    ("uyvy-offset", "yuv422", U8, 6, [(0, (3, 6, 2), (32, 2, 1))], UYVY, (21, 0, 6, 6, 3, 32)),
    # ---- NV16: (H, W) + (H, cw, 2)
    ("nv16-1x1", "yuv422", U8, 0, [(0, (1, 1), (1, 1)), (2, (1, 1, 2), (2, 2, 1))], {}, (22, 2, 0, 1, 1, 2)),
    ("nv16-row", "yuv422", U8, 0, [(0, (1, 4), (4, 1)), (4, (1, 2, 2), (4, 2, 1))], {}, (22, 4, 0, 4, 1, 4)),
    ("nv16-row-odd", "yuv422", U8, 0, [(0, (1, 5), (9, 1)), (6, (1, 3, 2), (9, 2, 1))], {}, (22, 6, 0, 5, 1, 6)),
    ("nv16-col", "yuv422", U8, 0, [(0, (4, 1), (2, 1)), (8, (4, 1, 2), (2, 2, 1))], {}, (22, 8, 0, 1, 4, 2)),
    ("nv16-5x3", "yuv422", U8, 0, [(0, (3, 5), (6, 1)), (18, (3, 3, 2), (6, 2, 1))], {}, (22, 18, 0, 5, 3, 6)),
    ("nv16-pitched", "yuv422", U8, 0, [(0, (3, 5), (16, 1)), (48, (3, 3, 2), (16, 2, 1))], {}, (22, 48, 0, 5, 3, 16)),
    ("nv16-offset-spare-rows", "yuv422", U8, 5, [(0, (3, 5), (16, 1)), (64, (3, 3, 2), (16, 2, 1))], {},
     (22, 64, 5, 5, 3, 16)),
    # ---- I422: (H, W) + two (H, cw); Cb rows at (stride + 1) / 2, Cr H rows later
    ("i422-1x1", "yuv422", U8, 0, [(0, (1, 1), (1, 1)), (1, (1, 1), (1, 1)), (2, (1, 1), (1, 1))], {}, (23, 1, 0, 1, 1, 1)),
    ("i422-row", "yuv422", U8, 0, [(0, (1, 4), (4, 1)), (4, (1, 2), (2, 1)), (6, (1, 2), (2, 1))], {}, (23, 4, 0, 4, 1, 4)),
    ("i422-col", "yuv422", U8, 0, [(0, (4, 1), (1, 1)), (4, (4, 1), (1, 1)), (8, (4, 1), (1, 1))], {}, (23, 4, 0, 1, 4, 1)),
    ("i422-5x3", "yuv422", U8, 0, [(0, (3, 5), (5, 1)), (15, (3, 3), (3, 1)), (24, (3, 3), (3, 1))], {},
     (23, 15, 0, 5, 3, 5)),
    ("i422-pitched", "yuv422", U8, 0, [(0, (3, 5), (16, 1)), (48, (3, 3), (8, 1)), (72, (3, 3), (8, 1))], {},
     (23, 48, 0, 5, 3, 16)),
    ("i422-odd-pitch", "yuv422", U8, 0, [(0, (3, 5), (7, 1)), (21, (3, 3), (4, 1)), (33, (3, 3), (4, 1))], {},
     (23, 21, 0, 5, 3, 7)),
    ("i422-offset-spare-rows", "yuv422", U8, 5, [(0, (3, 5), (16, 1)), (64, (3, 3), (8, 1)), (88, (3, 3), (8, 1))], {},
     (23, 64, 5, 5, 3, 16)),
    # ---- P010: 16-bit (H, W) + (ch, 2 * cw); every figure expected is twice the elements'
    ("p010-1x1", "yuv10", I16, 0, [(0, (1, 1), (1, 1)), (2, (1, 2), (2, 1))], {}, (32, 4, 0, 1, 1, 4)),
    ("p010-row", "yuv10", I16, 0, [(0, (1, 4), (4, 1)), (4, (1, 4), (4, 1))], {}, (32, 8, 0, 4, 1, 8)),
    ("p010-row-odd", "yuv10", I16, 0, [(0, (1, 5), (9, 1)), (6, (1, 6), (9, 1))], {}, (32, 12, 0, 5, 1, 12)),
    ("p010-col", "yuv10", I16, 0, [(0, (4, 1), (2, 1)), (8, (2, 2), (2, 1))], {}, (32, 16, 0, 1, 4, 4)),
    ("p010-h2", "yuv10", I16, 0, [(0, (2, 4), (6, 1)), (12, (1, 4), (50, 1))], {}, (32, 24, 0, 4, 2, 12)),
    ("p010-5x3", "yuv10", I16, 0, [(0, (3, 5), (6, 1)), (18, (2, 6), (6, 1))], {}, (32, 36, 0, 5, 3, 12)),
    ("p010-pitched", "yuv10", I16, 0, [(0, (3, 5), (16, 1)), (48, (2, 6), (16, 1))], {}, (32, 96, 0, 5, 3, 32)),
    ("p010-offset-spare-rows", "yuv10", I16, 5, [(0, (3, 5), (16, 1)), (64, (2, 6), (16, 1))], {},
     (32, 128, 10, 5, 3, 32)),
    # ---- I010: 16-bit (H, W) + two (ch, cw); Cb rows at 2 * ceil(stride / 4) bytes, Cr ch rows later
    ("i010-1x1", "yuv10", I16, 0, [(0, (1, 1), (1, 1)), (1, (1, 1), (1, 1)), (2, (1, 1), (1, 1))], {}, (33, 2, 0, 1, 1, 2)),
    ("i010-row", "yuv10", I16, 0, [(0, (1, 4), (4, 1)), (4, (1, 2), (2, 1)), (6, (1, 2), (2, 1))], {}, (33, 8, 0, 4, 1, 8)),
    ("i010-col", "yuv10", I16, 0, [(0, (4, 1), (1, 1)), (4, (2, 1), (1, 1)), (6, (2, 1), (1, 1))], {}, (33, 8, 0, 1, 4, 2)),
    ("i010-h2", "yuv10", I16, 0, [(0, (2, 4), (4, 1)), (8, (1, 2), (50, 1)), (10, (1, 2), (60, 1))], {},
     (33, 16, 0, 4, 2, 8)),
    ("i010-5x3", "yuv10", I16, 0, [(0, (3, 5), (5, 1)), (15, (2, 3), (3, 1)), (21, (2, 3), (3, 1))], {},
     (33, 30, 0, 5, 3, 10)),
    ("i010-pitched", "yuv10", I16, 0, [(0, (3, 5), (16, 1)), (48, (2, 3), (8, 1)), (64, (2, 3), (8, 1))], {},
     (33, 96, 0, 5, 3, 32)),
    ("i010-odd-pitch", "yuv10", I16, 0, [(0, (3, 5), (7, 1)), (21, (2, 3), (4, 1)), (29, (2, 3), (4, 1))], {},
     (33, 42, 0, 5, 3, 14)),
    ("i010-offset-spare-rows", "yuv10", I16, 5, [(0, (3, 5), (16, 1)), (64, (2, 3), (8, 1)), (80, (2, 3), (8, 1))], {},
     (33, 128, 10, 5, 3, 32)),
    # ---- Y210: one 16-bit (H, 4 * cw); the width is 2 * cw
    ("y210-2x1", "yuv422p10", I16, 0, [(0, (1, 4), (4, 1))], {}, (40, 0, 0, 2, 1, 8)),
    ("y210-row", "yuv422p10", I16, 0, [(0, (1, 8), (77, 1))], {}, (40, 0, 0, 4, 1, 16)),
    ("y210-one-group-col", "yuv422p10", I16, 0, [(0, (4, 4), (4, 1))], {}, (40, 0, 0, 2, 4, 8)),
    ("y210-6x3", "yuv422p10", I16, 0, [(0, (3, 12), (12, 1))], {}, (40, 0, 0, 6, 3, 24)),
    ("y210-pitched", "yuv422p10", I16, 0, [(0, (3, 12), (20, 1))], {}, (40, 0, 0, 6, 3, 40)),
    ("y210-offset", "yuv422p10", I16, 3, [(0, (3, 12), (20, 1))], {}, (40, 0, 6, 6, 3, 40)),
    # ---- P210: 16-bit (H, W) + (H, 2 * cw)
    ("p210-1x1", "yuv422p10", I16, 0, [(0, (1, 1), (1, 1)), (2, (1, 2), (2, 1))], {}, (41, 4, 0, 1, 1, 4)),
    ("p210-row", "yuv422p10", I16, 0, [(0, (1, 4), (4, 1)), (4, (1, 4), (4, 1))], {}, (41, 8, 0, 4, 1, 8)),
    ("p210-row-odd", "yuv422p10", I16, 0, [(0, (1, 5), (9, 1)), (6, (1, 6), (9, 1))], {}, (41, 12, 0, 5, 1, 12)),
    ("p210-col", "yuv422p10", I16, 0, [(0, (4, 1), (2, 1)), (8, (4, 2), (2, 1))], {}, (41, 16, 0, 1, 4, 4)),
    ("p210-5x3", "yuv422p10", I16, 0, [(0, (3, 5), (6, 1)), (18, (3, 6), (6, 1))], {}, (41, 36, 0, 5, 3, 12)),
    ("p210-pitched", "yuv422p10", I16, 0, [(0, (3, 5), (16, 1)), (48, (3, 6), (16, 1))], {}, (41, 96, 0, 5, 3, 32)),
    ("p210-offset-spare-rows", "yuv422p10", I16, 5, [(0, (3, 5), (16, 1)), (64, (3, 6), (16, 1))], {},
     (41, 128, 10, 5, 3, 32)),
    # ---- I210: 16-bit (H, W) + two (H, cw); Cb rows at 2 * ceil(stride / 4) bytes, Cr H rows later
    ("i210-1x1", "yuv422p10", I16, 0, [(0, (1, 1), (1, 1)), (1, (1, 1), (1, 1)), (2, (1, 1), (1, 1))], {},
     (42, 2, 0, 1, 1, 2)),
    ("i210-row", "yuv422p10", I16, 0, [(0, (1, 4), (4, 1)), (4, (1, 2), (2, 1)), (6, (1, 2), (2, 1))], {},
     (42, 8, 0, 4, 1, 8)),
    ("i210-col", "yuv422p10", I16, 0, [(0, (4, 1), (1, 1)), (4, (4, 1), (1, 1)), (8, (4, 1), (1, 1))], {},
     (42, 8, 0, 1, 4, 2)),
    ("i210-5x3", "yuv422p10", I16, 0, [(0, (3, 5), (5, 1)), (15, (3, 3), (3, 1)), (24, (3, 3), (3, 1))], {},
     (42, 30, 0, 5, 3, 10)),
    ("i210-pitched", "yuv422p10", I16, 0, [(0, (3, 5), (16, 1)), (48, (3, 3), (8, 1)), (72, (3, 3), (8, 1))], {},
     (42, 96, 0, 5, 3, 32)),
    ("i210-odd-pitch", "yuv422p10", I16, 0, [(0, (3, 5), (7, 1)), (21, (3, 3), (4, 1)), (33, (3, 3), (4, 1))], {},
     (42, 42, 0, 5, 3, 14)),
    ("i210-offset-spare-rows", "yuv422p10", I16, 5, [(0, (3, 5), (16, 1)), (64, (3, 3), (8, 1)), (88, (3, 3), (8, 1))], {},
     (42, 128, 10, 5, 3, 32)),
    # ---- V210: rows of bytes or of 32-bit words, the width explicit
    ("v210-1x1", "v210", U8, 0, [(0, (1, 16), (16, 1))], {"width": 1}, (48, 0, 0, 1, 1, 16)),
    ("v210-row", "v210", U8, 0, [(0, (1, 32), (999, 1))], {"width": 7}, (48, 0, 0, 7, 1, 32)),
    ("v210-col", "v210", U8, 0, [(0, (4, 16), (16, 1))], {"width": 1}, (48, 0, 0, 1, 4, 16)),
    ("v210-5x3", "v210", U8, 0, [(0, (3, 16), (16, 1))], {"width": 5}, (48, 0, 0, 5, 3, 16)),
    ("v210-7x3", "v210", U8, 0, [(0, (3, 32), (32, 1))], {"width": 7}, (48, 0, 0, 7, 3, 32)),
    ("v210-pitched", "v210", U8, 0, [(0, (3, 40), (128, 1))], {"width": 7}, (48, 0, 0, 7, 3, 128)),
    ("v210-offset", "v210", U8, 8, [(0, (3, 40), (128, 1))], {"width": 7}, (48, 0, 8, 7, 3, 128)),
    ("v210-words", "v210", I32, 0, [(0, (3, 8), (8, 1))], {"width": 7}, (48, 0, 0, 7, 3, 32)),
    ("v210-words-offset", "v210", I32, 1, [(0, (3, 8), (12, 1))], {"width": 7}, (48, 0, 4, 7, 3, 48)),
    ("v210-widest", "v210", U8, 0, [(0, (1, 174768), (174768, 1))], {"width": 65535}, (48, 0, 0, 65535, 1, 174768)),
]

Y53 = (0, (3, 5), (16, 1))  # a 5x3 Y plane at pitch 16
REFUSED = [
    # ---- wrong element size or a float type
    ("rgb-int16", "rgb", I16, 0, [(0, (2, 5, 3), (15, 3, 1))], {}),
    ("rgb-float8", "rgb", F8, 0, [(0, (2, 5, 3), (15, 3, 1))], {}),
    ("gray-float32", "rgb", F32, 0, [(0, (3, 5), (5, 1))], {}),
    ("yuv-int16", "yuv", I16, 0, [Y53, (48, (2, 3, 2), (16, 2, 1))], {}),
    ("yuv-float8", "yuv", F8, 0, [Y53, (48, (2, 3, 2), (16, 2, 1))], {}),
    ("yuv10-uint8", "yuv10", U8, 0, [Y53, (48, (2, 6), (16, 1))], {}),
    ("yuv10-float16", "yuv10", F16, 0, [Y53, (48, (2, 6), (16, 1))], {}),
    ("yuv10-int32", "yuv10", I32, 0, [Y53, (48, (2, 6), (16, 1))], {}),
    ("yuv422-int16", "yuv422", I16, 0, [Y53, (48, (3, 3, 2), (16, 2, 1))], {}),
    ("yuv422-float8", "yuv422", F8, 0, [(0, (3, 6, 2), (12, 2, 1))], YUYV),
    ("yuv422p10-uint8", "yuv422p10", U8, 0, [(0, (3, 12), (12, 1))], {}),
    ("yuv422p10-float16", "yuv422p10", F16, 0, [Y53, (48, (3, 6), (16, 1))], {}),
    ("v210-int16", "v210", I16, 0, [(0, (3, 16), (16, 1))], {"width": 7}),
    ("v210-float32", "v210", F32, 0, [(0, (3, 8), (8, 1))], {"width": 7}),
    # ---- wrong rank
    ("rgb-rank1", "rgb", U8, 0, [(0, (15,), (1,))], {}),
    ("rgb-rank4", "rgb", U8, 0, [(0, (1, 3, 5, 3), (45, 15, 3, 1))], {}),
    ("yuv-y-rank1", "yuv", U8, 0, [(0, (5,), (1,)), (48, (2, 3, 2), (16, 2, 1))], {}),
    ("yuv-y-rank3", "yuv", U8, 0, [(0, (3, 5, 1), (16, 1, 1)), (48, (2, 3, 2), (16, 2, 1))], {}),
    ("yuv-chroma-rank1", "yuv", U8, 0, [Y53, (48, (12,), (1,))], {}),
    ("yuv10-y-rank3", "yuv10", I16, 0, [(0, (3, 5, 1), (16, 1, 1)), (48, (2, 6), (16, 1))], {}),
    ("yuv10-chroma-rank3", "yuv10", I16, 0, [Y53, (48, (2, 3, 2), (16, 2, 1))], {}),
    ("yuv422-rank1", "yuv422", U8, 0, [(0, (12,), (1,))], YUYV),
    ("yuv422-rank4", "yuv422", U8, 0, [(0, (1, 3, 6, 2), (36, 12, 2, 1))], YUYV),
    ("yuv422-packed-pairs-of-3", "yuv422", U8, 0, [(0, (3, 6, 3), (18, 3, 1))], YUYV),
    ("yuv422p10-rank3", "yuv422p10", I16, 0, [(0, (3, 3, 4), (12, 4, 1))], {}),
    ("yuv422p10-chroma-rank3", "yuv422p10", I16, 0, [Y53, (48, (3, 3, 2), (16, 2, 1))], {}),
    ("v210-rank1", "v210", U8, 0, [(0, (48,), (1,))], {"width": 7}),
    ("v210-rank3", "v210", U8, 0, [(0, (3, 8, 4), (32, 4, 1))], {"width": 7}),
    ("rgb-5-channels", "rgb", U8, 0, [(0, (2, 5, 5), (25, 5, 1))], {}),
    # ---- an empty tensor
    ("gray-no-rows", "rgb", U8, 0, [(0, (0, 5), (5, 1))], {}),
    ("gray-no-columns", "rgb", U8, 0, [(0, (5, 0), (1, 1))], {}),
    ("yuv-empty", "yuv", U8, 0, [(0, (0, 4), (4, 1)), (0, (0, 2, 2), (4, 2, 1))], {}),
    ("yuv-empty-i420", "yuv", U8, 0, [(0, (4, 0), (1, 1)), (0, (2, 0), (1, 1)), (0, (2, 0), (1, 1))], {}),
    ("yuv10-empty", "yuv10", I16, 0, [(0, (0, 4), (4, 1)), (0, (0, 4), (4, 1))], {}),
    ("yuv422-empty-packed", "yuv422", U8, 0, [(0, (0, 4, 2), (8, 2, 1))], YUYV),
    ("yuv422-empty-planar", "yuv422", U8, 0, [(0, (0, 4), (4, 1)), (0, (0, 2, 2), (4, 2, 1))], {}),
    ("yuv422p10-empty-packed", "yuv422p10", I16, 0, [(0, (0, 8), (8, 1))], {}),
    ("yuv422p10-empty-planar", "yuv422p10", I16, 0, [(0, (0, 4), (4, 1)), (0, (0, 4), (4, 1))], {}),
    ("v210-empty", "v210", U8, 0, [(0, (0, 32), (32, 1))], {"width": 7}),
    # ---- chroma of another family's shape
    ("yuv-nv16-chroma", "yuv", U8, 0, [Y53, (48, (3, 3, 2), (16, 2, 1))], {}),
    ("yuv-i422-chroma", "yuv", U8, 0, [Y53, (48, (3, 3), (8, 1)), (72, (3, 3), (8, 1))], {}),
    ("yuv-p010-chroma", "yuv", U8, 0, [Y53, (48, (2, 6), (16, 1))], {}),
    ("yuv-one-planar-chroma", "yuv", U8, 0, [Y53, (48, (2, 3), (8, 1))], {}),
    ("yuv-two-paired-chromas", "yuv", U8, 0, [Y53, (48, (2, 3, 2), (16, 2, 1)), (80, (2, 3, 2), (16, 2, 1))], {}),
    ("yuv10-p210-chroma", "yuv10", I16, 0, [Y53, (48, (3, 6), (16, 1))], {}),
    ("yuv10-i210-chroma", "yuv10", I16, 0, [Y53, (48, (3, 3), (8, 1)), (72, (3, 3), (8, 1))], {}),
    ("yuv10-444-chroma", "yuv10", I16, 0, [Y53, (48, (3, 5), (16, 1)), (96, (3, 5), (16, 1))], {}),
    ("yuv422-nv12-chroma", "yuv422", U8, 0, [Y53, (48, (2, 3, 2), (16, 2, 1))], {}),
    ("yuv422-i420-chroma", "yuv422", U8, 0, [Y53, (48, (2, 3), (8, 1)), (64, (2, 3), (8, 1))], {}),
    ("yuv422-444-chroma", "yuv422", U8, 0, [Y53, (48, (3, 5), (16, 1)), (96, (3, 5), (16, 1))], {}),
    ("yuv422-no-chroma", "yuv422", U8, 0, [Y53], {}),
    ("yuv422-cr-alone", "yuv422", U8, 0, [Y53, None, (48, (3, 3), (8, 1))], {}),
    ("yuv422p10-p010-chroma", "yuv422p10", I16, 0, [Y53, (48, (2, 6), (16, 1))], {}),
    ("yuv422p10-i010-chroma", "yuv422p10", I16, 0, [Y53, (48, (2, 3), (8, 1)), (64, (2, 3), (8, 1))], {}),
    ("yuv422p10-cr-alone", "yuv422p10", I16, 0, [(0, (3, 12), (12, 1)), None, (48, (3, 3), (8, 1))], {}),
    # ---- chroma before Y, or on it
    ("nv12-chroma-first", "yuv", U8, 32, [Y53, (-32, (2, 3, 2), (16, 2, 1))], {}),
    ("nv12-chroma-on-y", "yuv", U8, 0, [Y53, (0, (2, 3, 2), (16, 2, 1))], {}),
    ("i420-chroma-first", "yuv", U8, 32, [Y53, (-32, (2, 3), (8, 1)), (-16, (2, 3), (8, 1))], {}),
    ("yuv444-chroma-first", "yuv", U8, 96, [Y53, (-48, (3, 5), (16, 1)), (-96, (3, 5), (16, 1))], {}),
    ("nv16-chroma-first", "yuv422", U8, 48, [Y53, (-48, (3, 3, 2), (16, 2, 1))], {}),
    ("i422-chroma-first", "yuv422", U8, 48, [Y53, (-48, (3, 3), (8, 1)), (-24, (3, 3), (8, 1))], {}),
    ("p010-chroma-first", "yuv10", I16, 32, [Y53, (-32, (2, 6), (16, 1))], {}),
    ("i010-chroma-first", "yuv10", I16, 32, [Y53, (-32, (2, 3), (8, 1)), (-16, (2, 3), (8, 1))], {}),
    ("p210-chroma-first", "yuv422p10", I16, 48, [Y53, (-48, (3, 6), (16, 1))], {}),
    ("i210-chroma-first", "yuv422p10", I16, 48, [Y53, (-48, (3, 3), (8, 1)), (-24, (3, 3), (8, 1))], {}),
    # ---- chroma from another allocation
    ("nv12-two-allocations", "yuv", U8, 0, [Y53, (48, (2, 3, 2), (16, 2, 1), "own")], {}),
    ("i420-cr-elsewhere", "yuv", U8, 0, [Y53, (48, (2, 3), (8, 1)), (64, (2, 3), (8, 1), "own")], {}),
    ("yuv444-cb-elsewhere", "yuv", U8, 0, [(0, (3, 5), (8, 1)), (24, (3, 5), (8, 1), "own"), (48, (3, 5), (8, 1))], {}),
    ("nv16-two-allocations", "yuv422", U8, 0, [Y53, (48, (3, 3, 2), (16, 2, 1), "own")], {}),
    ("i422-cr-elsewhere", "yuv422", U8, 0, [Y53, (48, (3, 3), (8, 1)), (72, (3, 3), (8, 1), "own")], {}),
    ("p010-two-allocations", "yuv10", I16, 0, [Y53, (48, (2, 6), (16, 1), "own")], {}),
    ("i010-cb-elsewhere", "yuv10", I16, 0, [Y53, (48, (2, 3), (8, 1), "own"), (64, (2, 3), (8, 1))], {}),
    ("p210-two-allocations", "yuv422p10", I16, 0, [Y53, (48, (3, 6), (16, 1), "own")], {}),
    ("i210-cr-elsewhere", "yuv422p10", I16, 0, [Y53, (48, (3, 3), (8, 1)), (72, (3, 3), (8, 1), "own")], {}),
    # ---- inner stride 2
    ("rgb8-inner-stride", "rgb", U8, 0, [(0, (2, 5, 3), (32, 6, 2))], {}),
    ("rgb8-pixels-apart", "rgb", U8, 0, [(0, (2, 5, 3), (32, 4, 1))], {}),
    ("rgbp-inner-stride", "rgb", U8, 0, [(0, (3, 3, 5), (48, 16, 2))], {}),
    ("gray-inner-stride", "rgb", U8, 0, [(0, (3, 5), (16, 2))], {}),
    ("nv12-y-inner-stride", "yuv", U8, 0, [(0, (3, 5), (16, 2)), (48, (2, 3, 2), (16, 2, 1))], {}),
    ("i420-cb-inner-stride", "yuv", U8, 0, [Y53, (48, (2, 3), (8, 2)), (64, (2, 3), (8, 1))], {}),
    ("i420-cr-inner-stride", "yuv", U8, 0, [Y53, (48, (2, 3), (8, 1)), (64, (2, 3), (8, 2))], {}),
    ("yuv444-cr-inner-stride", "yuv", U8, 0, [Y53, (48, (3, 5), (16, 1)), (96, (3, 5), (16, 2))], {}),
    ("yuyv-inner-stride", "yuv422", U8, 0, [(0, (3, 6, 2), (32, 4, 2))], YUYV),
    ("yuyv-pixels-apart", "yuv422", U8, 0, [(0, (3, 6, 2), (32, 4, 1))], YUYV),
    ("nv16-y-inner-stride", "yuv422", U8, 0, [(0, (3, 5), (16, 2)), (48, (3, 3, 2), (16, 2, 1))], {}),
    ("i422-cb-inner-stride", "yuv422", U8, 0, [Y53, (48, (3, 3), (8, 2)), (72, (3, 3), (8, 1))], {}),
    ("p010-y-inner-stride", "yuv10", I16, 0, [(0, (3, 5), (16, 2)), (48, (2, 6), (16, 1))], {}),
    ("i010-cr-inner-stride", "yuv10", I16, 0, [Y53, (48, (2, 3), (8, 1)), (64, (2, 3), (8, 2))], {}),
    ("y210-inner-stride", "yuv422p10", I16, 0, [(0, (3, 12), (32, 2))], {}),
    ("p210-y-inner-stride", "yuv422p10", I16, 0, [(0, (3, 5), (16, 2)), (48, (3, 6), (16, 1))], {}),
    ("i210-cb-inner-stride", "yuv422p10", I16, 0, [Y53, (48, (3, 3), (8, 2)), (72, (3, 3), (8, 1))], {}),
    ("v210-inner-stride", "v210", U8, 0, [(0, (3, 32), (64, 2))], {"width": 7}),
    # ---- unpacked Cb,Cr pairs
    ("nv12-pairs-apart", "yuv", U8, 0, [(0, (3, 5), (32, 1)), (96, (2, 3, 2), (32, 4, 1))], {}),
    ("nv12-pair-split", "yuv", U8, 0, [(0, (3, 5), (32, 1)), (96, (2, 3, 2), (32, 4, 2))], {}),
    ("nv12-pair-split-one-column", "yuv", U8, 0, [(0, (4, 1), (4, 1)), (16, (2, 1, 2), (4, 2, 2))], {}),
    ("nv16-pairs-apart", "yuv422", U8, 0, [(0, (3, 5), (32, 1)), (96, (3, 3, 2), (32, 4, 1))], {}),
    ("nv16-pair-split", "yuv422", U8, 0, [(0, (3, 5), (32, 1)), (96, (3, 3, 2), (32, 4, 2))], {}),
    ("p010-words-apart", "yuv10", I16, 0, [(0, (3, 5), (32, 1)), (96, (2, 6), (32, 2))], {}),
    ("p210-words-apart", "yuv422p10", I16, 0, [(0, (3, 5), (32, 1)), (96, (3, 6), (32, 2))], {}),
    # ---- a semi-planar chroma pitch that is not the Y pitch
    ("nv12-chroma-pitch", "yuv", U8, 0, [Y53, (48, (2, 3, 2), (8, 2, 1))], {}),
    ("nv16-chroma-pitch", "yuv422", U8, 0, [Y53, (48, (3, 3, 2), (8, 2, 1))], {}),
    ("p010-chroma-pitch", "yuv10", I16, 0, [Y53, (48, (2, 6), (8, 1))], {}),
    ("p210-chroma-pitch", "yuv422p10", I16, 0, [Y53, (48, (3, 6), (20, 1))], {}),
    # ---- a three-plane chroma pitch that is not the rule's (Cr where that pitch would put it)
    ("i420-chroma-at-y-pitch", "yuv", U8, 0, [Y53, (48, (2, 3), (16, 1)), (80, (2, 3), (16, 1))], {}),
    ("i420-chroma-packed", "yuv", U8, 0, [Y53, (48, (2, 3), (3, 1)), (54, (2, 3), (3, 1))], {}),
    ("i420-cr-pitch", "yuv", U8, 0, [Y53, (48, (2, 3), (8, 1)), (64, (2, 3), (7, 1))], {}),
    ("i420-odd-pitch-rounded-down", "yuv", U8, 0, [(0, (3, 5), (7, 1)), (21, (2, 3), (3, 1)), (27, (2, 3), (3, 1))], {}),
    ("i422-chroma-at-y-pitch", "yuv422", U8, 0, [Y53, (48, (3, 3), (16, 1)), (96, (3, 3), (16, 1))], {}),
    ("i422-cr-pitch", "yuv422", U8, 0, [Y53, (48, (3, 3), (8, 1)), (72, (3, 3), (9, 1))], {}),
    ("i010-chroma-at-y-pitch", "yuv10", I16, 0, [Y53, (48, (2, 3), (16, 1)), (80, (2, 3), (16, 1))], {}),
    ("i010-odd-pitch-rounded-down", "yuv10", I16, 0, [(0, (3, 5), (7, 1)), (21, (2, 3), (3, 1)), (27, (2, 3), (3, 1))], {}),
    ("i210-chroma-at-y-pitch", "yuv422p10", I16, 0, [Y53, (48, (3, 3), (16, 1)), (96, (3, 3), (16, 1))], {}),
    ("i210-cb-pitch", "yuv422p10", I16, 0, [Y53, (48, (3, 3), (9, 1)), (72, (3, 3), (8, 1))], {}),
    # ---- Cr not `rows` rows after Cb
    ("i420-cr-a-byte-late", "yuv", U8, 0, [Y53, (48, (2, 3), (8, 1)), (65, (2, 3), (8, 1))], {}),
    ("i420-cr-h-rows-later", "yuv", U8, 0, [Y53, (48, (2, 3), (8, 1)), (72, (2, 3), (8, 1))], {}),
    ("i420-cr-first", "yuv", U8, 0, [Y53, (64, (2, 3), (8, 1)), (48, (2, 3), (8, 1))], {}),
    ("i420-h2-cr-packed", "yuv", U8, 0, [(0, (2, 4), (6, 1)), (12, (1, 2), (3, 1)), (14, (1, 2), (3, 1))], {}),
    ("i422-cr-ch-rows-later", "yuv422", U8, 0, [Y53, (48, (3, 3), (8, 1)), (64, (3, 3), (8, 1))], {}),
    ("i422-row-cr-packed", "yuv422", U8, 0, [(0, (1, 5), (5, 1)), (5, (1, 3), (3, 1)), (7, (1, 3), (3, 1))], {}),
    ("i010-cr-a-word-late", "yuv10", I16, 0, [Y53, (48, (2, 3), (8, 1)), (65, (2, 3), (8, 1))], {}),
    ("i210-cr-ch-rows-later", "yuv422p10", I16, 0, [Y53, (48, (3, 3), (8, 1)), (64, (3, 3), (8, 1))], {}),
    # ---- unequally spaced 4:4:4 planes, or planes at another pitch
    ("yuv444-unequal", "yuv", U8, 0, [Y53, (48, (3, 5), (16, 1)), (112, (3, 5), (16, 1))], {}),
    ("yuv444-cr-first", "yuv", U8, 0, [Y53, (96, (3, 5), (16, 1)), (48, (3, 5), (16, 1))], {}),
    ("yuv444-cb-pitch", "yuv", U8, 0, [Y53, (48, (3, 5), (8, 1)), (96, (3, 5), (16, 1))], {}),
    # ---- overlapping rows
    ("rgb8-overlap", "rgb", U8, 0, [(0, (2, 5, 3), (14, 3, 1))], {}),
    ("rgba8-overlap", "rgb", U8, 0, [(0, (2, 5, 4), (16, 4, 1))], {}),
    ("rgbp-overlap", "rgb", U8, 0, [(0, (3, 3, 5), (15, 4, 1))], {}),
    ("gray-overlap", "rgb", U8, 0, [(0, (3, 5), (4, 1))], {}),
    ("gray-one-row-repeated", "rgb", U8, 0, [(0, (3, 5), (0, 1))], {}),
    ("nv12-overlap", "yuv", U8, 0, [(0, (3, 5), (4, 1)), (12, (2, 3, 2), (4, 2, 1))], {}),
    ("nv12-odd-width-at-w", "yuv", U8, 0, [(0, (3, 5), (5, 1)), (15, (2, 3, 2), (5, 2, 1))], {}),
    ("i420-overlap", "yuv", U8, 0, [(0, (3, 5), (4, 1)), (12, (2, 3), (2, 1)), (16, (2, 3), (2, 1))], {}),
    ("yuv444-overlap", "yuv", U8, 0, [(0, (3, 5), (4, 1)), (12, (3, 5), (4, 1)), (24, (3, 5), (4, 1))], {}),
    ("yuyv-overlap", "yuv422", U8, 0, [(0, (3, 6, 2), (10, 2, 1))], YUYV),
    ("nv16-odd-width-at-w", "yuv422", U8, 0, [(0, (3, 5), (5, 1)), (15, (3, 3, 2), (5, 2, 1))], {}),
    ("i422-overlap", "yuv422", U8, 0, [(0, (3, 5), (4, 1)), (12, (3, 3), (2, 1)), (18, (3, 3), (2, 1))], {}),
    ("p010-odd-width-at-w", "yuv10", I16, 0, [(0, (3, 5), (5, 1)), (15, (2, 6), (5, 1))], {}),
    ("i010-overlap", "yuv10", I16, 0, [(0, (3, 5), (4, 1)), (12, (2, 3), (2, 1)), (16, (2, 3), (2, 1))], {}),
    ("y210-overlap", "yuv422p10", I16, 0, [(0, (3, 12), (10, 1))], {}),
    ("p210-odd-width-at-w", "yuv422p10", I16, 0, [(0, (3, 5), (5, 1)), (15, (3, 6), (5, 1))], {}),
    ("i210-overlap", "yuv422p10", I16, 0, [(0, (3, 5), (4, 1)), (12, (3, 3), (2, 1)), (18, (3, 3), (2, 1))], {}),
    ("v210-overlap", "v210", U8, 0, [(0, (3, 32), (16, 1))], {"width": 7}),
    # ---- keywords and shapes that do not say one layout
    ("rgb-ambiguous-3x3", "rgb", U8, 0, [(0, (3, 5, 3), (15, 3, 1))], {}),
    ("rgb-ambiguous-3x4", "rgb", U8, 0, [(0, (3, 5, 4), (20, 4, 1))], {}),
    ("rgb-chw-is-not", "rgb", U8, 0, [(0, (2, 5, 3), (15, 3, 1))], CHW),
    ("rgb-hwc-is-not", "rgb", U8, 0, [(0, (3, 3, 5), (15, 5, 1))], HWC),
    ("rgb-unknown-layout", "rgb", U8, 0, [(0, (2, 5, 3), (15, 3, 1))], {"layout": "nhwc"}),
    ("rgb-unknown-order", "rgb", U8, 0, [(0, (2, 5, 3), (15, 3, 1))], {"order": "grb"}),
    ("rgbp-bgr", "rgb", U8, 0, [(0, (3, 3, 5), (15, 5, 1))], BGR),
    ("yuyv-odd-width", "yuv422", U8, 0, [(0, (3, 5, 2), (10, 2, 1))], YUYV),
    ("yuyv-width-1", "yuv422", U8, 0, [(0, (1, 1, 2), (2, 2, 1))], UYVY),
    ("yuv422-packed-no-layout", "yuv422", U8, 0, [(0, (3, 6, 2), (12, 2, 1))], {}),
    ("yuv422-packed-unknown-layout", "yuv422", U8, 0, [(0, (3, 6, 2), (12, 2, 1))], {"layout": "yvyu"}),
    ("yuv422-packed-with-chroma", "yuv422", U8, 0, [(0, (3, 6, 2), (12, 2, 1)), (36, (3, 3, 2), (12, 2, 1))], YUYV),
    ("nv16-with-layout", "yuv422", U8, 0, [Y53, (48, (3, 3, 2), (16, 2, 1))], YUYV),
    ("i422-with-layout", "yuv422", U8, 0, [Y53, (48, (3, 3), (8, 1)), (72, (3, 3), (8, 1))], UYVY),
    ("y210-half-a-group", "yuv422p10", I16, 0, [(0, (3, 6), (6, 1))], {}),
    ("y210-one-word", "yuv422p10", I16, 0, [(0, (3, 1), (1, 1))], {}),
    # ---- V210: what the library would refuse
    ("v210-short-rows", "v210", U8, 0, [(0, (3, 16), (16, 1))], {"width": 7}),
    ("v210-short-rows-of-words", "v210", I32, 0, [(0, (3, 7), (8, 1))], {"width": 7}),
    ("v210-pitch-not-4n", "v210", U8, 0, [(0, (3, 32), (34, 1))], {"width": 7}),
    ("v210-base-not-4n", "v210", U8, 2, [(0, (3, 32), (32, 1))], {"width": 7}),
    ("v210-width-0", "v210", U8, 0, [(0, (3, 32), (32, 1))], {"width": 0}),
    ("v210-width-65536", "v210", U8, 0, [(0, (3, 32), (32, 1))], {"width": 65536}),
]


def ids(cases):
    return [c[0] for c in cases]


def test_case_ids_are_unique_and_every_layout_is_reached():
    names = ids(ACCEPTED) + ids(REFUSED)
    assert len(set(names)) == len(names)
    assert {c[6][0] for c in ACCEPTED} == {0, 1, 2, 3, 4, 8, 16, 17, 18, 20, 21, 22, 23, 32, 33, 40, 41, 42, 48}


@pytest.mark.parametrize("case", ACCEPTED, ids=ids(ACCEPTED))
def test_accepted(case):
    _, method, dtype, off, specs, kw, want = case
    fmt, plane_stride, ptr, w, h, stride = want
    maxval = 200 if method == "rgb" else 255
    enc = Recorder()
    got = run(enc, method, dtype, off, specs, kw)
    # out=None: the bytes come back, from a host buffer of the library's bound, with no output flag
    assert type(got) is bytes and len(got) == 7
    assert enc.calls == [(fmt, plane_stride, ptr, w, h, stride, J.max_jpeg_bytes(w, h), 77, maxval, 0)]
    assert enc.input_format() == IDLE and enc._fmt == IDLE[0]
    # a device `out`: its address and size, the output flag, and the length comes back
    enc = Recorder()
    assert run(enc, method, dtype, off, specs, kw, out=DeviceOut()) == 7
    assert enc.calls == [(fmt, plane_stride, ptr, w, h, stride, 555, 77, maxval, J.JPGE_DEVICE_OUTPUT)]
    assert enc.input_format() == IDLE
    # a failing encode_ptr: the error passes through, the input format is put back
    enc = Recorder(fail=True)
    with pytest.raises(RuntimeError, match="encode_ptr failed"):
        run(enc, method, dtype, off, specs, kw)
    assert enc.calls == [(fmt, plane_stride, ptr, w, h, stride, J.max_jpeg_bytes(w, h), 77, maxval, 0)]
    assert enc.input_format() == IDLE and enc._fmt == IDLE[0]


@pytest.mark.parametrize("case", REFUSED, ids=ids(REFUSED))
def test_refused(case):
    _, method, dtype, off, specs, kw = case
    enc = Recorder()
    with pytest.raises(ValueError):
        run(enc, method, dtype, off, specs, kw)
    assert enc.calls == [] and enc.input_format() == IDLE and enc._fmt == IDLE[0]


@pytest.mark.parametrize("shape, strides, want", [((0, 5, 3), (15, 3, 1), (0, 0, 5, 0, 15)),
                                                  ((3, 4, 0), (4, 1, 1), (4, 4, 0, 4, 1))])
def test_empty_colour_tensor_is_left_to_the_library(shape, strides, want):
    """Every other entry refuses an empty tensor itself; encode_tensor refuses an empty gray plane,
    but hands an empty colour tensor on with a width or height of 0 (and torch's null pointer),
    which jpge_encode_rgb8 refuses with JPGE_E_ARG."""
    enc = Recorder()
    run(enc, "rgb", U8, 0, [(0, shape, strides)], {})
    assert [c[:2] + c[3:6] for c in enc.calls] == [want] and enc.input_format() == IDLE


BAD_OUT = [torch.zeros(4096, dtype=U8), torch.zeros(4096, dtype=I16), torch.zeros(64, 64, dtype=U8)[:, :32]]


@pytest.mark.parametrize("bad", range(len(BAD_OUT)))
@pytest.mark.parametrize("case", [c for c in ACCEPTED if c[0].endswith("-5x3") or c[0].endswith("-6x3")],
                         ids=lambda c: c[0])
def test_out_that_is_no_contiguous_uint8_device_tensor(case, bad):
    _, method, dtype, off, specs, kw, _ = case
    enc = Recorder()
    with pytest.raises(ValueError, match="out"):
        run(enc, method, dtype, off, specs, kw, out=BAD_OUT[bad])
    assert enc.calls == [] and enc.input_format() == IDLE
