"""Single-frame calls, the stripe phases and encode_planes all run on lane 0's first slot
of a context, and the plane stages share its scratch buffers.  Whatever a call finds
there from the call before must not show: every output here is byte-exact against the
same call on a fresh context (the stripes also against the oracle).  Also the stage
entries' device-buffer branches (jpge.h JPGE_DEVICE_INPUT / JPGE_DEVICE_OUTPUT), which
the Python methods never take, and a slot's workspace growing and being reused."""
import ctypes

import numpy as np
import pytest

import _oracle
import _yuv
import jpgenc_amd as J
from jpgenc_amd import stripes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV_IN, DEV_OUT = J.JPGE_DEVICE_INPUT, J.JPGE_DEVICE_OUTPUT


def _padded_planes(rgb):
    """loadPPM's planes (Image.cpp:393-531): edge-replicated to whole 16x16 MCUs."""
    h, w = rgb.shape[:2]
    ys = np.minimum(np.arange((h + 15) // 16 * 16), h - 1)
    xs = np.minimum(np.arange((w + 15) // 16 * 16), w - 1)
    p = rgb[ys][:, xs].astype(np.float64)
    return [np.ascontiguousarray(p[..., c]) for c in range(3)]


def _planes_call(w, h, quality=90):
    rgb = J.synth_rgb8(w + h, w, h)
    planes = _padded_planes(rgb)
    return lambda enc: enc.encode_planes(*planes, w, h, J.JPGE_TO_RGB, quality)


def _encode_call(w, h, quality=90):
    rgb = J.synth_rgb8(w * 3 + h, w, h)
    return lambda enc: enc.encode(rgb, quality)


def _nv12_call(w, h, quality=75):
    frame = _yuv.build(J.JPGE_FMT_NV12, *_yuv.samples(J.JPGE_FMT_NV12, 5, w, h))

    def call(enc):
        enc.set_input_format(J.JPGE_FMT_NV12)
        try:
            return enc.encode(frame, quality)
        finally:
            enc.set_input_format(J.JPGE_FMT_RGB8)
    return call


def _two_stripes_call(w, h, quality=90):
    """Both stripes of a two-stripe encode on ONE context.  The phases keep one stripe's
    state at a time, so a stripe is transformed (and counted) again before its code and
    pack phases: the exchanges of jpgenc_amd.stripes.encode_stripes_local, in sequence."""
    rgb = J.synth_rgb8(21, w, h)
    rows = stripes.stripe_rows((h + 15) // 16, 2)
    stride = w * 3

    def call(enc):
        dev = torch.from_numpy(rgb.reshape(-1)).cuda()
        out = torch.zeros(J.max_jpeg_bytes(w, h), dtype=torch.uint8, device="cuda")

        def counted(r, seed):
            last = enc.stripe_transform(dev.data_ptr() + rows[r][0] * 16 * stride, stride, w, h, rows[r][0], rows[r][1],
                                        quality)
            return last, enc.stripe_stats(seed)

        zero = np.zeros(3, np.int32)
        last0, st0 = counted(0, zero)
        _, st1 = counted(1, last0)
        counts, first = stripes.combine_stats([st0[0], st1[0]], [st0[1], st1[1]])
        sum1, _ = enc.stripe_code(counts, first)   # (stripe 1 is the one in place)
        counted(0, zero)
        sum0, _ = enc.stripe_code(counts, first)
        enc.stripe_pack([sum0, sum1], 0, out.data_ptr(), out.numel())
        counted(1, last0)
        assert enc.stripe_code(counts, first)[0] == sum1
        total = enc.stripe_pack([sum0, sum1], 1, out.data_ptr(), out.numel())[2]
        torch.cuda.synchronize()
        return out[:total].cpu().numpy().tobytes()
    call.oracle = _oracle.encode(rgb, quality)
    return call


def _fresh(lanes, call):
    with J.Encoder(0, lanes=lanes) as enc:
        return call(enc)


@pytest.mark.parametrize("lanes", [1, 0])
def test_mixed_paths_on_one_context(lanes):
    enc_a, planes, striped = _encode_call(64, 48), _planes_call(26, 19), _two_stripes_call(48, 64)
    nv12 = _nv12_call(34, 20)
    want = {k: _fresh(lanes, c) for k, c in (("encode", enc_a), ("planes", planes), ("stripes", striped), ("nv12", nv12))}
    with J.Encoder(0, lanes=lanes) as fresh:
        fresh.set_huffman(J.JPGE_HUFF_STANDARD)
        want["fixed"] = enc_a(fresh)
    assert want["stripes"] == striped.oracle
    with J.Encoder(0, lanes=lanes) as enc:
        enc.set_timing(1)
        assert enc_a(enc) == want["encode"]                      # 1
        assert planes(enc) == want["planes"]                     # 2
        assert striped(enc) == want["stripes"]                   # 3
        enc.set_huffman(J.JPGE_HUFF_STANDARD)
        assert enc_a(enc) == want["fixed"]                       # 4
        with pytest.raises(J.JpgeError) as refused:              # 5
            planes(enc)
        assert refused.value.status == 1  # JPGE_E_ARG
        enc.set_huffman(J.JPGE_HUFF_OPTIMAL)
        assert planes(enc) == want["planes"]                     # 6
        assert nv12(enc) == want["nv12"]                         # 7
        assert planes(enc) == want["planes"]                     # 8
        assert enc.timing()["frames"] == 3  # (the encode calls: 1, 4 and 7)


def test_growth_then_reuse():
    small, large = _encode_call(17, 9), _encode_call(200, 136)
    p_small, p_large = _planes_call(16, 16), _planes_call(64, 48)
    want = [_fresh(0, c) for c in (small, large, p_small, p_large)]
    with J.Encoder(0) as enc:
        assert [small(enc), large(enc), small(enc)] == [want[0], want[1], want[0]]
        assert [p_small(enc), p_large(enc), p_small(enc)] == [want[2], want[3], want[2]]


# ---- the stage entries on device buffers ----
def _stage(name, enc, ins, outs, args, flags):
    """One stage entry through the C ABI: ins / outs are numpy arrays; with a device flag
    the call gets torch device copies of them instead, and device outputs are read back."""
    din = [torch.from_numpy(a).cuda() for a in ins] if flags & DEV_IN else None
    dout = [torch.from_numpy(np.zeros_like(a)).cuda() for a in outs] if flags & DEV_OUT else None
    host = [np.zeros_like(a) for a in outs]
    pi = [t.data_ptr() for t in din] if din else [J._p(a) for a in ins]
    po = [t.data_ptr() for t in dout] if dout else [J._p(a) for a in host]
    torch.cuda.synchronize()
    J._check(args(J.lib(), enc.ctx, pi, po, flags), name)
    return [t.cpu().numpy() for t in dout] if dout else host


@pytest.mark.parametrize("flags", [0, DEV_IN, DEV_OUT, DEV_IN | DEV_OUT])
@pytest.mark.parametrize("shape", [(16, 16), (48, 64)])
def test_stage_entries_on_device_buffers(encoder, shape, flags):
    h, w = shape
    rng = np.random.default_rng(h * w)
    p = [rng.normal(100, 80, shape) for _ in range(3)]
    u32 = ctypes.c_uint32
    qy = J.quality_tables(75)[0]
    # (name, inputs, an array shaped like each output, the call, the flags-0 result)
    cases = [
        ("color_convert", p, p,
         lambda L, c, i, o, f: L.jpge_color_convert(c, *i, *o, h * w, J.JPGE_TO_YCBCR, f),
         encoder.color_convert(*p, J.JPGE_TO_YCBCR)),
        ("subsample_plane 420", p[:1], [np.zeros((h // 2, w // 2))],
         lambda L, c, i, o, f: L.jpge_subsample_plane(c, i[0], h, w, 420, o[0], ctypes.byref(u32()), ctypes.byref(u32()), f),
         [encoder.subsample_plane(p[0], 420)]),
        ("subsample_plane 444", p[:1], p[:1],
         lambda L, c, i, o, f: L.jpge_subsample_plane(c, i[0], h, w, 444, o[0], ctypes.byref(u32()), ctypes.byref(u32()), f),
         [encoder.subsample_plane(p[0], 444)]),
        ("dct_plane", p[:1], p[:1],
         lambda L, c, i, o, f: L.jpge_dct_plane(c, i[0], h, w, J.DCT_ARAI, o[0], f),
         [encoder.dct_plane(p[0], J.DCT_ARAI)]),
        ("quantize_plane", p[:1], [np.zeros(shape, np.int32)],
         lambda L, c, i, o, f: L.jpge_quantize_plane(c, i[0], h, w, J._p(qy), o[0], f),
         [encoder.quantize_plane(p[0], qy)]),
    ]
    for name, ins, like, call, want in cases:
        got = _stage(name, encoder, ins, like, call, flags)
        assert len(got) == len(want)
        for g, x in zip(got, want):
            assert g.dtype == x.dtype and g.tobytes() == x.tobytes(), name
