#!/usr/bin/env python3
"""K1 (the transform kernel) for the 4:2:2 input layouts (YUYV, UYVY, NV16, I422) in JPGE_S422,
next to YUV444_PLANAR and RGB8 in the same mode and NV12 in its own (4:2:0), by the method of
tools/measure_formats_yuv.py: 3840x2160 Q90 from device input on a 1-lane Encoder with
per-kernel events (set_timing(1)), D distinct frames per layout, the layouts taken in turn
within each pass so that drift hits them alike.

The frames are the RGB frames' own Y, Cb, Cr (rounded to 8 bits; 4:2:2 chroma: the even
column's sample of each pair, which YUV444_PLANAR repeats, so that those five layouts hold the
same picture and must give the same bytes: checked).  Reports, per layout, the median `fdct`
kernel time, its 10th and 90th percentiles (the spread the comparison's margin is) and its
ratio to YUV444_PLANAR in the same run.  Prints one JSON line; --out also writes it to a file.

    python tools/measure_formats_422.py --out profiles/formats_422_k1.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before libjpge: one HIP runtime per process)

import jpgenc_amd as J  # noqa: E402
from tools.measure_formats_yuv import half, ycc  # noqa: E402

NAMES = {J.JPGE_FMT_YUYV: "yuyv", J.JPGE_FMT_UYVY: "uyvy", J.JPGE_FMT_NV16: "nv16", J.JPGE_FMT_I422: "i422",
         J.JPGE_FMT_YUV444_PLANAR: "yuv444_planar", J.JPGE_FMT_RGB8: "rgb8", J.JPGE_FMT_NV12: "nv12"}
MODE = {f: 422 for f in NAMES}
MODE[J.JPGE_FMT_NV12] = 420
SAME = (J.JPGE_FMT_YUYV, J.JPGE_FMT_UYVY, J.JPGE_FMT_NV16, J.JPGE_FMT_I422, J.JPGE_FMT_YUV444_PLANAR)


def to_layout(rgb, fmt):
    """Device RGB frame -> (tensors, keyword arguments) of the encode_tensor* call for layout
    fmt: views of one allocation each."""
    if fmt == J.JPGE_FMT_RGB8:
        return (rgb.clone(),), {}
    y, cb, cr = ycc(rgb)
    h, w = y.shape
    if fmt == J.JPGE_FMT_NV12:
        cb, cr = half(cb), half(cr)
        t = torch.cat([y, torch.stack([cb, cr], dim=2).view(h // 2, w)]).contiguous()  # (H + H/2, W)
        return (t[:h], t[h:].view(h // 2, w // 2, 2)), {}
    cb, cr = cb[:, ::2].contiguous(), cr[:, ::2].contiguous()  # the kept sample of each pair
    if fmt == J.JPGE_FMT_YUV444_PLANAR:
        t = torch.stack([y, cb.repeat_interleave(2, dim=1), cr.repeat_interleave(2, dim=1)]).contiguous()
        return (t[0], t[1], t[2]), {}
    if fmt in (J.JPGE_FMT_YUYV, J.JPGE_FMT_UYVY):
        c = torch.stack([cb, cr], dim=2).view(h, w)  # Cb Cr Cb Cr ...: pixel x's chroma byte
        pair = (y, c) if fmt == J.JPGE_FMT_YUYV else (c, y)
        return (torch.stack(pair, dim=2).contiguous(),), {"layout": NAMES[fmt]}
    if fmt == J.JPGE_FMT_NV16:
        t = torch.cat([y, torch.stack([cb, cr], dim=2).view(h, w)]).contiguous()  # (2 H, W)
        return (t[:h], t[h:].view(h, w // 2, 2)), {}
    t = torch.cat([y.reshape(-1), cb.reshape(-1), cr.reshape(-1)]).contiguous()
    n, c = w * h, (w // 2) * h
    return (t[:n].view(h, w), t[n:n + c].view(h, w // 2), t[n + c:].view(h, w // 2)), {}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--distinct", type=int, default=16, help="distinct frames per layout")
    ap.add_argument("--passes", type=int, default=6, help="timed passes over every layout's frames")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kind", type=int, default=0, choices=[0, 1, 2], help="synth_rgb8 picture (measure_formats_yuv.py)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("measure_formats_422: no GPU (a measurement does not fall back)")
    W, H, D = args.width, args.height, args.distinct
    if W % 32 or H % 2:
        sys.exit("measure_formats_422: a width that is a multiple of 32 and an even height (the fast path of every layout)")
    fmts = list(NAMES)
    rgb = [torch.from_numpy(J.synth_rgb8(3 + i, W, H, kind=args.kind)).cuda() for i in range(D)]
    frames = {f: [to_layout(r, f) for r in rgb] for f in fmts}
    del rgb
    out = torch.zeros(J.max_jpeg_bytes(W, H), dtype=torch.uint8, device="cuda")
    times = {f: [] for f in fmts}
    first = {}
    with J.Encoder(0, lanes=1) as enc:
        enc.set_timing(1)
        for p in range(args.warmup + args.passes):
            for i in range(D):
                for f in fmts:  # the layouts in turn
                    t, kw = frames[f][i]
                    enc.set_subsampling(MODE[f])
                    if f == J.JPGE_FMT_RGB8:
                        n = enc.encode_tensor(t[0], quality=args.quality, out=out)
                    elif f in (J.JPGE_FMT_NV12, J.JPGE_FMT_YUV444_PLANAR):
                        n = enc.encode_tensor_yuv(*t, quality=args.quality, out=out)
                    else:
                        n = enc.encode_tensor_yuv422(*t, quality=args.quality, out=out, **kw)
                    if p == 0 and i == 0:
                        torch.cuda.synchronize()
                        first[f] = out[:n].cpu().numpy().tobytes()
                    if p >= args.warmup:
                        times[f].append(enc.timing()["fdct"])
    same = all(first[f] == first[J.JPGE_FMT_YUV444_PLANAR] for f in SAME)
    med = {f: statistics.median(times[f]) for f in fmts}
    base = med[J.JPGE_FMT_YUV444_PLANAR]
    res = {"what": "K1 (fdct) kernel time per input layout, 1-lane encoder, device input, kernel events",
           "width": W, "height": H, "quality": args.quality, "picture_kind": args.kind, "distinct_inputs": D,
           "passes": args.passes, "samples_per_layout": len(times[J.JPGE_FMT_YUV444_PLANAR]),
           "422_layouts_bytes_equal_repeated_444": same, "device": torch.cuda.get_device_name(0), "layouts": {}}
    for f in fmts:
        q = statistics.quantiles(times[f], n=10)
        mb = sum(t.numel() for t in frames[f][0][0]) / 1e6
        res["layouts"][NAMES[f]] = {"subsampling": MODE[f], "input_mb": round(mb, 1), "fdct_ms_median": round(med[f], 5),
                                    "fdct_ms_p10": round(q[0], 5), "fdct_ms_p90": round(q[-1], 5),
                                    "fdct_ms_min": round(min(times[f]), 5), "fdct_ms_max": round(max(times[f]), 5),
                                    "ratio_to_yuv444_planar": round(med[f] / base, 4),
                                    "jpg_bytes_first_frame": len(first[f])}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
