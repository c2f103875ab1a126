#!/usr/bin/env python3
"""The one-component layout (JPGE_FMT_GRAY8) next to the workaround it replaces and to the
RGB8 headline shape, by the method of tools/measure_formats_yuv.py: 3840x2160 Q90 from
device input on a 1-lane Encoder with per-kernel events (set_timing(1)), D distinct frames
per input, the inputs taken in turn within each pass so that drift hits them alike.

Three inputs of the same pictures (the photo-like frames' green channel as luminance):
  gray8            the (H, W) plane, one-component stream;
  yuv444_flat      YUV444_PLANAR at S444 with Cb = Cr = 128: the three-component workaround;
  rgb8_420         the RGB frame itself at 4:2:0 (the benchmark's shape).
Reports, per input, the median K1 (fdct), K2 (dc_stats) and entropy-stage (code + pack)
kernel times and the median wall time of the whole call (device input, device output), with
the 10th and 90th percentiles, and the ratio gray8 / yuv444_flat of each.  The gray file's
coefficients must equal the workaround's Y plane; that is checked on the first frame.
Prints one JSON line; --out also writes it to a file.

    python tools/measure_formats_gray.py --out profiles/formats_gray.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before libjpge: one HIP runtime per process)

import jpgenc_amd as J  # noqa: E402

INPUTS = ("gray8", "yuv444_flat", "rgb8_420")
STAGES = ("fdct", "dc_stats", "entropy")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--distinct", type=int, default=8, help="distinct frames per input")
    ap.add_argument("--passes", type=int, default=6, help="timed passes over every input's frames")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("measure_formats_gray: no GPU (a measurement does not fall back)")
    W, H, D = args.width, args.height, args.distinct
    if W % 16:
        sys.exit("measure_formats_gray: a width that is a multiple of 16 (the fast path of every input)")
    frames = {k: [] for k in INPUTS}
    for i in range(D):
        rgb = torch.from_numpy(J.synth_rgb8(3 + i, W, H)).cuda()
        y = rgb[:, :, 1].contiguous()
        frames["gray8"].append(y)
        frames["yuv444_flat"].append(torch.stack([y, torch.full_like(y, 128), torch.full_like(y, 128)]).contiguous())
        frames["rgb8_420"].append(rgb)
    out = torch.zeros(J.max_jpeg_bytes(W, H), dtype=torch.uint8, device="cuda")
    times = {k: {s: [] for s in STAGES + ("call",)} for k in INPUTS}
    first = {}
    with J.Encoder(0, lanes=1) as enc:
        enc.set_timing(1)

        def encode(k, t):
            if k == "gray8":
                return enc.encode_tensor(t, quality=args.quality, out=out)
            if k == "rgb8_420":
                enc.set_subsampling(420)
                return enc.encode_tensor(t, quality=args.quality, out=out)
            enc.set_subsampling(444)
            return enc.encode_tensor_yuv(t[0], t[1], t[2], quality=args.quality, out=out)

        for p in range(args.warmup + args.passes):
            for i in range(D):
                for k in INPUTS:  # the inputs in turn
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    n = encode(k, frames[k][i])
                    torch.cuda.synchronize()
                    dt = (time.perf_counter() - t0) * 1e3
                    if p == 0 and i == 0:
                        first[k] = out[:n].cpu().numpy().tobytes()
                    if p >= args.warmup:
                        tm = enc.timing()
                        for s in STAGES:
                            times[k][s].append(tm[s])
                        times[k]["call"].append(dt)
    gi, gy, _, _ = J.decode_coeffs(first["gray8"])
    fi, fy, fcb, fcr = J.decode_coeffs(first["yuv444_flat"])
    same = gi.c_blocks == 0 and np.array_equal(gy, fy) and not fcb.any() and not fcr.any()

    def summary(v):
        q = statistics.quantiles(v, n=10)
        return {"median": round(statistics.median(v), 5), "p10": round(q[0], 5), "p90": round(q[-1], 5)}

    res = {"what": "kernel times (events) and whole-call wall time per 4K frame, 1-lane encoder, device input and "
                   "output; ms", "width": W, "height": H, "quality": args.quality, "distinct_inputs": D,
           "passes": args.passes, "samples_per_input": len(times["gray8"]["call"]),
           "gray_y_equals_workaround_y": bool(same), "device": torch.cuda.get_device_name(0), "inputs": {}}
    for k in INPUTS:
        res["inputs"][k] = {s + "_ms": summary(times[k][s]) for s in STAGES + ("call",)}
        res["inputs"][k]["input_mb"] = round(frames[k][0].numel() / 1e6, 1)
        res["inputs"][k]["jpg_bytes_first_frame"] = len(first[k])
    res["ratio_gray_to_workaround"] = {
        s: round(statistics.median(times["gray8"][s]) / statistics.median(times["yuv444_flat"][s]), 4)
        for s in STAGES + ("call",)}
    res["ratio_gray_to_rgb8_420"] = {
        s: round(statistics.median(times["gray8"][s]) / statistics.median(times["rgb8_420"][s]), 4)
        for s in STAGES + ("call",)}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
