#!/usr/bin/env python3
"""K1 (the transform kernel) per input layout: 3840x2160 4:2:0 Q90 from device input on a
1-lane Encoder with per-kernel events (set_timing(1)), over D distinct frames per layout
whose bytes together exceed the 256 MB MALL (as bench.py's 4K workload does), the
layouts taken in turn within each pass so that drift hits them alike.

Reports, per layout, the median `fdct` kernel time and its ratio to RGB8 in the same run,
and, for the caller's alternative, a plain torch repack to interleaved RGB
(`permute(1, 2, 0).contiguous()`, `[..., :3].contiguous()`, `flip(-1)`) timed with device
events: "repack + RGB8 K1" against the layout's own K1.  Every layout's first output is
compared with the RGB8 bytes.  Prints one JSON line; --out also writes it to a file.

    python tools/measure_formats.py --out profiles/formats_k1.json
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

NAMES = {J.JPGE_FMT_RGB8: "rgb8", J.JPGE_FMT_BGR8: "bgr8", J.JPGE_FMT_RGBA8: "rgba8", J.JPGE_FMT_BGRA8: "bgra8",
         J.JPGE_FMT_RGB8_PLANAR: "rgb8_planar"}


def to_layout(rgb, fmt):
    """Device (H, W, 3) RGB tensor -> the layout's tensor (alpha: random bytes)."""
    if fmt == J.JPGE_FMT_RGB8:
        return rgb.clone()
    if fmt == J.JPGE_FMT_BGR8:
        return rgb.flip(-1).contiguous()
    if fmt == J.JPGE_FMT_RGB8_PLANAR:
        return rgb.permute(2, 0, 1).contiguous()
    c = rgb if fmt == J.JPGE_FMT_RGBA8 else rgb.flip(-1)
    a = torch.randint(0, 256, rgb.shape[:2] + (1,), dtype=torch.uint8, device=rgb.device)
    return torch.cat([c, a], dim=2).contiguous()


def repack(t, fmt):
    """What a caller without the layout support runs first: the frame as interleaved RGB."""
    if fmt == J.JPGE_FMT_BGR8:
        return t.flip(-1).contiguous()
    if fmt == J.JPGE_FMT_RGBA8:
        return t[..., :3].contiguous()
    if fmt == J.JPGE_FMT_BGRA8:
        return t[..., :3].flip(-1).contiguous()
    if fmt == J.JPGE_FMT_RGB8_PLANAR:
        return t.permute(1, 2, 0).contiguous()
    return t


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--distinct", type=int, default=16, help="distinct frames per layout (16 x 24.9 MB > the MALL)")
    ap.add_argument("--passes", type=int, default=6, help="timed passes over every layout's frames")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("measure_formats: no GPU (a measurement does not fall back)")
    W, H, D = args.width, args.height, args.distinct
    fmts = list(NAMES)
    rgb = [torch.from_numpy(J.synth_rgb8(3 + i, W, H)).cuda() for i in range(D)]
    frames = {f: [to_layout(r, f) for r in rgb] for f in fmts}
    del rgb
    cap = J.max_jpeg_bytes(W, H)
    out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    times = {f: [] for f in fmts}
    first = {}
    with J.Encoder(0, lanes=1) as enc:
        enc.set_timing(1)
        for p in range(args.warmup + args.passes):
            for i in range(D):
                for f in fmts:  # the layouts in turn
                    t = frames[f][i]
                    n = enc.encode_tensor(t, quality=args.quality, out=out,
                                          order="bgr" if f in (J.JPGE_FMT_BGR8, J.JPGE_FMT_BGRA8) else "rgb")
                    if p == 0 and i == 0:
                        torch.cuda.synchronize()
                        first[f] = out[:n].cpu().numpy().tobytes()
                    if p >= args.warmup:
                        times[f].append(enc.timing()["fdct"])
    same = all(first[f] == first[J.JPGE_FMT_RGB8] for f in fmts)
    # the repack a caller would run instead, device events around each call
    rep = {f: [] for f in fmts if f != J.JPGE_FMT_RGB8}
    for p in range(args.warmup + args.passes):
        for i in range(D):
            for f in rep:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r = repack(frames[f][i], f)
                e1.record()
                e1.synchronize()
                del r
                if p >= args.warmup:
                    rep[f].append(e0.elapsed_time(e1))
    med = {f: statistics.median(times[f]) for f in fmts}
    base = med[J.JPGE_FMT_RGB8]
    res = {"what": "K1 (fdct) kernel time per input layout, 1-lane encoder, device input, kernel events",
           "width": W, "height": H, "quality": args.quality, "subsampling": 420, "distinct_inputs": D,
           "passes": args.passes, "samples_per_layout": len(times[J.JPGE_FMT_RGB8]),
           "outputs_equal_rgb8": same, "device": torch.cuda.get_device_name(0), "layouts": {}}
    for f in fmts:
        bpp, planes = J.input_format_info(f)
        q = statistics.quantiles(times[f], n=10)
        e = {"input_mb": round(W * H * bpp * planes / 1e6, 1), "fdct_ms_median": round(med[f], 5),
             "fdct_ms_p10": round(q[0], 5), "fdct_ms_p90": round(q[-1], 5), "ratio_to_rgb8": round(med[f] / base, 4)}
        if f in rep:
            r = statistics.median(rep[f])
            e["torch_repack_ms_median"] = round(r, 5)
            e["repack_plus_rgb8_fdct_ms"] = round(r + base, 5)
            e["direct_over_repack_path"] = round(med[f] / (r + base), 4)
        res["layouts"][NAMES[f]] = e
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
