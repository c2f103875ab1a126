#!/usr/bin/env python3
"""K1 (the transform kernel) for v210 frames next to Y210 frames of the same samples and next to
the caller's workaround, by the method of tools/measure_formats_422p10.py: 3840x2160 Q90 from
device input on a 1-lane Encoder with per-kernel events (set_timing(1)), D distinct photo-like
frames taken in turn, the settings interleaved within each pass so that drift hits them alike.

Settings: v210 and Y210, each in subsampling mode 422 and 420, under FULL_601 and LIMITED_709; and
the workaround: a torch pass that unpacks the v210 surface to a Y210 surface (three fields of
every 32-bit word to 16-bit words, regrouped Y0 Cb Y1 Cr; checked before timing to yield the Y210
surface of the same samples), timed with events of its own, followed by Y210's K1 on its output.
The frames are the RGB frames' own Y, Cb, Cr kept at 10 bits, chroma the mean of each horizontal
pair.  Reports, per setting, the median, the 10th and 90th percentiles, for the workaround the
pass, the K1 and their sum, and v210's ratio to Y210.  Before timing, the v210 and the Y210 frame
of the first picture are encoded to the host in every mode and preset and their bytes compared.
Accepted: v210's K1 median below the workaround's sum in every column, and the bytes equal.
Prints one JSON line; --out also writes it to a file.

    python tools/measure_v210.py --out profiles/v210_k1.json
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

PRESETS = {"full601": J.JPGE_YUV_FULL_601, "limited709": J.JPGE_YUV_LIMITED_709}
MODES = (422, 420)
LAYOUTS = ("v210", "y210")


def ycc10(rgb):
    """Device (H, W, 3) uint8 RGB -> full-range 10-bit (y, cb, cr) device planes (JFIF constants,
    scaled by 4), chroma the mean of each horizontal pair: int32 samples 0..1020."""
    r, g, b = (rgb[..., c].float() for c in range(3))
    y = .299 * r + .587 * g + .114 * b
    cb = 128 - .1687 * r - .3312 * g + .5 * b
    cr = 128 + .5 * r - .4186 * g - .0813 * b
    h, w = y.shape
    half = lambda c: c.view(h, w // 2, 2).mean(dim=2)
    return tuple((4 * p).round().clamp(0, 1020).to(torch.int32) for p in (y, half(cb), half(cr)))


def surfaces(y, cb, cr):
    """The two surfaces of one picture: v210 (H, W * 2 / 3) int32, a row the stream Cb0 Y0 Cr0 Y1 ...
    three samples to a word; Y210 (H, 2 W) int16 of groups Y0 Cb Y1 Cr, samples in the top 10 bits."""
    h, w = y.shape
    s = torch.stack([cb, y[:, 0::2], cr, y[:, 1::2]], dim=2).reshape(h, 2 * w)
    v210 = (s[:, 0::3] | (s[:, 1::3] << 10) | (s[:, 2::3] << 20)).contiguous()
    y210 = (torch.stack([y[:, 0::2], cb, y[:, 1::2], cr], dim=2).reshape(h, 2 * w) << 6).to(torch.int16).contiguous()
    return {"v210": v210, "y210": y210}


def unpack(v210, y210):
    """The workaround's pass: a v210 surface to the Y210 surface of its samples.  torch ops on the
    whole surface."""
    h = v210.shape[0]
    s = torch.stack([v210 & 0x3FF, (v210 >> 10) & 0x3FF, (v210 >> 20) & 0x3FF], dim=2).view(h, -1, 4)  # Cb Y0 Cr Y1
    y210.copy_((s[:, :, [1, 0, 3, 2]] << 6).view(h, -1))


def encode(enc, layout, surf, w, quality, out=None):
    if layout == "v210":
        return enc.encode_tensor_v210(surf, w, quality=quality, out=out)
    return enc.encode_tensor_yuv422p10(surf, quality=quality, out=out)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--distinct", type=int, default=16, help="distinct frames per setting")
    ap.add_argument("--passes", type=int, default=4, help="timed passes over every setting's frames")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("measure_v210: no GPU (a measurement does not fall back)")
    W, H, D = args.width, args.height, args.distinct
    if W % 96 or H % 2:
        sys.exit("measure_v210: a width that is a multiple of 96 (whole groups, 16-byte aligned rows of both layouts) and an even height")
    frames = [surfaces(*ycc10(torch.from_numpy(J.synth_rgb8(3 + i, W, H, kind=0)).cuda())) for i in range(D)]
    scratch = torch.empty_like(frames[0]["y210"])
    same_samples = True
    for f in frames:  # the workaround yields the Y210 surface of the same samples
        scratch.zero_()
        unpack(f["v210"], scratch)
        same_samples = same_samples and bool(torch.equal(scratch, f["y210"]))
    out = torch.zeros(J.max_jpeg_bytes(W, H), dtype=torch.uint8, device="cuda")
    settings = [(l, m, x) for l in LAYOUTS for m in MODES for x in PRESETS]
    times = {s: [] for s in settings}
    work = {(m, x): {"pass": [], "k1": []} for m in MODES for x in PRESETS}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    equal = True
    with J.Encoder(0, lanes=1) as enc:
        for m in MODES:  # v210 and Y210 of the same samples give the same bytes
            for x in PRESETS:
                enc.set_subsampling(m)
                enc.set_yuv_transform(PRESETS[x])
                files = [encode(enc, l, frames[0][l], W, args.quality) for l in LAYOUTS]
                equal = equal and files[0] == files[1] and len(files[0]) > 1000
        enc.set_timing(1)
        for p in range(args.warmup + args.passes):
            for i in range(D):
                for (l, m, x) in settings:  # the settings in turn
                    enc.set_subsampling(m)
                    enc.set_yuv_transform(PRESETS[x])
                    encode(enc, l, frames[i][l], W, args.quality, out)
                    if p >= args.warmup:
                        times[(l, m, x)].append(enc.timing()["fdct"])
                for (m, x) in work:  # the workaround: the unpacking pass, then Y210's K1 on its output
                    enc.set_subsampling(m)
                    enc.set_yuv_transform(PRESETS[x])
                    ev[0].record()
                    unpack(frames[i]["v210"], scratch)
                    ev[1].record()
                    encode(enc, "y210", scratch, W, args.quality, out)
                    torch.cuda.synchronize()
                    if p >= args.warmup:
                        work[(m, x)]["pass"].append(ev[0].elapsed_time(ev[1]))
                        work[(m, x)]["k1"].append(enc.timing()["fdct"])

    def stat(v):
        q = statistics.quantiles(v, n=10)
        return {"ms_median": round(statistics.median(v), 5), "ms_p10": round(q[0], 5), "ms_p90": round(q[-1], 5)}

    res = {"what": "K1 (fdct) kernel time of v210 frames, of Y210 frames of the same samples, and of the workaround (a torch "
                   "pass unpacking v210 to Y210, by its own events, plus Y210's K1); 1-lane encoder, device input",
           "width": W, "height": H, "quality": args.quality, "subsampling": list(MODES), "picture_kind": 0,
           "distinct_inputs": D, "passes": args.passes, "samples_per_setting": len(times[settings[0]]),
           "device": torch.cuda.get_device_name(0), "v210_equals_y210_bytes": equal,
           "workaround_yields_same_samples": same_samples, "settings": {}, "v210_over_y210": {}, "workaround": {}}
    med = lambda k: statistics.median(times[k])
    for (l, m, x) in settings:
        res["settings"][f"{l}_{m}_{x}"] = stat(times[(l, m, x)])
    ok = equal and same_samples
    for (m, x), v in work.items():
        res["v210_over_y210"][f"{m}_{x}"] = round(med(("v210", m, x)) / med(("y210", m, x)), 4)
        total = [a + b for a, b in zip(v["pass"], v["k1"])]
        below = med(("v210", m, x)) < statistics.median(total)
        ok = ok and below
        res["workaround"][f"{m}_{x}"] = {"unpacking_pass": stat(v["pass"]), "y210_k1": stat(v["k1"]), "sum": stat(total),
                                         "k1_over_sum": round(med(("v210", m, x)) / statistics.median(total), 4),
                                         "k1_below_sum": below}
    res["accepted"] = ok
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
