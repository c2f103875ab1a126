#!/usr/bin/env python3
"""K1 (the transform kernel) for the 10-bit 4:2:0 layouts (P010, I010) next to NV12 and next to
the caller's workaround, by the method of tools/measure_formats_yuv.py: 3840x2160 Q90 from
device input on a 1-lane Encoder with per-kernel events (set_timing(1)), D distinct photo-like
frames taken in turn, the settings interleaved within each pass so that drift hits them alike.

Settings: P010, I010 and NV12, each under FULL_601 and LIMITED_709, and the workaround: a torch
pass that narrows the P010 frame to NV12 (every word's sample rounded to 8 bits, one kernel
over the surface), timed with events of its own, followed by NV12's K1 on the result.  The
10-bit frames are the RGB frames' own Y, Cb, Cr kept at 10 bits; the NV12 frames are the
workaround's output, so every setting transforms the same picture.  Reports, per setting, the
median, the 10th and 90th percentiles, and for the workaround the pass, the K1 and their sum.
Prints one JSON line; --out also writes it to a file.

    python tools/measure_formats_p010.py --out profiles/formats_p010_k1.json
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


def ycc10(rgb):
    """Device (H, W, 3) uint8 RGB -> full-range 10-bit (y, cb, cr) device planes (JFIF constants,
    scaled by 4), chroma the 2x2 mean: int16 samples 0..1020."""
    r, g, b = (rgb[..., c].float() for c in range(3))
    y = .299 * r + .587 * g + .114 * b
    cb = 128 - .1687 * r - .3312 * g + .5 * b
    cr = 128 + .5 * r - .4186 * g - .0813 * b
    h, w = y.shape
    half = lambda c: c.view(h // 2, 2, w // 2, 2).mean(dim=(1, 3))
    return tuple((4 * p).round().clamp(0, 1020).to(torch.int16) for p in (y, half(cb), half(cr)))


def p010(y, cb, cr):
    """One (H + H/2, W) int16 surface: Y rows, then rows of Cb,Cr word pairs; samples in the top 10 bits."""
    h, w = y.shape
    t = torch.cat([y, torch.stack([cb, cr], dim=2).view(h // 2, w)]).contiguous()
    t = (t.int() << 6).to(torch.int16)  # (wraps into the sign bit: the word's bits are what counts)
    return t[:h], t[h:]


def i010(y, cb, cr):
    h, w = y.shape
    t = torch.cat([y.reshape(-1), cb.reshape(-1), cr.reshape(-1)]).contiguous()
    n, c = w * h, (w // 2) * (h // 2)
    return t[:n].view(h, w), t[n:n + c].view(h // 2, w // 2), t[n + c:].view(h // 2, w // 2)


def narrow(surf10, surf8):
    """The workaround's pass: every 16-bit word of a P010 surface to its sample rounded to 8 bits
    (s + 2) >> 2, clamped: an NV12 surface of the same shape.  torch ops on the whole surface."""
    s = (surf10.int() & 0xFFFF) >> 6
    torch.clamp((s + 2) >> 2, max=255, out=s)
    surf8.copy_(s)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--distinct", type=int, default=16, help="distinct frames per setting")
    ap.add_argument("--passes", type=int, default=6, help="timed passes over every setting's frames")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("measure_formats_p010: no GPU (a measurement does not fall back)")
    W, H, D = args.width, args.height, args.distinct
    if W % 32 or H % 2:
        sys.exit("measure_formats_p010: a width that is a multiple of 32 and an even height (the fast path of every layout)")
    frames = {"p010": [], "i010": [], "nv12": []}
    for i in range(D):
        planes = ycc10(torch.from_numpy(J.synth_rgb8(3 + i, W, H, kind=0)).cuda())
        frames["p010"].append(p010(*planes))
        frames["i010"].append(i010(*planes))
        s8 = torch.empty((H + H // 2, W), dtype=torch.uint8, device="cuda")
        y10, c10 = frames["p010"][-1]
        narrow(y10._base if y10._base is not None else y10, s8)
        frames["nv12"].append((s8[:H], s8[H:].view(H // 2, W // 2, 2)))
    scratch = torch.empty((H + H // 2, W), dtype=torch.uint8, device="cuda")
    out = torch.zeros(J.max_jpeg_bytes(W, H), dtype=torch.uint8, device="cuda")
    settings = [(l, x) for l in ("p010", "i010", "nv12") for x in PRESETS]
    times = {s: [] for s in settings}
    work = {x: {"pass": [], "k1": []} for x in PRESETS}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    with J.Encoder(0, lanes=1) as enc:
        enc.set_timing(1)
        for p in range(args.warmup + args.passes):
            for i in range(D):
                for (l, x) in settings:  # the settings in turn
                    enc.set_yuv_transform(PRESETS[x])
                    t = frames[l][i]
                    if l == "nv12":
                        enc.encode_tensor_yuv(*t, quality=args.quality, out=out)
                    else:
                        enc.encode_tensor_yuv10(*t, quality=args.quality, out=out)
                    if p >= args.warmup:
                        times[(l, x)].append(enc.timing()["fdct"])
                for x in PRESETS:  # the workaround: the narrowing pass, then NV12's K1 on its output
                    enc.set_yuv_transform(PRESETS[x])
                    y10 = frames["p010"][i][0]
                    ev[0].record()
                    narrow(y10._base, scratch)
                    ev[1].record()
                    enc.encode_tensor_yuv(scratch[:H], scratch[H:].view(H // 2, W // 2, 2), quality=args.quality, out=out)
                    torch.cuda.synchronize()
                    if p >= args.warmup:
                        work[x]["pass"].append(ev[0].elapsed_time(ev[1]))
                        work[x]["k1"].append(enc.timing()["fdct"])

    def stat(v):
        q = statistics.quantiles(v, n=10)
        return {"ms_median": round(statistics.median(v), 5), "ms_p10": round(q[0], 5), "ms_p90": round(q[-1], 5)}

    res = {"what": "K1 (fdct) kernel time of the 10-bit layouts, of NV12, and of the workaround (a torch pass "
                   "narrowing P010 to NV12, by its own events, plus NV12's K1); 1-lane encoder, device input",
           "width": W, "height": H, "quality": args.quality, "subsampling": 420, "picture_kind": 0, "distinct_inputs": D,
           "passes": args.passes, "samples_per_setting": len(times[settings[0]]), "device": torch.cuda.get_device_name(0),
           "settings": {}, "workaround": {}}
    for (l, x) in settings:
        res["settings"][f"{l}_{x}"] = stat(times[(l, x)])
    for x in PRESETS:
        total = [a + b for a, b in zip(work[x]["pass"], work[x]["k1"])]
        res["workaround"][x] = {"narrowing_pass": stat(work[x]["pass"]), "nv12_k1": stat(work[x]["k1"]), "sum": stat(total),
                                "p010_k1_over_sum": round(statistics.median(times[("p010", x)]) / statistics.median(total), 4)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
