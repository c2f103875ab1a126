#!/usr/bin/env python3
"""K1 (the transform kernel) for the 10-bit 4:2:2 layouts (Y210, P210, I210) next to their 8-bit
counterparts (YUYV, NV16, I422) and next to the caller's workaround, by the method of
tools/measure_formats_p010.py: 3840x2160 Q90 from device input on a 1-lane Encoder with
per-kernel events (set_timing(1)), D distinct photo-like frames taken in turn, the settings
interleaved within each pass so that drift hits them alike.

Settings: the six layouts, each in subsampling mode 422 and 420, under FULL_601 and LIMITED_709;
and per 10-bit layout the workaround: a torch pass that narrows the frame to its 8-bit
counterpart (every word's sample rounded to 8 bits, one kernel chain over the surface), timed
with events of its own, followed by that layout's K1 on the result.  The 10-bit frames are the
RGB frames' own Y, Cb, Cr kept at 10 bits, chroma the mean of each horizontal pair; the 8-bit
frames are the workaround's output, so every setting transforms the same picture.  Reports, per
setting, the median, the 10th and 90th percentiles, for the workaround the pass, the K1 and
their sum, and each 10-bit layout's ratio to its counterpart.  Before timing, the three 10-bit
layouts of the first frame are encoded to the host in every mode and preset and their bytes
compared.  Prints one JSON line; --out also writes it to a file.

    python tools/measure_formats_422p10.py --out profiles/formats_422p10_k1.json
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
TEN = ("y210", "p210", "i210")
EIGHT = {"y210": "yuyv", "p210": "nv16", "i210": "i422"}


def ycc10(rgb):
    """Device (H, W, 3) uint8 RGB -> full-range 10-bit (y, cb, cr) device planes (JFIF constants,
    scaled by 4), chroma the mean of each horizontal pair: int16 samples 0..1020."""
    r, g, b = (rgb[..., c].float() for c in range(3))
    y = .299 * r + .587 * g + .114 * b
    cb = 128 - .1687 * r - .3312 * g + .5 * b
    cr = 128 + .5 * r - .4186 * g - .0813 * b
    h, w = y.shape
    half = lambda c: c.view(h, w // 2, 2).mean(dim=2)
    return tuple((4 * p).round().clamp(0, 1020).to(torch.int16) for p in (y, half(cb), half(cr)))


def high(t):
    """Samples into the top 10 bits of their words (wraps into the sign bit: the bits are what counts)."""
    return (t.int() << 6).to(torch.int16)


def surfaces(y, cb, cr):
    """The three 10-bit surfaces of one picture, each one int16 allocation: Y210 (H, 2 W) of groups
    Y0 Cb Y1 Cr; P210 (2 H, W), Y rows then rows of Cb,Cr pairs; I210 flat, Y then Cb then Cr."""
    h, w = y.shape
    y210 = high(torch.stack([y[:, 0::2], cb, y[:, 1::2], cr], dim=2).reshape(h, 2 * w)).contiguous()
    p210 = high(torch.cat([y, torch.stack([cb, cr], dim=2).view(h, w)])).contiguous()
    i210 = torch.cat([y.reshape(-1), cb.reshape(-1), cr.reshape(-1)]).contiguous()
    return {"y210": y210, "p210": p210, "i210": i210}


def views(layout, surf, h, w):
    """The tensors the encode entries take, as views of a layout's surface (10-bit or 8-bit)."""
    cw = w // 2
    if layout == "y210":
        return (surf,)
    if layout == "yuyv":
        return (surf.view(h, w, 2),)
    if layout == "p210":
        return surf[:h], surf[h:]
    if layout == "nv16":
        return surf[:h], surf[h:].view(h, cw, 2)
    n, c = w * h, cw * h
    return surf[:n].view(h, w), surf[n:n + c].view(h, cw), surf[n + c:].view(h, cw)


def narrow(layout, surf10, surf8):
    """The workaround's pass: every 16-bit word of a 10-bit surface to its sample rounded to 8 bits
    (s + 2) >> 2, clamped: the 8-bit counterpart's surface, of the same shape.  torch ops on the
    whole surface."""
    s = surf10.int() & 0xFFFF
    s = s & 0x3FF if layout == "i210" else s >> 6
    torch.clamp((s + 2) >> 2, max=255, out=s)
    surf8.copy_(s)


def encode(enc, layout, t, quality, out=None):
    if layout in TEN:
        return enc.encode_tensor_yuv422p10(*t, quality=quality, out=out)
    return enc.encode_tensor_yuv422(*t, quality=quality, out=out, layout="yuyv" if layout == "yuyv" else None)


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
        sys.exit("measure_formats_422p10: no GPU (a measurement does not fall back)")
    W, H, D = args.width, args.height, args.distinct
    if W % 32 or H % 2:
        sys.exit("measure_formats_422p10: a width that is a multiple of 32 and an even height (the fast path of every layout)")
    ten, eight = [], []
    for i in range(D):
        s10 = surfaces(*ycc10(torch.from_numpy(J.synth_rgb8(3 + i, W, H, kind=0)).cuda()))
        s8 = {}
        for l in TEN:
            s8[EIGHT[l]] = torch.empty(s10[l].shape, dtype=torch.uint8, device="cuda")
            narrow(l, s10[l], s8[EIGHT[l]])
        ten.append(s10)
        eight.append(s8)
    scratch = {l: torch.empty(ten[0][l].shape, dtype=torch.uint8, device="cuda") for l in TEN}
    out = torch.zeros(J.max_jpeg_bytes(W, H), dtype=torch.uint8, device="cuda")
    layouts = TEN + tuple(EIGHT[l] for l in TEN)
    settings = [(l, m, x) for l in layouts for m in MODES for x in PRESETS]
    times = {s: [] for s in settings}
    work = {(l, m, x): {"pass": [], "k1": []} for l in TEN for m in MODES for x in PRESETS}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    equal = True
    with J.Encoder(0, lanes=1) as enc:
        for m in MODES:  # the three layouts of the same samples give the same bytes
            for x in PRESETS:
                enc.set_subsampling(m)
                enc.set_yuv_transform(PRESETS[x])
                files = [encode(enc, l, views(l, ten[0][l], H, W), args.quality) for l in TEN]
                equal = equal and files[0] == files[1] == files[2] and len(files[0]) > 1000
        enc.set_timing(1)
        for p in range(args.warmup + args.passes):
            for i in range(D):
                for (l, m, x) in settings:  # the settings in turn
                    enc.set_subsampling(m)
                    enc.set_yuv_transform(PRESETS[x])
                    encode(enc, l, views(l, (ten if l in TEN else eight)[i][l], H, W), args.quality, out)
                    if p >= args.warmup:
                        times[(l, m, x)].append(enc.timing()["fdct"])
                for (l, m, x) in work:  # the workaround: the narrowing pass, then the 8-bit layout's K1 on its output
                    enc.set_subsampling(m)
                    enc.set_yuv_transform(PRESETS[x])
                    ev[0].record()
                    narrow(l, ten[i][l], scratch[l])
                    ev[1].record()
                    encode(enc, EIGHT[l], views(EIGHT[l], scratch[l], H, W), args.quality, out)
                    torch.cuda.synchronize()
                    if p >= args.warmup:
                        work[(l, m, x)]["pass"].append(ev[0].elapsed_time(ev[1]))
                        work[(l, m, x)]["k1"].append(enc.timing()["fdct"])

    def stat(v):
        q = statistics.quantiles(v, n=10)
        return {"ms_median": round(statistics.median(v), 5), "ms_p10": round(q[0], 5), "ms_p90": round(q[-1], 5)}

    res = {"what": "K1 (fdct) kernel time of the 10-bit 4:2:2 layouts, of their 8-bit counterparts, and of the workaround "
                   "(a torch pass narrowing the frame to the 8-bit layout, by its own events, plus that layout's K1); "
                   "1-lane encoder, device input",
           "width": W, "height": H, "quality": args.quality, "subsampling": list(MODES), "picture_kind": 0,
           "distinct_inputs": D, "passes": args.passes, "samples_per_setting": len(times[settings[0]]),
           "device": torch.cuda.get_device_name(0), "three_layouts_equal_bytes": equal, "settings": {}, "ratio_to_8bit": {},
           "workaround": {}}
    med = lambda k: statistics.median(times[k])
    for (l, m, x) in settings:
        res["settings"][f"{l}_{m}_{x}"] = stat(times[(l, m, x)])
    ok = equal
    for (l, m, x), v in work.items():
        res["ratio_to_8bit"][f"{l}_{m}_{x}"] = round(med((l, m, x)) / med((EIGHT[l], m, x)), 4)
        total = [a + b for a, b in zip(v["pass"], v["k1"])]
        below = med((l, m, x)) < statistics.median(total)
        ok = ok and below
        res["workaround"][f"{l}_{m}_{x}"] = {"narrowing_pass": stat(v["pass"]), f"{EIGHT[l]}_k1": stat(v["k1"]), "sum": stat(total),
                                             "k1_over_sum": round(med((l, m, x)) / statistics.median(total), 4),
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
