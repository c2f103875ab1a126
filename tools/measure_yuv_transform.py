#!/usr/bin/env python3
"""K1 (the transform kernel) for NV12 under the sample transform (jpge_set_yuv_transform), by
the method of tools/measure_formats_yuv.py: 3840x2160 4:2:0 Q90 from device input on a 1-lane
Encoder with per-kernel events (set_timing(1)), D distinct photo-like frames taken in turn, the
settings interleaved within each pass so that drift hits them alike.

The frames are studio-swing BT.709 NV12 (what a video decoder hands over), made from the RGB
frames.  Settings, all on the same bytes:
  full601      the kExact instance (reads the bytes as full-range BT.601: the washed-out file)
  limited601   the transform instance, range expansion only
  limited709   the transform instance, range expansion and the matrix
  workaround   what a caller had to do before: a torch elementwise pass that rewrites the frame to
               full-range BT.601 8-bit NV12 (timed with events of its own), then full601
Reports, per setting, the median `fdct` kernel time with its 10th and 90th percentiles and its
ratio to full601 in the same run; for the workaround also the pass and pass + K1.  Prints one
JSON line; --out also writes it to a file.

    python tools/measure_yuv_transform.py --out profiles/yuv_transform_k1.json
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

SETTINGS = ("full601", "limited601", "limited709", "workaround")
PRESET = {"full601": J.JPGE_YUV_FULL_601, "limited601": J.JPGE_YUV_LIMITED_601, "limited709": J.JPGE_YUV_LIMITED_709,
          "workaround": J.JPGE_YUV_FULL_601}


def nv12_limited709(rgb):
    """Device (H, W, 3) uint8 RGB -> a studio-swing BT.709 NV12 surface (H + H/2, W) uint8."""
    r, g, b = (rgb[..., c].double() for c in range(3))
    y = .2126 * r + .7152 * g + .0722 * b
    cb, cr = (b - y) / 1.8556, (r - y) / 1.5748
    h, w = y.shape
    mean = lambda c: c.view(h // 2, 2, w // 2, 2).mean(dim=(1, 3))  # noqa: E731
    yq = (16 + y * (219 / 255)).round().clamp(0, 255).to(torch.uint8)
    cq = [(128 + mean(c) * (224 / 255)).round().clamp(0, 255).to(torch.uint8) for c in (cb, cr)]
    return torch.cat([yq, torch.stack(cq, dim=2).view(h // 2, w)]).contiguous()


def views(surf, h, w):
    return surf[:h], surf[h:].view(h // 2, w // 2, 2)


def rewrite(src, dst, h, w, t):
    """The workaround's pass: src (studio-swing BT.709 NV12) -> dst, full-range BT.601 NV12
    rounded to 8 bits, with the preset's coefficients t (fp32 arithmetic, as such a pass is
    usually written)."""
    y, c = views(src, h, w)
    u, v = c[..., 0].float() - 128, c[..., 1].float() - 128
    up = lambda p: p.repeat_interleave(2, dim=0).repeat_interleave(2, dim=1)  # noqa: E731
    dy, dc = views(dst, h, w)
    dy.copy_((t[1] * (y.float() - t[0]) + t[2] * up(u) + t[3] * up(v)).round().clamp(0, 255))
    dc[..., 0].copy_((t[4] * u + t[5] * v + 128).round().clamp(0, 255))
    dc[..., 1].copy_((t[6] * u + t[7] * v + 128).round().clamp(0, 255))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--distinct", type=int, default=16, help="distinct frames")
    ap.add_argument("--passes", type=int, default=6, help="timed passes over the frames")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("measure_yuv_transform: no GPU (a measurement does not fall back)")
    W, H, D = args.width, args.height, args.distinct
    if W % 32 or H % 2:
        sys.exit("measure_yuv_transform: a width that is a multiple of 32 and an even height (the fast path)")
    frames = [nv12_limited709(torch.from_numpy(J.synth_rgb8(3 + i, W, H, kind=0)).cuda()) for i in range(D)]
    fixed = torch.zeros_like(frames[0])  # the workaround's rewritten frame
    t709 = J.yuv_preset(J.JPGE_YUV_LIMITED_709)
    out = torch.zeros(J.max_jpeg_bytes(W, H), dtype=torch.uint8, device="cuda")
    times = {s: [] for s in SETTINGS}
    pass_ms = []
    size = {}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    with J.Encoder(0, lanes=1) as enc:
        enc.set_timing(1)
        for p in range(args.warmup + args.passes):
            for i in range(D):
                for s in SETTINGS:  # the settings in turn
                    src = frames[i]
                    if s == "workaround":
                        ev[0].record()
                        rewrite(src, fixed, H, W, t709)
                        ev[1].record()
                        src = fixed
                    enc.set_yuv_transform(PRESET[s])
                    n = enc.encode_tensor_yuv(*views(src, H, W), quality=args.quality, out=out)
                    if p == 0 and i == 0:
                        size[s] = int(n)
                    if p >= args.warmup:
                        times[s].append(enc.timing()["fdct"])
                        if s == "workaround":
                            torch.cuda.synchronize()
                            pass_ms.append(ev[0].elapsed_time(ev[1]))
    med = {s: statistics.median(times[s]) for s in SETTINGS}
    base = med["full601"]
    res = {"what": "K1 (fdct) kernel time for NV12 per sample-transform setting, 1-lane encoder, device input, kernel events",
           "width": W, "height": H, "quality": args.quality, "subsampling": 420, "picture_kind": 0,
           "input": "studio-swing BT.709 NV12 of synth_rgb8 frames", "distinct_inputs": D, "passes": args.passes,
           "samples_per_setting": len(times["full601"]), "device": torch.cuda.get_device_name(0), "settings": {}}
    for s in SETTINGS:
        q = statistics.quantiles(times[s], n=10)
        res["settings"][s] = {"fdct_ms_median": round(med[s], 5), "fdct_ms_p10": round(q[0], 5), "fdct_ms_p90": round(q[-1], 5),
                              "fdct_ms_min": round(min(times[s]), 5), "fdct_ms_max": round(max(times[s]), 5),
                              "ratio_to_full601": round(med[s] / base, 4), "jpg_bytes_first_frame": size[s]}
    q = statistics.quantiles(pass_ms, n=10)
    pm = statistics.median(pass_ms)
    res["settings"]["workaround"].update({"pass_ms_median": round(pm, 5), "pass_ms_p10": round(q[0], 5),
                                          "pass_ms_p90": round(q[-1], 5), "pass_plus_fdct_ms_median": round(pm + med["workaround"], 5),
                                          "pass_plus_fdct_ratio_to_limited709": round((pm + med["workaround"]) / med["limited709"], 3)})
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
