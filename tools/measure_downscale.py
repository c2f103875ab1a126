#!/usr/bin/env python3
"""K1 (the transform kernel) with the box downscale inside it (Encoder.set_downscale), next to
its floor and to the caller's workaround, by the method of tools/measure_formats_p010.py: Q90
from device input on a 1-lane Encoder with per-kernel events (set_timing(1)), D distinct
photo-like frames taken in turn, the settings interleaved within each pass so that drift hits
them alike.

Rows: 3840x2160 -> 1920x1080 at factor 2 and 7680x4320 -> 1920x1080 at factor 4, RGB8 and NV12
each; the floor, K1 at factor 1 on the 1920x1080 frame D itself; and the workaround, the torch
pass a caller would write that produces D (checked once against downscale_frame) timed with
events of its own, followed by K1 on D: the pass, the K1 and their sum.  Beside each fused row,
the source bytes over 8 TB/s: the read bound.  Reports medians and 10th / 90th percentiles.

Also the pipeline condition: a 4-lane batch of 3840x2160 RGB8 frames at factor 2 against the
same batch at factor 1 (the full-size headline workload), wall time per source frame.
Prints one JSON line; --out also writes it to a file.

    python tools/measure_downscale.py --out profiles/downscale_k1.json
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

HBM_BYTES_PER_S = 8e12


def box(t, s):
    """The workaround's pass: (H, W, C) uint8 -> the rounded s x s means (H and W multiples of s)."""
    h, w, c = t.shape
    x = t.view(h // s, s, w // s, s, c).to(torch.int32).sum(dim=(1, 3))
    return ((x + s * s // 2) // (s * s)).to(torch.uint8)


def nv12_of(rgb):
    """Device (H, W, 3) RGB -> one (H + H/2, W) uint8 NV12 surface (JFIF constants, 2x2 mean chroma)."""
    r, g, b = (rgb[..., c].float() for c in range(3))
    h, w = r.shape
    y = .299 * r + .587 * g + .114 * b
    half = lambda p: p.view(h // 2, 2, w // 2, 2).mean(dim=(1, 3))
    cb, cr = half(128 - .1687 * r - .3312 * g + .5 * b), half(128 + .5 * r - .4186 * g - .0813 * b)
    q = lambda p: p.round().clamp(0, 255).to(torch.uint8)
    return torch.cat([q(y), torch.stack([q(cb), q(cr)], dim=2).view(h // 2, w)]).contiguous()


def nv12_views(surf):
    h = surf.shape[0] * 2 // 3
    return surf[:h], surf[h:].view(h // 2, surf.shape[1] // 2, 2)


def box_nv12(surf, s, out):
    """The workaround's pass on an NV12 surface: the Y plane and the Cb,Cr plane, each in its domain."""
    y, c = nv12_views(surf)
    oy, oc = nv12_views(out)
    oy.copy_(box(y.unsqueeze(2), s).squeeze(2))
    oc.copy_(box(c, s))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--distinct", type=int, default=16, help="distinct frames per setting")
    ap.add_argument("--passes", type=int, default=4, help="timed passes over every setting's frames")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=32, help="frames of the 4-lane batches")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("measure_downscale: no GPU (a measurement does not fall back)")
    W, H, N, Q = 1920, 1080, args.distinct, args.quality
    # 4K pictures from the synthesiser; an 8K picture is four of them side by side (distinct per index)
    k4 = [torch.from_numpy(J.synth_rgb8(3 + i, 2 * W, 2 * H, kind=0)).cuda() for i in range(N)]
    def k8(i):
        top = torch.cat([k4[i], k4[(i + 1) % N]], dim=1)
        return torch.cat([top, torch.cat([k4[(i + 2) % N], k4[(i + 3) % N]], dim=1)], dim=0).contiguous()
    src = {("rgb8", 2): k4, ("rgb8", 4): [k8(i) for i in range(N)]}
    for s in (2, 4):
        src[("nv12", s)] = [nv12_of(t) for t in src[("rgb8", s)]]
    # D of every source, by the workaround's pass; the first of each checked against downscale_frame
    dst = {}
    for (l, s), frames in src.items():
        if l == "rgb8":
            dst[(l, s)] = [box(t, s) for t in frames]
            want = J.downscale_frame(frames[0].cpu().numpy(), J.JPGE_FMT_RGB8, s)
            assert np.array_equal(dst[(l, s)][0].cpu().numpy(), want), "the torch pass does not yield D"
        else:
            dst[(l, s)] = []
            for t in frames:
                o = torch.empty((H + H // 2, W), dtype=torch.uint8, device="cuda")
                box_nv12(t, s, o)
                dst[(l, s)].append(o)
            y, c = (p.cpu().numpy() for p in nv12_views(frames[0]))
            want = J.downscale_frame(J.pack_yuv420(J.JPGE_FMT_NV12, y, c[:, :, 0], c[:, :, 1])[0], J.JPGE_FMT_NV12, s)
            assert np.array_equal(dst[(l, s)][0].cpu().numpy().reshape(-1), np.asarray(want)), "the torch pass does not yield D"
    scratch = {"rgb8": torch.empty((H, W, 3), dtype=torch.uint8, device="cuda"),
               "nv12": torch.empty((H + H // 2, W), dtype=torch.uint8, device="cuda")}
    out = torch.zeros(J.max_jpeg_bytes(W, H), dtype=torch.uint8, device="cuda")
    keys = [(l, s) for s in (2, 4) for l in ("rgb8", "nv12")]
    fused = {k: [] for k in keys}
    floor = {k: [] for k in keys}
    work = {k: {"pass": [], "k1": []} for k in keys}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def k1(enc, l, t, s):
        enc.set_downscale(s)
        if l == "rgb8":
            enc.encode_tensor(t, Q, out=out)
        else:
            enc.encode_tensor_yuv(*nv12_views(t), quality=Q, out=out)
        return enc.timing()["fdct"]

    with J.Encoder(0, lanes=1) as enc:
        enc.set_timing(1)
        for p in range(args.warmup + args.passes):
            for i in range(N):
                for k in keys:  # the settings in turn
                    l, s = k
                    a = k1(enc, l, src[k][i], s)
                    b = k1(enc, l, dst[k][i], 1)
                    ev[0].record()
                    if l == "rgb8":
                        scratch[l].copy_(box(src[k][i], s))
                    else:
                        box_nv12(src[k][i], s, scratch[l])
                    ev[1].record()
                    c = k1(enc, l, scratch[l], 1)
                    torch.cuda.synchronize()
                    if p >= args.warmup:
                        fused[k].append(a)
                        floor[k].append(b)
                        work[k]["pass"].append(ev[0].elapsed_time(ev[1]))
                        work[k]["k1"].append(c)

    # the pipeline condition: 4 lanes, 4K RGB8 frames, factor 2 against factor 1
    batch = {}
    frames = [(k4[i % N].data_ptr(), 2 * W, 2 * H, 2 * W * 3) for i in range(args.batch)]
    cap = J.max_jpeg_bytes(2 * W, 2 * H)
    outs_t = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(args.batch)]
    outs = [(o.data_ptr(), cap) for o in outs_t]
    with J.Encoder(0, lanes=4) as enc:
        samples = {1: [], 2: []}
        for rep in range(2 + 8):
            for s in (1, 2):
                enc.set_downscale(s)
                t0 = time.perf_counter()
                enc.encode_batch_dev(frames, outs, Q)
                dt = time.perf_counter() - t0
                if rep >= 2:
                    samples[s].append(1e3 * dt / args.batch)
        batch = {f"factor{s}_ms_per_source_frame": {"median": round(statistics.median(v), 5), "min": round(min(v), 5),
                                                      "max": round(max(v), 5)} for s, v in samples.items()}

    def stat(v):
        q = statistics.quantiles(v, n=10)
        return {"ms_median": round(statistics.median(v), 5), "ms_p10": round(q[0], 5), "ms_p90": round(q[-1], 5)}

    res = {"what": "K1 (fdct) kernel time with the box downscale inside it, of its floor (K1 on the 1920x1080 frame D) and of "
                   "the workaround (a torch pass producing D, by its own events, plus K1 on D); 1-lane encoder, device input",
           "output": [W, H], "quality": Q, "subsampling": 420, "picture_kind": 0, "distinct_inputs": N, "passes": args.passes,
           "samples_per_setting": len(fused[keys[0]]), "device": torch.cuda.get_device_name(0), "rows": {},
           "batch_4lane_4k_rgb8": dict(batch, frames=args.batch)}
    for k in keys:
        l, s = k
        nbytes = (3 if l == "rgb8" else 1.5) * (W * s) * (H * s)
        total = [a + b for a, b in zip(work[k]["pass"], work[k]["k1"])]
        res["rows"][f"{l}_factor{s}"] = {
            "source": [W * s, H * s], "fused_k1": stat(fused[k]), "floor_k1_on_D": stat(floor[k]),
            "read_bound_ms": round(1e3 * nbytes / HBM_BYTES_PER_S, 5),
            "workaround": {"torch_pass": stat(work[k]["pass"]), "k1_on_D": stat(work[k]["k1"]), "sum": stat(total)},
            "fused_over_workaround": round(statistics.median(fused[k]) / statistics.median(total), 4)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
