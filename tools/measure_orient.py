#!/usr/bin/env python3
"""K1 (the transform kernel) with the orientation inside it (Encoder.set_orientation), next to
its floor and to the caller's workaround, by the method of tools/measure_downscale.py: Q90 from
device input on a 1-lane Encoder with per-kernel events (set_timing(1)), D distinct photo-like
frames taken in turn, the settings interleaved within each pass so that drift hits them alike.

Rows: a 3840x2160 source in RGB8 and in BGRA8 under each orientation 1..7.  Per row: the fused
K1; the floor, K1 with JPGE_ORIENT_NONE on the pre-oriented frame O; the workaround, the torch
pass a caller would write that produces O (flip / rot90 / transpose + .contiguous(), checked once
against orient_frame) timed with events of its own, followed by K1 on its output: the pass, the
K1 and their sum; and the source bytes over 8 TB/s, the read bound.  One more row: RGB8 at
3832x2160 mirrored (FLIP_H), a width whose rows are no multiple of 16 bytes, so that every tile
takes the byte path.  Reports medians and 10th / 90th percentiles.
Prints one JSON line; --out also writes it to a file.

    python tools/measure_orient.py --out profiles/orient_k1.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before libjpge: one HIP runtime per process)

import jpgenc_amd as J  # noqa: E402

HBM_BYTES_PER_S = 8e12
NAMES = ("none", "flip_h", "rot180", "flip_v", "transpose", "rot90", "transverse", "rot270")
# the workaround's pass: what a caller would write for each orientation, t is (H, W, C)
PASS = (
    None,
    lambda t: t.flip(1).contiguous(),
    lambda t: t.flip(0, 1).contiguous(),
    lambda t: t.flip(0).contiguous(),
    lambda t: t.transpose(0, 1).contiguous(),
    lambda t: torch.rot90(t, -1, (0, 1)).contiguous(),
    lambda t: torch.rot90(t, 2, (0, 1)).transpose(0, 1).contiguous(),
    lambda t: torch.rot90(t, 1, (0, 1)).contiguous(),
)
FMT = {"rgb8": J.JPGE_FMT_RGB8, "bgra8": J.JPGE_FMT_BGRA8}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--distinct", type=int, default=16, help="distinct frames per setting")
    ap.add_argument("--passes", type=int, default=4, help="timed passes over every setting's frames")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("measure_orient: no GPU (a measurement does not fall back)")
    W, H, N, Q = 3840, 2160, args.distinct, args.quality
    rgb = [torch.from_numpy(J.synth_rgb8(3 + i, W, H, kind=0)).cuda() for i in range(N)]

    def bgra(t):
        a = torch.full((t.shape[0], t.shape[1], 1), 255, dtype=torch.uint8, device="cuda")
        return torch.cat([t.flip(2), a], dim=2).contiguous()

    src = {"rgb8": rgb, "bgra8": [bgra(t) for t in rgb], "rgb8_w3832": [t[:, :3832].contiguous() for t in rgb]}
    # (layout of the sources, orientation): the 14 rows, then the row that misses the alignment
    keys = [(l, o) for o in range(1, 8) for l in ("rgb8", "bgra8")] + [("rgb8_w3832", 1)]
    fmt_of = lambda l: FMT[l.split("_")[0]]
    pre = {}  # O of every source, by the workaround's pass; the first of each checked against orient_frame
    for l, o in keys:
        pre[(l, o)] = [PASS[o](t) for t in src[l]]
        want = J.orient_frame(src[l][0].cpu().numpy(), fmt_of(l), o)
        assert np.array_equal(pre[(l, o)][0].cpu().numpy(), want), "the torch pass does not yield O"
    out = torch.zeros(max(J.max_jpeg_bytes(W, H), J.max_jpeg_bytes(H, W)), dtype=torch.uint8, device="cuda")
    fused = {k: [] for k in keys}
    floor = {k: [] for k in keys}
    work = {k: {"pass": [], "k1": []} for k in keys}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def k1(enc, l, t, o):
        enc.set_orientation(o)
        enc.encode_tensor(t, Q, out=out, order="bgr" if l.startswith("bgra8") else "rgb")
        return enc.timing()["fdct"]

    with J.Encoder(0, lanes=1) as enc:
        enc.set_timing(1)
        for p in range(args.warmup + args.passes):
            for i in range(N):
                for k in keys:  # the settings in turn
                    l, o = k
                    a = k1(enc, l, src[l][i], o)
                    b = k1(enc, l, pre[k][i], 0)
                    ev[0].record()
                    turned = PASS[o](src[l][i])
                    ev[1].record()
                    c = k1(enc, l, turned, 0)
                    torch.cuda.synchronize()
                    if p >= args.warmup:
                        fused[k].append(a)
                        floor[k].append(b)
                        work[k]["pass"].append(ev[0].elapsed_time(ev[1]))
                        work[k]["k1"].append(c)

    def stat(v):
        q = statistics.quantiles(v, n=10)
        return {"ms_median": round(statistics.median(v), 5), "ms_p10": round(q[0], 5), "ms_p90": round(q[-1], 5)}

    res = {"what": "K1 (fdct) kernel time with the orientation inside it, of its floor (K1 with no orientation on the "
                   "pre-oriented frame O) and of the workaround (a torch pass producing O, by its own events, plus K1 on O); "
                   "1-lane encoder, device input",
           "quality": Q, "subsampling": 420, "picture_kind": 0, "distinct_inputs": N, "passes": args.passes,
           "samples_per_setting": len(fused[keys[0]]), "device": torch.cuda.get_device_name(0), "rows": {}}
    for k in keys:
        l, o = k
        h, w, c = src[l][0].shape
        total = [a + b for a, b in zip(work[k]["pass"], work[k]["k1"])]
        res["rows"][f"{l}_{NAMES[o]}"] = {
            "source": [w, h], "orientation": o, "fused_k1": stat(fused[k]), "floor_k1_on_O": stat(floor[k]),
            "read_bound_ms": round(1e3 * (c * w * h) / HBM_BYTES_PER_S, 5),
            "workaround": {"torch_pass": stat(work[k]["pass"]), "k1_on_O": stat(work[k]["k1"]), "sum": stat(total)},
            "fused_over_floor": round(statistics.median(fused[k]) / statistics.median(floor[k]), 4),
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
