#!/usr/bin/env python3
"""K1 (the transform kernel) with the bilinear demosaic inside it (JPGE_FMT_BAYER_*), next to its
floor and to the caller's workaround, by the method of tools/measure_orient.py: Q90 from device
input on a 1-lane Encoder with per-kernel events (set_timing(1)), D distinct photo-like frames
(mosaics of synth_rgb8 frames) taken in turn, the settings interleaved within each pass so that
drift hits them alike.

Rows: a 3840x2160 mosaic in RGGB and in GRBG, from an aligned tensor and from an unaligned one
(base + 1, an odd pitch: every tile takes the byte path).  Per row: the fused K1; the floor, K1 as
RGB8 on the pre-demosaiced frame D; the workaround, the torch pass a caller would write that
produces D (reflect-padded slices, integer means, torch.where by site, checked once against
demosaic_frame) timed with events of its own, followed by K1 on its output: the pass, the K1 and
their sum; and W * H bytes over 8 TB/s, the read bound.  Reports medians and 10th / 90th percentiles.
Prints one JSON line; --out also writes it to a file.

    python tools/measure_bayer.py --out profiles/bayer_k1.json
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
FMT = {"rggb": J.JPGE_FMT_BAYER_RGGB8, "grbg": J.JPGE_FMT_BAYER_GRBG8}


def colours(name, h, w):
    """(h, w) numpy: 0 R, 1 G, 2 B of every site."""
    cell = np.array(["rgb".index(c) for c in name]).reshape(2, 2)
    return cell[np.arange(h)[:, None] & 1, np.arange(w)[None, :] & 1]


class TorchDemosaic:
    """The workaround's pass for one pattern and size: the masks are built once, as a caller would."""

    def __init__(self, name, h, w, device="cuda"):
        col = colours(name, h, w)
        row_colour = colours(name, h, w + 1)[:, 1:]  # the colour beside a site, on its row
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self.is_g = dev(col == 1)
        self.own = [dev(col == k) for k in (0, 2)]
        self.on_row = [dev((col == 1) & (row_colour == k)) for k in (0, 2)]

    def __call__(self, t):
        v = t.to(torch.int16)
        v = torch.cat([v[1:2], v, v[-2:-1]], 0)
        v = torch.cat([v[:, 1:2], v, v[:, -2:-1]], 1)
        c = v[1:-1, 1:-1]
        up, down, left, right = v[:-2, 1:-1], v[2:, 1:-1], v[1:-1, :-2], v[1:-1, 2:]
        plus = (up + down + left + right + 2) >> 2
        diag = (v[:-2, :-2] + v[:-2, 2:] + v[2:, :-2] + v[2:, 2:] + 2) >> 2
        rowm, colm = (left + right + 1) >> 1, (up + down + 1) >> 1
        g = torch.where(self.is_g, c, plus)
        rb = [torch.where(self.own[i], c, torch.where(self.is_g, torch.where(self.on_row[i], rowm, colm), diag)) for i in (0, 1)]
        return torch.stack([rb[0], g, rb[1]], 2).to(torch.uint8).contiguous()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--distinct", type=int, default=16, help="distinct frames per setting")
    ap.add_argument("--passes", type=int, default=4, help="timed passes over every setting's frames")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("measure_bayer: no GPU (a measurement does not fall back)")
    W, H, N, Q = 3840, 2160, args.distinct, args.quality
    rgb = [J.synth_rgb8(3 + i, W, H, kind=0) for i in range(N)]

    def view(a, aligned):
        """The (H, W) mosaic on the device: dense rows, or base + 1 and an odd pitch."""
        if aligned:
            return torch.from_numpy(a).cuda()
        st = W + 17
        host = np.zeros(1 + st * H, np.uint8)
        host[1:].reshape(H, st)[:, :W] = a
        return torch.as_strided(torch.from_numpy(host).cuda(), (H, W), (st, 1), 1)

    keys = [(n, al) for n in FMT for al in (True, False)]
    src, pre, demosaic = {}, {}, {}
    for n in FMT:
        demosaic[n] = TorchDemosaic(n, H, W)
        mos = [np.ascontiguousarray(np.take_along_axis(f, colours(n, H, W)[..., None], 2)[..., 0]) for f in rgb]
        for al in (True, False):
            src[(n, al)] = [view(a, al) for a in mos]
        pre[n] = [demosaic[n](t) for t in src[(n, True)]]
        want = J.demosaic_frame(mos[0], FMT[n])
        assert np.array_equal(pre[n][0].cpu().numpy(), want), "the torch pass does not yield D"
        assert np.array_equal(demosaic[n](src[(n, False)][0]).cpu().numpy(), want), "the torch pass does not yield D"
    del rgb
    out = torch.zeros(J.max_jpeg_bytes(W, H), dtype=torch.uint8, device="cuda")
    fused = {k: [] for k in keys}
    floor = {k: [] for k in keys}
    work = {k: {"pass": [], "k1": []} for k in keys}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def k1(enc, t, layout=None):
        enc.encode_tensor(t, Q, out=out, layout=layout)
        return enc.timing()["fdct"]

    with J.Encoder(0, lanes=1) as enc:
        enc.set_timing(1)
        for p in range(args.warmup + args.passes):
            for i in range(N):
                for k in keys:  # the settings in turn
                    n, al = k
                    a = k1(enc, src[k][i], "bayer_" + n)
                    b = k1(enc, pre[n][i])
                    ev[0].record()
                    d = demosaic[n](src[k][i])
                    ev[1].record()
                    c = k1(enc, d)
                    torch.cuda.synchronize()
                    if p >= args.warmup:
                        fused[k].append(a)
                        floor[k].append(b)
                        work[k]["pass"].append(ev[0].elapsed_time(ev[1]))
                        work[k]["k1"].append(c)

    def stat(v):
        q = statistics.quantiles(v, n=10)
        return {"ms_median": round(statistics.median(v), 5), "ms_p10": round(q[0], 5), "ms_p90": round(q[-1], 5)}

    res = {"what": "K1 (fdct) kernel time with the bilinear demosaic inside it, of its floor (K1 as RGB8 on the "
                   "pre-demosaiced frame D) and of the workaround (a torch pass producing D, by its own events, plus K1 on D); "
                   "1-lane encoder, device input",
           "quality": Q, "subsampling": 420, "picture_kind": 0, "distinct_inputs": N, "passes": args.passes,
           "samples_per_setting": len(fused[keys[0]]), "device": torch.cuda.get_device_name(0), "rows": {}}
    for k in keys:
        n, al = k
        total = [a + b for a, b in zip(work[k]["pass"], work[k]["k1"])]
        res["rows"][f"{n}_{'aligned' if al else 'unaligned'}"] = {
            "source": [W, H], "fused_k1": stat(fused[k]), "floor_k1_rgb8_on_D": stat(floor[k]),
            "read_bound_ms": round(1e3 * (W * H) / HBM_BYTES_PER_S, 5),
            "workaround": {"torch_pass": stat(work[k]["pass"]), "k1_on_D": stat(work[k]["k1"]), "sum": stat(total)},
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
