#!/usr/bin/env python3
"""K1 (the transform kernel) with the per-channel lookup tables inside it (jpge_set_channel_lut),
next to its floor and to the caller's workaround, by the method of tools/measure_bayer.py: Q90 from
device input on a 1-lane Encoder with per-kernel events (set_timing(1)), D distinct photo-like
frames (synth_rgb8) taken in turn, the settings interleaved within each pass so that drift hits
them alike.  The tables are a gamma curve for R, G and B with different gains.

Rows: a 3840x2160 frame as RGB8 from an aligned tensor and from an unaligned one (base + 1, an odd
pitch: every tile takes the byte path), as BGRA8 aligned, and as an RGGB mosaic aligned.  Per row:
the fused K1; the floor, K1 without tables as RGB8 on the pre-mapped frame M (the kernels of a
context that never set tables); the workaround, the torch gather pass a caller would write
(lut[c][t[..., c].long()], checked once against lut_frame) timed with events of its own, followed
by K1 without tables on its output: the pass, the K1 and their sum.  For the mosaic the workaround's
pass is the gather alone, on the demosaiced frame.  Reports medians and 10th / 90th percentiles.
Prints one JSON line; --out also writes it to a file.

    python tools/measure_lut.py --out profiles/lut_k1.json
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


def tables():
    i = np.arange(256) / 255.0
    return np.stack([np.clip(np.round(255.0 * g * i ** (1 / 2.2)), 0, 255).astype(np.uint8) for g in (1.10, 1.00, 0.85)])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--distinct", type=int, default=16, help="distinct frames per setting")
    ap.add_argument("--passes", type=int, default=4, help="timed passes over every setting's frames")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("measure_lut: no GPU (a measurement does not fall back)")
    W, H, N, Q = 3840, 2160, args.distinct, args.quality
    lut = tables()
    lut_dev = torch.from_numpy(lut).cuda()
    rgb = [J.synth_rgb8(3 + i, W, H, kind=0) for i in range(N)]
    cell = np.array([[0, 1], [1, 2]])[np.arange(H)[:, None] & 1, np.arange(W)[None, :] & 1]  # RGGB

    def unaligned(a):
        st = 3 * W + 17
        host = np.zeros(1 + st * H, np.uint8)
        host[1:].reshape(H, st)[:, :3 * W] = a.reshape(H, 3 * W)
        return torch.as_strided(torch.from_numpy(host).cuda(), (H, W, 3), (st, 3, 1), 1)

    def gather(t, order):
        """The workaround's pass: every colour byte through its table; a fourth byte kept."""
        out = t.clone() if t.shape[2] == 4 else torch.empty_like(t)
        for c, k in enumerate(order):
            out[..., k] = lut_dev[c][t[..., k].long()]
        return out

    # key -> (encode_tensor arguments of the fused encode, the frames, the workaround's input, its channel order)
    rows = {}
    rows["rgb8_aligned"] = ({"layout": "hwc"}, [torch.from_numpy(f).cuda() for f in rgb], None, (0, 1, 2))
    rows["rgb8_unaligned"] = ({"layout": "hwc"}, [unaligned(f) for f in rgb], None, (0, 1, 2))
    bgra = [np.ascontiguousarray(np.concatenate([f[..., ::-1], np.full((H, W, 1), 255, np.uint8)], 2)) for f in rgb]
    rows["bgra8_aligned"] = ({"layout": "hwc", "order": "bgr"}, [torch.from_numpy(f).cuda() for f in bgra], None, (2, 1, 0))
    mos = [np.ascontiguousarray(np.take_along_axis(f, cell[..., None], 2)[..., 0]) for f in rgb]
    dem = [torch.from_numpy(J.demosaic_frame(m, J.JPGE_FMT_BAYER_RGGB8)).cuda() for m in mos]
    rows["rggb_aligned"] = ({"layout": "bayer_rggb"}, [torch.from_numpy(m).cuda() for m in mos], dem, (0, 1, 2))
    keys = list(rows)
    # the pre-mapped RGB8 frames M, and the check of the torch pass against lut_frame
    pre = {}
    for k in keys:
        kw, src, wsrc, order = rows[k]
        win = wsrc if wsrc is not None else src
        g0 = gather(win[0], order)
        fmt = J.JPGE_FMT_BGRA8 if k == "bgra8_aligned" else J.JPGE_FMT_RGB8
        assert np.array_equal(g0.cpu().numpy(), J.lut_frame(win[0].cpu().numpy(), fmt, lut)), "the torch pass does not yield lut_frame's frame"
        pre[k] = [gather(t, order)[..., list(order)].contiguous() for t in win]
    del rgb, bgra, mos
    out = torch.zeros(J.max_jpeg_bytes(W, H), dtype=torch.uint8, device="cuda")
    fused = {k: [] for k in keys}
    floor = {k: [] for k in keys}
    work = {k: {"pass": [], "k1": []} for k in keys}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def k1(enc, t, **kw):
        enc.encode_tensor(t, Q, out=out, **kw)
        return enc.timing()["fdct"]

    with J.Encoder(0, lanes=1) as enc:
        enc.set_timing(1)
        for p in range(args.warmup + args.passes):
            for i in range(N):
                for k in keys:  # the settings in turn
                    kw, src, wsrc, order = rows[k]
                    enc.set_channel_lut(lut)
                    a = k1(enc, src[i], **kw)
                    enc.set_channel_lut(None)
                    b = k1(enc, pre[k][i], layout="hwc")
                    win = (wsrc if wsrc is not None else src)[i]
                    ev[0].record()
                    d = gather(win, order)
                    ev[1].record()
                    wkw = {"layout": "hwc"} if wsrc is not None else kw
                    c = k1(enc, d, **wkw)
                    torch.cuda.synchronize()
                    if p >= args.warmup:
                        fused[k].append(a)
                        floor[k].append(b)
                        work[k]["pass"].append(ev[0].elapsed_time(ev[1]))
                        work[k]["k1"].append(c)

    def stat(v):
        q = statistics.quantiles(v, n=10)
        return {"ms_median": round(statistics.median(v), 5), "ms_p10": round(q[0], 5), "ms_p90": round(q[-1], 5)}

    res = {"what": "K1 (fdct) kernel time with the per-channel lookup tables inside it, of its floor (K1 without tables as "
                   "RGB8 on the pre-mapped frame M) and of the workaround (a torch gather pass, by its own events, plus K1 "
                   "without tables on its output); 1-lane encoder, device input",
           "quality": Q, "subsampling": 420, "picture_kind": 0, "distinct_inputs": N, "passes": args.passes,
           "samples_per_setting": len(fused[keys[0]]), "device": torch.cuda.get_device_name(0), "rows": {}}
    for k in keys:
        total = [a + b for a, b in zip(work[k]["pass"], work[k]["k1"])]
        res["rows"][k] = {
            "source": [W, H], "fused_k1": stat(fused[k]), "floor_k1_rgb8_on_M": stat(floor[k]),
            "workaround": {"torch_pass": stat(work[k]["pass"]), "k1_on_its_output": stat(work[k]["k1"]), "sum": stat(total)},
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
