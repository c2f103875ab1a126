#!/usr/bin/env python3
"""JPGE_HUFF_OPTIMAL next to JPGE_HUFF_STANDARD (jpge_set_huffman) on the benchmark's
workloads: the same frames, the same context, the two modes alternating in one process
(`--pairs` interleaved pairs, so that drift hits both alike).  bench.py keeps measuring the
default mode; this tool records what the other mode changes.

  throughput   GPix/s of encode_batch from and to device memory: 3840x2160 Q90 (a step of
               --frames-4k frames over --distinct-4k inputs) and the batch of 256 distinct
               1920x1080 Q90 frames (bench.py's seeds);
  host CPU     process CPU seconds (user + system, every thread) per second of those steps;
  latency      one 3840x2160 frame per jpge_encode_rgb8 call on a 1-lane context, device
               input and output: median and p99 of the call's wall time;
  K2           the statistics kernel's time per launch of a set of 4 frames, alone on the
               GPU (a 1-lane context, every launch with its own dispatch-bound events:
               jpge_set_timing(1)), for the instance with histograms and the one without;
  size         bytes(STANDARD) / bytes(OPTIMAL) over the 4K inputs at Q50, Q90 and Q100.

Prints one JSON line; --out also writes it to a file.

    python tools/huffman_modes.py --out profiles/huffman_modes.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402,F401
import torch  # noqa: E402  (before libjpge: one HIP runtime per process)

import jpgenc_amd as J  # noqa: E402

MODES = (("optimal", J.JPGE_HUFF_OPTIMAL), ("standard", J.JPGE_HUFF_STANDARD))


def cpu_s() -> float:
    t = os.times()
    return t.user + t.system


def cap_of(w, h):  # (bench.py's output slots)
    return min(J.max_jpeg_bytes(w, h), (w * h * 3 // 2 + 4095) // 4096 * 4096)


def med(v):
    return round(statistics.median(v), 4)


def throughput(enc, frames, outd, npx, quality, steps, pairs, warmup):
    """Per mode: GPix/s and host CPUs of `steps` encode_batch calls, `pairs` times, alternating."""
    res = {k: {"gpix_s": [], "host_cpus": [], "bytes_per_step": None} for k, _ in MODES}
    for k, m in MODES:
        enc.set_huffman(m)
        for _ in range(warmup):
            enc.encode_batch_dev(frames, outd, quality=quality)
    for _ in range(pairs):
        for k, m in MODES:
            enc.set_huffman(m)
            enc.encode_batch_dev(frames, outd, quality=quality)  # (the mode's first step: slots refill their headers)
            torch.cuda.synchronize()
            c0, t0 = cpu_s(), time.perf_counter()
            for _ in range(steps):
                lens = enc.encode_batch_dev(frames, outd, quality=quality)
            dt, dc = time.perf_counter() - t0, cpu_s() - c0
            res[k]["gpix_s"].append(round(npx * steps / dt / 1e9, 3))
            res[k]["host_cpus"].append(round(dc / dt, 3))
            res[k]["bytes_per_step"] = int(sum(lens))
    enc.set_huffman(J.JPGE_HUFF_OPTIMAL)
    for k, _ in MODES:
        res[k]["gpix_s_median"] = med(res[k]["gpix_s"])
        res[k]["host_cpus_median"] = med(res[k]["host_cpus"])
    res["standard_over_optimal_gpix"] = round(res["standard"]["gpix_s_median"] / res["optimal"]["gpix_s_median"], 4)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=4, help="interleaved (optimal, standard) pairs per line")
    ap.add_argument("--frames-4k", type=int, default=512)
    ap.add_argument("--distinct-4k", type=int, default=16)
    ap.add_argument("--frames-1080", type=int, default=256)
    ap.add_argument("--steps-4k", type=int, default=60)
    ap.add_argument("--steps-1080", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--latency-calls", type=int, default=3000, help="calls per mode and pair")
    ap.add_argument("--solo-batches", type=int, default=40)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("huffman_modes: no GPU (a measurement does not fall back)")
    if args.pairs < 3:
        sys.exit("huffman_modes: at least three interleaved pairs")
    q = args.quality
    res = {"what": "JPGE_HUFF_OPTIMAL vs JPGE_HUFF_STANDARD, the same frames and context, modes alternating in one "
                   "process", "device": torch.cuda.get_device_name(0), "quality": q, "pairs": args.pairs}

    # ---- inputs ----
    W4, H4, W2, H2 = 3840, 2160, 1920, 1080
    D4 = max(1, min(args.distinct_4k, args.frames_4k))
    in4 = [torch.from_numpy(J.synth_rgb8(1 + i, W4, H4).reshape(-1)).cuda() for i in range(D4)]
    in2 = [torch.from_numpy(J.synth_rgb8(1000 + i, W2, H2).reshape(-1)).cuda() for i in range(args.frames_1080)]
    cap4, cap2 = cap_of(W4, H4), cap_of(W2, H2)
    out4 = torch.empty(args.frames_4k * cap4, dtype=torch.uint8, device="cuda")
    out2 = torch.empty(args.frames_1080 * cap2, dtype=torch.uint8, device="cuda")
    fr4 = [(in4[i % D4].data_ptr(), W4, H4, W4 * 3) for i in range(args.frames_4k)]
    od4 = [(out4.data_ptr() + i * cap4, cap4) for i in range(args.frames_4k)]
    fr2 = [(t.data_ptr(), W2, H2, W2 * 3) for t in in2]
    od2 = [(out2.data_ptr() + i * cap2, cap2) for i in range(args.frames_1080)]

    # ---- throughput and host CPU (the default lanes) ----
    with J.Encoder(0) as enc:
        res["lanes"] = enc.lanes()
        res["4k"] = throughput(enc, fr4, od4, float(W4 * H4 * args.frames_4k), q, args.steps_4k, args.pairs, args.warmup)
        res["4k"].update(frames_per_step=args.frames_4k, distinct=D4, steps=args.steps_4k)
        res["batch1080"] = throughput(enc, fr2, od2, float(W2 * H2 * args.frames_1080), q, args.steps_1080, args.pairs,
                                      args.warmup)
        res["batch1080"].update(frames_per_step=args.frames_1080, distinct=args.frames_1080, steps=args.steps_1080)

        # ---- size ----
        size = {}
        for qq in (50, 90, 100):
            n = {}
            for k, m in MODES:
                enc.set_huffman(m)
                n[k] = int(sum(enc.encode_batch_dev(fr4[:D4], od4[:D4], quality=qq)))
            size[f"q{qq}"] = {"optimal_bytes": n["optimal"], "standard_bytes": n["standard"],
                              "standard_over_optimal": round(n["standard"] / n["optimal"], 4)}
        enc.set_huffman(J.JPGE_HUFF_OPTIMAL)
        res["size_4k_inputs"] = size

    # ---- single-image latency (1 lane, device in and out) ----
    with J.Encoder(0, lanes=1) as lone:
        lat = {k: [] for k, _ in MODES}
        for k, m in MODES:
            lone.set_huffman(m)
            for i in range(20):
                lone.encode_ptr(in4[i % D4].data_ptr(), W4, H4, W4 * 3, out4.data_ptr(), cap4, quality=q)
        for _ in range(args.pairs):
            for k, m in MODES:
                lone.set_huffman(m)
                lone.encode_ptr(in4[0].data_ptr(), W4, H4, W4 * 3, out4.data_ptr(), cap4, quality=q)
                torch.cuda.synchronize()
                for i in range(args.latency_calls):
                    t0 = time.perf_counter()
                    lone.encode_ptr(in4[i % D4].data_ptr(), W4, H4, W4 * 3, out4.data_ptr(), cap4, quality=q)
                    lat[k].append((time.perf_counter() - t0) * 1e6)
                torch.cuda.synchronize()
        res["latency_4k_us"] = {}
        for k, _ in MODES:
            v = sorted(lat[k])
            res["latency_4k_us"][k] = {"median": round(statistics.median(v), 2), "p99": round(v[int(0.99 * (len(v) - 1))], 2),
                                       "p10": round(v[int(0.10 * (len(v) - 1))], 2), "calls": len(v)}

    # ---- K2 alone, per set of 4 (bench.py's solo shape: a 1-lane context in frame sets) ----
    env = {"JPGE_SET": "4", "JPGE_EXT_PLACE": "1"}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        solo = J.Encoder(0, lanes=1)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    k2 = {}
    try:
        for name, fr, od in (("4k", fr4[:32], od4[:32]), ("1080p", fr2[:64], od2[:64])):
            k2[name] = {k: [] for k, _ in MODES}
            for k, m in MODES:
                solo.set_huffman(m)
                for _ in range(4):
                    solo.encode_batch_dev(fr, od, quality=q)
            for _ in range(args.pairs):
                for k, m in MODES:
                    solo.set_huffman(m)
                    solo.encode_batch_dev(fr, od, quality=q)
                    solo.set_timing(1)
                    solo.reset_timing()
                    for _ in range(args.solo_batches):
                        solo.encode_batch_dev(fr, od, quality=q)
                    tm = solo.timing()
                    solo.set_timing(0)
                    k2[name][k].append({"k2_us_per_set": round(tm["dc_stats_sum"] / tm["launches"] * 1e3, 3),
                                        "k1_us_per_set": round(tm["fdct_sum"] / tm["launches"] * 1e3, 3),
                                        "entropy_us_per_set": round(tm["entropy_sum"] / tm["launches"] * 1e3, 3),
                                        "frames_per_launch": round(tm["frames"] / tm["launches"], 2)})
            for k, _ in MODES:
                k2[name][k + "_k2_us_per_set_median"] = med([r["k2_us_per_set"] for r in k2[name][k]])
            k2[name]["standard_over_optimal_k2"] = round(k2[name]["standard_k2_us_per_set_median"] /
                                                         k2[name]["optimal_k2_us_per_set_median"], 4)
    finally:
        solo.close()
    res["k2_solo"] = k2

    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
