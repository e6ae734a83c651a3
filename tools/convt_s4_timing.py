#!/usr/bin/env python
"""Times the stride-4 transposed conv (ConvTranspose1d k = 8, stride 4, padding 2, bias-free + LeakyReLU: LearnedUpSample of
the multi-scale band generator) on its phase-split matrix-pipe routes against the direct kernels the same calls ran on
before -- the same build with MSYNTH_CONVT_S4=0, which dispatches those kernels unchanged -- for the four generator shapes at
B = 32 and the three passes each, and one D + G trainer pair of MultiScaleWithDeRecompose at B = 32 x 8192 samples.

Every side of every round runs in a fresh child process (the switch is read per call, but code objects, the allocator and the
captured graphs are per process); the two sides alternate, `--rounds` times, and the medians over the rounds are compared.
Times are device events around `--iters` back-to-back calls after `--warmup` calls of the same shape.

    python tools/convt_s4_timing.py --out profiles/convt_s4_timing.json
    python tools/convt_s4_timing.py --profile-dir <dir> --stats-out profiles/multiscale_gan_kernel_stats.csv
        (rocprofv3 --kernel-trace --stats around a child that runs the trainer pair only: kernel tracing, nothing else)
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "music-synthesis_amd"), ROOT):
    sys.path.insert(0, p)

SHAPES = [(32, 512, 32, 256), (32, 256, 128, 128), (32, 128, 512, 64), (32, 64, 2048, 32)]     # B, Cin, Lin, Cout
PASSES = ("fwd", "bwd_data", "bwd_weight")
K, S, PAD = 8, 4, 2
STEP_B, STEP_T, STEP_N = 32, 32, 8192


def timed(fn, warmup, iters):
    """-> microseconds per call"""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters


def child_ops(args):
    import torch
    from featuresynth._ops import prims as P
    out = {}
    for B, Cin, Lin, Cout in SHAPES:
        gen = torch.Generator(device="cuda").manual_seed(Cin)
        x = torch.randn(B, Cin, Lin, device="cuda", generator=gen)
        w = torch.randn(Cin, Cout, K, device="cuda", generator=gen) * 0.02
        d, lo = P.convt_desc(x.shape, w.shape, S, PAD, act=1)
        y = torch.empty(B, Cout, lo, device="cuda")
        gy = torch.randn(B, Cout, lo, device="cuda", generator=gen)
        gx, gw, gb = torch.empty_like(x), torch.empty_like(w), torch.empty(Cout, device="cuda")
        P.convt1d_fwd(x, w, None, d, lo, out=y)
        calls = {"fwd": lambda: P.convt1d_fwd(x, w, None, d, lo, out=y),
                 "bwd_data": lambda: P.convt1d_bwd_data(gy, y, w, d, out=gx),
                 "bwd_weight": lambda: P.convt1d_bwd_weight(x, gy, y, d, w.shape, gw=gw, gb=gb)}
        lib = P.L.load()
        for which, name in enumerate(PASSES):
            out["%dx%dx%d->%d/%s" % (B, Cin, Lin, Cout, name)] = {
                "us": timed(calls[name], args.warmup, args.iters),
                "kernel": lib.ms_convt1d_kernel_name(d, which).decode(),
                "mac": B * Cin * Lin * Cout * K}
    return out


def child_step(args):
    """one D + G trainer pair, replayed from the captured graphs"""
    import torch
    from featuresynth._synthetic import synthetic_features, synthetic_samples
    from featuresynth.experiment import MultiScaleWithDeRecompose
    torch.manual_seed(0)
    exp = MultiScaleWithDeRecompose().to("cuda")
    s = torch.from_numpy(synthetic_samples(STEP_B, STEP_N)).cuda()
    f = torch.from_numpy(synthetic_features(STEP_B, 128, STEP_T)).cuda()

    def pair():
        exp.discriminator_trainer(s, f)
        exp.generator_trainer(s, f)
    us = timed(pair, 3, args.step_iters)          # (call 1 eager, call 2 captures, call 3 replays)
    return {"pair_us": us, "d": exp._d_trainer.graph_status()["mode"], "g": exp._g_trainer.graph_status()["mode"]}


def run_child(what, side, args, wrap=None):
    env = dict(os.environ)
    env.pop("MSYNTH_CONVT_S4", None)
    if side == "parent":
        env["MSYNTH_CONVT_S4"] = "0"
    cmd = [sys.executable, os.path.abspath(__file__), "--child", what, "--warmup", str(args.warmup), "--iters", str(args.iters),
           "--step-iters", str(args.step_iters)]
    out = subprocess.check_output((wrap or []) + cmd, env=env, text=True, timeout=900)
    for line in reversed(out.splitlines()):
        if line.startswith("RESULT "):
            return json.loads(line[len("RESULT "):])
    raise RuntimeError("child printed no result:\n" + out[-2000:])


def kernel_stats(args):
    """rocprofv3 --kernel-trace --stats around the trainer pair; keeps the per-kernel totals"""
    os.makedirs(args.profile_dir, exist_ok=True)
    wrap = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", args.profile_dir, "--"]
    run_child("step", "new", args, wrap)
    found = sorted(glob.glob(os.path.join(args.profile_dir, "**", "*kernel_stats.csv"), recursive=True))
    if not found:
        raise RuntimeError("no kernel_stats.csv under %s" % args.profile_dir)
    rows = list(csv.reader(open(found[-1])))
    with open(args.stats_out, "w", newline="") as fo:
        csv.writer(fo).writerows(rows[:1] + rows[1:61])             # the header and the 60 largest kernels
    print("%s: %d of %d kernels" % (args.stats_out, min(60, len(rows) - 1), len(rows) - 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--step-iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-step", action="store_true", help="the twelve op cells only")
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-dir", default=None, help="run the trainer pair under rocprofv3 --kernel-trace --stats here")
    ap.add_argument("--stats-out", default=os.path.join(ROOT, "profiles", "multiscale_gan_kernel_stats.csv"))
    ap.add_argument("--child", choices=["ops", "step"], default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        import torch
        assert torch.cuda.is_available(), "a measurement needs the GPU"
        res = child_ops(args) if args.child == "ops" else child_step(args)
        print("RESULT " + json.dumps(res))
        return
    if args.profile_dir:
        kernel_stats(args)
        return
    cells, steps = {}, {"new": [], "parent": []}
    for _ in range(args.rounds):
        for side in ("new", "parent"):
            for key, r in run_child("ops", side, args).items():
                c = cells.setdefault(key, {"mac": r["mac"], "new_us": [], "parent_us": []})
                c[side + "_us"].append(round(r["us"], 2))
                c[side + "_kernel"] = r["kernel"]
            if not args.no_step:
                steps[side].append(round(run_child("step", side, args)["pair_us"], 1))
    slower = []
    for key, c in cells.items():
        c["new_median_us"], c["parent_median_us"] = statistics.median(c["new_us"]), statistics.median(c["parent_us"])
        c["speedup"] = round(c["parent_median_us"] / c["new_median_us"], 2)
        c["new_tflops"] = round(2.0 * c["mac"] / c["new_median_us"] * 1e-6, 2)
        if c["new_median_us"] > c["parent_median_us"]:
            slower.append(key)
    result = {"unit": "microseconds per call, device events", "warmup": args.warmup, "iters": args.iters, "rounds": args.rounds,
              "parent_side": "the same build with MSYNTH_CONVT_S4=0 (the direct kernels, unchanged)", "cells": cells,
              "cells_where_the_new_route_is_slower": slower}
    if not args.no_step:
        result["trainer_pair_B32_N8192"] = {
            "unit": "microseconds per D + G pair of MultiScaleWithDeRecompose, graph replay", "new_us": steps["new"],
            "parent_us": steps["parent"], "new_median_us": statistics.median(steps["new"]),
            "parent_median_us": statistics.median(steps["parent"])}
    text = json.dumps(result, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
