#!/usr/bin/env python
"""Times the four band passes (split, split backward, merge, merge backward; csrc/bands.hip) against the same transforms
written with torch.fft on the device -- the stock path -- with device events after a warm-up, at the training shape
(B = 32, N = 8192, m = 512), the inference shape (B = 1, N = 32768, m = 2048) and, for the grid choice, B = 256 at
N = 8192.  The two analysis passes are timed on both grids: one workgroup per row, and one per (row, band)
(MSYNTH_BAND_SPLIT).

    python tools/band_timing.py --out profiles/bands_timing.json
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- \\
        python tools/band_timing.py --shape train --no-ab --iters 20                             (kernel tracing only)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "music-synthesis_amd"), ROOT):
    sys.path.insert(0, p)

import torch  # noqa: E402

import bands_ref as R  # noqa: E402
from featuresynth._ops import bands as HB  # noqa: E402

SHAPES = [("train", 32, 8192, 512), ("inference", 1, 32768, 2048), ("batch256", 256, 8192, 512)]


def timed(fn, warmup, iters):
    """-> microseconds per call"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", choices=[s[0] for s in SHAPES], default=None, help="one shape only (a profiler run)")
    ap.add_argument("--no-ab", action="store_true", help="skip the forced-grid A/B of the analysis passes")
    args = ap.parse_args()
    assert torch.cuda.is_available()
    result = {"device": torch.cuda.get_device_name(0), "unit": "microseconds per call", "warmup": args.warmup,
              "iters": args.iters, "shapes": {}}
    for name, B, N, m in SHAPES:
        if args.shape not in (None, name):
            continue
        sizes = R.band_sizes(N, m)
        gen = torch.Generator(device="cuda").manual_seed(N)
        x = torch.randn(B, 1, N, device="cuda", generator=gen)
        bands = [torch.randn(B, 1, S, device="cuda", generator=gen) for S in sizes]
        gy = torch.randn(B, 1, N, device="cuda", generator=gen)
        row = {"B": B, "N": N, "min_size": m}
        for grid in (() if args.no_ab else ("row", "row_band")):
            os.environ["MSYNTH_BAND_SPLIT"] = "0" if grid == "row" else "1"
            row["hip_split_fwd_" + grid] = timed(lambda: HB.analysis("ms_band_decompose_fwd", x, sizes, True), args.warmup, args.iters)
            row["hip_merge_bwd_" + grid] = timed(lambda: HB.analysis("ms_band_recompose_bwd", gy, sizes, True), args.warmup, args.iters)
        os.environ.pop("MSYNTH_BAND_SPLIT", None)
        row["hip_split_fwd_default"] = timed(lambda: HB.analysis("ms_band_decompose_fwd", x, sizes, True), args.warmup, args.iters)
        row["hip_merge_bwd_default"] = timed(lambda: HB.analysis("ms_band_recompose_bwd", gy, sizes, True), args.warmup, args.iters)
        row["hip_merge_fwd"] = timed(lambda: HB.synthesis("ms_band_recompose_fwd", bands, sizes, True, N), args.warmup, args.iters)
        row["hip_split_bwd"] = timed(lambda: HB.synthesis("ms_band_decompose_bwd", bands, sizes, True, N), args.warmup, args.iters)
        # the stock path: torch.fft forward, autograd backward
        xs = x.clone().requires_grad_(True)
        bs = {S: b.clone().requires_grad_(True) for S, b in zip(sizes, bands)}
        row["stock_split_fwd"] = timed(lambda: R.decompose(x, m), args.warmup, args.iters)
        row["stock_merge_fwd"] = timed(lambda: R.recompose(dict(zip(sizes, bands)), N), args.warmup, args.iters)
        outs = R.decompose(xs, m)
        row["stock_split_bwd"] = timed(lambda: torch.autograd.grad([outs[S] for S in sizes], xs, bands, retain_graph=True),
                                       args.warmup, args.iters)
        y = R.recompose(bs, N)
        row["stock_merge_bwd"] = timed(lambda: torch.autograd.grad(y, [bs[S] for S in sizes], gy, retain_graph=True),
                                       args.warmup, args.iters)
        result["shapes"][name] = {k: (round(v, 2) if isinstance(v, float) else v) for k, v in row.items()}
    text = json.dumps(result, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
