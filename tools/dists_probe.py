#!/usr/bin/env python3
"""DISTS of 50 resident seeded 256 x 256 uint8 pairs: this project's route (dists_hip.HipDists: split-precision convolutions,
csrc/dists.hip) alternating with dists_model.DistsVGG16 on the library's kernels on the same GPU -- fp32, and fp16 under
autocast --, 7 timed rounds after warm-up, median and spread (max - min) of the rounds, pairs/s, and how far each route is from the
module's fp64 forward on the first 4 pairs.  Seeded stand-in parameters: rates only.

    python tools/dists_probe.py [--rounds 7] [--batch 50] [--size 256] [--only hip|torch32|torch16]  > profiles/r20a_dists_probe.txt

--only hip with --rounds 1 is the target of a separate `rocprofv3 --kernel-trace --stats` pass (no counters, no other tracing);
`--summarize DIR` condenses that pass's output into the table of profiles/r20b_dists_kernel_stats.txt and adds, per kernel of
csrc/dists.hip, every call's duration in launch order (the sibling of tools/lpips_probe.py, whose timing and summary code this
imports)."""
import argparse
import csv
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from lpips_probe import report, summarize, timed  # noqa: E402

OWN = ("l2pool3s2_split_kernel", "dists_sum_kernel", "dists_mean_kernel", "dists_center_kernel", "dists_finish_kernel",
       "dists_image_sums_kernel", "lpips_input_kernel")


def own_kernels(d):
    """Every call of this route's own kernels in launch order, in us (kernel_trace.csv of the pass)."""
    traces = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not traces:
        return
    rows = sorted(csv.DictReader(open(traces[0])), key=lambda r: int(r["Start_Timestamp"]))
    for name in OWN:
        ts = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if name in r["Kernel_Name"]]
        if ts:
            print(f"{name:28s} {len(ts):4d} calls, us in launch order: " + " ".join(f"{t:.1f}" for t in ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--iters", type=int, default=2, help="calls per timed round")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--only", choices=["hip", "torch32", "torch16"], default=None)
    ap.add_argument("--summarize", default=None, metavar="DIR")
    args = ap.parse_args()
    if args.summarize:
        summarize(args.summarize)
        return own_kernels(args.summarize)
    import numpy as np
    import torch
    from tise_toolbox_amd import dists_model
    from tise_toolbox_amd.dists_hip import HipDists
    dev = torch.device("cuda:0")
    h = w = args.size
    g = torch.Generator().manual_seed(0)
    base = torch.nn.functional.avg_pool2d(torch.randn((args.batch, 3, h + 8, w + 8), generator=g), 9, 1)
    x = ((base - base.amin()) / (base.amax() - base.amin()) * 255.0).round()
    y = (x + 10.0 * torch.randn(x.shape, generator=g)).round().clamp(0, 255)
    x, y = (t.permute(0, 2, 3, 1).contiguous().to(torch.uint8).to(dev) for t in (x, y))
    model = dists_model.DistsVGG16().init_synthetic(0)
    hip = HipDists(model, dev)
    on_gpu = dists_model.DistsVGG16().init_synthetic(0).to(dev)

    def torch32():
        with torch.no_grad():
            return on_gpu(x, y).double().cpu().numpy()

    def torch16():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            return on_gpu(x, y).double().cpu().numpy()
    fns = {"hip": lambda: hip(x, y), "torch32": torch32, "torch16": torch16}
    fns = {k: f for k, f in fns.items() if args.only in (None, k)}
    print(f"{args.batch} resident {h} x {w} uint8 pairs (smooth, seeded; seeded stand-in parameters), {args.rounds} rounds of {args.iters} calls; "
          f"a call ends with the read-back of the {args.batch} values")
    if args.only is None:
        m64 = dists_model.DistsVGG16().init_synthetic(0).double()
        with torch.no_grad():
            want = m64(x[:4].cpu(), y[:4].cpu()).numpy()
        for k, f in fns.items():
            got = f()[:4]
            print(f"  {k:8s} worst |value - fp64 module| over 4 pairs = {np.abs(got - want).max():.3e} (values {want.min():.4f} .. {want.max():.4f})")
    report(timed(fns, args.rounds, args.iters), args.batch)


if __name__ == "__main__":
    main()
