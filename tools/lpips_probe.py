#!/usr/bin/env python3
"""LPIPS (VGG-16) of 50 resident seeded 256 x 256 uint8 pairs: this project's route (lpips_hip.HipLpips: split-precision
convolutions, csrc/lpips.hip) alternating with lpips_model.LpipsVGG16 on the library's kernels on the same GPU -- fp32, and
fp16 under autocast --, 7 timed rounds after warm-up, median and spread (max - min) of the rounds, pairs/s, and how far each route
is from the module's fp64 forward on the first 4 pairs.  Seeded stand-in parameters: rates only.

    python tools/lpips_probe.py [--rounds 7] [--batch 50] [--size 256] [--only hip|torch32|torch16]  > profiles/r19a_lpips_probe.txt

--only hip with --rounds 1 is the target of a separate `rocprofv3 --kernel-trace --stats` pass; `--summarize DIR` condenses that
pass's output (kernel_stats.csv or the rocpd database) into the table of profiles/r19b_lpips_kernel_stats.txt."""
import argparse
import collections
import csv
import glob
import os
import re
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fns, rounds, iters):
    import torch
    times = {k: [] for k in fns}
    for f in fns.values():                                                 # warm-up: allocator, code objects, fall-back packings
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, f in fns.items():                                           # alternating: all see the same clocks
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                f()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / iters)
    return times


def report(times, batch):
    for k, ts in times.items():
        med = statistics.median(ts)
        print(f"  {k:8s} median {med * 1e3:9.3f} ms  spread {(max(ts) - min(ts)) * 1e3:7.3f} ms  min {min(ts) * 1e3:9.3f}  max {max(ts) * 1e3:9.3f}"
              f"  -> {batch / med:9.1f} pairs/s")
    if "hip" in times:
        a = statistics.median(times["hip"])
        for k in times:
            if k != "hip":
                b = statistics.median(times[k])
                both = max(times["hip"]) - min(times["hip"]) + max(times[k]) - min(times[k])
                print(f"  hip / {k} = {a / b:.3f}; difference {(a - b) * 1e3:+.3f} ms against the two spreads together {both * 1e3:.3f} ms")


def summarize(d):
    per = collections.defaultdict(list)
    dbs = glob.glob(os.path.join(d, "**", "*_results.db"), recursive=True)
    traces = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if traces:
        for r in csv.DictReader(open(traces[0])):
            per[r["Kernel_Name"]].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    elif dbs:
        import sqlite3
        for n, s0, e0 in sqlite3.connect(dbs[0]).execute("select name, start, end from kernels"):
            per[n].append(e0 - s0)
    else:
        raise SystemExit(f"no kernel trace under {d}")
    total = sum(sum(v) for v in per.values())
    print(f"{'kernel':70s} {'calls':>6s} {'total ms':>10s} {'avg us':>9s} {'min us':>9s} {'max us':>9s} {'share %':>8s}")
    for n, v in sorted(per.items(), key=lambda kv: -sum(kv[1])):
        m = re.match(r"_ZN12_GLOBAL__N_1(\d+)", n)                           # a template instance rocprofv3 left mangled
        name = n[m.end():m.end() + int(m.group(1))] if m else n.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0][:70]
        print(f"{name:70s} {len(v):6d} {sum(v) / 1e6:10.3f} {sum(v) / len(v) / 1e3:9.1f} {min(v) / 1e3:9.1f} {max(v) / 1e3:9.1f} {100.0 * sum(v) / total:8.2f}")
    print(f"{'all kernels':70s} {'':6s} {total / 1e6:10.3f}")


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
        return summarize(args.summarize)
    import numpy as np
    import torch
    from tise_toolbox_amd import lpips_model
    from tise_toolbox_amd.lpips_hip import HipLpips
    dev = torch.device("cuda:0")
    h = w = args.size
    g = torch.Generator().manual_seed(0)
    base = torch.nn.functional.avg_pool2d(torch.randn((args.batch, 3, h + 8, w + 8), generator=g), 9, 1)
    x = ((base - base.amin()) / (base.amax() - base.amin()) * 255.0).round()
    y = (x + 10.0 * torch.randn(x.shape, generator=g)).round().clamp(0, 255)
    x, y = (t.permute(0, 2, 3, 1).contiguous().to(torch.uint8).to(dev) for t in (x, y))
    model = lpips_model.LpipsVGG16().init_synthetic(0)
    hip = HipLpips(model, dev)
    on_gpu = lpips_model.LpipsVGG16().init_synthetic(0).to(dev)

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
        m64 = lpips_model.LpipsVGG16().init_synthetic(0).double()
        with torch.no_grad():
            want = m64(x[:4].cpu(), y[:4].cpu()).numpy()
        for k, f in fns.items():
            got = f()[:4]
            print(f"  {k:8s} worst |value - fp64 module| over 4 pairs = {np.abs(got - want).max():.3e} (values {want.min():.4f} .. {want.max():.4f})")
    report(timed(fns, args.rounds, args.iters), args.batch)


if __name__ == "__main__":
    main()
