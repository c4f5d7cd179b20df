#!/usr/bin/env python3
"""fid_score --mode clean's float route (tise_resize_f32 + the fp32 stem + trunk) against the reference's uint8 route (the uint8
resize + the uint8 stem + the same trunk) on the SAME resident batch of 256 x 256 images, Inception-2015, seeded parameters:
the two alternate in one process, at least 5 timed rounds each after warm-up, median and spread (max - min) of the rounds,
images/s; then the two resize launches alone, with their algorithmic bytes (h*w*3 read + oh*ow*12 written for the float
kernel, oh*ow*3 written for the uint8 one) over the time.

    python tools/clean_resize_probe.py [--rounds 7] [--batches 50 1000] [--only clean|reference]  > profiles/r13a_clean_resize_probe.txt

--only clean with --rounds 1 is the target of a separate `rocprofv3 --kernel-trace --stats` pass (the per-kernel split:
profiles/r13b_clean_resize_kernel_stats.txt)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tise_toolbox_amd import device
from tise_toolbox_amd.engine import RealismEngine

NET = "inception-2015"


def timed(fns, rounds, iters):
    times = {k: [] for k in fns}
    for f in fns.values():                                                 # warm-up: plans, allocator, code objects
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, f in fns.items():                                           # alternating: both see the same clocks
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                f()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / iters)
    return times


def report(times, batch, unit_bytes=None):
    for k, ts in times.items():
        med = statistics.median(ts)
        bw = f"  {unit_bytes[k] * batch / med / 1e9:7.1f} GB/s algorithmic" if unit_bytes else ""
        print(f"  {k:10s} median {med * 1e3:8.3f} ms  spread {(max(ts) - min(ts)) * 1e3:6.3f} ms  min {min(ts) * 1e3:8.3f}  max {max(ts) * 1e3:8.3f}"
              f"  -> {batch / med:9.1f} images/s{bw}")
    if len(times) == 2:
        c, r = statistics.median(times["clean"]), statistics.median(times["reference"])
        both = sum(max(ts) - min(ts) for ts in times.values())
        print(f"  clean / reference = {c / r:.3f}; difference {abs(c - r) * 1e3:.3f} ms against the two spreads together {both * 1e3:.3f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batches", type=int, nargs="+", default=[50, 1000])
    ap.add_argument("--iters", type=int, default=4, help="passes per timed round")
    ap.add_argument("--only", choices=["clean", "reference"], default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    engines = {k: RealismEngine(dims=2048, seed=0, network=NET, resize=k) for k in ("clean", "reference") if args.only in (None, k)}
    g = torch.Generator(device="cpu").manual_seed(0)
    print(f"Inception-2015, seeded parameters, 256 x 256 resident uint8 images, {args.rounds} rounds of {args.iters} passes")
    for batch in args.batches:
        x = torch.randint(0, 256, (batch, 256, 256, 3), dtype=torch.uint8, generator=g).to(dev)
        with torch.no_grad():
            print(f"batch {batch}: resize + trunk (features_from_u8)")
            report(timed({k: (lambda e=e: e.features_from_u8(x)) for k, e in engines.items()}, args.rounds, args.iters), batch)
            print(f"batch {batch}: the resize launch alone")
            alone = {"clean": lambda: device.resize_f32(x, (299, 299)), "reference": lambda: device.resize_u8_only(x, (299, 299))}
            nbytes = {"clean": 256 * 256 * 3 + 299 * 299 * 12, "reference": 256 * 256 * 3 + 299 * 299 * 3}
            report(timed({k: alone[k] for k in engines}, args.rounds, args.iters * 4), batch, nbytes)


if __name__ == "__main__":
    main()
