#!/usr/bin/env python3
"""The ADM suite's device route (adm_eval: tise_resize_tf1_f32 + the fp32 stem + trunk [+ tise_split_tap_rows + the spatial
fp64 accumulator]) against the reference's uint8 route on the SAME resident batch of seeded 256 x 256 uint8 images,
Inception-2015, seeded parameters, batch 1000.  Three routes alternate in one process -- resize="tf1" with spatial=True,
resize="tf1" alone, the uint8 route -- each a whole step (features + the pool3 statistics update [+ the spatial one]), 7 timed
rounds after warm-up, median and spread (max - min), images/s; then the TF1 resize launch alone with its algorithmic bytes
(h*w*3 read + oh*ow*12 written) over the time.

    python tools/adm_probe.py [--rounds 7] [--batch 1000] [--only tf1+spatial|tf1|uint8]  > profiles/r14a_adm_probe.txt

--only tf1+spatial with --rounds 1 is the target of a separate `rocprofv3 --kernel-trace --stats` pass (the per-kernel times of
tise_resize_tf1_f32, tise_split_tap_rows and the spatial accumulator update: profiles/r14b_adm_kernel_stats.txt)."""
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
ROUTES = {"tf1+spatial": dict(resize="tf1", spatial=True), "tf1": dict(resize="tf1"), "uint8": dict()}


def timed(fns, rounds, iters):
    times = {k: [] for k in fns}
    for f in fns.values():                                                 # warm-up: allocator, code objects
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


def report(times, batch, unit_bytes=None):
    for k, ts in times.items():
        med = statistics.median(ts)
        bw = f"  {unit_bytes * batch / med / 1e9:7.1f} GB/s algorithmic" if unit_bytes else ""
        print(f"  {k:12s} median {med * 1e3:8.3f} ms  spread {(max(ts) - min(ts)) * 1e3:6.3f} ms  min {min(ts) * 1e3:8.3f}  max {max(ts) * 1e3:8.3f}"
              f"  -> {batch / med:9.1f} images/s{bw}")
    if "uint8" in times:
        base = statistics.median(times["uint8"])
        for k in times:
            if k != "uint8":
                m = statistics.median(times[k])
                both = (max(times[k]) - min(times[k])) + (max(times["uint8"]) - min(times["uint8"]))
                print(f"  {k} / uint8 = {m / base:.3f}; difference {abs(m - base) * 1e3:.3f} ms against the two spreads together {both * 1e3:.3f} ms")
    if "tf1+spatial" in times and "tf1" in times:
        a, b = statistics.median(times["tf1+spatial"]), statistics.median(times["tf1"])
        both = sum(max(times[k]) - min(times[k]) for k in ("tf1+spatial", "tf1"))
        print(f"  tf1+spatial - tf1 = {(a - b) * 1e3:.3f} ms (tap + spatial accumulator) against the two spreads together {both * 1e3:.3f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=4, help="steps per timed round")
    ap.add_argument("--only", choices=list(ROUTES), default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    engines = {k: RealismEngine(dims=2048, seed=0, network=NET, **kw) for k, kw in ROUTES.items() if args.only in (None, k)}
    g = torch.Generator(device="cpu").manual_seed(0)
    batch = args.batch
    x = torch.randint(0, 256, (batch, 256, 256, 3), dtype=torch.uint8, generator=g).to(dev)
    print(f"Inception-2015, seeded parameters, {batch} resident 256 x 256 uint8 images, {args.rounds} rounds of {args.iters} steps")
    for e in engines.values():
        e.begin()
    with torch.no_grad():
        print(f"batch {batch}: a whole step (resize + trunk + fp64 statistics update{'s' if 'tf1+spatial' in engines else ''})")
        report(timed({k: (lambda e=e: e.step_u8(x)) for k, e in engines.items()}, args.rounds, args.iters), batch)
        if args.only in (None, "tf1"):
            print(f"batch {batch}: the TF1 resize launch alone")
            report(timed({"tf1 resize": lambda: device.resize_tf1_f32(x, (299, 299))}, args.rounds, args.iters * 4), batch,
                   256 * 256 * 3 + 299 * 299 * 12)


if __name__ == "__main__":
    main()
