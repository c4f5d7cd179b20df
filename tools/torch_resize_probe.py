#!/usr/bin/env python3
"""fid_score --mode pytorch-fid's float route (tise_resize_torch_f32 + the fp32 stem + trunk) beside --mode torch-fidelity's
(tise_resize_tf1_f32 + the same stem and trunk) and the reference's uint8 route (the uint8 resize + the uint8 stem + the same
trunk) on the SAME resident batch of 256 x 256 images, Inception-2015, seeded parameters: the three alternate in one process,
7 timed rounds of 4 passes each after warm-up, median and spread (max - min) of the rounds, images/s; then the three resize
launches alone, with their algorithmic bytes (h*w*3 read + oh*ow*12 written for the float kernels, oh*ow*3 written for the
uint8 one) over the time.  tise_resize_tf1_f32 is the yardstick of the new kernel: the same bytes, the same gather.

    python tools/torch_resize_probe.py [--rounds 7] [--batches 50 1000] [--only torch|tf1|uint8]  > profiles/r17a_torch_resize_probe.txt

--only torch with --rounds 1 is the target of a separate `rocprofv3 --kernel-trace --stats` pass (the kernels' own times:
profiles/r17b_torch_resize_kernel_stats.txt)."""
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
RESIZE = {"torch": "torch", "tf1": "tf1", "uint8": "reference"}            # route -> RealismEngine(resize=...)


def timed(fns, rounds, iters):
    times = {k: [] for k in fns}
    for f in fns.values():                                                 # warm-up: plans, allocator, code objects
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
        bw = f"  {unit_bytes[k] * batch / med / 1e9:7.1f} GB/s algorithmic" if unit_bytes else ""
        print(f"  {k:6s} median {med * 1e3:8.3f} ms  spread {(max(ts) - min(ts)) * 1e3:6.3f} ms  min {min(ts) * 1e3:8.3f}  max {max(ts) * 1e3:8.3f}"
              f"  -> {batch / med:9.1f} images/s{bw}")
    for other in ("tf1", "uint8"):
        if "torch" in times and other in times:
            a, b = statistics.median(times["torch"]), statistics.median(times[other])
            both = sum(max(times[k]) - min(times[k]) for k in ("torch", other))
            print(f"  torch / {other} = {a / b:.3f}; difference {(a - b) * 1e3:+.3f} ms against the two spreads together {both * 1e3:.3f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batches", type=int, nargs="+", default=[50, 1000])
    ap.add_argument("--iters", type=int, default=4, help="passes per timed round")
    ap.add_argument("--only", choices=list(RESIZE), default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    engines = {k: RealismEngine(dims=2048, seed=0, network=NET, resize=r) for k, r in RESIZE.items() if args.only in (None, k)}
    g = torch.Generator(device="cpu").manual_seed(0)
    print(f"Inception-2015, seeded parameters, 256 x 256 resident uint8 images, {args.rounds} rounds of {args.iters} passes")
    for batch in args.batches:
        x = torch.randint(0, 256, (batch, 256, 256, 3), dtype=torch.uint8, generator=g).to(dev)
        with torch.no_grad():
            print(f"batch {batch}: resize + trunk (features_from_u8)")
            report(timed({k: (lambda e=e: e.features_from_u8(x)) for k, e in engines.items()}, args.rounds, args.iters), batch)
            print(f"batch {batch}: the resize launch alone")
            alone = {"torch": lambda: device.resize_torch_f32(x, (299, 299)), "tf1": lambda: device.resize_tf1_f32(x, (299, 299)),
                     "uint8": lambda: device.resize_u8_only(x, (299, 299))}
            nbytes = {"torch": 256 * 256 * 3 + 299 * 299 * 12, "tf1": 256 * 256 * 3 + 299 * 299 * 12, "uint8": 256 * 256 * 3 + 299 * 299 * 3}
            report(timed({k: alone[k] for k in engines}, args.rounds, args.iters * 4), batch, nbytes)


if __name__ == "__main__":
    main()
