#!/usr/bin/env python3
"""ViT-L/14@336 image tower at CMMD's default batch of 50: the hand-written towers (clip_hip.HipTowers) against the fp16 library
module (what TISE_CLIP=torch selects), alternating in one process on the same seeded parameters and the same batch; at least 5
timed rounds each after warm-up, median and spread (max - min) of the rounds, images/s.

    python tools/clip_l14_probe.py [--rounds 7] [--batch 50] [--only hip|torch]

--only hip with one round is the target of a separate `rocprofv3 --kernel-trace --stats` pass (the per-kernel split)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tise_toolbox_amd import clip_hip, clip_model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--iters", type=int, default=4, help="tower passes per timed round")
    ap.add_argument("--only", choices=["hip", "torch"], default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    model = clip_model.build_clip(arch="ViT-L/14@336").to(dev).half()
    towers = clip_hip.HipTowers(model, dev)
    x = torch.randn((args.batch, 3, 336, 336), device=dev, dtype=torch.float16)
    paths = {"hip": towers.encode_image, "torch": lambda t: model.encode_image(t)}
    if args.only:
        paths = {args.only: paths[args.only]}
    times = {k: [] for k in paths}
    with torch.no_grad():
        for f in paths.values():                                           # warm-up: allocator, library kernel selection
            for _ in range(2):
                f(x)
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for k, f in paths.items():                                     # alternating: both see the same clocks
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.iters):
                    f(x)
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) / args.iters)
    print(f"ViT-L/14@336 image tower, batch {args.batch}, {args.rounds} rounds of {args.iters} passes, seeded parameters")
    for k, ts in times.items():
        med = statistics.median(ts)
        print(f"{k:6s} median {med * 1e3:8.2f} ms  spread {(max(ts) - min(ts)) * 1e3:6.2f} ms  min {min(ts) * 1e3:8.2f}  max {max(ts) * 1e3:8.2f}"
              f"  -> {args.batch / med:8.1f} images/s")
    if len(times) == 2:
        h, t = statistics.median(times["hip"]), statistics.median(times["torch"])
        both = (max(times["hip"]) - min(times["hip"])) + (max(times["torch"]) - min(times["torch"]))
        print(f"hip / torch = {h / t:.3f}; difference {abs(h - t) * 1e3:.2f} ms against the two spreads together {both * 1e3:.2f} ms")


if __name__ == "__main__":
    main()
