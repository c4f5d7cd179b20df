#!/usr/bin/env python3
"""DINOv2 ViT-L/14 at FD-DINOv2's default batch of 50 (257 tokens at 224): the hand-written tower (dinov2_hip.HipDino, fp32
residual stream) against the module under torch.autocast(fp16) on library kernels (what TISE_DINO=torch selects), alternating in
one process on the same seeded parameters and the same resident preprocessed batch; 7 timed rounds of 4 passes each after
warm-up, median and spread (max - min) of the rounds, images/s.

It also times what the fp32 stream costs in one GEMM: tise_gemm_f16_res32 (fp32 residual read, LayerScale, fp32 write) against
tise_gemm_f16 with an fp16 residual at the tower's fc2 shape, 12 850 x 1024 x 4096, alternating, the same rounds.

    python tools/dinov2_probe.py [--rounds 7] [--batch 50] [--only hip|torch] [--arch vitl14]

--only hip with one round is the target of a separate `rocprofv3 --kernel-trace --stats` pass (the per-kernel split)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tise_toolbox_amd import clip_hip, dinov2_hip, dinov2_model


def _rounds(paths, rounds, iters):
    times = {k: [] for k in paths}
    for f in paths.values():                                               # warm-up: allocator, library kernel selection
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, f in paths.items():                                         # alternating: both see the same clocks
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                f()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / iters)
    return times


def _report(times, unit, per=None):
    for k, ts in times.items():
        med = statistics.median(ts)
        tail = f"  -> {per / med:8.1f} images/s" if per else ""
        print(f"{k:12s} median {med * unit[0]:9.3f} {unit[1]}  spread {(max(ts) - min(ts)) * unit[0]:8.3f} {unit[1]}  min {min(ts) * unit[0]:9.3f}"
              f"  max {max(ts) * unit[0]:9.3f}{tail}")
    if len(times) == 2:
        (ka, a), (kb, b) = times.items()
        ma, mb = statistics.median(a), statistics.median(b)
        both = (max(a) - min(a)) + (max(b) - min(b))
        print(f"{ka} / {kb} = {ma / mb:.3f}; difference {abs(ma - mb) * unit[0]:.3f} {unit[1]} against the two spreads together {both * unit[0]:.3f} {unit[1]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--iters", type=int, default=4, help="tower passes per timed round")
    ap.add_argument("--only", choices=["hip", "torch"], default=None)
    ap.add_argument("--arch", default="vitl14")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    model = dinov2_model.build_dinov2(None, 0, args.arch).to(dev)
    hip, auto = dinov2_hip.HipDino(model, dev), dinov2_hip.AutocastDino(model, dev)
    x = torch.randn((args.batch, 3, hip.resolution, hip.resolution), device=dev, dtype=torch.float16)
    paths = {"hip": lambda: hip.encode_image(x), "torch": lambda: auto.encode_image(x)}
    if args.only:
        paths = {args.only: paths[args.only]}
    with torch.no_grad():
        times = _rounds(paths, args.rounds, args.iters)
        print(f"DINOv2 {args.arch} tower, batch {args.batch}, {args.rounds} rounds of {args.iters} passes, seeded parameters")
        _report(times, (1e3, "ms"), args.batch)
        if args.only:
            return
        seq = (hip.resolution // hip.patch) ** 2 + 1
        m, n, k = args.batch * seq, hip.width, 4 * hip.width
        a = torch.randn((m, k), device=dev).half()
        w = (torch.randn((n, k), device=dev) * k ** -0.5).half()
        b = torch.randn(n, device=dev).half()
        ls = torch.rand(n, device=dev) + 0.5
        r32, r16 = torch.randn((m, n), device=dev), torch.randn((m, n), device=dev).half()
        o32, o16 = torch.empty_like(r32), torch.empty_like(r16)
        gemms = {"res32 (fp32)": lambda: dinov2_hip.gemm_res32(a, w, b, ls, r32, o32),
                 "f16 residual": lambda: clip_hip.gemm(a, w, b, r16, 0, out=o16)}
        gt = _rounds(gemms, args.rounds, 20)
        print(f"fc2 GEMM {m} x {n} x {k}: fp32 stream epilogue against the fp16 residual epilogue, {args.rounds} rounds of 20 launches")
        _report(gt, (1e6, "us"))
        for kname, ts in gt.items():
            print(f"{kname:12s} {2.0 * m * n * k / statistics.median(ts) / 1e12:7.1f} TFLOP/s")


if __name__ == "__main__":
    main()
