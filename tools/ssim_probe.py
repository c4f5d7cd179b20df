#!/usr/bin/env python3
"""SSIM of resident 256 x 256 uint8 pairs: this project's route (device.ssim_pairs: tise_ssim_pairs, csrc/ssim.hip) alternating with
a plain-torch fp64 route (the five moments as depthwise F.conv2d with the 11 x 11 window on the same GPU), seeded smooth pairs,
7 timed rounds after warm-up, median and spread (max - min) of the rounds, pairs/s, and the kernel route's algorithmic bytes
(2 * 3 * H * W per pair at scale 1: both images read once) over its time.  Then the whole per-batch work of paired.py
(psnr_ssim_from_images with and without the five-scale pyramid), host arithmetic and read-back included.

    python tools/ssim_probe.py [--rounds 7] [--batches 50 1000] [--only hip|torch]  > profiles/r18a_ssim_probe.txt

--only hip with --rounds 1 is the target of a separate `rocprofv3 --kernel-trace --stats` pass (the kernels' own times:
profiles/r18b_ssim_kernel_stats.txt)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

from tise_toolbox_amd import device, paired

C1, C2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2


def window():
    i = np.arange(11, dtype=np.float64)
    g = np.exp(-(i - 5.0) ** 2 / 4.5)
    return g / g.sum()


def torch_ssim(x, y, kernel):
    """(N,H,W,3) uint8 -> (N,3,2) fp64 {ssim mean, cs mean}: the definition in plain torch, fp64, one conv2d per moment."""
    x, y = x.permute(0, 3, 1, 2).double(), y.permute(0, 3, 1, 2).double()
    blur = lambda z: F.conv2d(z, kernel, groups=3)
    mx, my = blur(x), blur(y)
    mxx, myy, mxy = mx * mx, my * my, mx * my
    sxx, syy, sxy = blur(x * x) - mxx, blur(y * y) - myy, blur(x * y) - mxy
    cs = (2.0 * sxy + C2) / (sxx + syy + C2)
    s = (2.0 * mxy + C1) / (mxx + myy + C1) * cs
    return torch.stack([s.mean(dim=(2, 3)), cs.mean(dim=(2, 3))], dim=2)


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
        bw = f"  {unit_bytes * batch / med / 1e9:7.1f} GB/s algorithmic" if unit_bytes and k == "hip" else ""
        print(f"  {k:12s} median {med * 1e3:8.3f} ms  spread {(max(ts) - min(ts)) * 1e3:6.3f} ms  min {min(ts) * 1e3:8.3f}  max {max(ts) * 1e3:8.3f}"
              f"  -> {batch / med:9.1f} pairs/s{bw}")
    if "hip" in times and "torch" in times:
        a, b = statistics.median(times["hip"]), statistics.median(times["torch"])
        both = sum(max(times[k]) - min(times[k]) for k in ("hip", "torch"))
        print(f"  hip / torch = {a / b:.3f}; difference {(a - b) * 1e3:+.3f} ms against the two spreads together {both * 1e3:.3f} ms")


def smooth_pairs(batch, h, w, dev, seed=0):
    """Blurred noise rescaled to 0..255, and the same plus N(0, 10) noise, clipped (made on the device, seeded)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    z = torch.randn((batch, 1, h + 16, w + 16), generator=g, device=dev).expand(-1, 3, -1, -1).contiguous()
    z = z + 0.5 * torch.randn(z.shape, generator=g, device=dev)
    box = torch.full((3, 1, 5, 5), 1.0 / 25.0, device=dev)
    for _ in range(3):
        z = F.conv2d(z, box, groups=3, padding=2)
    z = z[:, :, 8:8 + h, 8:8 + w]
    lo, hi = z.amin(dim=(1, 2, 3), keepdim=True), z.amax(dim=(1, 2, 3), keepdim=True)
    x = ((z - lo) / (hi - lo) * 255.0).round()
    y = (x + 10.0 * torch.randn(x.shape, generator=g, device=dev)).round().clamp(0, 255)
    to_u8 = lambda t: t.permute(0, 2, 3, 1).contiguous().to(torch.uint8)
    return to_u8(x), to_u8(y)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batches", type=int, nargs="+", default=[50, 1000])
    ap.add_argument("--iters", type=int, default=4, help="launches per timed round")
    ap.add_argument("--only", choices=["hip", "torch"], default=None)
    ap.add_argument("--size", type=int, default=256)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = window()
    kernel = torch.as_tensor(np.outer(g, g), device=dev).expand(3, 1, 11, 11).contiguous()
    h = w = args.size
    print(f"{h} x {w} resident uint8 pairs (smooth, seeded), {args.rounds} rounds of {args.iters} launches; algorithmic bytes {2 * 3 * h * w} per pair")
    for batch in args.batches:
        x, y = smooth_pairs(batch, h, w, dev)
        fns = {"hip": lambda: device.ssim_pairs(x, y), "torch": lambda: torch_ssim(x, y, kernel)}
        fns = {k: f for k, f in fns.items() if args.only in (None, k)}
        if len(fns) == 2:
            d = float((fns["hip"]() - fns["torch"]()).abs().max())
            print(f"batch {batch}: worst |hip - torch| over the (n, 3, 2) means = {d:.3e}")
        print(f"batch {batch}: the SSIM map means of scale 1")
        report(timed(fns, args.rounds, args.iters), batch, 2 * 3 * h * w)
        if args.only in (None, "hip"):
            print(f"batch {batch}: paired.psnr_ssim_from_images (launches, read-back and host arithmetic)")
            report(timed({"psnr+ssim": lambda: paired.psnr_ssim_from_images(x, y), "+ms-ssim": lambda: paired.psnr_ssim_from_images(x, y, True)},
                         args.rounds, args.iters), batch)


if __name__ == "__main__":
    main()
