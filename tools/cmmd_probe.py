#!/usr/bin/env python3
"""CMMD kernel probe (csrc/mmd.hip, tise_mmd_rbf_grouped) on an MI355X: 30 000 + 30 000 x 512 seeded unit rows, this route
(device.GaussianMMD: norm pre-pass, one tile launch, one reduction launch) ALTERNATING with a plain-torch fp64 route on the same
GPU (row blocks of the three kernel matrices by torch.cdist-free expansion in fp64: x @ y.T, exp, sum), so that both see the same
clocks and neighbours.

    python tools/cmmd_probe.py --out profiles/r11a_cmmd_probe.txt
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/cmmd_probe.py --repeats 3 --warmup 1 --no-torch --out DIR/probe.txt
        # kernel times of this route, a run of its own; copy DIR's kernel statistics to profiles/r11b_cmmd_kernel_stats.txt

Timing: HIP events on the stream around each route, warm-up first, median of the repeats (min .. max).  The C entry copies its
48-byte-per-segment table and waits for that copy before it launches, so its window holds that wait besides the three kernels.
What the kernel statistics are for: the share of mmd_tiles_kernel<1> against the polynomial instantiation's time on the same tile
count tells what the 16 fp64 exp per thread cost beside the tile's MFMA work -- nobody has measured that; no rate is claimed.
A run without a GPU fails.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tise_toolbox_amd import cmmd, device  # noqa: E402


def unit_rows(rows, d, seed, dev, shift=0.0):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    x = torch.randn((rows, d), generator=g, device=dev, dtype=torch.float32) + shift
    return cmmd.normalize_rows(x)


def torch_sums(x, y, gamma, block=2048):
    """(Sxx, Syy, Sxy) in fp64 with library kernels only: row blocks of each kernel matrix, never a whole one."""
    xd, yd = x.double(), y.double()
    nx, ny = (xd * xd).sum(1), (yd * yd).sum(1)

    def block_sum(a, na, b, nb, skip_diagonal):
        total = torch.zeros((), dtype=torch.float64, device=a.device)
        for i in range(0, a.shape[0], block):
            d2 = ((na[i:i + block, None] + nb[None, :]) - 2.0 * (a[i:i + block] @ b.T)).clamp_min_(0.0)
            k = torch.exp(-gamma * d2)
            if skip_diagonal:
                r = torch.arange(k.shape[0], device=a.device)
                k[r, i + r] = 0.0
            total += k.sum()
        return total
    return torch.stack([block_sum(xd, nx, xd, nx, True), block_sum(yd, ny, yd, ny, True), block_sum(xd, nx, yd, ny, False)])


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=30000)
    ap.add_argument("--dims", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-torch", action="store_true", help="this route only (the rocprofv3 pass)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "cmmd_probe needs a HIP device"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n, d = args.rows, args.dims
    x, y = unit_rows(n, d, 1, dev), unit_rows(n, d, 2, dev, shift=0.05)
    mmd = device.GaussianMMD(dev, cmmd.GAMMA)
    routes = {"hip": lambda: mmd.sums(x, y, [0, n], [0, n])[0]}
    if not args.no_torch:
        routes["torch fp64"] = lambda: torch_sums(x, y, cmmd.GAMMA)
    times, last = {k: [] for k in routes}, {}
    for it in range(args.warmup + args.repeats):                              # alternating: hip, torch, hip, torch, ...
        for name, fn in routes.items():
            ms, out = timed(fn)
            last[name] = out.cpu().numpy()
            if it >= args.warmup:
                times[name].append(ms)
    tiles = (n + 63) // 64
    tiles = tiles * (tiles + 1) + tiles * tiles
    lines = [f"cmmd_probe: {torch.cuda.get_device_name(0)}, {n} + {n} x {d} seeded unit rows, gamma {cmmd.GAMMA}, warm-up {args.warmup}, "
             f"median of {args.repeats} (min .. max), HIP events around each route, routes alternating; {tiles} tiles of 64 x 64"]
    for name, t in times.items():
        lines.append(f"{name:>10s}: {np.median(t):.3f} ms ({min(t):.3f} .. {max(t):.3f})   sums {last[name].tolist()}   "
                     f"CMMD {cmmd.cmmd_from_sums(last[name], n, n)!r}")
    if "torch fp64" in last:
        rel = np.abs(last["hip"] - last["torch fp64"]) / np.abs(last["torch fp64"])
        lines.append(f"largest relative difference of a sum between the routes: {rel.max():.3e}")
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
