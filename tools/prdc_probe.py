#!/usr/bin/env python3
"""Precision / recall / density / coverage probe (csrc/knn.hip) on an MI355X: this package's three passes (radii of the real side,
radii of the generated side, the cross counts) against a plain-torch fp64 route on the SAME GPU in the SAME run, alternating.

    python tools/prdc_probe.py --out profiles/r10a_prdc_probe.txt
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/prdc_probe.py --repeats 1 --warmup 0 --no-torch --out DIR/probe.txt
                                                                           # kernel times, a run of its own

Rows: seeded pool3-like features, 30 000 + 30 000 x 2048, k = 5.  The torch route is what a user would write without this
package: row chunks, ``X @ Y.T`` in fp64 (rocBLAS), the expansion, ``topk`` for the radii, comparisons and ``sum`` / ``any`` for
the counts -- chunked so that no n x n matrix is held.  Timing: HIP events around each whole route, warm-up first, the routes
alternate, median and spread (min .. max) of the repeats.  The two tile kernels are also timed alone: flop = tiles visited x
64 * 64 * 2 * d against the 78.6 TFLOP/s fp64 MFMA peak.  ``--images-per-second R`` puts the kernel route beside the image loop
of a job of the same size (rows / R seconds per side).  A run without a GPU fails.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tise_toolbox_amd import device  # noqa: E402

PEAK = 78.6e12


def features(rows, d, seed, dev, shift=0.0):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return torch.randn((rows, d), generator=g, device=dev, dtype=torch.float32).abs_().mul_(0.5).add_(shift)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def kernel_route(knn, R, F, k):
    cnt, rec, prec = knn.counts(R, knn.radius2(R, k), F, knn.radius2(F, k))
    return torch.stack([prec.sum(), rec.sum(), cnt.sum(dtype=torch.int64), (cnt > 0).sum()])


def torch_route(R, F, k, chunk):
    """fp64 throughout; the same definitions (strict comparisons on squared values, k-th smallest over the other rows)."""
    R64, F64 = R.double(), F.double()
    nR, nF = (R64 * R64).sum(1), (F64 * F64).sum(1)

    def radii(X, nX):
        out = torch.empty(X.shape[0], dtype=torch.float64, device=X.device)
        for lo in range(0, X.shape[0], chunk):
            hi = min(lo + chunk, X.shape[0])
            d2 = ((nX[lo:hi, None] + nX[None, :]) - 2.0 * (X[lo:hi] @ X.T)).clamp_(min=0.0)
            d2[torch.arange(hi - lo, device=X.device), torch.arange(lo, hi, device=X.device)] = float("inf")
            out[lo:hi] = torch.topk(d2, k, dim=1, largest=False).values[:, k - 1]
        return out
    rR, rF = radii(R64, nR), radii(F64, nF)
    cnt = torch.empty(R.shape[0], dtype=torch.int64, device=R.device)
    rec = torch.empty(R.shape[0], dtype=torch.bool, device=R.device)
    prec = torch.zeros(F.shape[0], dtype=torch.bool, device=R.device)
    for lo in range(0, R.shape[0], chunk):
        hi = min(lo + chunk, R.shape[0])
        d2 = ((nR[lo:hi, None] + nF[None, :]) - 2.0 * (R64[lo:hi] @ F64.T)).clamp_(min=0.0)
        inside = d2 < rR[lo:hi, None]
        cnt[lo:hi] = inside.sum(1)
        prec |= inside.any(0)
        rec[lo:hi] = (d2 < rF[None, :]).any(1)
    return torch.stack([prec.sum(), rec.sum(), cnt.sum(), (cnt > 0).sum()])


def stats(ms):
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=30000)
    ap.add_argument("--dims", type=int, default=2048)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=2048, help="rows per chunk of the torch route")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-torch", action="store_true", help="the kernel route alone (the rocprofv3 pass)")
    ap.add_argument("--images-per-second", type=float, default=0.0,
                    help="image-loop rate of a job (bench.py's value) to set the metric's time against; 0 = not reported")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "prdc_probe needs a HIP device"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n, d, k = args.rows, args.dims, args.k
    R, F = features(n, d, 1, dev), features(n, d, 2, dev, 0.02)
    knn = device.KnnManifold(dev)
    lines = [f"prdc_probe: {torch.cuda.get_device_name(0)}, {n} + {n} x {d} fp32 rows, k = {k}, warm-up {args.warmup}, median of "
             f"{args.repeats} (min .. max), HIP events around each route, routes alternating; peak {PEAK / 1e12:.1f} TFLOP/s fp64 MFMA"]
    for _ in range(args.warmup):
        kernel_route(knn, R, F, k)
        if not args.no_torch:
            torch_route(R, F, k, args.chunk)
    torch.cuda.synchronize()
    t_kernel, t_torch, v_kernel, v_torch = [], [], None, None
    for _ in range(args.repeats):
        ms, v_kernel = timed(lambda: kernel_route(knn, R, F, k))
        t_kernel.append(ms)
        if not args.no_torch:
            ms, v_torch = timed(lambda: torch_route(R, F, k, args.chunk))
            t_torch.append(ms)
    km = stats(t_kernel)
    lines.append(f"kernel route (3 passes): {km[0]:.1f} ms ({km[1]:.1f} .. {km[2]:.1f})")
    sums = v_kernel.cpu().tolist()
    lines.append(f"    precision {sums[0] / n:.6f} recall {sums[1] / n:.6f} density {sums[2] / (k * n):.6f} coverage {sums[3] / n:.6f}")
    if not args.no_torch:
        tm = stats(t_torch)
        lines.append(f"torch fp64 route (chunks of {args.chunk} rows, X @ Y.T, topk): {tm[0]:.1f} ms ({tm[1]:.1f} .. {tm[2]:.1f})")
        lines.append(f"    integer sums equal the kernel route's: {v_torch.cpu().tolist() == sums} (an undecidable comparison may differ: "
                     f"kernel {sums}, torch {v_torch.cpu().tolist()})")
        gap, spreads = tm[0] - km[0], (km[2] - km[1]) + (tm[2] - tm[1])
        lines.append(f"    torch median - kernel median = {gap:.1f} ms against the two spreads together {spreads:.1f} ms: the kernel route "
                     f"{'beats' if gap > spreads else 'does NOT beat'} the torch route by more than the spreads")
    # the two tile kernels alone
    tiles = ((n + 63) // 64) ** 2
    flop = tiles * 64 * 64 * 2 * d
    r2R, r2F = knn.radius2(R, k), knn.radius2(F, k)
    for name, fn in (("tise_knn_radius2 (norms + radius kernel + merge)", lambda: knn.radius2(R, k)),
                     ("tise_prdc_counts (norms + counts kernel)", lambda: knn.counts(R, r2R, F, r2F))):
        ms = stats([timed(fn)[0] for _ in range(max(3, args.repeats))])
        rate = flop / (ms[0] * 1e-3)
        lines.append(f"{name}: {tiles} tiles, {flop:.4e} flop, {ms[0]:.1f} ms ({ms[1]:.1f} .. {ms[2]:.1f}) -> {rate / 1e12:.2f} TFLOP/s = "
                     f"{rate / PEAK:.3f} of peak")
    if args.images_per_second > 0:
        loop = 2 * n / args.images_per_second
        lines.append(f"image loop of the same job at {args.images_per_second:.0f} images/s: {loop:.1f} s for {2 * n} images; the metric's "
                     f"{km[0] / 1e3:.2f} s is {km[0] / 1e3 / loop:.3f} of it")
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
