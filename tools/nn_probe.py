#!/usr/bin/env python3
"""Nearest-training-row probe (nn_argmin_kernel, csrc/knn.hip) on an MI355X: ``KnnManifold.nearest`` against dgm-eval's route --
``torch.cdist`` in fp32 over row chunks, then ``min`` -- on the SAME GPU in the SAME process, alternating.

    python tools/nn_probe.py --out profiles/r16a_nn_probe.txt
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/nn_probe.py --rounds 1 --warmup 0 --no-torch --out DIR/probe.txt
                                                                           # kernel times, a run of its own

Rows: seeded pool3-like features, 50 000 training + 50 000 generated rows at every width of ``--dims`` (1024 and 2048).  A round
is: the cross pass of each route (generated against training), then the within-set pass of each (training against itself).
Timing: HIP events around each pass, warm-up first, the routes alternate, median and spread (min .. max) of the rounds.  Printed
beside the times: the share of generated rows for which both routes name the same training row, AuthPct from each route, and the
within-set pass against ``radius2(k = 1)`` at the same shape (the same MFMA work; the gap is set against the two spreads).
flop = tiles visited x 64 * 64 * 2 * d against the 78.6 TFLOP/s fp64 MFMA peak.  A run without a GPU fails.
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


def cdist_nearest(Q, B, chunk, exclude_diagonal=False):
    """dgm-eval's route: fp32 distances (not squared) of a chunk of rows against all of B, then min -> (distance, index)."""
    dist = torch.empty(Q.shape[0], dtype=torch.float32, device=Q.device)
    idx = torch.empty(Q.shape[0], dtype=torch.int64, device=Q.device)
    for lo in range(0, Q.shape[0], chunk):
        hi = min(lo + chunk, Q.shape[0])
        m = torch.cdist(Q[lo:hi], B)
        if exclude_diagonal:
            m[torch.arange(hi - lo, device=Q.device), torch.arange(lo, hi, device=Q.device)] = float("inf")
        dist[lo:hi], idx[lo:hi] = m.min(dim=1)
    return dist, idx


def stats(ms):
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def fmt(s):
    return f"{s[0]:.1f} ms ({s[1]:.1f} .. {s[2]:.1f})"


def probe(n, m, d, args, dev, lines):
    T, G = features(n, d, 1, dev), features(m, d, 2, dev, 0.02)
    knn = device.KnnManifold(dev)
    routes = {"kernel cross": lambda: knn.nearest(G, T), "kernel within": lambda: knn.nearest(T, T, exclude_diagonal=True),
              "radius2(k = 1)": lambda: knn.radius2(T, 1)}
    if not args.no_torch:
        routes["cdist cross"] = lambda: cdist_nearest(G, T, args.chunk)
        routes["cdist within"] = lambda: cdist_nearest(T, T, args.chunk, True)
    order = [k for k in ("kernel cross", "cdist cross", "kernel within", "cdist within", "radius2(k = 1)") if k in routes]
    for _ in range(args.warmup):
        for name in order:
            routes[name]()
    torch.cuda.synchronize()
    ms, out = {k: [] for k in order}, {}
    for _ in range(args.rounds):
        for name in order:
            t, out[name] = timed(routes[name])
            ms[name].append(t)
    st = {k: stats(v) for k, v in ms.items()}
    lines.append(f"--- {n} training + {m} generated rows x {d}")
    for name in order:
        tiles = ((m if "cross" in name else n) + 63) // 64 * ((n + 63) // 64)
        flop = tiles * 64 * 64 * 2 * d
        rate = "" if name.startswith("cdist") else f" -> {flop / (st[name][0] * 1e-3) / 1e12:.2f} TFLOP/s fp64 = {flop / (st[name][0] * 1e-3) / PEAK:.3f} of peak"
        lines.append(f"{name:>16}: {fmt(st[name])}{rate}")
    d1, j = out["kernel cross"]
    d2t = out["kernel within"][0]
    auth = (d2t[j.long()] < d1).double().mean().item() * 100
    lines.append(f"    kernel route: AuthPct {auth:.4f}; within-set d2 has the bits of radius2(k = 1): {torch.equal(d2t, out['radius2(k = 1)'])}")
    gap = st["kernel within"][0] - st["radius2(k = 1)"][0]
    spreads = (st["kernel within"][2] - st["kernel within"][1]) + (st["radius2(k = 1)"][2] - st["radius2(k = 1)"][1])
    lines.append(f"    within-set pass - radius2(k = 1) = {gap:+.1f} ms against the two spreads together {spreads:.1f} ms"
                 + (": the per-tile staging and scan of knn_radius2_kernel that nn_argmin_kernel does not have" if gap < -spreads else
                    ": the index bookkeeping of nn_argmin_kernel" if gap > spreads else ": inside the spreads"))
    if not args.no_torch:
        c1, cj = out["cdist cross"]
        ct = out["cdist within"][0]
        cauth = (ct[cj] < c1).double().mean().item() * 100
        lines.append(f"    cdist route:  AuthPct {cauth:.4f}; the same training row as the kernel route for {(cj == j.long()).double().mean().item() * 100:.4f} % "
                     f"of the generated rows; largest |sqrt(d2) - cdist| / cdist {((d1.sqrt() - c1.double()).abs() / c1.double()).max().item():.3e}")
        for a, b in (("kernel cross", "cdist cross"), ("kernel within", "cdist within")):
            lines.append(f"    {a} / {b} = {st[a][0] / st[b][0]:.2f} (fp64 on the matrix cores against fp32 rocBLAS + an n x chunk matrix)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train-rows", type=int, default=50000)
    ap.add_argument("--gen-rows", type=int, default=50000)
    ap.add_argument("--dims", type=int, nargs="+", default=[1024, 2048])
    ap.add_argument("--chunk", type=int, default=4096, help="query rows per torch.cdist call")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-torch", action="store_true", help="the kernel route alone (the rocprofv3 pass)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "nn_probe needs a HIP device"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lines = [f"nn_probe: {torch.cuda.get_device_name(0)}, warm-up {args.warmup}, median of {args.rounds} rounds (min .. max), HIP events "
             f"around each pass, routes alternating; peak {PEAK / 1e12:.1f} TFLOP/s fp64 MFMA; cdist in chunks of {args.chunk} rows"]
    for d in args.dims:
        probe(args.train_rows, args.gen_rows, d, args, dev, lines)
        print("\n".join(lines), flush=True)
        if args.out:                                                       # after every width: a later one that runs out of time loses nothing
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
