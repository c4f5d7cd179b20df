#!/usr/bin/env python3
"""KID kernel probe (csrc/mmd.hip) on an MI355X: time of the launch pair of tise_mmd_poly3_grouped, its fp64 rate and share of
the 78.6 TFLOP/s fp64 MFMA peak, against tise_stats_update_cov on 5 000 rows in the SAME run (the yardstick of the shared tile).

    python tools/kid_probe.py --out profiles/r09a_kid_probe.txt           # cases a, b, c + the yardstick
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/kid_probe.py --case a --repeats 3 --warmup 1 --out DIR/probe.txt
                                                                           # kernel times of (a), a run of its own

Cases: (a) 100 subsets x 1 000 rows drawn from 30 000 x 2048 seeded features per side (indexed form); (b) the full set,
30 000 vs 30 000 (one group, contiguous); (c) 80 classes of 40-48 rows per side (contiguous).
Timing: HIP events on the stream around the C entry, warm-up first, median of the repeats.  The entry copies its 48-byte-per-
segment table and waits for that copy before it launches, so the window holds that wait (tens of microseconds of host latency)
besides the two kernels; it matters for (c) only and the output says so.  Flop = tiles visited x 64 * 64 * 2 * d (the work the
tile list holds: masked rows of edge tiles included, the mirrored half of a symmetric block not).  A run without a GPU fails.
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tise_toolbox_amd import _lib, device, kid  # noqa: E402

PEAK = 78.6e12


def features(rows, d, seed, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return torch.randn((rows, d), generator=g, device=dev, dtype=torch.float32).abs_().mul_(0.5)


def median_ms(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def mmd_case(X, Y, ox, oy, ix, iy, dev):
    """-> (callable that enqueues one tise_mmd_poly3_grouped, tiles in its list, output tensor)"""
    ox, oy = np.ascontiguousarray(ox, dtype=np.int64), np.ascontiguousarray(oy, dtype=np.int64)
    ng = ox.size - 1
    pox, poy = ox.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), oy.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    nb = ctypes.c_size_t()
    _lib.call("tise_mmd_poly3_workspace_bytes", pox, poy, ng, ctypes.byref(nb))
    table = (ng * 3 * 48 + 255) // 256 * 256
    tiles = (nb.value - table) // 8
    ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    out = torch.empty((ng, 3), dtype=torch.float64, device=dev)
    ixd = torch.from_numpy(device.mmd_index(ix, X.shape[0], "index_x")).to(dev) if ix is not None else None
    iyd = torch.from_numpy(device.mmd_index(iy, Y.shape[0], "index_y")).to(dev) if iy is not None else None

    def run():
        _lib.call("tise_mmd_poly3_grouped", X.data_ptr(), X.shape[0], X.stride(0), ixd.data_ptr() if ixd is not None else None,
                  ixd.numel() if ixd is not None else 0, pox, Y.data_ptr(), Y.shape[0], Y.stride(0),
                  iyd.data_ptr() if iyd is not None else None, iyd.numel() if iyd is not None else 0, poy, ng, X.shape[1],
                  out.data_ptr(), ws.data_ptr(), nb.value, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    run.keep = (ox, oy, ixd, iyd, ws)
    return run, tiles, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="all", choices=["a", "b", "c", "all"])
    ap.add_argument("--rows", type=int, default=30000)
    ap.add_argument("--dims", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "kid_probe needs a HIP device"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    d = args.dims
    X, Y = features(args.rows, d, 1, dev), features(args.rows, d, 2, dev)
    lines = [f"kid_probe: {torch.cuda.get_device_name(0)}, {args.rows} x {d} fp32 features per side, warm-up {args.warmup}, "
             f"median of {args.repeats} (min .. max), HIP events around the C entry; peak {PEAK / 1e12:.1f} TFLOP/s fp64 MFMA"]
    fractions = {}

    def report(tag, what, run, tiles, repeats=None):
        med, lo, hi = median_ms(run, args.warmup, repeats or args.repeats)
        flop = tiles * 64 * 64 * 2 * d
        rate = flop / (med * 1e-3)
        fractions[tag] = rate / PEAK
        lines.append(f"({tag}) {what}: {tiles} tiles, {flop:.4e} flop, {med:.3f} ms ({lo:.3f} .. {hi:.3f}) -> {rate / 1e12:.2f} TFLOP/s = "
                     f"{rate / PEAK:.3f} of peak")
        print(lines[-1], flush=True)

    if args.case in ("a", "all"):
        i1, i2, m = kid.subset_indices(args.rows, args.rows, 100, 1000, 0)
        offs = np.arange(101, dtype=np.int64) * m
        run, tiles, out = mmd_case(X, Y, offs, offs, i1, i2, dev)
        report("a", f"100 subsets x {m} rows, indexed", run, tiles)
        s = out.cpu().numpy()
        v = s[:, 0] / (m * (m - 1)) + s[:, 1] / (m * (m - 1)) - 2 * s[:, 2] / (m * m)
        lines.append(f"    KID of the two seeded sets (one distribution): {np.mean(v):.6e} +- {np.std(v):.6e}")
    if args.case in ("b", "all"):
        run, tiles, _ = mmd_case(X, Y, [0, args.rows], [0, args.rows], None, None, dev)
        report("b", f"full set {args.rows} vs {args.rows}, one group", run, tiles, repeats=3)
    if args.case in ("c", "all"):
        rng = np.random.default_rng(5)
        ox = np.concatenate([[0], np.cumsum(rng.integers(40, 49, 80))])
        oy = np.concatenate([[0], np.cumsum(rng.integers(40, 49, 80))])
        run, tiles, _ = mmd_case(X, Y, ox, oy, None, None, dev)
        report("c", "80 classes of 40-48 rows per side", run, tiles)
        lines.append("    (c) is 240 workgroups of one mostly-masked tile each on 256 compute units plus the table copy's wait and two "
                     "launches: launch- and tail-bound, its share of peak is not a statement about the tile")
    if args.case == "all":
        acc = device.StatsAccumulator(d, dev)
        feats = X[:5000]
        med, lo, hi = median_ms(lambda: acc.update_parts(feats, cov=True, col_sum=False), args.warmup, args.repeats)
        flop = 5000 * d * (d + 64)
        rate = flop / (med * 1e-3)
        lines.append(f"(yardstick) tise_stats_update_cov, 5000 x {d}: {flop:.4e} flop, {med:.3f} ms ({lo:.3f} .. {hi:.3f}) -> "
                     f"{rate / 1e12:.2f} TFLOP/s = {rate / PEAK:.3f} of peak")
        lines.append(f"    (a) / yardstick = {fractions['a'] / (rate / PEAK):.2f}")
        print("\n".join(lines[-2:]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
