#!/usr/bin/env python3
"""CountSeg rows (confidence and density mean of 80 classes) of 50 resident seeded 448 x 448 uint8 images: this project's route
(countseg_hip.HipCountSeg: the split-precision ResNet-50 as a map, one 2048 -> 240 SplitConv, csrc/countseg.hip) alternating with
countseg_model.CountSeg on the library's kernels on the same GPU (the TISE_COUNTSEG=torch route) -- fp32, and fp16 under autocast --,
7 timed rounds of 2 calls after warm-up, median and spread (max - min) of the rounds, images/s, and how far each route is from the
module's fp64 forward on the first 2 images.  Seeded stand-in parameters: rates only.

    python tools/countseg_probe.py [--rounds 7] [--batch 50] [--size 448] [--only hip|torch32|torch16]  > profiles/r24a_countseg_probe.txt

--only hip with --rounds 1 is the target of a separate `rocprofv3 --kernel-trace --stats` pass (no counters, no other tracing);
`--summarize DIR` condenses that pass's output into a per-kernel table (tools/lpips_probe.py's summary code) and adds the shares of
the trunk, the mix convolution and the head: profiles/r24b_countseg_kernel_stats.txt."""
import argparse
import csv
import glob
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from lpips_probe import summarize, timed  # noqa: E402


def shares(d):
    """The shares of the trunk, the mix convolution (the convolution launch right before each head launch) and the head."""
    traces = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not traces:
        return
    rows = sorted(csv.DictReader(open(traces[0])), key=lambda r: int(r["Start_Timestamp"]))
    dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    total = sum(dur(r) for r in rows)
    head = [dur(r) for r in rows if "countseg_head_kernel" in r["Kernel_Name"]]
    mix, since = [], []
    for r in rows:                                                          # the convolution launch right before each head launch
        if "countseg_head_kernel" in r["Kernel_Name"]:
            if since:
                mix.append(since[-1])
            since = []
        elif "conv" in r["Kernel_Name"] and "stem" not in r["Kernel_Name"]:
            since.append(dur(r))
    if not head:
        return
    trunk = total - sum(head) - sum(mix)
    print(f"head  countseg_head_kernel      {len(head):4d} calls, {sum(head) / total * 100:6.2f} % of all kernel time; us: " + " ".join(f"{t:.1f}" for t in head[-8:]))
    print(f"mix   the 2048 -> 240 SplitConv  {len(mix):4d} calls, {sum(mix) / total * 100:6.2f} % of all kernel time; us: " + " ".join(f"{t:.1f}" for t in mix[-8:]))
    print(f"trunk everything else            {trunk / total * 100:6.2f} % of all kernel time ({trunk / 1e3:.3f} ms of {total / 1e3:.3f} ms)")


def conv_kernels(counter, size):
    """Which convolution kernel each 3 x 3 layer of the trunk takes at this size (a host computation: SplitConv's own rule)."""
    from tise_toolbox_amd import conv_split, resnet_model
    s = resnet_model.halved(resnet_model.halved(size))
    for i, blk in enumerate(counter.trunk.blocks):
        conv = blk.conv2
        ow = conv.out_hw(s, s)[1]
        took = conv.variant
        if took == "rowwin" and not (conv_split.rowwin_fits(ow, conv.kw) and conv_split.rowwin_divides(ow, conv.kw)):
            took = "fast (row-window fall-back)"
        print(f"  block {i:2d} conv2 {conv.cin:4d} -> {conv.cout:4d} stride {conv.stride[0]} OW {ow:3d}: {took}, tile width {32 * conv.tn}")
        s = ow
    print(f"  mix 2048 -> 240 at OW {s}: {counter.mix.variant}, tile width {32 * counter.mix.tn}; every 1 x 1 convolution: fast")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--iters", type=int, default=2, help="calls per timed round")
    ap.add_argument("--size", type=int, default=448)
    ap.add_argument("--only", choices=["hip", "torch32", "torch16"], default=None)
    ap.add_argument("--summarize", default=None, metavar="DIR")
    args = ap.parse_args()
    if args.summarize:
        summarize(args.summarize)
        return shares(args.summarize)
    import torch
    from tise_toolbox_amd import countseg_hip, countseg_model
    dev = torch.device("cuda:0")
    h = w = args.size
    from tests import _countseg_ref
    x = torch.from_numpy(_countseg_ref.images(args.batch, h, w, 0)).to(dev)
    model = countseg_model.CountSeg().init_synthetic(0)
    routes = {"hip": lambda: countseg_hip.HipCountSeg(model, dev),
              "torch32": lambda: countseg_hip.TorchCountSeg(countseg_model.CountSeg().init_synthetic(0), dev),
              "torch16": lambda: countseg_hip.TorchCountSeg(countseg_model.CountSeg().init_synthetic(0), dev, autocast=True)}
    routes = {k: f() for k, f in routes.items() if args.only in (None, k)}
    fns = {k: (lambda t=t: t.rows_from_u8(x).cpu()) for k, t in routes.items()}
    print(f"{args.batch} resident {h} x {w} uint8 images (smooth seeded images plus noise; seeded stand-in parameters), {args.rounds} rounds of "
          f"{args.iters} calls; a call ends with the read-back of the {args.batch} x 160 fp64 rows")
    if "hip" in routes:
        conv_kernels(routes["hip"], args.size)
    if args.only is None:
        with torch.no_grad():
            conf, den, cnt = countseg_model.CountSeg().init_synthetic(0).double()(x[:2].cpu())
            m, d = countseg_model.CountSeg().init_synthetic(0).double().maps(x[:2].cpu())
        want = torch.cat([conf, den], 1)
        scale = max(float(m.abs().max()), float(d.abs().max()))
        for k, f in fns.items():
            got = f()[:2]
            same = bool((routes[k].last_peaks[:2].cpu() == cnt).all())
            print(f"  {k:8s} worst |row - fp64 module| / largest |map value| over 2 images = {float((got - want).abs().max()) / scale:.3e}; "
                  f"peak counts {'equal' if same else 'DIFFER'}")
    times = timed(fns, args.rounds, args.iters)
    for k, ts in times.items():
        med = statistics.median(ts)
        print(f"  {k:8s} median {med * 1e3:9.3f} ms  spread {(max(ts) - min(ts)) * 1e3:7.3f} ms  min {min(ts) * 1e3:9.3f}  max {max(ts) * 1e3:9.3f}"
              f"  -> {args.batch / med:9.1f} images/s")
    if "hip" in times:
        a = statistics.median(times["hip"])
        for k in times:
            if k != "hip":
                b = statistics.median(times[k])
                both = max(times["hip"]) - min(times["hip"]) + max(times[k]) - min(times[k])
                print(f"  hip / {k} = {a / b:.3f}; difference {(a - b) * 1e3:+.3f} ms against the two spreads together {both * 1e3:.3f} ms")


if __name__ == "__main__":
    main()
