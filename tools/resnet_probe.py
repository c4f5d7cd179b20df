#!/usr/bin/env python3
"""ResNet-50 features of 50 resident seeded 224 x 224 uint8 images: resnet_hip.HipResNet50 with the matrix-core stem ("mfma"), the
same with route "padded" (conv1 as a 32-channel SplitConv), and resnet_model.ResNet50 on the library's kernels on the same GPU --
fp32, and fp16 under autocast --, alternating, 7 timed rounds after warm-up, median and spread (max - min) of the rounds, images/s,
and how far each route is from the module's fp64 forward on the first 2 images.  Seeded stand-in parameters: rates only.

    python tools/resnet_probe.py [--rounds 7] [--batch 50] [--size 224] [--only mfma|padded|torch32|torch16]

--only mfma (or padded) with --rounds 1 is the target of a separate `rocprofv3 --kernel-trace --stats` pass (no counters, no other
tracing); `--summarize DIR` condenses that pass's output into a per-kernel table (tools/lpips_probe.py's summary code) and adds the
stem's share of the kernel time and the residual kernel's algorithmic rate: 12 C bytes per pixel over its time, per call."""
import argparse
import csv
import glob
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from lpips_probe import summarize, timed  # noqa: E402

STEM_KERNELS = ("stem7_mfma_u8_kernel", "resnet_input_kernel")
# (pixels per 224 x 224 image, channels) of the sixteen residual launches, in launch order
RESIDUAL_SHAPES = [(56 * 56, 256)] * 3 + [(28 * 28, 512)] * 4 + [(14 * 14, 1024)] * 6 + [(7 * 7, 2048)] * 3


def own_kernels(d, batch, size):
    traces = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not traces:
        return
    rows = sorted(csv.DictReader(open(traces[0])), key=lambda r: int(r["Start_Timestamp"]))
    dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    total = sum(dur(r) for r in rows)
    for name in STEM_KERNELS + ("maxpool3s2p1_split_kernel", "residual_relu_split_kernel"):
        ts = [dur(r) for r in rows if name in r["Kernel_Name"]]
        if ts:
            print(f"{name:28s} {len(ts):4d} calls, {sum(ts) / total * 100:6.2f} % of all kernel time; us in launch order (last 16): "
                  + " ".join(f"{t:.1f}" for t in ts[-16:]))
    res = [dur(r) for r in rows if "residual_relu_split_kernel" in r["Kernel_Name"]]
    if res and len(res) % 16 == 0 and size == 224:
        last = res[-16:]
        for (px, c), t in zip(RESIDUAL_SHAPES, last):
            print(f"  residual {px:5d} px x {c:4d} ch x {batch} images: {t:7.1f} us = {12.0 * c * px * batch / t / 1e6:6.2f} TB/s algorithmic")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--iters", type=int, default=2, help="calls per timed round")
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--only", choices=["mfma", "padded", "torch32", "torch16"], default=None)
    ap.add_argument("--summarize", default=None, metavar="DIR")
    args = ap.parse_args()
    if args.summarize:
        summarize(args.summarize)
        return own_kernels(args.summarize, args.batch, args.size)
    import torch
    from tise_toolbox_amd import resnet_hip, resnet_model
    dev = torch.device("cuda:0")
    h = w = args.size
    g = torch.Generator().manual_seed(0)
    x = torch.randint(0, 256, (args.batch, h, w, 3), generator=g, dtype=torch.uint8).to(dev)
    model = resnet_model.ResNet50().init_synthetic(0)
    towers = {"mfma": lambda: resnet_hip.HipResNet50(model, dev, stem="mfma"),
              "padded": lambda: resnet_hip.HipResNet50(model, dev, stem="padded"),
              "torch32": lambda: resnet_hip.TorchResNet50(resnet_model.ResNet50().init_synthetic(0), dev),
              "torch16": lambda: resnet_hip.TorchResNet50(resnet_model.ResNet50().init_synthetic(0), dev, autocast=True)}
    towers = {k: f() for k, f in towers.items() if args.only in (None, k)}
    fns = {k: (lambda t=t: t.features_from_u8(x).cpu()) for k, t in towers.items()}
    print(f"{args.batch} resident {h} x {w} uint8 images (uniform random bytes, seeded; seeded stand-in parameters), {args.rounds} rounds of "
          f"{args.iters} calls; a call ends with the read-back of the {args.batch} x 2048 features")
    if args.only is None:
        with torch.no_grad():
            want = resnet_model.ResNet50().init_synthetic(0).double()(x[:2].cpu())
        for k, f in fns.items():
            got = f()[:2].double()
            print(f"  {k:8s} worst ||row - fp64 module|| / ||.|| over 2 images = {((got - want).norm(dim=1) / want.norm(dim=1)).max():.3e}")
    times = timed(fns, args.rounds, args.iters)
    for k, ts in times.items():
        med = statistics.median(ts)
        print(f"  {k:8s} median {med * 1e3:9.3f} ms  spread {(max(ts) - min(ts)) * 1e3:7.3f} ms  min {min(ts) * 1e3:9.3f}  max {max(ts) * 1e3:9.3f}"
              f"  -> {args.batch / med:9.1f} images/s")
    if "mfma" in times:
        a = statistics.median(times["mfma"])
        for k in times:
            if k != "mfma":
                b = statistics.median(times[k])
                both = max(times["mfma"]) - min(times["mfma"]) + max(times[k]) - min(times[k])
                print(f"  mfma / {k} = {a / b:.3f}; difference {(a - b) * 1e3:+.3f} ms against the two spreads together {both * 1e3:.3f} ms")


if __name__ == "__main__":
    main()
