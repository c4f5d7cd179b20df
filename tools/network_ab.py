#!/usr/bin/env python3
"""Same-process A/B of the split trunk's throughput: --network torchvision against --network inception-2015 or slim.

The two networks run the same convolutions; the 2015 graph's average pools divide by the in-map tap count and its
Mixed_7c pool branch is a stand-alone 3x3 / stride 1 max pool (8 x 8 x 2048 per image) before a 1x1 conv instead of a
segment of the fused 1x1.  Both trunks are built once, then timed in alternation (A B A B ...) on one device-resident
uint8 batch, pool3 + the W-only logits per pass, device events around each pass.  Weights are torch's default
initialisation (throughput does not depend on them), so no stand-in calibration runs.  ``--variant slim``: the TF-slim
bird network -- the exclude-padding pools in all nine blocks (Mixed_7c's at 8 x 8 inside the fused 1x1's pool segment) and
the 51-class head; its tree gets torch's default parameters directly (its weight files are TensorFlow checkpoints).

    python tools/network_ab.py --batch 250 --reps 12 --out profiles/network_ab.json
    python tools/network_ab.py --variant slim --batch 250 --reps 12 --out profiles/network_ab_slim_mi355x.json
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(network, dev, tmp):
    from tise_toolbox_amd import device, inception
    from tise_toolbox_amd.inception import Inception3, InceptionV3, network_classes
    from tise_toolbox_amd.trunk import SplitTrunk
    torch.manual_seed(0)
    tree = Inception3(num_classes=network_classes(network), aux_logits=network == "torchvision", network=network)
    if network == "slim":
        old = inception.build_inception3
        inception.build_inception3 = lambda *a, **k: tree.eval()
        try:
            model = InceptionV3([3], network=network).to(dev).eval()
        finally:
            inception.build_inception3 = old
    else:
        path = os.path.join(tmp, f"{network}.pth")
        torch.save(tree.state_dict(), path)
        model = InceptionV3([3], weights=path, network=network).to(dev).eval()
    lut = torch.from_numpy(device.make_lut(network=network).reshape(-1)).to(dev)
    return SplitTrunk(model, dev), lut


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=250)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default="")
    ap.add_argument("--variant", type=str, default="inception-2015", choices=["inception-2015", "slim"])
    a = ap.parse_args()
    from tise_toolbox_amd import _lib
    _lib.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    g = torch.Generator().manual_seed(1)
    u8 = torch.randint(0, 256, (a.batch, 299, 299, 3), generator=g, dtype=torch.uint8).to(dev)
    with tempfile.TemporaryDirectory() as tmp:
        trunks = {net: build(net, dev, tmp) for net in ("torchvision", a.variant)}

    def once(net):
        trunk, lut = trunks[net]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        trunk.forward_u8(u8, lut)
        trunk.fc_logits(a.batch)
        e1.record()
        return e0, e1

    with torch.no_grad():
        for _ in range(a.warmup):
            for net in trunks:
                once(net)
        torch.cuda.synchronize()
        ms = {net: [] for net in trunks}
        for _ in range(a.reps):
            for net in trunks:                                        # alternation: drifts hit both sides alike
                e0, e1 = once(net)
                torch.cuda.synchronize()
                ms[net].append(e0.elapsed_time(e1))
    res = {"variant": a.variant, "batch": a.batch, "reps": a.reps, "device": torch.cuda.get_device_name(dev), "torch": torch.__version__}
    for net, v in ms.items():
        v = np.asarray(v)
        res[net] = {"ms_per_pass_median": float(np.median(v)), "ms_min": float(v.min()), "ms_max": float(v.max()),
                    "images_per_s_median": float(a.batch / np.median(v) * 1e3)}
    res["variant_over_default_time"] = res[a.variant]["ms_per_pass_median"] / res["torchvision"]["ms_per_pass_median"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
