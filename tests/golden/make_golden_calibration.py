#!/usr/bin/env python3
"""Golden vectors for IS* temperature calibration, produced by the reference's own temperature_scaling.py.

``classifier_calibration/temperature_scaling.py`` is imported by path and run as it is; only ``.cuda()`` (of modules
and tensors) is made an identity so that it runs on the CPU.  ``ModelWithTemperature(nn.Identity(), init_temp)``
.set_temperature(loader) gets one batch (logits, labels): the reference itself computes the NLL / ECE before, runs its
LBFGS (with its never-zeroed gradient) and prints its three lines.

Each fixture calib_<name>.npz stores seeded logits (int8 multiples of 2^-3, exact in fp16 and fp32: logits = q *
scale), the labels, the column offset c0 (the bird rule's dropped background class: the reference is handed
logits[:, c0:]), the LBFGS settings, and what the reference produced: T, NLL / ECE before and after (its fp32 values,
at full precision) and the printed lines.  Numbers only; no reference text.  Every stored case converges.

    python tests/golden/make_golden_calibration.py        (needs /root/reference; run in the build container)
"""
import contextlib
import importlib.util
import io
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/classifier_calibration/temperature_scaling.py"
sys.dont_write_bytecode = True
SCALE = 0.125

# name, N, width, c0, init_temp, seed, noise sd, label boost, share of rows whose label gets the boost
CASES = [
    ("c50", 3000, 50, 0, 1.0, 54, 2.0, 6.0, 0.7),
    ("c80", 2000, 80, 0, 0.23, 80, 0.4, 2.0, 0.7),
    ("c1000", 1000, 1000, 0, 1.0, 1000, 2.5, 9.0, 0.75),
    ("c1008", 1000, 1008, 0, 1.0, 1008, 1.0, 5.0, 0.5),
    ("bird51", 2000, 51, 1, 1.0, 51, 2.0, 5.0, 0.65),
]


def load_reference():
    spec = importlib.util.spec_from_file_location("ref_temperature_scaling", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_case(n, width, c0, seed, sd, boost, share):
    rng = np.random.default_rng(seed)
    C = width - c0
    labels = rng.integers(0, C, size=n)
    z = rng.standard_normal((n, width)) * sd
    hit = rng.random(n) < share
    z[np.arange(n)[hit], c0 + labels[hit]] += boost
    q = np.clip(np.round(z / SCALE), -128, 127).astype(np.int8)
    return q, labels.astype(np.int32)


def run_reference(mod, logits, labels, init_temp):
    model = mod.ModelWithTemperature(nn.Identity(), init_temp=init_temp)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        model.set_temperature([(torch.from_numpy(logits), torch.from_numpy(labels.astype(np.int64)))])
    t = model.temperature.detach()
    nll = nn.CrossEntropyLoss()
    ece = mod._ECELoss()
    lab = torch.from_numpy(labels.astype(np.int64))
    x = torch.from_numpy(logits)
    with torch.no_grad():
        rec = {"T": float(t.item()),
               "nll_before": float(nll(x, lab).item()), "ece_before": float(ece(x, lab).item()),
               "nll_after": float(nll(model.temperature_scale(x), lab).item()),
               "ece_after": float(ece(model.temperature_scale(x), lab).item())}
    return rec, out.getvalue()


def main():
    nn.Module.cuda = lambda self, *a, **k: self
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.manual_seed(0)
    mod = load_reference()
    for name, n, width, c0, init_temp, seed, sd, boost, share in CASES:
        q, labels = make_case(n, width, c0, seed, sd, boost, share)
        logits = q.astype(np.float32) * np.float32(SCALE)
        rec, text = run_reference(mod, np.ascontiguousarray(logits[:, c0:]), labels, init_temp)
        assert 0.05 < rec["T"] < 20.0, (name, rec)                   # converging cases only
        path = os.path.join(HERE, f"calib_{name}.npz")
        np.savez_compressed(path, q=q, scale=np.float32(SCALE), labels=labels, c0=np.int32(c0),
                            init_temp=np.float64(init_temp), lr=np.float64(0.01), max_iter=np.int32(50),
                            printed=np.array(text.rstrip("\n").split("\n")),
                            **{k: np.float64(v) for k, v in rec.items()})
        print(f"{name}: T = {rec['T']!r}  NLL {rec['nll_before']:.4f} -> {rec['nll_after']:.4f}  "
              f"ECE {rec['ece_before']:.4f} -> {rec['ece_after']:.4f}  ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
