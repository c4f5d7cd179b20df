#!/usr/bin/env python3
"""Time csrc/calibrate.hip at the calibration size: one evaluation (tise_calib_eval) = one pass over N x C fp32 logits.

    python tools/calib_probe.py [--rows 50000] [--classes 1000] [--reps 200] [--fit]

Prints the mean time per evaluation from HIP events around ``reps`` back-to-back launches (after a warm-up), the bytes
one evaluation must read (N C 4 + N 4) and the achieved rate against the 6.29 TB/s measured copy rate of MI355X_MICROARCH
.md.  ``--fit`` then runs one whole set_temperature_from_logits (LBFGS, up to 62 evaluations); run it under
``rocprofv3 --kernel-trace --stats`` for the per-kernel record."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tise_toolbox_amd import calibration, device  # noqa: E402

COPY_RATE = 6.29e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50000)
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--fit", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    logits = torch.randn((a.rows, a.classes), generator=g, device=dev) * 2.0
    labels = torch.randint(0, a.classes, (a.rows,), generator=g, device=dev)
    ev = device.CalibrationEvaluator(logits, labels)
    for _ in range(10):
        ev.raw(0.598)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    from tise_toolbox_amd import _lib
    from tise_toolbox_amd.device import _ptr, _stream
    t0.record()
    for _ in range(a.reps):                                  # launches only (ev.raw also copies the sums to the host)
        _lib.call("tise_calib_eval", _ptr(ev.logits), ev.rows, ev.logits.stride(0), 0, ev.C, _ptr(ev.labels), 0.598,
                  _ptr(ev.edges), ev.n_bins, _ptr(ev._out), _ptr(ev._ws), ev._ws.numel(), _stream())
    t1.record()
    t1.synchronize()
    us = t0.elapsed_time(t1) * 1e3 / a.reps
    nbytes = a.rows * a.classes * 4 + a.rows * 4
    print(f"calib eval {a.rows} x {a.classes}: {us:.1f} us per evaluation (rows + fold kernels, {a.reps} back to back); "
          f"{nbytes / 1e6:.1f} MB -> {nbytes / us / 1e3:.0f} GB/s = {nbytes / us * 1e6 / COPY_RATE:.2f} of the "
          f"6.29 TB/s copy rate", flush=True)
    if a.fit:
        h = time.perf_counter()
        res = calibration.set_temperature_from_logits(logits, labels.cpu().numpy())
        print(f"fit: T = {res['temperature']!r} in {time.perf_counter() - h:.3f} s (host clock, includes the LBFGS loop "
              f"and one device->host copy per evaluation)", flush=True)


if __name__ == "__main__":
    main()
