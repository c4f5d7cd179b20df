#!/usr/bin/env python3
"""Record the raw outputs of the gathered-row tile's entry points (csrc/rows_tile.h: tise_mmd_poly3_grouped, tise_mmd_rbf_grouped,
tise_knn_radius2, tise_prdc_counts) on the fixed cases of tests/_rows_tile_cases.py (bits_mmd_cases, bits_knn_cases) into
tests/golden/rows_tile_bits.npz, the file tests/test_gpu_rows_tile_bits.py compares byte for byte.

    python tools/record_rows_tile_bits.py                       # -> tests/golden/rows_tile_bits.npz
    python tools/record_rows_tile_bits.py --out DIR/file.npz

The summation orders of these kernels are frozen, so the file is re-recorded for one reason only: a compiler or math-library
change that moves the bits of the fp64 ``exp`` (the tise_mmd_rbf entries).  Say so, with the commit, in the test's docstring.
A run without a GPU fails.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _rows_tile_cases as tc  # noqa: E402
from tests.test_gpu_rows_tile_bits import rows_tile_bits  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", tc.BITS_FILE))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "record_rows_tile_bits needs a HIP device"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    bits = rows_tile_bits(dev)
    again = rows_tile_bits(dev)
    assert all(bits[k].tobytes() == again[k].tobytes() for k in bits), "two runs differ: nothing to record"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **bits)
    nan = sum(int(np.isnan(a).sum()) for a in bits.values() if a.dtype == np.float64)
    print(f"{len(bits)} arrays, {sum(a.nbytes for a in bits.values())} bytes raw, {nan} NaN values, "
          f"{os.path.getsize(args.out)} bytes -> {args.out}")


if __name__ == "__main__":
    main()
