"""Writes tests/golden/torch_bilinear_f32.npz: torch's own CPU ``F.interpolate(x, size, mode="bilinear", align_corners=False)``
of seeded images divided by 255, so that the comparison of tests/_torch_resize_ref.py with torch also holds on a machine with
another torch build.  Run once, by hand, from the repository root:

    python tests/golden/make_golden_torch_resize.py

The file holds, per case i, ``case_i`` = (seed, n, h, w, oh, ow, kernel) as strings and either ``out_i`` -- torch's
(n, oh, ow, 3) float32 output -- or, for the 299 x 299 outputs (2 MB each), ``sha_i`` (the SHA-256 of the output's bytes: equal
digests are equal bits) and ``rows_i`` (every 53rd output row, to show where a mismatch lies).  ``kernel`` names which of
torch's two CPU kernels served the call, found by comparing with both restatements: "generic" (what csrc/resize_torch.hip
computes; every 299 x 299 case must be this one) or "channels_last" (the small outputs).  Written with torch 2.10.0+rocm7.0 on
8 threads (``torch`` and ``threads`` arrays)."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import _torch_resize_ref as ref  # noqa: E402

# (seed, n, h, w, oh, ow)
CASES = [(31, 2, 1, 1, 299, 299), (32, 2, 2, 5, 299, 299), (33, 2, 64, 64, 299, 299), (34, 2, 256, 256, 299, 299),
         (35, 2, 299, 299, 299, 299), (36, 2, 150, 700, 299, 299), (37, 2, 512, 384, 299, 299), (38, 2, 640, 427, 299, 299),
         (39, 2, 1024, 1024, 299, 299), (40, 2, 300, 299, 299, 299), (41, 2, 700, 3, 299, 299),
         (42, 2, 64, 64, 5, 7), (43, 2, 640, 427, 5, 7), (44, 2, 1, 1, 5, 7), (45, 2, 700, 3, 5, 7), (46, 2, 299, 299, 5, 7),
         (47, 2, 64, 64, 1, 1), (48, 2, 640, 427, 1, 1), (49, 2, 512, 384, 1, 1), (50, 2, 2, 5, 1, 1)]
ROW_STEP = 53


def main():
    import torch
    if torch.get_num_threads() < 2:
        raise SystemExit("record with more than one torch thread: one thread takes torch's other kernel at every size")
    out = {"torch": np.asarray(torch.__version__), "threads": np.asarray(torch.get_num_threads()), "n_cases": np.asarray(len(CASES)),
           "row_step": np.asarray(ROW_STEP)}
    for i, (seed, n, h, w, oh, ow) in enumerate(CASES):
        x = ref.unit(ref.content(seed, n, h, w))
        y = ref.torch_interpolate(x, (oh, ow))
        assert y.shape == (n, oh, ow, 3) and y.dtype == np.float32
        assert np.array_equal(ref.bits(y), ref.bits(ref.torch_interpolate(x, (oh, ow), channels_last=True)))
        same = {k: np.array_equal(ref.bits(f(x, (oh, ow))), ref.bits(y))
                for k, f in (("generic", ref.interpolate), ("channels_last", ref.interpolate_channels_last_kernel))}
        assert same["generic"] or same["channels_last"], (i, same)
        kernel = "generic" if same["generic"] and (oh, ow) == (299, 299) else "channels_last" if same["channels_last"] else "generic"
        assert (oh, ow) != (299, 299) or kernel == "generic"
        out[f"case_{i}"] = np.asarray([str(v) for v in (seed, n, h, w, oh, ow)] + [kernel])
        if oh * ow > 100 * 299:
            out[f"sha_{i}"] = np.asarray(hashlib.sha256(np.ascontiguousarray(y).tobytes()).hexdigest())
            out[f"rows_{i}"] = np.ascontiguousarray(y[:, ::ROW_STEP])
        else:
            out[f"out_{i}"] = y
    path = os.path.join(ROOT, "tests", "golden", "torch_bilinear_f32.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
