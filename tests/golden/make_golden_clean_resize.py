"""Writes tests/golden/pil_resize_f32.npz: Pillow's own float32 (mode "F") resize of seeded images, so that the GPU tests of
csrc/resize_f32.hip do not depend on the Pillow of the machine they run on.  Run once, by hand, from the repository root:

    python tests/golden/make_golden_clean_resize.py

The file holds, per case i, ``case_i`` = (content kind, seed, h, w, oh, ow, filter) as strings and either ``out_i`` -- Pillow's
(oh, ow, 3) float32 output, channel by channel as clean-fid resizes -- or, for the 299 x 299 outputs (1 MB each), ``sha_i`` (the
SHA-256 of the output's bytes: equal digests are equal bits) and ``rows_i`` (every 13th output row, to show where a mismatch
lies).  Written with Pillow 12.2.0 (``pillow`` array); nothing is clipped or quantised."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import _clean_resize_ref as ref  # noqa: E402

# (kind, seed, h, w, oh, ow, filter)
CASES = [
    ("rand", 11, 37, 53, 41, 37, "bicubic"),        # up on both axes
    ("bw", 12, 37, 53, 41, 37, "bicubic"),          # 0/255 content: overshoot below 0 and above 255
    ("rand", 13, 37, 53, 41, 37, "bilinear"),
    ("rand", 14, 64, 2000, 37, 100, "bicubic"),     # down with many taps per window
    ("rand", 15, 2000, 64, 37, 100, "bicubic"),     # ... vertically: hundreds of source rows per output row
    ("bw", 16, 1000, 9, 16, 299, "bicubic"),        # more than 100 times taller than wide: Image.resize runs the vertical pass first
    ("rand", 17, 1000, 9, 299, 299, "bicubic"),     # the same rule at the network's size
    ("rand", 18, 256, 256, 299, 299, "bicubic"),    # the flagship shape
    ("rand", 19, 1, 1, 37, 41, "bicubic"),
    ("rand", 20, 37, 53, 37, 41, "bicubic"),        # identity on y
    ("rand", 21, 37, 53, 41, 53, "bicubic"),        # identity on x
    ("bw", 22, 64, 2000, 37, 100, "bilinear"),
]
ROW_STEP = 13


def main():
    import PIL
    out = {"pillow": np.asarray(PIL.__version__), "n_cases": np.asarray(len(CASES)), "row_step": np.asarray(ROW_STEP)}
    for i, (kind, seed, h, w, oh, ow, filt) in enumerate(CASES):
        y = ref.pil_resize_f32(ref.content(kind, seed, h, w), (oh, ow), filt)
        assert y.shape == (oh, ow, 3) and y.dtype == np.float32
        out[f"case_{i}"] = np.asarray([kind, str(seed), str(h), str(w), str(oh), str(ow), filt])
        if oh * ow > 100 * 299:
            out[f"sha_{i}"] = np.asarray(hashlib.sha256(np.ascontiguousarray(y).tobytes()).hexdigest())
            out[f"rows_{i}"] = np.ascontiguousarray(y[::ROW_STEP])
        else:
            out[f"out_{i}"] = y
    path = os.path.join(ROOT, "tests", "golden", "pil_resize_f32.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
