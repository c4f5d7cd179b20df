"""GPU: the raw outputs of the four entry points over the gathered-row tile (csrc/rows_tile.h) -- tise_mmd_poly3_grouped,
tise_mmd_rbf_grouped, tise_knn_radius2, tise_prdc_counts -- byte for byte against tests/golden/rows_tile_bits.npz, NaN positions
compared as bits.  The cases are tests/_rows_tile_cases.py's bits_mmd_cases() and bits_knn_cases(): widths 3, 64, 67 and 191, the
contiguous and the gathered route, k in {1, 5}, col_splits in {0, 3}, and a NaN in the last row of either side at d = 67.

The file was recorded by tools/record_rows_tile_bits.py at commit fcfd167, the last one before csrc/rows_tile.h existed, when
every kernel still carried its own copy of the lane map, the norm pass and the distance expansion.  The summation orders of these
kernels are frozen ("What rows_tile.h owns"), so a difference here is a change of behaviour.  The ONLY legitimate reason
to re-record is a compiler or math-library change that moves the bits of the fp64 ``exp`` (the tise_mmd_rbf entries); say so, with
the commit, in this paragraph."""
import os

import numpy as np
import pytest

from tests import _rows_tile_cases as tc

KNN_NAMES = ("r2_real", "r2_fake", "cnt", "rec", "prec")


def rows_tile_bits(dev):
    """Every launch of the case lists through the raw C ABI (tests/_rows_tile_gpu.py: NaN-padded uploads, pre-filled outputs)
    -> {key: numpy array}: what the recorder writes and the test compares."""
    from tests import _rows_tile_gpu as tg
    out = {}
    for key, fn, X, Y, ix, iy, gamma in tc.bits_mmd_cases():
        out[key] = tg.mmd_cabi(fn, X, Y, tc.MMD_OX, tc.MMD_OY, dev, ix, iy, gamma)
    for key, R, F, k, splits in tc.bits_knn_cases():
        for name, a in zip(KNN_NAMES, tg.knn_cabi(R, F, k, splits, dev)):
            out[f"{key}/{name}"] = a
    return out


@pytest.mark.gpu
def test_every_output_has_the_recorded_bits(cuda_device, golden_dir):
    with np.load(os.path.join(golden_dir, tc.BITS_FILE)) as f:
        want = {k: f[k] for k in f.files}
    got = rows_tile_bits(cuda_device)
    assert sorted(got) == sorted(want) and len(want) == 20 + 5 * 18
    assert any(np.isnan(a).any() for k, a in want.items() if "nan-last" in k)          # the non-finite cases are in the file
    bad = [k for k in want if got[k].dtype != want[k].dtype or got[k].shape != want[k].shape or got[k].tobytes() != want[k].tobytes()]
    assert not bad, (len(bad), bad[:8], got[bad[0]], want[bad[0]])
