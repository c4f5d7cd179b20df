"""Inputs of the width sweep and of the non-finite-row tests of the gathered-row fp64 tile (csrc/rows_tile.h:
gemm_tile_64x64_rows_f32 / GtRowFetch), shared by tests/test_gpu_kid.py, tests/test_gpu_cmmd.py, tests/test_gpu_prdc.py and their
host-side companions (seeded; nothing here touches a GPU).

WIDTHS holds every residue mod 4 (the fetch reads a row in groups of four columns and the last, partial group element by
element), widths below one 64-column slab, one column either side of the slab edge, and a partial second and third slab; 64 is the
control.  The rows are few: the largest launch is 140 rows x 191 columns."""
import functools

import numpy as np

from tests import _prdc_ref
from tests._prdc_cases import MIN_MARGIN, pool3_like

WIDTHS = [1, 2, 3, 4, 5, 7, 61, 62, 63, 64, 65, 66, 67, 127, 129, 130, 191]

# ---- the two MMD kernels: three groups per side, no size a multiple of 64 ------------------------------------------------------
MMD_SIZES_X = [5, 65, 70]
MMD_SIZES_Y = [65, 70, 5]
MMD_OX = np.concatenate([[0], np.cumsum(MMD_SIZES_X)]).astype(np.int64)
MMD_OY = np.concatenate([[0], np.cumsum(MMD_SIZES_Y)]).astype(np.int64)
MMD_ROWS = 140

# the mask census (k == 1 for every pair): the empty group, the 1-row group, a full tile and sizes either side of it
CENSUS_SIZES_X = [0, 1, 5, 64, 70]
CENSUS_SIZES_Y = [1, 0, 70, 5, 64]
CENSUS_WIDTHS = [3, 64, 67]


def census_expected():
    """Sxx, Syy, Sxy of a kernel that is 1 for every pair: n (n - 1), m (m - 1), n m."""
    return np.array([[n * (n - 1), m * (m - 1), n * m] for n, m in zip(CENSUS_SIZES_X, CENSUS_SIZES_Y)], dtype=np.float64)


def unit_rows(rows, d, seed, shift=0.0):
    a = np.random.default_rng(seed).standard_normal((rows, d)) + shift
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def mmd_rows(d, family="pool3"):
    """-> (X, Y), 140 rows each, read-only.  "pool3": non-negative pool3-scaled rows; "unit": unit-norm rows (CMMD's input)."""
    if family == "pool3":
        X, Y = pool3_like(MMD_ROWS, d, 7000 + d), pool3_like(MMD_ROWS, d, 8000 + d, shift=0.02)
    else:
        X, Y = unit_rows(MMD_ROWS, d, 7100 + d), unit_rows(MMD_ROWS, d, 8100 + d, 0.1)
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y


def shuffled(a, seed):
    """-> (rows of ``a`` in a seeded random order, index) with shuffled[index] == a: the gathered route to the same groups."""
    perm = np.random.default_rng(seed).permutation(len(a))
    out = np.empty_like(a)
    out[perm] = a
    return out, perm.astype(np.int64)


def group_sums(sums_fn, X, Y, ox=MMD_OX, oy=MMD_OY):
    """``sums_fn(xs, ys) -> (Sxx, Syy, Sxy)`` on every group of contiguous rows -> (n_groups, 3) array."""
    return np.array([sums_fn(X[ox[g]:ox[g + 1]], Y[oy[g]:oy[g + 1]]) for g in range(len(ox) - 1)])


BAD_VALUES = [float("nan"), float("inf"), float("-inf")]
BAD_IDS = ["nan", "+inf", "-inf"]
NONFINITE_WIDTHS = [64, 67]


def mmd_bad_rows():
    """(side, group, position in the group): a group's first row, and the last row of a group whose size is no multiple of 64 --
    the row GtRowFetch::bind replicates into the masked rows of the group's last tile -- on either side."""
    return [("x", 1, 0), ("x", 2, MMD_SIZES_X[2] - 1), ("y", 0, MMD_SIZES_Y[0] - 1), ("y", 2, 0)]


def with_bad_row(a, row, value, col=None):
    """A writable copy of ``a`` with one element of ``row`` replaced (column: the middle one unless given)."""
    out = np.array(a, copy=True)
    out[row, a.shape[1] // 2 if col is None else col] = value
    return out


# ---- the k-NN kernels: n = 70 real rows, m = 65 generated ones ----------------------------------------------------------------
PRDC_N, PRDC_M = 70, 65
PRDC_K = [1, 5]
PRDC_SPLITS = [0, 1, 3]
EXACT_BELOW = 61             # widths under it: integer-valued features, every sum exact in any order


def prdc_is_exact(d):
    return d < EXACT_BELOW


@functools.lru_cache(maxsize=None)
def prdc_rows(d):
    """-> (R, F), read-only.  d < 61: integer-valued fp32 features, values -4 .. 4 (the expansion of d2 cancels badly at these
    widths, so neither a relative tolerance on r2 nor the 1e-9 decision margin would be honest; with integers every sum is exact
    and the results must EQUAL the reference, ties included).  d >= 61: pool3-scaled float rows under tests/_prdc_cases' rules."""
    if prdc_is_exact(d):
        rng = np.random.default_rng(9000 + d)
        R = rng.integers(-4, 5, (PRDC_N, d)).astype(np.float32)
        F = rng.integers(-4, 5, (PRDC_M, d)).astype(np.float32)
    else:
        R, F = pool3_like(PRDC_N, d, 9100 + d), pool3_like(PRDC_M, d, 9200 + d, 0.02)
    R.setflags(write=False)
    F.setflags(write=False)
    return R, F


@functools.lru_cache(maxsize=None)
def prdc_reference(d, k):
    """_prdc_ref.prdc of prdc_rows(d); computed once, shared, never changed."""
    return _prdc_ref.prdc(*prdc_rows(d), k)


def prdc_ties(ref):
    """Exact ties d2 == r2 of a reference result against (the real radii, the generated radii)."""
    return int(np.sum(ref["cross"] == ref["r2_real"][:, None])), int(np.sum(ref["cross"] == ref["r2_fake"][None, :]))


def prdc_bad_rows():
    """(side, row): the first row, and the last row of a side whose size is no multiple of 64 (replicated into the masked rows)."""
    return [("real", 0), ("real", PRDC_N - 1), ("fake", 0), ("fake", PRDC_M - 1)]


# ---- the recorded bits (tests/golden/rows_tile_bits.npz) ----------------------------------------------------------------------
BITS_WIDTHS = [3, 64, 67, 191]
BITS_NONFINITE_WIDTH = 67
BITS_SPLITS = [0, 3]
BITS_GAMMA = 1 / 200                # tests/test_gpu_cmmd.py's GAMMA
BITS_FILE = "rows_tile_bits.npz"


def bits_mmd_cases():
    """(key, fn, X, Y, index_x | None, index_y | None, gamma | None) of the recorded launches of tise_mmd_poly3_grouped ("pool3"
    rows) and tise_mmd_rbf_grouped ("unit" rows), groups MMD_OX / MMD_OY: the contiguous and the gathered route at every width of
    BITS_WIDTHS, and at d = 67 a NaN in the last row of either side -- the row GtRowFetch::bind replicates into the masked rows."""
    out = []
    for fn, family, gamma in (("tise_mmd_poly3", "pool3", None), ("tise_mmd_rbf", "unit", BITS_GAMMA)):
        for d in BITS_WIDTHS:
            X, Y = mmd_rows(d, family)
            (Xs, ix), (Ys, iy) = shuffled(X, 11 + d), shuffled(Y, 12 + d)
            out.append((f"{fn}/d{d}/contiguous", fn, X, Y, None, None, gamma))
            out.append((f"{fn}/d{d}/gathered", fn, Xs, Ys, ix, iy, gamma))
        X, Y = mmd_rows(BITS_NONFINITE_WIDTH, family)
        nan = float("nan")
        out.append((f"{fn}/d{BITS_NONFINITE_WIDTH}/nan-last-x", fn, with_bad_row(X, MMD_ROWS - 1, nan), Y, None, None, gamma))
        out.append((f"{fn}/d{BITS_NONFINITE_WIDTH}/nan-last-y", fn, X, with_bad_row(Y, MMD_ROWS - 1, nan), None, None, gamma))
    return out


def bits_knn_cases():
    """(key, R, F, k, col_splits) of the recorded launches of tise_knn_radius2 (both sides) and tise_prdc_counts: prdc_rows(d) at
    every width of BITS_WIDTHS, k of PRDC_K, col_splits of BITS_SPLITS, and at d = 67 a NaN in the last row of either side."""
    out = [(f"knn/d{d}/k{k}/s{s}", *prdc_rows(d), k, s) for d in BITS_WIDTHS for k in PRDC_K for s in BITS_SPLITS]
    R, F = prdc_rows(BITS_NONFINITE_WIDTH)
    nan = float("nan")
    out.append((f"knn/d{BITS_NONFINITE_WIDTH}/nan-last-real", with_bad_row(R, PRDC_N - 1, nan), F, 5, 0))
    out.append((f"knn/d{BITS_NONFINITE_WIDTH}/nan-last-fake", R, with_bad_row(F, PRDC_M - 1, nan), 5, 0))
    return out


def check_prdc_case_properties(d, k):
    """What the GPU tests rely on, from the reference alone: ties on both sides for the exact widths, the decision margin for the
    float ones.  -> the figure (ties or margin)."""
    ref = prdc_reference(d, k)
    if prdc_is_exact(d):
        ties = prdc_ties(ref)
        assert ties[0] > 0 and ties[1] > 0, (d, k, ties)
        return ties
    margin = _prdc_ref.smallest_margin(ref)
    assert margin >= MIN_MARGIN, (d, k, margin)
    return margin
