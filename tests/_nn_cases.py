"""Inputs shared by tests/test_nn_host.py, tests/test_gpu_nn_argmin.py and tests/test_gpu_memorization.py (seeded; nothing here
touches a GPU).  In the authenticity tests the query rows are the generated side and the base rows the training side."""
import functools

import numpy as np

from tests import _nn_ref
from tests import _prdc_cases as pc

# (query rows, base rows, d): one row; both sides of the 64-row tile edge on both operands; d % 4 != 0; d % 64 != 0 (the GT_RK
# slab); d = 1; a lopsided pair and its swap
SHAPES = [(1, 1, 4), (1, 65, 64), (63, 64, 64), (64, 63, 100), (65, 129, 192), (129, 65, 68), (193, 257, 100), (130, 1000, 2048),
          (1000, 130, 1024), (300, 260, 1), (70, 70, 65), (6, 700, 192), (700, 6, 192)]
SPLITS = pc.RADII_SPLITS
PAD = pc.PAD
MIN_MARGIN = pc.MIN_MARGIN
CONTRACT_D = [64, 100]


def shape_id(s):
    return "q%d-b%d-d%d" % s


@functools.lru_cache(maxsize=None)
def float_rows(q, b, d):
    Q, B = pc.pool3_like(q, d, 7000 + d + q, 0.02), pc.pool3_like(b, d, 9000 + d + b)
    Q.setflags(write=False)
    B.setflags(write=False)
    return Q, B


@functools.lru_cache(maxsize=None)
def float_case(q, b, d):
    """-> (Q, B, ref): ref holds the cross pass (d2, idx, cross), the base set's own pass when b >= 2 (d2_self, idx_self, self) and
    the authenticity result (auth) when b >= 2."""
    Q, B = float_rows(q, b, d)
    d2, idx, cross = _nn_ref.nearest(Q, B)
    ref = dict(d2=d2, idx=idx, cross=cross)
    if b >= 2:
        ref["d2_self"], ref["idx_self"], ref["self"] = _nn_ref.nearest(B, B, exclude_diagonal=True)
        ref["auth"] = _nn_ref.authentic(B, Q)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return Q, B, ref


def smallest_margin(ref):
    """Smallest relative gap of any decision of a float case: best against second-best d2 in the cross and the within-set pass,
    and |d2_train[j*] - d2_gen| / d2_gen of the authenticity comparison."""
    gaps = [_nn_ref.second_best_gap(ref["cross"])]
    if "self" in ref:
        gaps.append(_nn_ref.second_best_gap(ref["self"]))
        a = ref["auth"]
        gaps.append(float(np.min(np.abs(a["d2_train"][a["idx"]] - a["d2_gen"]) / a["d2_gen"])))
    return min(gaps)


def exact_d2(Q, B):
    """int64 squared distances of integer-valued rows."""
    q, b = np.asarray(Q).astype(np.int64), np.asarray(B).astype(np.int64)
    out = np.empty((len(q), len(b)), dtype=np.int64)
    for i in range(len(q)):
        diff = b - q[i]
        out[i] = (diff * diff).sum(axis=1)
    return out


DUPLICATES_0 = (5, 6, 21, 37, 70, 135, 199)      # one thread's two columns (5, 21), a neighbouring lane (6), the other wave column
                                                 # (37), and tiles 1, 2, 3: with two or more splits they span different splits
DUPLICATES_0B = (150, 100)                       # a second group whose first copy is not in the first tile


@functools.lru_cache(maxsize=None)
def integer_case(which):
    """Integer-valued fp32 features: every sum is exact in any order, so equal distances are exact ties and d2 equals the int64
    value.  -> (Q, B, int64 cross matrix, int64 within-set matrix of B)
    0: values -3 .. 3, d = 96, 150 query rows, 200 base rows (4 column tiles).  Base rows DUPLICATES_0 are copies of row 5 and rows
       DUPLICATES_0B copies of row 100.  Query row 3 IS base row 5 (d2 = 0), query row 71 is base row 5 with one coordinate moved by
       1 (d2 = 1 to all seven copies), query row 10 is base row 100.
    1: values -1 .. 1, d = 24, 70 query rows, 300 base rows (5 column tiles): so few distinct distances that nearly every row has
       its minimum at several base rows, in several tiles."""
    rng = np.random.default_rng(11 + which)
    if which == 0:
        Q = rng.integers(-3, 4, (150, 96)).astype(np.float32)
        B = rng.integers(-3, 4, (200, 96)).astype(np.float32)
        for j in DUPLICATES_0:
            B[j] = B[5]
        B[150] = B[100]
        Q[3] = B[5]
        Q[71] = B[5]
        Q[71, 40] += 1.0
        Q[10] = B[100]
    else:
        Q = rng.integers(-1, 2, (70, 24)).astype(np.float32)
        B = rng.integers(-1, 2, (300, 24)).astype(np.float32)
    Q.setflags(write=False)
    B.setflags(write=False)
    return Q, B, exact_d2(Q, B), exact_d2(B, B)


def exact_nearest(D, exclude_diagonal=False):
    """(d2 int64, smallest index of the minimum) per row of an int64 distance matrix."""
    D = D.copy()
    if exclude_diagonal:
        np.fill_diagonal(D, np.iinfo(np.int64).max)
    idx = np.argmin(D, axis=1)
    return D[np.arange(len(D)), idx], idx.astype(np.int32)


# ---- Vendi and FD-infinity ------------------------------------------------------------------------------------------------
VENDI_SHAPES = [(40, 64), (200, 64), (100, 1024)]
FDINF_M = [20, 400, 60000]
FDINF_CASE = (400, 400, 64)


@functools.lru_cache(maxsize=None)
def vendi_rows(n, d):
    """Rows with a decaying spectrum: a few strong directions plus noise, so that the score is neither 1 nor min(n, d)."""
    rng = np.random.default_rng(3000 + n + d)
    basis = rng.standard_normal((8, d))
    X = (rng.standard_normal((n, 8)) * np.array([4, 3, 2, 2, 1, 1, .5, .5])) @ basis + 0.3 * rng.standard_normal((n, d))
    X = X.astype(np.float32)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def fdinf_rows():
    n, m, d = FDINF_CASE
    R, G = pc.pool3_like(n, d, 4100), pc.pool3_like(m, d, 4200, 0.05)
    R.setflags(write=False)
    G.setflags(write=False)
    return R, G
