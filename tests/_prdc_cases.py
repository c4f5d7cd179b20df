"""Inputs shared by tests/test_prdc_host.py and tests/test_gpu_prdc.py (seeded; nothing here touches a GPU)."""
import functools

import numpy as np

from tests import _prdc_ref

RADII_K = [1, 3, 5, 16]
RADII_D = [64, 100, 192, 2048]
RADII_SPLITS = [0, 1, 2, 3, 7]
PAD = 12                     # padding columns of every uploaded row, filled with 7.0: never to be read

# (n, m, d, k, shift); the last two are the lopsided pair and its swap
COUNT_SHAPES = [(300, 260, 64, 5, .02), (130, 65, 2048, 3, .02), (193, 257, 100, 5, .05), (1000, 1000, 2048, 5, .03),
                (6, 700, 192, 5, .02), (700, 6, 192, 5, .02)]
COUNT_SPLITS = [0, 1, 3]
MIN_MARGIN = 1e-9            # every decision's |d2 - r2| / r2 on the float cases, asserted from the reference alone


def radii_rows(k):
    """Row counts of the radii test for one k: k + 1 (the smallest legal set) and both sides of the 64-row tile edges."""
    return [k + 1, 63, 64, 65, 127, 128, 129, 193, 1000]


def pool3_like(rows, d, seed, shift=0.0):
    """Seeded, non-negative, pool3-scaled rows."""
    return (np.abs(np.random.default_rng(seed).standard_normal((rows, d))) * 0.5 + shift).astype(np.float32)


@functools.lru_cache(maxsize=None)
def radii_set(n, d):
    """-> (X, its own fp64 d2 matrix sorted along the rows): sorted[:, k] is r2 for every k."""
    X = pool3_like(n, d, 1000 * d + n)
    s = np.sort(_prdc_ref.d2_expansion(X, X), axis=1)
    X.setflags(write=False)
    s.setflags(write=False)
    return X, s


@functools.lru_cache(maxsize=None)
def count_case(n, m, d, k, shift):
    """-> (R, F, reference result of _prdc_ref.prdc)"""
    R, F = pool3_like(n, d, 1 + d, 0.0), pool3_like(m, d, 2 + d, shift)
    R.setflags(write=False)
    F.setflags(write=False)
    return R, F, _prdc_ref.prdc(R, F, k)


@functools.lru_cache(maxsize=None)
def integer_case(which):
    """Integer-valued fp32 features: every sum is exact in any order, so ties d2 == r2 are exact ties.
    0: values -3 .. 3, n = 200, m = 150, d = 96, k = 5.
    1: values -1 .. 1, d = 24, n = 150, m = 140, k = 5; rows 10 .. 17 of R are 8 copies of one row (r2 = 0 there), and rows 0 .. 2
       of F are rows 40 .. 42 of R."""
    rng = np.random.default_rng(5)
    if which == 0:
        R = rng.integers(-3, 4, (200, 96)).astype(np.float32)
        F = rng.integers(-3, 4, (150, 96)).astype(np.float32)
    else:
        R = rng.integers(-1, 2, (150, 24)).astype(np.float32)
        F = rng.integers(-1, 2, (140, 24)).astype(np.float32)
        R[10:18] = R[10]
        F[0:3] = R[40:43]
    R.setflags(write=False)
    F.setflags(write=False)
    return R, F, 5, _prdc_ref.prdc(R, F, 5)
