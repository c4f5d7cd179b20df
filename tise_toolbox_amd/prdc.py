"""Precision, recall, density and coverage on MI355X: the k-nearest-neighbour manifold metrics of Kynkaanniemi et al. 2019
("Improved Precision and Recall Metric for Assessing Generative Models", k = 3) and Naeem et al. 2020 ("Reliable Fidelity and
Diversity Metrics for Generative Models", the ``prdc`` package, k = 5), in the pool3 space FID and KID use.

The reference toolbox has FID only; FID and KID are single numbers and cannot tell a generator that leaves the real manifold
(fidelity) from one that covers only a part of it (diversity).  With R the n real rows (``--path1``), F the m generated rows
(``--path2``), both fp32:

    d2(a, b)  = max(0, (|a|^2 + |b|^2) - 2 a.b)                   in fp64
    r2_R(i)   = the k-th smallest of { d2(R_i, R_j) : j != i }     (the packages' "k + 1-th smallest including self"); r2_F alike
    cnt(i)    = #{ j : d2(R_i, F_j) < r2_R(i) }
    rec(i)    = exists j : d2(R_i, F_j) < r2_F(j)                 prec(j) = exists i : d2(R_i, F_j) < r2_R(i)
    precision = mean_j prec(j)      recall = mean_i rec(i)      density = sum_i cnt(i) / (k m)      coverage = mean_i [cnt(i) > 0]

Every comparison is strict and made on the squared values, as in ``prdc``.  The three passes (radii of R, radii of F, the cross
counts) run in ``device.KnnManifold`` (csrc/knn.hip: fp64 MFMA, no n x n matrix); this module turns the integer results into the
four numbers on the host.  A pair of rows has the same d2 bits in every pass and in either order, so a set compared with itself
meets exact ties at the k-th neighbour and gives precision = recall = density = coverage = 1 exactly.

Duplicate rows: for non-integer features the d2 of two identical rows is a rounding residue of the expansion (the norms are
rounded sums, the dot product is rounded once per accumulation step), of the order of 1e-16 |a|^2, not 0 -- the sklearn-based
packages compute the same expansion and behave the same way.  Integer-valued features (all sums exact) give exactly 0.

Non-finite features: a row that holds a NaN or an infinity has no distance to anything.  The kernels give it r2 = NaN and keep
it out of every other row's neighbours and balls (include/tise_hip.h); ``prdc_from_features`` then raises ValueError, as the
``prdc`` package does (sklearn's pairwise_distances refuses such input) -- four numbers computed around a hole would look valid.

Limits: 1 <= k <= 16, k + 1 <= rows <= 2^24 per side.  There is no CPU fallback.
"""
from collections import OrderedDict

import torch

from . import device
from .engine import require_gpu
from .feature_space import rows_f32


def refuse_nonfinite_rows(sides):
    """``sides``: (name, number of rows that hold a NaN or an infinity, index of the first of them) per side, host integers.
    Raises ValueError for the first side that has such rows -- the ``prdc`` package refuses this input too.  Host only."""
    for what, count, first in sides:
        if count:
            raise ValueError(f"the {what} side has {count} feature row{'s' if count > 1 else ''} with a NaN or an infinity "
                             f"(the first is row {first}); precision, recall, density and coverage are not defined for them")


def prdc_from_features(real, fake, nearest_k=5):
    """``real`` (n, dims), ``fake`` (m, dims): device tensors or numpy arrays -> OrderedDict precision, recall, density,
    coverage (Python floats; the four divisions are done here, from integer sums)."""
    k = int(nearest_k)
    if not 1 <= k <= 16:
        raise ValueError(f"nearest_k must lie in 1 .. 16 (got {nearest_k})")
    for what, f in (("real", real), ("fake", fake)):
        shape = tuple(f.shape)
        if len(shape) != 2:
            raise ValueError("features must be (rows, dims)")
        if shape[0] < k + 1:
            raise ValueError(f"the {what} side has {shape[0]} rows; nearest_k = {k} needs at least {k + 1}")
    if real.shape[1] != fake.shape[1]:
        raise ValueError(f"feature widths differ: {real.shape[1]} and {fake.shape[1]}")
    require_gpu()
    dev = real.device if isinstance(real, torch.Tensor) and real.is_cuda else torch.device("cuda", torch.cuda.current_device())
    R, F = rows_f32(real, dev), rows_f32(fake, dev)
    knn = device.KnnManifold(dev)
    r2R, r2F = knn.radius2(R, k), knn.radius2(F, k)
    cnt, rec, prec = knn.counts(R, r2R, F, r2F)
    n, m = R.shape[0], F.shape[0]
    # r2 is NaN exactly for the rows that hold a non-finite value: their number and the first of them, per side
    bad = []
    for r2 in (r2R, r2F):
        nan = torch.isnan(r2)
        bad += [nan.sum(), torch.where(nan, torch.arange(r2.shape[0], device=dev), r2.shape[0]).min()]
    # ONE device -> host copy of eight integers
    sums = torch.stack([prec.sum(), rec.sum(), cnt.sum(dtype=torch.int64), (cnt > 0).sum()] + bad).cpu().tolist()
    refuse_nonfinite_rows((("real", sums[4], sums[5]), ("fake", sums[6], sums[7])))
    return OrderedDict([("precision", sums[0] / m), ("recall", sums[1] / n), ("density", sums[2] / (k * m)),
                        ("coverage", sums[3] / n)])
