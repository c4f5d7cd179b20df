"""Authenticity (AuthPct) on MI355X: is the generator copying its training set?

Alaa et al. 2022 ("How Faithful is your Synthetic Data?"), as the `dgm-eval` package of Stein et al. 2023 computes it
(``authpct.py``; the definition is RESTATED FROM MEMORY, README).  With T the n training rows, G the m generated rows, both fp32,
and d2 the fp64 squared distance of prdc.py:

    j*(g)     = the training row nearest to G_g (the smallest index on a tie),   d1^2(g) = d2(G_g, T_j*(g))
    d2^2(t)   = min over t' != t of d2(T_t, T_t')                                 (the training set's own nearest-neighbour distance)
    authentic(g) = d2^2(j*(g)) < d1^2(g)                                          strict, on the squared fp64 values
    AuthPct   = 100 x mean_g authentic(g)

A sample that sits closer to a training row than that row's own nearest training neighbour does is counted as a copy.  Both
searches run in ``device.KnnManifold.nearest`` (tise_nn_argmin, csrc/knn.hip: fp64 MFMA, no m x n matrix, bitwise reproducible);
the comparison and the count are done on the device, the division here.  dgm-eval compares fp32 ``torch.cdist`` values (not
squared; the square root is monotonic), so the two can part only where fp32 rounding makes or breaks a tie.

``nearest_train`` returns the per-sample evidence -- which training row, how far -- which is what one looks at in practice.

Non-finite features: a row that holds a NaN or an infinity has no distance to anything; ValueError, as prdc.prdc_from_features.
Limits: 2 <= training rows, 1 <= generated rows, at most 2^24 per side.  There is no CPU fallback.
"""
import numpy as np
import torch

from . import device
from .engine import require_gpu
from .feature_space import rows_f32


def _check_shapes(train, gen):
    for f in (train, gen):
        if len(tuple(f.shape)) != 2:
            raise ValueError("features must be (rows, dims)")
    if train.shape[0] < 2:
        raise ValueError(f"the training side has {train.shape[0]} row{'s' if train.shape[0] != 1 else ''}; authenticity needs each "
                         "training row's nearest OTHER training row: at least 2")
    if gen.shape[0] < 1:
        raise ValueError("the generated side has no rows")
    if train.shape[1] != gen.shape[1]:
        raise ValueError(f"feature widths differ: {train.shape[1]} and {gen.shape[1]}")
    if train.shape[1] < 1:
        raise ValueError("features need at least one column")


def refuse_nonfinite_rows(sides):
    """``sides``: (name, number of rows that hold a NaN or an infinity, index of the first of them) per side, host integers.
    Raises ValueError for the first side that has such rows.  Host only."""
    for what, count, first in sides:
        if count:
            raise ValueError(f"the {what} side has {count} feature row{'s' if count > 1 else ''} with a NaN or an infinity "
                             f"(the first is row {first}); authenticity is not defined for them")


def _search(train, gen):
    """-> (idx int32 (m,), d2_gen fp64 (m,), d2_train fp64 (n,), authentic bool (m,)) device tensors, non-finite rows refused."""
    _check_shapes(train, gen)
    require_gpu()
    dev = train.device if isinstance(train, torch.Tensor) and train.is_cuda else torch.device("cuda", torch.cuda.current_device())
    T, G = rows_f32(train, dev), rows_f32(gen, dev)
    knn = device.KnnManifold(dev)
    d2_gen, idx = knn.nearest(G, T)
    d2_train, _ = knn.nearest(T, T, exclude_diagonal=True)
    # d2 is NaN exactly for the query rows that hold a non-finite value: their number and the first of them, per side
    bad = []
    for d2 in (d2_train, d2_gen):
        nan = torch.isnan(d2)
        bad += [nan.sum(), torch.where(nan, torch.arange(d2.shape[0], device=dev), d2.shape[0]).min()]
    bad = torch.stack(bad).cpu().tolist()                                  # ONE device -> host copy of four integers
    refuse_nonfinite_rows((("training", bad[0], bad[1]), ("generated", bad[2], bad[3])))
    authentic = d2_train[idx.long()] < d2_gen
    return idx, d2_gen, d2_train, authentic


def nearest_train(train, gen):
    """``train`` (n, dims), ``gen`` (m, dims): device tensors or numpy arrays -> dict of numpy arrays: ``idx`` (m,) int32 the
    nearest training row of every generated row, ``d2_gen`` (m,) fp64 its squared distance, ``d2_train`` (n,) fp64 every training
    row's squared distance to its nearest other training row, ``authentic`` (m,) bool."""
    idx, d2_gen, d2_train, authentic = _search(train, gen)
    return dict(idx=idx.cpu().numpy(), d2_gen=d2_gen.cpu().numpy(), d2_train=d2_train.cpu().numpy(), authentic=authentic.cpu().numpy())


def authpct_from_counts(n_authentic, m):
    """100 x the authentic share, from the integer count (host)."""
    return 100.0 * int(n_authentic) / int(m)


def authpct_from_features(train, gen):
    """AuthPct of ``gen`` against ``train`` (device tensors or numpy arrays, (rows, dims)) -> Python float in [0, 100]."""
    authentic = _search(train, gen)[3]
    return authpct_from_counts(authentic.sum().item(), authentic.shape[0])
