"""Kernel Inception Distance on MI355X (Binkowski et al. 2018, "Demystifying MMD GANs").

The reference toolbox has FID only.  KID is its standard companion where FID is a poor estimator -- a few dozen to a few
thousand images per set: the per-class O-FID (40-48 crops per class, rank <= 47 covariances in 2048 dimensions), 1 000 + 1 000
image runs, CUB-sized sets.  It is an UNBIASED estimate of MMD^2 between the two sets of pool3 features under the kernel

    k(x, y) = (x.y / d + 1)^3,         MMD^2_u = Sxx / (n (n - 1)) + Syy / (m (m - 1)) - 2 Sxy / (n m)

with Sxx, Syy the kernel sums over i != j and Sxy over all pairs.  The sums come from ``device.PolynomialMMD``
(csrc/mmd.hip: fp64 MFMA, every subset or class in one launch); this module holds the sampling rule and the bookkeeping.

Sampling rule (torch-fidelity ``kid_features_to_metric`` / StyleGAN2-ADA ``kernel_inception_distance``): ``subsets`` subsets
of ``m = min(subset_size, n1, n2)`` rows per side, drawn without replacement by ONE ``numpy.random.RandomState(seed)`` consumed
in subset order -- for each subset the generated side (f2, ``--path2``) first, then the reference side (f1, ``--path1``);
the result is the mean and the standard deviation (ddof 0) of the subsets' MMD^2.  ``subset_size = 0`` is the full-set
estimator: one group of all rows of both sides (n1 != n2 allowed), standard deviation NaN.
"""
from collections import OrderedDict

import numpy as np
import torch

from . import device
from .engine import require_gpu
from .feature_space import rows_f32


def subset_indices(n1, n2, subsets=100, subset_size=1000, seed=0):
    """-> (index1, index2, m): two int64 arrays of subsets * m row numbers (subset s = entries s * m .. (s + 1) * m - 1), drawn as
    the module docstring says.  Host only."""
    n1, n2, subsets, subset_size = int(n1), int(n2), int(subsets), int(subset_size)
    if subsets < 1 or subset_size < 1:
        raise ValueError("subsets and subset_size must be positive (subset_size = 0, the full-set estimator, draws nothing)")
    m = min(subset_size, n1, n2)
    if m < 2:
        raise ValueError(f"KID needs at least 2 rows per side and subset (got {n1} and {n2} rows, subset size {subset_size})")
    rng = np.random.RandomState(int(seed))
    i1 = np.empty((subsets, m), dtype=np.int64)
    i2 = np.empty((subsets, m), dtype=np.int64)
    for s in range(subsets):
        i2[s] = rng.choice(n2, m, replace=False)          # generated side first
        i1[s] = rng.choice(n1, m, replace=False)
    return i1.reshape(-1), i2.reshape(-1), m


def kid_from_features(f1, f2, subsets=100, subset_size=1000, seed=0):
    """KID of two feature sets (device tensors or numpy arrays, (n, dims)) -> (mean, std) as Python floats.
    All subsets go through ONE grouped launch with one index upload per side."""
    require_gpu()
    dev = f1.device if isinstance(f1, torch.Tensor) and f1.is_cuda else torch.device("cuda", torch.cuda.current_device())
    f1, f2 = rows_f32(f1, dev), rows_f32(f2, dev)
    if f1.shape[1] != f2.shape[1]:
        raise ValueError(f"feature widths differ: {f1.shape[1]} and {f2.shape[1]}")
    mmd = device.PolynomialMMD(dev)
    if int(subset_size) == 0:
        v = mmd.mmd2(f1, f2, [0, f1.shape[0]], [0, f2.shape[0]]).cpu().numpy()
        return float(v[0]), float("nan")
    i1, i2, m = subset_indices(f1.shape[0], f2.shape[0], subsets, subset_size, seed)
    offs = np.arange(int(subsets) + 1, dtype=np.int64) * m
    v = mmd.mmd2(f1, f2, offs, offs, i1, i2).cpu().numpy()
    return float(np.mean(v)), float(np.std(v))


def per_class_kid(feats1_sorted, offsets1, feats2_sorted, offsets2, names, min_count=2):
    """One full-set KID per class: rows offsets[i]:offsets[i + 1] of each (class-sorted) feature matrix belong to names[i].
    ONE grouped launch over the classes, no index.  -> (OrderedDict class -> kid, skipped) like calculate_per_class_fid;
    ``skipped`` lists the classes with fewer than ``min_count`` (at least 2) rows on a side."""
    require_gpu()
    dev = feats1_sorted.device if isinstance(feats1_sorted, torch.Tensor) and feats1_sorted.is_cuda else torch.device("cuda", torch.cuda.current_device())
    f1, f2 = rows_f32(feats1_sorted, dev), rows_f32(feats2_sorted, dev)
    o1, o2 = np.asarray(offsets1, dtype=np.int64), np.asarray(offsets2, dtype=np.int64)
    if o1.size != len(names) + 1 or o2.size != len(names) + 1:
        raise ValueError("offsets need one more entry than there are class names")
    out, skipped = OrderedDict(), []
    if not len(names):
        return out, skipped
    v = device.PolynomialMMD(dev).mmd2(f1, f2, o1, o2).cpu().numpy()
    need = max(2, int(min_count))
    for i, c in enumerate(names):
        if o1[i + 1] - o1[i] < need or o2[i + 1] - o2[i] < need:
            skipped.append(c)
        else:
            out[c] = float(v[i])
    return out, skipped
