"""Plain numpy restatement of the Kernel Inception Distance, written from the published definition (Binkowski et al. 2018,
"Demystifying MMD GANs", section 2 and appendix: unbiased MMD^2 under k(x, y) = (x.y / d + 1)^3; sampling as in
torch-fidelity / the StyleGAN2-ADA metrics).  Test infrastructure only: the product never imports it.

``dtype=np.longdouble`` gives the extended-precision variant that sizes the tolerances of tests/test_gpu_kid.py."""
import numpy as np


def poly3_sums(x, y, dtype=np.float64):
    """-> (Sxx, Syy, Sxy): sums of k over i != j inside each set and over all pairs across them.  Empty sets give zeros."""
    x = np.asarray(x).astype(dtype)
    y = np.asarray(y).astype(dtype)
    d = dtype(x.shape[1])
    one = dtype(1)

    def gram(a, b):
        return ((a @ b.T) / d + one) ** 3

    def off_diagonal(a):
        if a.shape[0] == 0:
            return dtype(0)
        k = gram(a, a)
        np.fill_diagonal(k, 0)
        return k.sum(dtype=dtype)

    sxy = gram(x, y).sum(dtype=dtype) if x.shape[0] and y.shape[0] else dtype(0)
    return off_diagonal(x), off_diagonal(y), sxy


def mmd2_from_sums(sxx, syy, sxy, n, m):
    """Unbiased estimator; NaN when a side has fewer than 2 rows."""
    if n < 2 or m < 2:
        return float("nan")
    return sxx / (n * (n - 1)) + syy / (m * (m - 1)) - 2 * sxy / (n * m)


def mmd2(x, y, dtype=np.float64):
    return mmd2_from_sums(*poly3_sums(x, y, dtype), len(x), len(y))


def subset_indices(n1, n2, subsets, subset_size, seed):
    """One RandomState consumed in subset order; per subset the generated side (f2 / path2) first, then the reference side."""
    m = min(subset_size, n1, n2)
    rng = np.random.RandomState(seed)
    i1, i2 = [], []
    for _ in range(subsets):
        i2.append(rng.choice(n2, m, replace=False))
        i1.append(rng.choice(n1, m, replace=False))
    return i1, i2, m


def kid_from_features(f1, f2, subsets=100, subset_size=1000, seed=0, dtype=np.float64, return_terms=False):
    """-> (mean, std ddof 0) of the subsets' MMD^2; subset_size = 0: the full-set estimator, std NaN.
    ``return_terms``: also the largest |Sxx| / (n (n - 1)) + |Syy| / (m (m - 1)) + 2 |Sxy| / (n m) met -- the scale a relative
    error of the three sums is multiplied by on its way into the estimator."""
    f1, f2 = np.asarray(f1), np.asarray(f2)
    if subset_size == 0:
        s = poly3_sums(f1, f2, dtype)
        n, m = len(f1), len(f2)
        out = (float(mmd2_from_sums(*s, n, m)), float("nan"))
        scale = float(abs(s[0]) / (n * (n - 1)) + abs(s[1]) / (m * (m - 1)) + 2 * abs(s[2]) / (n * m))
        return out + (scale,) if return_terms else out
    i1, i2, m = subset_indices(len(f1), len(f2), subsets, subset_size, seed)
    vals, scale = [], 0.0
    for a, b in zip(i1, i2):
        s = poly3_sums(f1[a], f2[b], dtype)
        vals.append(mmd2_from_sums(*s, m, m))
        scale = max(scale, float(abs(s[0]) / (m * (m - 1)) + abs(s[1]) / (m * (m - 1)) + 2 * abs(s[2]) / (m * m)))
    vals = np.asarray(vals, dtype=dtype)
    out = (float(np.mean(vals)), float(np.std(vals)))
    return out + (scale,) if return_terms else out


def per_class_kid(feats1_sorted, offsets1, feats2_sorted, offsets2, names, min_count=2):
    from collections import OrderedDict
    out, skipped = OrderedDict(), []
    for i, c in enumerate(names):
        x = feats1_sorted[offsets1[i]:offsets1[i + 1]]
        y = feats2_sorted[offsets2[i]:offsets2[i + 1]]
        if len(x) < max(2, min_count) or len(y) < max(2, min_count):
            skipped.append(c)
        else:
            out[c] = float(mmd2(x, y))
    return out, skipped
