"""Plain numpy restatement of CMMD, written from the published definition (Jayasumana et al., CVPR 2024, "Rethinking FID":
MMD^2 under k(a, b) = exp(-|a - b|^2 / (2 sigma^2)), sigma = 10, on L2-normalised embeddings, reported x 1000).  Test
infrastructure only: the product never imports it.

``rbf_sums`` restates what the kernel computes (csrc/mmd.hip), with the same parenthesisation of d^2, the clamp and the diagonal
left out; ``dtype=np.longdouble`` gives the extended-precision variant that sizes the tolerances of tests/test_gpu_cmmd.py.
``cmmd_v`` / ``cmmd_u`` are the textbook forms on full kernel matrices from |a - b|^2 itself: independent of the sums."""
import numpy as np

SIGMA = 10.0
SCALE = 1000.0


def rbf_sums(xs, ys, gamma, dtype=np.float64):
    """-> (Sxx, Syy, Sxy) of k(a, b) = exp(-gamma max(0, (|a|^2 + |b|^2) - 2 a.b)): over i != j inside each set, over all pairs
    across them.  Empty sets give zeros."""
    x = np.asarray(xs).astype(dtype)
    y = np.asarray(ys).astype(dtype)
    g = dtype(gamma)
    zero, two = dtype(0), dtype(2)

    def kernel(a, b):
        na, nb = (a * a).sum(axis=1, dtype=dtype), (b * b).sum(axis=1, dtype=dtype)
        d2 = np.maximum(zero, (na[:, None] + nb[None, :]) - two * (a @ b.T))
        return np.exp(-g * d2)

    def off_diagonal(a):
        if a.shape[0] == 0:
            return zero
        k = kernel(a, a)
        np.fill_diagonal(k, 0)
        return k.sum(dtype=dtype)

    sxy = kernel(x, y).sum(dtype=dtype) if x.shape[0] and y.shape[0] else zero
    return off_diagonal(x), off_diagonal(y), sxy


def _full_kernel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d2 = np.stack([((row[None, :] - b) ** 2).sum(axis=1) for row in a]) if len(a) else np.zeros((0, len(b)))
    return np.exp(-d2 / (2 * SIGMA ** 2))


def cmmd_v(x, y):
    """The published implementation's V-statistic: the means of the three full kernel matrices, diagonals included."""
    return SCALE * (_full_kernel(x, x).mean() + _full_kernel(y, y).mean() - 2 * _full_kernel(x, y).mean())


def cmmd_u(x, y):
    """The paper's unbiased estimator: within-set means over i != j."""
    n, m = len(x), len(y)
    kxx, kyy = _full_kernel(x, x), _full_kernel(y, y)
    sxx, syy = kxx.sum() - np.trace(kxx), kyy.sum() - np.trace(kyy)
    return SCALE * (sxx / (n * (n - 1)) + syy / (m * (m - 1)) - 2 * _full_kernel(x, y).mean())
