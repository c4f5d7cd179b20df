"""The Vendi score on MI355X: how many effectively different samples are there?

Friedman & Dieng 2022 ("The Vendi Score: A Diversity Evaluation Metric for Machine Learning"), with the choices of the `dgm-eval`
package of Stein et al. 2023: the linear kernel on L2-normalised rows, order q = 1 (the definition is RESTATED FROM MEMORY,
README).  With X the n rows, normalised in fp32 (cmmd.normalize_rows), and lambda the eigenvalues of K / n, K = X X^T:

    Vendi_1   = exp(- sum over lambda > 0 of lambda ln lambda)            the exponential of the Shannon entropy of the spectrum
    Vendi_q   = exp(ln(sum lambda^q) / (1 - q))                           q != 1, q >= 0 (Renyi);   Vendi_inf = 1 / max lambda

n identical rows give 1, n mutually orthogonal rows give n.  The non-zero eigenvalues of X X^T / n (n x n) and of X^T X / n
(d x d) are the same, so the smaller of the two Gram matrices is formed -- in fp64 on the matrix cores, from the fp64 widening of
the fp32 rows (device.gemm_f64, over row chunks for the d x d form) -- and its eigenvalues come from the Frechet solver's symmetric
eigenvalue routine (tise_eigvalsh: tridiagonalisation + bisection).  The entropy is summed on the host in fp64.  No new kernel.

A row that holds a NaN or an infinity, or a zero row (it has no direction), is refused with ValueError.
"""
import math

import numpy as np
import torch

from . import device
from .engine import frechet_solver, require_gpu
from .feature_space import rows_f32

GRAM_CHUNK = 8192            # rows widened to fp64 at a time in the d x d route


def vendi_from_eigenvalues(lam, q=1.0):
    """The score from the spectrum of K / n (any array; entries <= 0 are the null space's and its rounding, and are dropped).  Host."""
    q = float(q)
    if math.isnan(q) or q < 0:
        raise ValueError(f"the order q must be >= 0 (got {q})")
    lam = np.asarray(lam, dtype=np.float64).reshape(-1)
    lam = lam[lam > 0]
    if lam.size == 0:
        raise ValueError("no positive eigenvalue")
    if q == 1.0:
        return float(np.exp(-np.sum(lam * np.log(lam))))
    if math.isinf(q):
        return float(np.exp(-np.log(lam.max())))
    return float(np.exp(np.log(np.sum(lam ** q)) / (1.0 - q)))


def gram_route(n, d, route=None):
    """"rows" (the n x n matrix X X^T) or "cols" (the d x d matrix X^T X): the caller's choice, else the smaller.  Host."""
    if route is None:
        return "rows" if n <= d else "cols"
    if route not in ("rows", "cols"):
        raise ValueError(f"route must be 'rows', 'cols' or None (got {route!r})")
    return route


def vendi_eigenvalues(f, route=None):
    """``f`` (n, dims): a device tensor or numpy array -> the eigenvalues of the chosen Gram matrix / n, ascending, fp64 numpy
    (min(n, dims) of them on the default route)."""
    from . import cmmd
    if len(tuple(f.shape)) != 2 or f.shape[0] < 1 or f.shape[1] < 1:
        raise ValueError("features must be (rows, dims) with at least one row and one column")
    route = gram_route(f.shape[0], f.shape[1], route)
    require_gpu()
    dev = f.device if isinstance(f, torch.Tensor) and f.is_cuda else torch.device("cuda", torch.cuda.current_device())
    x = cmmd.normalize_rows(rows_f32(f, dev))
    n, d = x.shape
    bad = ~torch.isfinite(x).all(dim=1)
    count, first = torch.stack([bad.sum(), torch.where(bad, torch.arange(n, device=dev), n).min()]).cpu().tolist()
    if count:
        raise ValueError(f"{count} feature row{'s' if count > 1 else ''} cannot be normalised: a NaN, an infinity or a zero row "
                         f"(the first is row {first}); the Vendi score is not defined for them")
    with torch.cuda.device(dev):
        if route == "rows":
            x64 = x.double()
            g = device.gemm_f64(x64, x64.t())
        else:
            g = torch.zeros((d, d), dtype=torch.float64, device=dev)
            for i in range(0, n, GRAM_CHUNK):
                x64 = x[i:i + GRAM_CHUNK].double()
                g += device.gemm_f64(x64.t(), x64)
        g /= n
        k = g.shape[0]
        if k == 1:
            return g.reshape(1).cpu().numpy()
        return frechet_solver(k, dev).eigvalsh(g).cpu().numpy()


def vendi_from_features(f, q=1.0, route=None):
    """The Vendi score of order ``q`` of one feature set (device tensor or numpy array, (n, dims)) -> Python float in [1, n]."""
    vendi_from_eigenvalues([1.0], q)                                       # a bad order: say so before the GPU is asked for
    return vendi_from_eigenvalues(vendi_eigenvalues(f, route), q)
