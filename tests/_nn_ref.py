"""Plain numpy restatement of the nearest-row search, AuthPct (Alaa et al. 2022, as dgm-eval states it), the Vendi score (Friedman
& Dieng 2022; linear kernel on L2-normalised rows) and FD-infinity (Chong & Forsyth 2020), written from the published definitions.
Test infrastructure only: the product never imports it.

    d2(a, b) = max(0, (|a|^2 + |b|^2) - 2 a.b)  in fp64 (tests/_prdc_ref.d2_expansion, the form the kernels implement)
    nearest(Q, B): for every row of Q the smallest d2 over the rows of B and the SMALLEST index that attains it
    authentic(g) = d2_train[j*(g)] < d2_gen[g], strict, on squared values;  AuthPct = 100 x mean
    Vendi_q = exp(Renyi entropy of order q of the eigenvalues of X X^T / n), X = rows / |rows| in fp32
    FD-infinity = intercept of the least-squares line of FD_N over 1 / N"""
import numpy as np

from tests import _prdc_ref


def nearest(Q, B, exclude_diagonal=False, d2=None):
    """-> (d2 (n,) fp64, idx (n,) int32, the n x m matrix used).  A NaN entry (a non-finite row) is never the minimum; a row
    with no finite candidate gets (+inf, -1), a NaN query row (NaN, -1)."""
    with np.errstate(invalid="ignore", over="ignore"):                    # non-finite rows are legal inputs here
        D = np.array(_prdc_ref.d2_expansion(Q, B) if d2 is None else d2, dtype=np.float64)
    if exclude_diagonal:
        assert D.shape[0] == D.shape[1]
        np.fill_diagonal(D, np.inf)
    bad_q = ~np.isfinite(np.asarray(Q, dtype=np.float64)).all(axis=1)
    bad_b = ~np.isfinite(np.asarray(B, dtype=np.float64)).all(axis=1)
    D[:, bad_b] = np.inf
    D[bad_q, :] = np.inf
    idx = np.argmin(D, axis=1).astype(np.int32)                           # np.argmin: the first (smallest) index of the minimum
    best = D[np.arange(D.shape[0]), idx]
    idx[np.isinf(best)] = -1
    best[bad_q] = np.nan
    return best, idx, D


def authentic(train, gen):
    """-> dict(idx, d2_gen, d2_train, authentic, authpct)"""
    d2_gen, idx, _ = nearest(gen, train)
    d2_train, _, _ = nearest(train, train, exclude_diagonal=True)
    a = d2_train[idx] < d2_gen
    return dict(idx=idx, d2_gen=d2_gen, d2_train=d2_train, authentic=a, authpct=100.0 * int(a.sum()) / len(a))


def second_best_gap(D):
    """Smallest relative gap (second smallest - smallest) / smallest over the rows of a candidate matrix with >= 2 finite
    entries per row (inf where a row has fewer)."""
    s = np.sort(D, axis=1)
    if s.shape[1] < 2:
        return np.inf
    ok = np.isfinite(s[:, 1])
    return float(np.min((s[ok, 1] - s[ok, 0]) / s[ok, 0])) if ok.any() else np.inf


def normalize_rows_f32(f):
    f = np.asarray(f, dtype=np.float32)
    return f / np.linalg.norm(f, axis=1, keepdims=True).astype(np.float32)


def vendi_eigenvalues(f, route, normalized=False):
    """Eigenvalues (np.linalg.eigvalsh, fp64) of X X^T / n ("rows") or X^T X / n ("cols"), X normalised in fp32 (``normalized``:
    ``f`` holds unit rows already)."""
    x = (np.asarray(f, dtype=np.float32) if normalized else normalize_rows_f32(f)).astype(np.float64)
    g = x @ x.T if route == "rows" else x.T @ x
    return np.linalg.eigvalsh(g / x.shape[0])


def vendi_from_eigenvalues(lam, q=1.0):
    lam = np.asarray(lam, dtype=np.float64)
    lam = lam[lam > 0]
    if q == 1.0:
        return float(np.exp(-np.sum(lam * np.log(lam))))
    if np.isinf(q):
        return float(1.0 / lam.max())
    return float(np.sum(lam ** q) ** (1.0 / (1.0 - q)))


def vendi(f, q=1.0, route="rows", normalized=False):
    return vendi_from_eigenvalues(vendi_eigenvalues(f, route, normalized), q)


def fd_infinity_sizes(m, num_points=15):
    return np.linspace(min(5000, max(m // 10, 2)), m, num_points).astype(np.int32)


def fd_infinity(ref, gen, subsets, frechet):
    """``frechet(mu1, sigma1, mu2, sigma2) -> float``; ``subsets``: index arrays into gen.  -> (intercept, fds)"""
    ref, gen = np.asarray(ref, dtype=np.float64), np.asarray(gen, dtype=np.float64)
    mu_r, sigma_r = ref.mean(axis=0), np.cov(ref, rowvar=False)
    fds = []
    for index in subsets:
        g = gen[index]
        fds.append(float(frechet(mu_r, sigma_r, g.mean(axis=0), np.cov(g, rowvar=False))))
    return float(np.polyfit(1.0 / np.array([len(s) for s in subsets], dtype=np.float64), fds, 1)[1]), np.array(fds)
