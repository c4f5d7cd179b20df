"""References, bounds and inputs of tests/test_gpu_frechet_kernels.py, and a child-process entry point.

``TISE_SYTRD_ROWS``, ``TISE_SYTRD_TWO_LAUNCH`` and ``TISE_BISECT_NP`` are read once per process (csrc/frechet.hip), so
the kernel instances they select can only be reached from a fresh process: ``python tests/_frechet_child.py`` runs every
case of ``EIG_CHILD_CASES`` through ``tise_eigvalsh`` under the environment it was started with and prints one JSON
list (case name, error / bound ratio, ascending order, digest of the output) on stdout.  Not collected by pytest (no
``test_`` prefix); the parent test starts it, one child at a time.

Notation: u = 2^-53 (fp64 unit roundoff), eps = 2u, gamma_k = k u / (1 - k u).

Eigenvalue bound (every tise_eigvalsh case and every eigenvalue of the distance).  Reference: A = H diag(lam) H^T
formed in long double (64-bit significand) with H a product of Householder reflectors, exactly orthogonal; symmetrised,
then rounded to the fp64 matrix A64 the device sees.  By Weyl the eigenvalues of A64 lie within
    w = ||A64 - A_ld||_F + 16 n u_ld ||lam||_inf * (reflectors)        (u_ld = 2^-64: the long double formation)
of lam.  The device adds the Householder backward error c n eps ||A||_2 (c = 32) and bisection: the bracket stops at
width <= eps max(|glo|, |ghi|) + 2 pivmin (bisect_kernel), |glo|, |ghi| <= ||T||_inf + pad <= 3.01 ||A||_2, the output
is the midpoint, and a Sturm count is exact for a T perturbed by a few eps |T|: 4 eps ||A||_2 covers both.  So
    |w_i - lam_i| <= w + (32 n + 4) eps ||A||_2 + 2 pivmin,
which for w = 0 is (32 n + 4) eps ||A|| <= 7.2e-15 (n + 1) ||A||: tighter than the 5e-14 n max|lam| the older global
check used, at every n >= 1.
"""
import hashlib
import json
import math
import os
import sys

import numpy as np

U = 2.0 ** -53
EPS = 2.0 * U
U_LD = float(np.finfo(np.longdouble).eps) / 2.0
PIVMIN = 2.2250738585072014e-308
C_HH = 32


def gamma(k):
    return k * U / (1.0 - k * U)


# ------------------------------------------------------------------------------------------------- known spectra
def known_spectrum(lam, seed, nrefl=3):
    """(A64, w): A = H diag(lam) H^T in long double (H = nrefl random Householder reflectors), symmetrised and rounded
    to fp64; w = ||A64 - A_ld||_F (long double) + the long double formation error (Weyl term of the module docstring)."""
    lam = np.asarray(lam, dtype=np.longdouble)
    n = lam.size
    a = np.diag(lam)
    rng = np.random.default_rng(seed)
    for _ in range(nrefl if n > 1 else 0):
        v = rng.standard_normal(n).astype(np.longdouble)
        beta = 2.0 / np.dot(v, v)
        av = a @ v
        # (I - b v v^T) A (I - b v v^T) = A - b v (A v)^T - b (A v) v^T + b^2 (v^T A v) v v^T
        a = a - beta * np.outer(v, av) - beta * np.outer(av, v) + (beta * beta * np.dot(v, av)) * np.outer(v, v)
    a = (a + a.T) / 2
    a64 = a.astype(np.float64)
    w = float(np.sqrt(np.sum((a64.astype(np.longdouble) - a) ** 2)))
    w += 16.0 * n * U_LD * max(1, nrefl) * float(np.max(np.abs(lam))) if n else 0.0
    return a64, w


def eig_bound(n, norm2, weyl=0.0):
    return weyl + (C_HH * n + 4) * EPS * norm2 + 2.0 * PIVMIN * max(1.0, norm2 * norm2)


def toeplitz(n):
    """tridiag(-1, 2, -1): eigenvalues 2 - 2 cos(k pi / (n + 1)), k = 1..n (exact input; every column is already zero
    below the subdiagonal, so every reflector is the tau = 0 one)."""
    a = 2.0 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)
    k = np.arange(1, n + 1, dtype=np.longdouble)
    lam = 2 - 2 * np.cos(k * np.pi / np.longdouble(n + 1))
    return a, np.sort(lam.astype(np.float64)), 0.0


def spectrum_case(kind, n, seed):
    """(a64, sorted reference eigenvalues, Weyl term) for one named spectrum."""
    rng = np.random.default_rng(seed)
    if kind == "toeplitz":
        return toeplitz(n)
    if kind == "zero":
        return np.zeros((n, n)), np.zeros(n), 0.0
    if kind == "cI":
        return np.full(n, 0.75) * np.eye(n), np.full(n, 0.75), 0.0
    if kind == "diag":                                     # exact, tau = 0 in every column
        lam = rng.uniform(-2.0, 3.0, n)
        return np.diag(lam), np.sort(lam), 0.0
    if kind == "blockdiag":                                # two dense blocks, exactly zero off-diagonal blocks
        h = n // 2
        a1, w1 = known_spectrum(l1 := rng.uniform(0.0, 2.0, h), seed + 1)
        a2, w2 = known_spectrum(l2 := rng.uniform(-1.0, 1.0, n - h), seed + 2)
        a = np.zeros((n, n))
        a[:h, :h] = a1
        a[h:, h:] = a2
        return a, np.sort(np.concatenate([l1, l2])), w1 + w2
    if kind == "random":
        lam = rng.uniform(0.0, 3.0, n)
    elif kind == "repeats":                                # exact repeats and zeros (the rank-deficient FID spectrum)
        lam = np.concatenate([np.zeros(n // 3), np.full(n // 3, 0.5), rng.uniform(0, 3, n - 2 * (n // 3))])
    elif kind == "negatives":
        lam = rng.uniform(-3.0, 3.0, n)
    elif kind == "graded":                                 # 1 ... 1e-12
        lam = np.logspace(0, -12, n)
    else:
        raise ValueError(kind)
    a, w = known_spectrum(lam, seed)
    return a, np.sort(lam), w


def eig_record(w, ref, weyl, name, instance=None):
    """JSON-ready record: largest |w - ref| / bound, ascending order, digest."""
    n = ref.size
    norm2 = float(np.max(np.abs(ref))) if n else 0.0
    bound = eig_bound(n, norm2 + weyl, weyl)
    err = float(np.max(np.abs(w - ref))) if n else 0.0
    return dict(name=name, n=int(n), instance=instance, ratio=err / bound if bound > 0 else (0.0 if err == 0 else math.inf),
                err=err, bound=bound, ascending=bool(np.all(np.diff(w) >= 0.0)), finite=bool(np.all(np.isfinite(w))),
                digest=hashlib.sha1(np.ascontiguousarray(w).tobytes()).hexdigest())


# the cases every child runs: n = 9 / 65 / 513 / 2048 (fused8: one and several workgroups, a partial last one, the full
# 2048-row LDS), 300 and 1000 (not multiples of 64 or 256: the two-launch scheme's partial row and column chunks)
EIG_CHILD_CASES = [("random", 9), ("diag", 9), ("random", 65), ("cI", 65), ("repeats", 300), ("random", 513),
                   ("blockdiag", 1000), ("negatives", 2048)]


def sytrd_instance(n, env=None):
    """The tridiagonalisation kernel tise_eigvalsh runs for n (n >= 2) under env (run_eigvalsh_inplace's rule)."""
    env = os.environ if env is None else env
    if "TISE_SYTRD_TWO_LAUNCH" in env:
        return "sytrd_step+sytrd_update_matvec"
    if n <= 2048 and "TISE_SYTRD_FUSED_GENERIC" not in env:
        rows = env.get("TISE_SYTRD_ROWS", "8")
        rows = rows if rows in ("4", "16", "82") else "8"
        return {"8": "sytrd_fused8<8,1>", "4": "sytrd_fused8<4,1>", "16": "sytrd_fused8<8,2>", "82": "sytrd_fused8<4,2>"}[rows]
    return "sytrd_fused" if n <= 6144 else "sytrd_step+sytrd_update_matvec"


def bisect_instance(env=None):
    env = os.environ if env is None else env
    np_ = int(env.get("TISE_BISECT_NP", "1"))
    return f"bisect<{1 if np_ == 1 else 4 if np_ == 4 else 2}>"


def instance(n, env=None):
    return f"{sytrd_instance(n, env)} {bisect_instance(env)}"


def run_eig_case(kind, n, dev, solver=None):
    import torch
    from tise_toolbox_amd import device
    a, ref, weyl = spectrum_case(kind, n, seed=n * 7 + len(kind))
    solver = solver or device.FrechetSolver(n, dev)
    w = solver.eigvalsh(torch.as_tensor(a, device=dev)).cpu().numpy()
    return eig_record(w, ref, weyl, f"{kind}_n{n}", instance(n))


def main():
    import torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    from tise_toolbox_amd import _lib
    assert torch.cuda.is_available(), "no HIP device"
    _lib.load()
    dev = torch.device("cuda", 0)
    recs = [run_eig_case(kind, n, dev) for kind, n in EIG_CHILD_CASES]
    json.dump(recs, sys.stdout)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()
