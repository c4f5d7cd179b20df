"""GPU: every stage of the Frechet solver (csrc/frechet.hip) pinned to references that do not use scipy's sqrtm, at
every kernel instance and at the panel, tile and early-out edges.

Notation (tests/_frechet_child.py): u = 2^-53, eps = 2u, gamma_k = k u / (1 - k u).  References are exact (integer or
closed-form inputs), long double constructions with a Weyl term, or fp64 LAPACK/BLAS with their own error added to the
bound.  Each bound is derived in the test's docstring; the largest observed error / bound ratio of each group is printed.
Process-static switches run in child processes (tests/_frechet_child.py), one at a time, each under a time limit.
"""
import functools
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

from tests import _cases
from tests import _frechet_child as fc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U, EPS, gamma = fc.U, fc.EPS, fc.gamma


@pytest.fixture(scope="module")
def dev(cuda_device):
    return cuda_device


def _solver(d, dev):
    from tise_toolbox_amd import device
    return device.FrechetSolver(d, dev)


# ================================================================================================== GEMM
_GEMM_DIMS = (1, 15, 16, 17, 63, 64, 65, 127, 129)


def _gemm_cases():
    rng = np.random.default_rng(5)
    cases = [(m, n, k) for m, n, k in zip(_GEMM_DIMS, _GEMM_DIMS[::-1], rng.permutation(_GEMM_DIMS))]
    cases += [(65, 17, 1), (129, 127, 15), (17, 65, 16), (64, 64, 17), (127, 129, 129), (16, 16, 0), (63, 65, 0)]
    return cases


def _gemm_raw(a, sam, sak, b, sbk, sbn, c, ldc, m, n, k):
    from tise_toolbox_amd import _lib, device
    _lib.call("tise_gemm_f64", device._ptr(a), sam, sak, device._ptr(b), sbk, sbn, device._ptr(c), ldc, m, n, k,
              device._stream())
    torch.cuda.synchronize()


def _layouts(x):
    """(tensor holding the data, stride along dim 0, stride along dim 1) for the row- and the column-major copy."""
    r, c = x.shape
    row = torch.as_tensor(np.ascontiguousarray(x))
    col = torch.as_tensor(np.ascontiguousarray(x.T))
    return ((row, c, 1), (col, 1, r))


@pytest.mark.parametrize("m,n,k", _gemm_cases())
def test_gemm_componentwise_and_untouched(dev, m, n, k):
    """tise_gemm_f64, all four stride layouts.  Random inputs: |C - AB| <= gamma_k (|A||B|) per element (each fp64 MFMA
    step is a correctly rounded fused multiply-add); the exact AB is formed in long double, whose own error
    gamma_k^ld (|A||B|) is added.  Integer inputs (|sum| < 2^53): the result is EXACT.  The output is written with
    ldc = n + 7 into a NaN-filled buffer: nothing outside the m x n block changes.  k = 0 writes zeros."""
    rng = np.random.default_rng(m * 10007 + n * 101 + k)
    worst = 0.0
    for kind in ("randn", "int"):
        a = rng.standard_normal((m, k)) if kind == "randn" else rng.integers(-64, 65, (m, k)).astype(np.float64)
        b = rng.standard_normal((k, n)) if kind == "randn" else rng.integers(-64, 65, (k, n)).astype(np.float64)
        exact = a.astype(np.longdouble) @ b.astype(np.longdouble)
        mag = np.abs(a) @ np.abs(b)
        bound = (gamma(k) + 2.0 * k * fc.U_LD) * mag if kind == "randn" else np.zeros((m, n))
        for ta, sam, sak in _layouts(a):
            for tb, sbk, sbn in _layouts(b):
                ta_d, tb_d = (ta.to(dev), tb.to(dev)) if k else (torch.ones(1, dtype=torch.float64, device=dev),) * 2
                ldc = n + 7
                buf = torch.full((m + 1, ldc), float("nan"), dtype=torch.float64, device=dev)
                _gemm_raw(ta_d, sam, sak, tb_d, sbk, sbn, buf, ldc, m, n, k)
                got = buf.cpu().numpy()
                c = got[:m, :n]
                err = np.abs(c.astype(np.longdouble) - exact).astype(np.float64)
                assert np.all(err <= bound), (kind, sam, sak, sbk, sbn, float(err.max()))
                if kind == "randn" and k:
                    worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
                assert np.all(np.isnan(got[:m, n:])) and np.all(np.isnan(got[m:])), "wrote outside the m x n block"
    print(f"gemm m={m} n={n} k={k}: worst ratio {worst:.3g}")


def test_gemm_empty_shapes_are_noops(dev):
    """m = 0 and n = 0 return OK and write nothing (real device addresses: an empty tensor has a null pointer)."""
    a = torch.ones((16, 16), dtype=torch.float64, device=dev)
    c = torch.full((16, 16), float("nan"), dtype=torch.float64, device=dev)
    _gemm_raw(a, 16, 1, a, 16, 1, c, 16, 0, 16, 16)
    _gemm_raw(a, 16, 1, a, 16, 1, c, 16, 16, 0, 16)
    assert bool(torch.isnan(c).all())


# ================================================================================================== Cholesky
def _full_sigma(d, seed):
    """fp64 SPD matrix, G G^T / m with m = d + 32 samples: full numerical rank at every d here."""
    g = np.random.default_rng(seed).standard_normal((d, d + 32))
    return (g @ g.T) / (d + 32)


def _lowrank_sigma(d, r, seed):
    """Exact rank r, dense: G G^T with integer G (d x r, entries in [-3, 3]); every product and sum is exact."""
    g = np.random.default_rng(seed).integers(-3, 4, (d, r)).astype(np.float64)
    return g @ g.T


def _padded_sigma(d, r, seed):
    """Exact rank r that the pivoted rule must find EXACTLY: an r x r SPD block on randomly placed rows / columns, the
    other d - r rows and columns exactly zero (their downdated diagonal stays 0.0, so the pivot after step r is 0)."""
    rng = np.random.default_rng(seed)
    idx = np.sort(rng.permutation(d)[:r])
    s = np.zeros((d, d))
    if r:
        s[np.ix_(idx, idx)] = _full_sigma(r, seed + 1)
    return s


@functools.lru_cache(maxsize=None)
def _factor_case(d, kind, seed):
    if kind == "full":
        return _full_sigma(d, seed)
    if kind == "lowrank":
        return _lowrank_sigma(d, d // 2, seed)
    return _padded_sigma(d, int(kind[6:]), seed)                # "padded<r>"


def _prefactor(d, s, dev, pivoted, monkeypatch):
    solver = _solver(d, dev)
    if pivoted:
        monkeypatch.setenv("TISE_CHOL_PIVOTED", "1")
    else:
        monkeypatch.delenv("TISE_CHOL_PIVOTED", raising=False)
    solver.prefactor(torch.as_tensor(s, device=dev))
    lt, r, unpivoted = solver.factor()
    monkeypatch.delenv("TISE_CHOL_PIVOTED", raising=False)
    return lt.cpu().numpy(), r, unpivoted


def _check_factor(s, lt, r, unpivoted, rank_exact):
    """Checks of the docstring of test_cholesky_factor; returns (residual ratio, extra-pivot ratio)."""
    d = s.shape[0]
    g = gamma(d + 1)
    assert np.all(np.isfinite(lt))
    assert np.all(lt[r:] == 0.0), "rows >= rank must be zero"
    alt = np.abs(lt)
    mag = alt.T @ alt                                         # |L||L^T|
    res = np.abs(s - lt.T @ lt)                               # the check's own product rounds: + gamma_d |L||L^T|
    bound = (g + gamma(d)) * mag * (1 + 4 * U) + U * np.abs(s)
    diag = np.diag(s)

    def residual_ratio(b):
        ratio = float(np.max(res / np.maximum(b, 1e-300)))
        assert ratio <= 1.0, ratio
        return ratio
    extra = 0.0
    if r == d:
        ratio = residual_ratio(bound)
    if unpivoted:
        assert r == d
        assert np.all(np.tril(lt, -1) == 0.0), "unpivoted L^T must be upper triangular"
        assert np.all(np.diag(lt) > 0.0)
        return ratio, extra
    if r == 0:
        assert rank_exact == 0 and np.all(s == 0.0)
        return 0.0, extra
    # pivot of column k: a column whose entries in rows k+1 .. r-1 are all zero (chosen columns get exact zeros
    # afterwards) and whose row-k entry is positive; among several (a noise column may round to exact zeros too) the
    # largest, which sqrt(pivot) is (|l_ik| <= l_kk by Cauchy-Schwarz on the positive semi-definite Schur complement)
    nz = lt[:r] != 0.0
    last = np.where(nz.any(axis=0), r - 1 - np.argmax(nz[::-1], axis=0), -1)
    piv = []
    for k in range(r):
        cand = np.setdiff1d(np.nonzero((last == k) & (lt[k] > 0.0))[0], piv)
        assert cand.size >= 1, f"column {k}: no pivot"
        piv.append(int(cand[np.argmax(lt[k, cand])]))
    piv = np.asarray(piv, dtype=np.int64)
    assert np.unique(piv).size == r, "pivot indices must be unique"
    lkk2 = lt[np.arange(r), piv] ** 2
    tol = 4.0 * g * float(diag.max())
    assert np.all(np.diff(lkk2) <= tol), "l_kk must be non-increasing within rounding"
    # diagonal pivoting: l_kk^2 is the largest downdated diagonal among the columns not chosen yet
    down = diag[None, :] - np.cumsum(np.vstack([np.zeros((1, d)), lt[:r - 1] ** 2]), axis=0)
    chosen = np.zeros(d, dtype=bool)
    for k in range(r):
        free = ~chosen
        assert lkk2[k] >= float(down[k][free].max()) - tol, f"pivot {k} is not the largest remaining diagonal"
        chosen[piv[k]] = True
    if r < d:
        # stopped early on an exact-rank input: Higham Thm 10.14 with S's exact Schur complement 0 after rank_exact
        # pivots, ||S - L1 L1^T||_2 <= 2 (r0 + 1) u (1 + ||W||_2)^2 ||S||_2 (x 2: second order), W = L11^-1 L21^T in
        # pivot order; the columns past r0 add their own |L2||L2^T|
        from scipy.linalg import solve_triangular
        r0 = rank_exact
        others = np.setdiff1d(np.arange(d), piv[:r0])
        l11 = lt[:r0][:, piv[:r0]].T
        w = solve_triangular(l11, lt[:r0][:, others], lower=True) if r0 else np.zeros((0, 0))
        nw = float(np.linalg.norm(w, 2)) if w.size else 0.0
        l2 = alt[r0:r]
        bound = bound + 4.0 * (r0 + 1) * U * (1.0 + nw) ** 2 * float(np.linalg.norm(s, 2)) + l2.T @ l2
        ratio = residual_ratio(bound)
    if rank_exact is not None:
        assert r >= rank_exact
        if r > rank_exact:                                    # the columns past the true rank: rounding only
            extra = float(lkk2[rank_exact:].max() / tol)
            assert extra <= 1.0, extra
    return ratio, extra


_FACTOR_CELLS = ([(d, False) for d in (1, 2, 15, 16, 17, 63)] +
                 [(d, p) for d in (64, 65, 127, 128, 129, 1000, 1024, 1025, 1536, 2047, 2048) for p in (False, True)] +
                 [(d, False) for d in (2049, 2304)])


@pytest.mark.parametrize("kind", ["full", "lowrank"])
@pytest.mark.parametrize("d,pivoted", _FACTOR_CELLS)
def test_cholesky_factor(dev, d, pivoted, kind, monkeypatch):
    """The factor tise_frechet_prefactor leaves (read back by tise_frechet_factor), every factorisation instance:
    d < 64 pivoted <1> only; 64 <= d <= 1024 unpivoted and pivoted <1> (TISE_CHOL_PIVOTED, read per call);
    1024 < d <= 2048 unpivoted and pivoted <2>; d > 2048 the unblocked pivoted kernels.

    Residual (Higham Thm 10.3, any summation order): |S - L L^T| <= gamma_{d+1} |L||L^T|, plus gamma_d |L||L^T| for
    the check's own fp64 product.  Rank-deficient stop: the rule ends when every remaining computed diagonal is <= 0,
    and the inputs have an exact rank r0 (integer or exactly zero rows), whose exact Schur complement is 0: Higham
    Thm 10.14, ||S - L1 L1^T||_2 <= 2 (r0 + 1) u (1 + ||W||_2)^2 ||S||_2 (doubled for the second order), W = L11^-1 L21^T
    of the first r0 pivots, plus |L2||L2^T| of the columns past r0, added to every element.  Pivoted: indices unique, l_kk^2 non-increasing and each the largest downdated diagonal left, both
    within tol = 4 gamma_{d+1} max S_ii (the downdated diagonal of the kernel and of this check round differently by
    at most 2 gamma_{d+1} D_i <= 4 gamma_{d+1} max S_ii).  The columns past the exact rank (integer input, so the exact
    Schur complement after the true rank is 0): their pivots are pure downdate rounding, l_kk^2 <= tol.  Full rank:
    rank d, and the unpivoted request is served by the unpivoted factor; rank-deficient: its pivot fails and the
    pivoted factor is returned."""
    s = _factor_case(d, kind, d * 3 + 1)
    lt, r, unpivoted = _prefactor(d, s, dev, pivoted, monkeypatch)
    rank_true = d if kind == "full" else d // 2
    if kind == "full":
        assert r == d
        assert unpivoted == (not pivoted and 64 <= d <= 2048)
    else:
        assert not unpivoted and r >= rank_true
    ratio, extra = _check_factor(s, lt, r, unpivoted, None if kind == "full" else rank_true)
    print(f"cholesky d={d} {'pivoted' if not unpivoted else 'unpivoted'} {kind}: rank {r}, residual ratio {ratio:.3g}, "
          f"extra pivots ratio {extra:.3g}")


@pytest.mark.parametrize("d,r", [(1000, 15), (1000, 16), (1000, 17), (1000, 127), (1000, 128), (1000, 129),
                                 (2048, 127), (2048, 128), (2048, 129), (2048, 1000),
                                 (2304, 127), (2304, 128), (2304, 129)])
def test_cholesky_rank_at_panel_and_early_out_edges(dev, d, r, monkeypatch):
    """Exact-rank inputs (an SPD block on scattered rows, zeros elsewhere) whose rank ends just before, at and after a
    16-pivot panel and the host's early-out cadence ((nblk & 7) == 7 blocked, (k & 127) == 127 unblocked): the rank is
    found EXACTLY, the factor satisfies the bounds of test_cholesky_factor, and the distance reports the rank and the
    rank-deficient flag."""
    s = _factor_case(d, f"padded{r}", 11 * r + d)
    lt, rk, unpivoted = _prefactor(d, s, dev, True, monkeypatch)
    assert rk == r and not unpivoted
    ratio, _ = _check_factor(s, lt, rk, unpivoted, r)
    res = _solver(d, dev).distance(np.zeros(d), s, np.zeros(d), np.eye(d))
    assert res["rank"] == r and res["flags"] == 2
    print(f"padded d={d} r={r}: residual ratio {ratio:.3g}")


def test_late_pivot_failure_falls_back_bit_identically(dev, monkeypatch):
    """Full rank, d = 1000, last column nearly dependent: the unpivoted factor's pivot in the LAST panel falls below
    1e-12 max S_ii, so run_chol restarts from S with the pivoted factorisation.  The fallback's factor and distance are
    bit-identical to the TISE_CHOL_PIVOTED run (run_pchol starts from S either way)."""
    d = 1000
    rng = np.random.default_rng(77)
    g = rng.standard_normal((d, d + 32))
    g[-1] = g[-2] + 1e-8 * rng.standard_normal(d + 32)
    s = (g @ g.T) / (d + 32)
    m1, m2 = rng.standard_normal(d) * 0.1, rng.standard_normal(d) * 0.1
    s2 = _full_sigma(d, 78)
    lt_a, r_a, unp_a = _prefactor(d, s, dev, False, monkeypatch)
    lt_b, r_b, unp_b = _prefactor(d, s, dev, True, monkeypatch)
    assert not unp_a and not unp_b and r_a == r_b
    assert np.array_equal(lt_a, lt_b)
    one = _solver(d, dev).distance(m1, s, m2, s2)
    monkeypatch.setenv("TISE_CHOL_PIVOTED", "1")
    two = _solver(d, dev).distance(m1, s, m2, s2)
    assert one == two


# ================================================================================================== eigenvalues
_EIG_NS = (2, 3, 7, 8, 9, 63, 64, 65, 511, 512, 513, 2047, 2048)
_EIG_KINDS = ("random", "repeats", "negatives", "graded", "cI", "diag", "blockdiag", "toeplitz", "zero")


def _eig_cells():
    cells = [("random", n) for n in _EIG_NS]
    cells += [(k, n) for k in _EIG_KINDS for n in (2, 9, 65, 513) if not (k == "random" and n in _EIG_NS)]
    cells += [(k, 2048) for k in ("repeats", "diag", "toeplitz")]
    cells += [(k, 1) for k in ("random", "zero", "negatives")]
    return cells


@pytest.mark.parametrize("kind,n", _eig_cells())
def test_eigvalsh_known_spectra(dev, kind, n):
    """tise_eigvalsh (default sytrd_fused8<8,1> + bisect<1>) against known spectra: |w_i - lam_i| <= Weyl term +
    (32 n + 4) eps ||A||_2 + 2 pivmin (derivation: tests/_frechet_child.py), output ascending.  c I and diagonal inputs
    take the tau = 0 reflector in every column, block-diagonal ones in some, Toeplitz (already tridiagonal) in all."""
    rec = fc.run_eig_case(kind, n, dev, _solver(max(n, 1), dev))
    print(f"eig {rec['name']}: ratio {rec['ratio']:.3g}")
    assert rec["finite"] and rec["ascending"], rec
    assert rec["ratio"] <= 1.0, rec


@pytest.mark.parametrize("n", [999, 1000, 1025])
def test_eigvalsh_smaller_than_the_handle(dev, n):
    """The r x r eigenproblem of a rank-deficient distance: n < d on a d = 2048 handle (the fused kernel's buffers are
    laid out for d, the matrix for n).  Same bound; the result is bit-identical to a handle sized to n."""
    rec = fc.run_eig_case("repeats", n, dev, _solver(2048, dev))
    own = fc.run_eig_case("repeats", n, dev, _solver(n, dev))
    print(f"eig n={n} on d=2048: ratio {rec['ratio']:.3g}")
    assert rec["ascending"] and rec["ratio"] <= 1.0, rec
    assert rec["digest"] == own["digest"]


@pytest.mark.parametrize("kind,n", [("random", 2), ("diag", 9), ("cI", 64), ("repeats", 300), ("blockdiag", 65),
                                    ("random", 2049)])
def test_eigvalsh_generic_fused_kernel(dev, kind, n, monkeypatch):
    """sytrd_fused_kernel: forced at small n by TISE_SYTRD_FUSED_GENERIC (read per call), and taken naturally at
    n = 2049 > 2048.  Same bound."""
    if n <= 2048:
        monkeypatch.setenv("TISE_SYTRD_FUSED_GENERIC", "1")
    rec = fc.run_eig_case(kind, n, dev, _solver(n, dev))
    assert rec["instance"].startswith("sytrd_fused ")
    print(f"eig generic {rec['name']}: ratio {rec['ratio']:.3g}")
    assert rec["finite"] and rec["ascending"] and rec["ratio"] <= 1.0, rec


_CHILD_ENVS = ({"TISE_SYTRD_ROWS": "4"}, {"TISE_SYTRD_ROWS": "16"}, {"TISE_SYTRD_ROWS": "82"},
               {"TISE_SYTRD_TWO_LAUNCH": "1"}, {"TISE_BISECT_NP": "2"}, {"TISE_BISECT_NP": "4"},
               {"TISE_SYTRD_ROWS": "8", "TISE_BISECT_NP": "1"})
_SWITCHES = ("TISE_SYTRD_ROWS", "TISE_SYTRD_TWO_LAUNCH", "TISE_BISECT_NP", "TISE_SYTRD_FUSED_GENERIC")


@pytest.mark.timeout(900)
def test_eigvalsh_process_static_switches_in_children(dev):
    """TISE_SYTRD_ROWS in {4, 16, 82} (sytrd_fused8 <4,1>, <8,2>, <4,2>), TISE_SYTRD_TWO_LAUNCH (sytrd_step +
    sytrd_update_matvec) and TISE_BISECT_NP in {2, 4} (bisect<2>, <4>) are read once per process: each runs in a child
    (tests/_frechet_child.py), one at a time under a time limit, no child after one fails, on n = 9 / 65 / 300 / 513 /
    1000 / 2048 with the bound of test_eigvalsh_known_spectra.  A child with the default selection spelled out must be
    bit-identical to this process, case by case; every other child must differ from it in the bits of at least one
    case, which shows that its switch replaced the kernel (the `instance` field is only the selection rule's label;
    the kernel trace of this test lists the instances themselves)."""
    here = {}
    for kind, n in fc.EIG_CHILD_CASES:
        rec = fc.run_eig_case(kind, n, dev, _solver(n, dev))
        assert rec["ratio"] <= 1.0 and rec["ascending"], rec
        here[rec["name"]] = rec
    for extra in _CHILD_ENVS:
        env = {k: v for k, v in os.environ.items() if k not in _SWITCHES}
        env.update(extra)
        env["PYTHONPATH"] = ROOT
        try:
            p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_frechet_child.py")], env=env, cwd=ROOT,
                               capture_output=True, text=True, timeout=240)
        except subprocess.TimeoutExpired as e:
            pytest.fail(f"child {extra} timed out; stderr:\n{e.stderr}")
        assert p.returncode == 0, f"child {extra} exit {p.returncode}; stderr:\n{p.stderr[-6000:]}"
        recs = json.loads(p.stdout.strip().splitlines()[-1])
        worst = max(recs, key=lambda r: r["ratio"])
        print(f"child {extra}: {sorted({r['instance'] for r in recs})}, worst ratio {worst['ratio']:.3g} ({worst['name']})")
        same = [rec["digest"] == here[rec["name"]]["digest"] for rec in recs]
        for rec in recs:
            assert rec["finite"] and rec["ascending"] and rec["ratio"] <= 1.0, (extra, rec)
        if all(rec["instance"] == here[rec["name"]]["instance"] for rec in recs):
            assert all(same), (extra, "the default selection spelled out must give the same bits")
        else:
            # another instance sums in another order (rows per workgroup, probes per lane, launches per column): on at
            # least one case its bits differ, i.e. the switch really replaced the kernel this process runs
            assert not all(same), (extra, "the switch changed nothing")


# ================================================================================================== distance
def _centred(n, d, seed, shift=0.0):
    x = _cases.pool3_like_features(n, d, seed, shift=shift).astype(np.float64)
    return x - x.mean(axis=0)


@functools.lru_cache(maxsize=None)
def _truth_case(d, n1, n2, seed, offset=0.0, identical=False):
    """Inputs and exact values of one distance case (module docstring of test_distance_against_sample_truth)."""
    a = _centred(n1, d, seed)
    b = a if identical else _centred(n2, d, seed + 1, shift=0.15)
    n2 = n1 if identical else n2
    rng = np.random.default_rng(seed + 7)
    mu1 = rng.standard_normal(d) * 0.1
    mu2 = mu1.copy() if identical else mu1 + rng.standard_normal(d) * 0.05
    c1, c2 = float(n1 - 1), float(n2 - 1)
    s1 = (a.T @ a) / c1
    s2 = s1.copy() if identical else (b.T @ b) / c2
    # E_i = S_i(fp64) - A^T A / c: the BLAS product and the division round (gamma_{n+1} |A|^T |A| / c)
    e1 = gamma(n1 + 1) * np.linalg.norm(np.abs(a).T @ np.abs(a)) / c1
    e2 = e1 if identical else gamma(n2 + 1) * np.linalg.norm(np.abs(b).T @ np.abs(b)) / c2
    # Tr sqrtm((S1 + o I)(S2 + o I)) = || A' B'^T ||_*, A' = [A / sqrt(c1); sqrt(o) I]: through R factors (QR, no squaring)
    ap = a / np.sqrt(c1)
    bp = b / np.sqrt(c2)
    if offset:
        ap = np.vstack([ap, np.sqrt(offset) * np.eye(d)])
        bp = np.vstack([bp, np.sqrt(offset) * np.eye(d)])
    ra = np.linalg.qr(ap, mode="r")
    rb = np.linalg.qr(bp, mode="r")
    core = ra @ rb.T
    sv = np.linalg.svd(core, compute_uv=False)
    k = sv.size
    # truth error (Mirsky: sum |sv^ - sv| <= ||Delta||_* <= sqrt(k) ||Delta||_F): QR backward error 16 sqrt(d) m u ||.||_F
    # per factor, the product gamma_d |R_A||R_B|^T, the SVD 16 k u sv_max
    na, nb = np.linalg.norm(ap), np.linalg.norm(bp)
    qa, qb = 16 * np.sqrt(d) * ap.shape[0] * U, 16 * np.sqrt(d) * bp.shape[0] * U
    delta_f = (qa + qb + qa * qb) * na * nb + gamma(d) * np.linalg.norm(np.abs(ra) @ np.abs(rb).T) + 16 * k * U * sv[0] * np.sqrt(k)
    truth_err = float(np.sqrt(k) * delta_f)
    lam = np.sort(sv.astype(np.float64) ** 2)[::-1]
    tc = float(np.sum(sv.astype(np.longdouble)))
    n1s, n2s = float(np.linalg.eigvalsh(s1)[-1]), float(np.linalg.eigvalsh(s2)[-1])
    dd = float(np.sum((mu1.astype(np.longdouble) - mu2) ** 2))
    t1 = float(np.sum(np.diag(s1).astype(np.longdouble)))
    t2 = float(np.sum(np.diag(s2).astype(np.longdouble)))
    return dict(mu1=mu1, s1=s1, mu2=mu2, s2=s2, lam=lam, tc=tc, truth_err=truth_err, e1=e1, e2=e2, n1s=n1s, n2s=n2s,
                dd=dd, t1=t1, t2=t2, d=d, offset=offset, fs2=float(np.linalg.norm(s2)),
                rank1=int(np.sum(np.linalg.svd(a if not offset else ap, compute_uv=False) > 1e-9 * np.sqrt(c1))))


def _tc_bound(case, r, chol=None):
    """|tr_covmean - truth| bound for a device result of rank r (test_distance_against_sample_truth); chol = a bound on
    ||L L^T - S1||_2 measured on the factor itself (_solve_measured), else the a-priori gamma_{d+1} tr S1 of a full-rank
    factor."""
    d, o = case["d"], case["offset"]
    t1, t2 = case["t1"] + d * o, case["t2"] + d * o
    n1s, n2s = case["n1s"] + o, case["n2s"] + o
    g = gamma(d + 1)
    if chol is None:
        assert r == d, "a stopped factor needs its measured residual"
        chol = g * t1
    delta = (n2s * (case["e1"] + chol) + (n1s + case["e1"] + chol) * case["e2"]
             + 2.01 * g * t1 * (case["fs2"] + np.sqrt(d) * o) + 2.0 * U * o * t1
             + fc.eig_bound(r, 1.01 * n1s * n2s))
    lam = np.zeros(max(r, case["lam"].size))
    lam[:case["lam"].size] = case["lam"]
    lam = lam[:r] if r >= np.count_nonzero(case["lam"]) else lam
    lo = np.sqrt(np.maximum(lam - delta, 0.0))
    hi = np.sqrt(lam + delta)
    sq = np.sqrt(lam)
    per = np.maximum(hi - sq, sq - lo)
    return float(per.sum() + case["truth_err"] + 4 * r * U * case["tc"]), delta


def _check_distance(case, res, label, chol=None, rank_true=None):
    """Every output field against the truth; returns the largest error / bound ratio."""
    d = case["d"]
    r = res["rank"]
    if rank_true is not None and rank_true < d:
        # the columns past the rank: a regression cap of two 16-pivot panels (observed: at most 12), so that a stopping
        # rule running on towards d cannot hide behind the sqrt(delta) each of its extra eigenvalues adds to the bound
        assert rank_true <= r <= rank_true + 32, (r, rank_true)
    tcb, delta = _tc_bound(case, r, chol)
    ddb = gamma(d + 2) * case["dd"]
    t1b, t2b = gamma(d) * case["t1"], gamma(d) * case["t2"]
    fidb = ddb + t1b + t2b + 2 * tcb + 4 * U * (case["dd"] + case["t1"] + case["t2"] + 2 * case["tc"])
    fid_true = case["dd"] + case["t1"] + case["t2"] - 2 * case["tc"]
    ratios = {"diff2": abs(res["diff2"] - case["dd"]) / max(ddb, 1e-300),
              "tr1": abs(res["tr1"] - case["t1"]) / t1b, "tr2": abs(res["tr2"] - case["t2"]) / t2b,
              "tr_covmean": abs(res["tr_covmean"] - case["tc"]) / tcb, "fid": abs(float(res["fid"]) - fid_true) / fidb}
    if case["dd"] == 0.0:
        assert res["diff2"] == 0.0
        ratios["diff2"] = 0.0
    print(f"{label}: rank {r} n_negative {res['n_negative']} flags {res['flags']} tc bound {tcb:.3g} "
          + " ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    for k, v in ratios.items():
        assert v <= 1.0, (label, k, v, res)
    # the counts: every eigenvalue of the device's r x r matrix is within delta of a true one (zeros past the rank)
    nonzero = int(np.count_nonzero(case["lam"] > delta))
    assert r >= nonzero
    assert res["n_negative"] <= r - nonzero, res
    assert res["flags"] & 1 == 0
    assert bool(res["flags"] & 2) == (r < d)
    return max(ratios.values())


def _solve_measured(case, dev):
    """One-call distance, then the same through prefactor + factor + distance_prefactored (bit-identical), and a bound on
    ||S1 - L L^T||_2 measured on the factor read back: ||S1 - fl(L L^T)||_F + gamma_d || |L||L^T| ||_F (the check's own
    product) -> (result, residual bound)."""
    d = case["d"]
    solver = _solver(d, dev)
    one = solver.distance(case["mu1"], case["s1"], case["mu2"], case["s2"])
    solver.prefactor(torch.as_tensor(case["s1"], device=dev))
    lt, r, _ = solver.factor()
    two = solver.distance_prefactored(case["mu1"], case["mu2"], case["s2"])
    assert one == two and r == one["rank"]
    lt = lt.cpu().numpy()
    alt = np.abs(lt)
    chol = (float(np.linalg.norm(case["s1"] - lt.T @ lt)) + gamma(d) * float(np.linalg.norm(alt.T @ alt))) * (1 + 4 * U)
    return one, chol


_TRUTH_CELLS = [(8, 60, 50), (64, 400, 350), (100, 700, 600), (192, 300, 280), (1000, 1300, 1250), (2048, 2400, 2350),
                (2304, 2600, 2500),                                                     # full rank (n > d)
                (64, 40, 45), (192, 96, 97), (1000, 300, 320), (2048, 1000, 1000)]      # rank-deficient; the last: config 1


@pytest.mark.timeout(600)
@pytest.mark.parametrize("d,n1,n2", _TRUTH_CELLS)
def test_distance_against_sample_truth(dev, d, n1, n2):
    """tise_frechet_distance against the truth from the samples: S_i = A_i^T A_i / (n_i - 1) with A_i centred, and
    Tr sqrtm(S1 S2) = ||A1 A2^T||_* / sqrt((n1 - 1)(n2 - 1)), evaluated through the R factors of A1 / sqrt(n1 - 1) and
    A2 / sqrt(n2 - 1) (QR: the condition number is never squared) and an SVD; that evaluation's error (QR backward
    error, the product, the SVD; Mirsky: sqrt(k) ||Delta||_F) is added to every bound.

    tr_covmean.  The device's r x r matrix has eigenvalues within
        delta = ||S2|| (||E1|| + ||dS||) + ||S1|| ||E2|| + 2.01 gamma_{d+1} tr S1 ||S2||_F + eig_bound(r, ||S1|| ||S2||)
    of lam_1 >= ... (the true eigenvalues of S1 S2, zeros past their rank), by Weyl on the symmetric forms
    S2^(1/2) X S2^(1/2) and L^T X L: E_i = the fp64 rounding of S_i (gamma_{n+1} |A|^T |A| / (n - 1)); dS = L L^T - S1
    of the Cholesky, MEASURED on the factor read back through tise_frechet_factor (_solve_measured; a priori it is
    <= gamma_{d+1} ||L||_F^2 = gamma_{d+1} tr S1 for a full-rank factor, but a stopped one also leaves its trailing
    residual, which depends on the data); the two GEMMs each <= gamma_d ||L||_F^2 ||S2||_F; then the eigensolver.  Hence
        |tr_covmean - truth| <= sum_i max(sqrt(lam_i + delta) - sqrt(lam_i), sqrt(lam_i) - sqrt(max(lam_i - delta, 0)))
    which is delta / (2 sqrt(lam_i)) per eigenvalue to first order when full rank, and sqrt(delta) per eigenvalue at 0
    when rank-deficient: (r - rank) sqrt(c eps ||S1|| ||S2||) with c ~ 2 d tr S1 ||S2||_F / (||S1|| ||S2||): the
    square root is not Lipschitz at 0.  diff2 <= gamma_{d+2} |mu1 - mu2|^2 (a rounded difference, square and sum),
    tr_i <= gamma_d tr S_i, fid = the sum of those with tr_covmean twice, plus 4 u of the terms for the final combination.
    rank = d when full rank; rank-deficient: rank(S1) = n1 - 1 <= rank <= n1 - 1 + 32 (a regression cap, not derived: the
    pivoted rule runs to the last positive pivot, see _check_distance) and the flags say so; n_negative <= the number
    of eigenvalues within delta of 0.  The prefactored form gives the same bits."""
    case = _truth_case(d, n1, n2, 1000 + d)
    res, chol = _solve_measured(case, dev)
    if n1 > d and n2 > d:
        assert res["rank"] == d and res["n_negative"] == 0
    _check_distance(case, res, f"truth d={d} n1={n1} n2={n2}", chol, min(d, n1 - 1))


@pytest.mark.parametrize("d,n", [(64, 500), (1000, 1200), (192, 90)])
def test_distance_identical_inputs(dev, d, n):
    """Identical inputs: truth tr_covmean = ||A A^T||_* / (n - 1) = tr S, fid = 0 up to the bound."""
    case = _truth_case(d, n, n, 2000 + d, identical=True)
    res, chol = _solve_measured(case, dev)
    _check_distance(case, res, f"identical d={d} n={n}", chol, min(d, n - 1))


@pytest.mark.parametrize("d,n1,n2,pivoted", [(100, 700, 600, False), (100, 60, 70, False), (100, 700, 600, True),
                                             (100, 60, 70, True), (2304, 2600, 2500, True), (2304, 1000, 1100, True)])
def test_distance_diag_offset_on_finite_input(dev, d, n1, n2, pivoted, monkeypatch):
    """diag_offset = 1e-6 on finite input, every factorisation: d <= 2048 unpivoted and blocked pivoted
    (pchol_copy_kernel adds the offset to the working copy of S1), d > 2048 the unblocked pivoted one (pchol_init_kernel
    adds it to the diagonal it pivots on, pchol_finish_kernel to each pivot column it reads from S1); the axpy kernel
    adds it to T1 for S2.  Full-rank and rank-deficient S1 at each.  The reference's retry formula the reference's retry formula (fid_score.py:156-160, :171): the offset goes
    inside sqrtm only, tr S1 and tr S2 do not take it.  Truth: Tr sqrtm((S1 + o I)(S2 + o I)) = ||A1' A2'^T||_* with
    A' = [A / sqrt(n - 1); sqrt(o) I]; bound of test_distance_against_sample_truth with S_i + o I."""
    o = 1e-6
    case = _truth_case(d, n1, n2, 3000 + d, offset=o)
    if pivoted and d <= 2048:
        monkeypatch.setenv("TISE_CHOL_PIVOTED", "1")
    res = _solver(d, dev).distance(case["mu1"], case["s1"], case["mu2"], case["s2"], diag_offset=o)
    assert res["rank"] == d                                      # S1 + o I is positive definite
    _check_distance(case, res, f"offset d={d} n1={n1} pivoted={pivoted}")


@pytest.mark.parametrize("d", [64, 100, 128, 1000, 2048])
def test_triangular_and_full_products_agree(dev, d, monkeypatch):
    """With the unpivoted factor the two GEMMs skip the zero blocks of L^T (gemm_f64_tri<0>, <1> + mirror_upper);
    TISE_FRECHET_FULL_GEMM (read per call) takes the full products (gemm_f64 + symmetrize).  Both are within the truth
    bound, so they are within twice the bound's device part of each other."""
    n1, n2 = d + 300, d + 250
    case = _truth_case(d, n1, n2, 4000 + d)
    tri = _solver(d, dev).distance(case["mu1"], case["s1"], case["mu2"], case["s2"])
    monkeypatch.setenv("TISE_FRECHET_FULL_GEMM", "1")
    full = _solver(d, dev).distance(case["mu1"], case["s1"], case["mu2"], case["s2"])
    _check_distance(case, tri, f"tri d={d}")
    _check_distance(case, full, f"full d={d}")
    tcb, _ = _tc_bound(case, d)
    assert abs(tri["tr_covmean"] - full["tr_covmean"]) <= 2 * (tcb - case["truth_err"])


@pytest.mark.parametrize("d,n1,n2", [(2304, 2600, 2500), (2048, 1000, 1000), (192, 96, 97)])
def test_prefactored_is_bit_identical(dev, d, n1, n2):
    """tise_frechet_prefactor + _distance_prefactored == tise_frechet_distance, bit for bit, at d > 2048 (unblocked
    pivoted factor) and rank-deficient (the pivoted factor and the r x r problem)."""
    case = _truth_case(d, n1, n2, 1000 + d)
    solver = _solver(d, dev)
    one = solver.distance(case["mu1"], case["s1"], case["mu2"], case["s2"])
    solver.prefactor(torch.as_tensor(case["s1"], device=dev))
    two = solver.distance_prefactored(case["mu1"], case["mu2"], case["s2"])
    assert one == two


def test_two_handles_on_two_streams_match_serial(dev):
    """Two handles solving at once on two streams (threads: the C calls release the GIL) give the bits of serial
    solves: the per-class O-FID path runs several solvers on their own streams."""
    cases = [_truth_case(1000, 1300, 1250, 1000 + 1000), _truth_case(1000, 300, 320, 1000 + 1000)]
    solvers = [_solver(1000, dev), _solver(1000, dev)]
    serial = [s.distance(c["mu1"], c["s1"], c["mu2"], c["s2"]) for s, c in zip(solvers, cases)]
    args = [tuple(torch.as_tensor(c[k], device=dev) for k in ("mu1", "s1", "mu2", "s2")) for c in cases]
    streams = [torch.cuda.Stream(device=dev) for _ in cases]
    torch.cuda.synchronize()
    out = [None, None]

    def run(i):
        with torch.cuda.stream(streams[i]):
            out[i] = solvers[i].distance(*args[i])
    ts = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=120)
    assert out == serial


def test_n_negative_counts_only_negative_eigenvalues(dev):
    """d = 1, S1 = 1, S2 = 0: the n = 1 copy path hands the exact eigenvalue 0.0 to the final kernel, which is not
    negative: n_negative = 0, tr_covmean = 0, fid = 1.  With S2 = -1 it is: n_negative = 1."""
    s = _solver(1, dev)
    res = s.distance(np.zeros(1), np.ones((1, 1)), np.zeros(1), np.zeros((1, 1)))
    assert res["n_negative"] == 0 and res["tr_covmean"] == 0.0 and res["fid"] == 1.0 and res["rank"] == 1
    res = s.distance(np.zeros(1), np.ones((1, 1)), np.zeros(1), -np.ones((1, 1)))
    assert res["n_negative"] == 1 and res["tr_covmean"] == 0.0


def test_factor_refuses_without_a_prefactored_matrix(dev):
    """tise_frechet_factor returns TISE_ERR_INVALID_ARG (called through the C ABI, below FrechetSolver.factor's own
    Python check) on a fresh handle, after tise_frechet_distance and after tise_pivoted_cholesky, both of which
    overwrite the factor buffer; right after tise_frechet_prefactor it succeeds."""
    import ctypes
    from tise_toolbox_amd import _lib, device
    d = 64
    s = torch.as_tensor(_full_sigma(d, 3), device=dev)
    solver = _solver(d, dev)
    lt = torch.empty((d, d), dtype=torch.float64, device=dev)
    r, unp = ctypes.c_int(-1), ctypes.c_int(-1)

    def raw():
        return _lib.load().tise_frechet_factor(solver._h, device._ptr(lt), ctypes.byref(r), ctypes.byref(unp),
                                               device._stream())
    assert raw() == _lib.TISE_ERR_INVALID_ARG
    solver.prefactor(s)
    assert raw() == _lib.TISE_OK and r.value == d and unp.value == 1
    solver.distance(np.zeros(d), s, np.zeros(d), s)
    assert raw() == _lib.TISE_ERR_INVALID_ARG
    solver.prefactor(s)
    solver.pivoted_cholesky(s)
    assert raw() == _lib.TISE_ERR_INVALID_ARG


# ================================================================================================== 50-digit stages
_MP_CELLS = [(8, 60, 50), (17, 5, 30), (33, 200, 150), (48, 30, 40)]


@pytest.mark.parametrize("d,n1,n2", _MP_CELLS)
def test_product_and_eigenvalues_against_mpmath(dev, d, n1, n2):
    """d <= 48 (always the pivoted factor: the unpivoted one starts at 64), mpmath at 50 digits as the exact answer for
    the fp64 data the device holds.

    Stage M = L^T S2 L: with the device's own factor (read back), M and its eigenvalues lam_i are formed exactly, so
    the distance's tr_covmean isolates the two GEMMs, the symmetrisation and the eigensolver:
        delta = (2 gamma_d + gamma_d^2) || |L^T||S2||L| ||_F + u ||M||_2 + eig_bound(r, ||M||_2),
        |tr_covmean - sum_i sqrt(max(lam_i, 0))| <= sum_i max(sqrt(lam_i + delta) - sqrt(lam_i),
                                                               sqrt(lam_i) - sqrt(max(lam_i - delta, 0))) + gamma_r tr.
    Stage eigsy: tise_eigvalsh on the fp64 S2 itself against mpmath's eigenvalues of the same matrix, the bound of
    test_eigvalsh_known_spectra with no Weyl term."""
    import mpmath as mp
    case = _truth_case(d, n1, n2, 5000 + d)
    solver = _solver(d, dev)
    solver.prefactor(torch.as_tensor(case["s1"], device=dev))
    lt, r, _ = solver.factor()
    res = solver.distance_prefactored(case["mu1"], case["mu2"], case["s2"])
    lt = lt.cpu().numpy()[:r]
    s2 = case["s2"]
    with mp.workdps(50):
        L = mp.matrix(lt.tolist())
        S2 = mp.matrix(s2.tolist())
        M = L * S2 * L.T
        ev = mp.eigsy(M, eigvals_only=True) if r else []
        lam = np.array([float(x) for x in ev])
        tc = float(mp.fsum(mp.sqrt(x) for x in ev if x > 0))
        lam2 = np.sort(np.array([float(x) for x in mp.eigsy(S2, eigvals_only=True)]))
    mnorm = float(np.max(np.abs(lam))) if r else 0.0
    g = gamma(d)
    delta = (2 * g + g * g) * float(np.linalg.norm(np.abs(lt) @ np.abs(s2) @ np.abs(lt).T)) + U * mnorm \
        + fc.eig_bound(r, mnorm)
    sq = np.sqrt(np.maximum(lam, 0.0))
    per = np.maximum(np.sqrt(np.maximum(lam, 0.0) + delta) - sq, sq - np.sqrt(np.maximum(lam - delta, 0.0)))
    bound = float(per.sum()) + gamma(max(r, 1)) * tc
    err = abs(res["tr_covmean"] - tc)
    w = solver.eigvalsh(torch.as_tensor(s2, device=dev)).cpu().numpy()
    ebound = fc.eig_bound(d, float(np.max(np.abs(lam2))))
    eerr = float(np.max(np.abs(w - lam2)))
    print(f"mpmath d={d} rank {r}: M stage ratio {err / bound:.3g}, eigsy ratio {eerr / ebound:.3g}")
    assert err <= bound, (err, bound)
    assert eerr <= ebound and np.all(np.diff(w) >= 0.0), (eerr, ebound)
