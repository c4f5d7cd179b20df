"""GPU: csrc/stats.hip (the fp64 {n, s = sum x, S = sum x x^T} behind every FID's mu / sigma) and csrc/is_score.hip (the
per-split IS* sums) pinned to plain CPU references at every kernel instance and dispatch edge.

Rounding points of stats.hip: fp32 rows are widened to fp64 exactly and every fp32 x fp32 product is exact in fp64, so
S and s differ from the exact sums only by the fp64 additions (fixed order inside a launch, any order across launches).
stats_finalize_kernel evaluates, per element and with no FMA contraction (checked on the gfx950 ISA: v_mul_f64, the
correctly rounded v_div_scale/v_div_fmas/v_div_fixup sequence, v_add_f64, the same division):
    mu = s / n          sigma = (S - (s_i s_j) / n) / (n - 1)        (n - 1 is exact)
Feature values k / 64 with integer |k| < 4096 make every product a multiple of 2^-12 below 2^12 in magnitude, so every
partial sum of up to 2^20 rows is a multiple of 2^-12 below 2^32: S, s and n are EXACT in fp64 whatever the order, equal
to the integer K^T K and sum K scaled by a power of two, and mu / sigma equal numpy's evaluation of the formula above
bit for bit.  For general fp32 data u = 2^-53 and gamma_N = N u / (1 - N u) bound a sum of N terms in any order.

Rounding points of is_score.hip, per row (z = logit row, C classes): zd = fl(z * fl(1 / T)) (fp64; NOT z / T, the
reference restates the same product), m = max zd, zz = zd - m and the column kernel's zd - lse (either may be contracted
into one FMA with the exact product, an extra error <= u |zd|), e = exp(zz), se = sum e, sz = sum e zz, l = log se,
lse = m + l, a = sz / se - l, and in the column kernel p = exp(zd - lse).  Then A_k = sum a_i, B_kc = sum p_ic over the
split's rows, pbar = B / n_k, H_k = sum pbar log pbar (0 log 0 = 0), score_k = exp(A_k / n_k - H_k), mean, std (ddof 0).
ocml's fp64 exp and log are within 1 ulp; EF = 4u allows 2.  The reference restates A, B and the scores in
np.longdouble from the same fp64 zd; each bound is evaluated per row / split / score from the reference's own
quantities (derivation in _is_reference) and carries a factor (1 + 2^-8) for the second-order terms and the
reference's own rounding (its unit is 2^11 times smaller).

Memory hygiene: every input lives inside a larger NaN-filled allocation (columns past d / C in a strided row, rows past
the last one, the floats before an offset base), so a kernel that reads any of it into a sum makes a result non-finite.
Every launch here is a legal input; nothing is read out of bounds."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from tests import _cases

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
EF = 4 * U
SLACK = 1.0 + 2.0 ** -8
NAN = float("nan")


def gamma(n):
    return n * U / (1.0 - n * U)


@pytest.fixture(scope="module")
def dev(cuda_device):
    return cuda_device


def _backed(dev, x, ld, off, extra_rows=3):
    """x (rows, w) float32 -> a (rows, w) view with row stride ld, `off` floats into a NaN-filled allocation that also has
    `extra_rows` rows past the end."""
    rows, w = x.shape
    back = torch.full((off + (rows + extra_rows) * ld,), NAN, dtype=torch.float32, device=dev)
    v = back.as_strided((rows, w), (ld, 1), off)
    v.copy_(torch.from_numpy(np.ascontiguousarray(x)))
    return back, v


def _ints(rows, d, seed, signed):
    rng = np.random.default_rng(seed)
    return rng.integers(-2048, 2048, (rows, d)) if signed else rng.integers(0, 4096, (rows, d))


def _exact_ref(k):
    """Exact (S, s) of the features k / 64: K^T K / 4096 and sum K / 64.  K^T K is formed by fp64 BLAS, which is exact
    because every partial sum is an integer below 2^37; small cases also check it against int64 arithmetic."""
    kf = k.astype(np.float64)
    ktk = kf.T @ kf
    if k.size * k.shape[1] <= 2 ** 24:
        assert np.array_equal(ktk, (k.T.astype(np.int64) @ k.astype(np.int64)).astype(np.float64))
    return ktk / 4096.0, kf.sum(0) / 64.0


@functools.lru_cache(maxsize=None)
def _upper(d):
    t = np.arange(d) // 64
    return t[None, :] >= t[:, None]                          # the 64x64 tiles the kernels write (tile_col >= tile_row)


def _read(acc):
    d = acc.dims
    b = acc.buffer().cpu().numpy()
    return b[:d * d].reshape(d, d), b[d * d:d * d + d], b[d * d + d], b[d * d + d + 1]


def _assert_exact(acc, S_ref, s_ref, n_ref, what):
    """S (upper tiles; the lower tiles are never written and stay 0), s and n bit for bit; None = must be all zero."""
    S, s, n, pad = _read(acc)
    up = _upper(acc.dims)
    if S_ref is None:
        assert not S.any(), f"{what}: S written"
    else:
        bad = ~(S == S_ref) & up
        assert not bad.any(), f"{what}: S differs at {np.argwhere(bad)[:5].tolist()}"
        assert not S[~up].any(), f"{what}: a lower tile was written"
    if s_ref is None:
        assert not s.any() and n == 0, f"{what}: s / n written"
    else:
        assert np.array_equal(s, s_ref), f"{what}: s differs at {np.flatnonzero(s != s_ref)[:5].tolist()}"
        assert n == n_ref, (what, n, n_ref)
    assert pad == 0


def _np_finalize(S, s, n):
    with np.errstate(divide="ignore", invalid="ignore"):
        return s / n, (S - np.outer(s, s) / n) / (n - 1.0)


def _path(d, ld, off):
    return "bk64" if d % 64 == 0 and ld % 4 == 0 and off % 4 == 0 else "generic"


# (d, ld - d, base offset in floats, rows).  Offsets 1 and 4 are 4- and 16-byte aligned: 1 takes the generic kernel, 4 stays
# on the fast one.  Every d, every ld and offset, every row count, and both paths at d % 64 == 0.
EXACT = [
    (1, 0, 0, 1), (1, 1, 1, 5000), (1, 4, 4, 513),
    (24, 0, 0, 63), (24, 1, 0, 512), (24, 4, 1, 129),
    (63, 0, 0, 4097), (63, 1, 1, 64), (63, 4, 4, 1),
    (64, 0, 0, 65), (64, 4, 4, 511), (64, 0, 1, 127), (64, 1, 0, 512), (64, 4, 0, 5000), (64, 0, 4, 1),
    (65, 0, 0, 513), (65, 1, 4, 64), (65, 4, 1, 4097),
    (100, 0, 0, 129), (100, 1, 1, 1), (100, 4, 4, 511),
    (130, 0, 0, 5000), (130, 1, 4, 127), (130, 4, 0, 65),
    (1000, 0, 0, 512), (1000, 1, 1, 63), (1000, 4, 4, 129),
    (1030, 0, 0, 65), (1030, 1, 1, 513), (1030, 4, 4, 1),
    (2048, 0, 0, 4097), (2048, 4, 4, 127), (2048, 0, 1, 511), (2048, 1, 0, 64), (2048, 4, 0, 513),
]


@pytest.mark.parametrize("d,ldx,off,rows", EXACT, ids=[f"d{c[0]}-ld+{c[1]}-off{c[2]}-r{c[3]}" for c in EXACT])
def test_stats_exact_every_instance(dev, d, ldx, off, rows):
    """Bound: 0.  Integer-valued data (module docstring): update() (fused bk64<true>, or generic syrk + colsum), the
    covariance kernel alone (bk64<false> or generic: s and n stay 0) and the column sums alone (sliced colsum from 512
    rows, plain below: S stays 0) each give S, s, n bit for bit; mu and sigma equal numpy's s / n and
    (S - s s^T / n) / (n - 1) bit for bit, and sigma is exactly symmetric (rows = 1: mu = the row, sigma all NaN, as
    np.cov(ddof=1) gives).  The padding columns, the rows past the end and the floats before the base are NaN."""
    from tise_toolbox_amd import device
    seed = d * 7919 + rows * 31 + ldx * 3 + off
    k = _ints(rows, d, seed, signed=bool(seed % 2))
    x = (k / 64.0).astype(np.float32)
    assert np.array_equal(x.astype(np.float64) * 64.0, k)
    S_ref, s_ref = _exact_ref(k)
    _, v = _backed(dev, x, d + ldx, off)
    what = f"{_path(d, d + ldx, off)} d={d} ld={d + ldx} off={off} rows={rows}"
    full, cov, col = (device.StatsAccumulator(d, dev) for _ in range(3))
    full.update(v)
    cov.update_parts(v, cov=True, col_sum=False)
    col.update_parts(v, cov=False, col_sum=True)
    _assert_exact(full, S_ref, s_ref, rows, "update " + what)
    _assert_exact(cov, S_ref, None, 0, "update_cov " + what)
    _assert_exact(col, None, s_ref, rows, "update_sum " + what)
    mu, sigma = (t.cpu().numpy() for t in full.finalize())
    mu_ref, sigma_ref = _np_finalize(S_ref, s_ref, float(rows))
    assert np.array_equal(mu, mu_ref), what
    if rows == 1:
        assert np.array_equal(mu, x[0].astype(np.float64)) and np.isnan(sigma).all(), what
    else:
        assert np.array_equal(sigma, sigma_ref), f"{what}: sigma differs at {np.argwhere(sigma != sigma_ref)[:5].tolist()}"
        assert np.array_equal(sigma, sigma.T), what


@pytest.mark.parametrize("d", [128, 130])
def test_stats_exact_chunks_shards_reset(dev, d):
    """Bound: 0.  Rows fed in chunks of 1, 63, 64, 65, 127, 129, 511, 512, 513 rows, alternating a 16-byte aligned and a
    4-byte aligned base (d = 128: the fast and the generic kernels fold into one buffer), equal the one-call sums bit for
    bit; so does the sum of per-shard buffers (the all-reduce).  reset() zeroes the whole buffer and the handle is then
    reused with the same result."""
    from tise_toolbox_amd import device
    chunks = [1, 63, 64, 65, 127, 129, 511, 512, 513]
    rows = sum(chunks)
    k = _ints(rows, d, 11 + d, signed=True)
    x = (k / 64.0).astype(np.float32)
    S_ref, s_ref = _exact_ref(k)
    a = device.StatsAccumulator(d, dev)
    shards = [device.StatsAccumulator(d, dev) for _ in range(3)]
    for rep in range(2):
        lo = 0
        for i, c in enumerate(chunks):
            _, v = _backed(dev, x[lo:lo + c], d, 4 if i % 2 == 0 else 1)
            a.update(v)
            if rep == 0:
                shards[i % 3].update(v)
            lo += c
        _assert_exact(a, S_ref, s_ref, rows, f"chunked d={d} pass {rep}")
        if rep == 0:
            merged = sum(sh.buffer() for sh in shards).cpu().numpy()
            assert np.array_equal(merged, a.buffer().cpu().numpy()), "sum of shard buffers != one buffer"
        a.reset()
        assert not a.buffer().cpu().numpy().any()


@pytest.mark.parametrize("d,rows", [(24, 600), (130, 5000), (2048, 512)])
def test_stats_colsum_twice_resets_tickets(dev, d, rows):
    """Bound: 0.  Two tise_stats_update_sum launches in a row on one handle give exactly 2x the sums of one (the sliced
    kernel's last workgroup per column tile must reset its ticket for the next launch), and a plain (< 512-row) launch
    between them does not disturb that."""
    from tise_toolbox_amd import device
    k = _ints(rows, d, 5 + d, signed=False)
    x = (k / 64.0).astype(np.float32)
    S_ref, s_ref = _exact_ref(k)
    _, v = _backed(dev, x, d, 0)
    acc = device.StatsAccumulator(d, dev)
    acc.update_parts(v, cov=False)
    _assert_exact(acc, None, s_ref, rows, "first launch")
    acc.update_parts(v, cov=False)
    _assert_exact(acc, None, 2 * s_ref, 2 * rows, "second launch")
    acc.update_parts(v[:100], cov=False)
    acc.update_parts(v, cov=False)
    _assert_exact(acc, None, 3 * s_ref + k[:100].sum(0) / 64.0, 3 * rows + 100, "third launch")


@pytest.mark.parametrize("d,off", [(128, 0), (130, 0), (128, 1)])
def test_stats_nan_inside_rows_propagates(dev, d, off):
    """A NaN inside the real rows makes exactly the S entries of its column (row and column of S, every stored tile) and
    its column sum non-finite; everything else stays exact (bound 0).  Nothing masks it."""
    from tise_toolbox_amd import device
    rows = 300
    k = _ints(rows, d, 3, signed=True)
    x = (k / 64.0).astype(np.float32)
    S_ref, s_ref = _exact_ref(k)
    hit = [5, 70]
    x[57, hit[0]] = np.nan
    x[280, hit[1]] = np.nan
    _, v = _backed(dev, x, d, off)
    acc = device.StatsAccumulator(d, dev)
    acc.update(v)
    S, s, n, _ = _read(acc)
    up = _upper(d)
    touched = np.zeros((d, d), bool)
    touched[hit, :] = True
    touched[:, hit] = True
    assert not np.isfinite(S[touched & up]).any()
    assert np.array_equal(S[~touched & up], S_ref[~touched & up])
    assert not np.isfinite(s[hit]).any()
    keep = np.setdiff1d(np.arange(d), hit)
    assert np.array_equal(s[keep], s_ref[keep]) and n == rows


def _logmag(rows, d, seed):
    """Full 24-bit mantissas, magnitudes log-uniform in [1e-6, 3e4], random signs."""
    rng = np.random.default_rng(seed)
    mag = 10.0 ** rng.uniform(-6.0, math.log10(3e4), (rows, d))
    return (mag * rng.choice([-1.0, 1.0], (rows, d))).astype(np.float32)


GENERAL = [(64, 0, 5000, "logmag"), (130, 0, 4097, "logmag"), (128, 1, 3000, "pool3"), (2048, 0, 1000, "pool3"),
           (1030, 4, 513, "pool3"), (2048, 1, 700, "logmag")]


@pytest.mark.parametrize("d,off,rows,kind", GENERAL, ids=[f"d{c[0]}-off{c[1]}-r{c[2]}-{c[3]}" for c in GENERAL])
def test_stats_general_fp32_per_element(dev, d, off, rows, kind):
    """Every fp32 x fp32 product is exact in fp64, so kernel and the fp64 CPU product X^T X differ only in the order of
    the N = rows additions, each within gamma_N of its absolute sum:
        |S - S_ref|_ij <= 2 gamma_N (|X|^T |X|)_ij            |s - s_ref|_i <= 2 gamma_N a_i,  a_i = sum |x_i|
    mu = s / n rounds once on each side:  |mu - mu_ref|_i <= 2 gamma_N a_i / n + 2 u |mu_ref|_i.
    sigma: the input perturbation is |dS| + |d(s_i s_j)| / n <= 2 gamma_N A_ij + (4 gamma_N + 4 gamma_N^2) a_i a_j / n
    (|s_i| <= a_i), and each side's evaluation (mul, div, sub, div) is within gamma_4 (|S_ij| + |s_i s_j| / n) / (n - 1):
        |sigma - sigma_ref|_ij <= [2 gamma_N A_ij + (4 gamma_N + 4 gamma_N^2) a_i a_j / n
                                   + 2 gamma_4 (|S_ij| + |s_i s_j| / n)] / (n - 1)
    All bounds times (1 + 2^-8) for their own evaluation.  Rows arrive in two calls (N counts them all)."""
    from tise_toolbox_amd import device
    x = _logmag(rows, d, d + rows) if kind == "logmag" else _cases.pool3_like_features(rows, d, seed=d + rows)
    x64 = x.astype(np.float64)
    ax = np.abs(x64)
    S_ref = x64.T @ x64
    A = ax.T @ ax
    s_ref = x64.sum(0)
    a = ax.sum(0)
    n = float(rows)
    acc = device.StatsAccumulator(d, dev)
    cut = rows // 3
    for lo, hi in ((0, cut), (cut, rows)):
        _, v = _backed(dev, x[lo:hi], d + 1 if off else d, off)
        acc.update(v)
    S, s, cnt, _ = _read(acc)
    assert cnt == n
    g = gamma(rows)
    up = _upper(d)
    rS = np.abs(S - S_ref)[up] / (SLACK * 2 * g * A[up])
    rs = np.abs(s - s_ref) / (SLACK * 2 * g * a)
    mu, sigma = (t.cpu().numpy() for t in acc.finalize())
    mu_ref, sigma_ref = _np_finalize(S_ref, s_ref, n)
    rmu = np.abs(mu - mu_ref) / (SLACK * (2 * g * a / n + 2 * U * np.abs(mu_ref)))
    bsig = (2 * g * A + (4 * g + 4 * g * g) * np.outer(a, a) / n
            + 2 * gamma(4) * (np.abs(S_ref) + np.abs(np.outer(s_ref, s_ref)) / n)) / (n - 1.0)
    rsig = np.abs(sigma - sigma_ref) / (SLACK * bsig)
    print(f"d={d} rows={rows} {kind}: ratio S {rS.max():.3g} s {rs.max():.3g} mu {rmu.max():.3g} sigma {rsig.max():.3g}")
    for name, r in (("S", rS), ("s", rs), ("mu", rmu), ("sigma", rsig)):
        assert np.isfinite(r).all() and r.max() <= 1.0, (name, float(np.nanmax(r)))
    assert np.array_equal(sigma, sigma.T)


def test_stats_finalize_edges(dev):
    """n = 0: mu and sigma all NaN (0 / 0).  Two finalizes in a row are identical bit for bit (finalize reads the buffer
    only); d = 1030 and 2048 run the grid-stride loop past the 4096-block cap (and are covered exactly in
    test_stats_exact_every_instance)."""
    from tise_toolbox_amd import device
    for d in (1030, 2048):
        acc = device.StatsAccumulator(d, dev)
        mu, sigma = acc.finalize()
        assert torch.isnan(mu).all() and torch.isnan(sigma).all()
        k = _ints(70, d, d, signed=True)
        _, v = _backed(dev, (k / 64.0).astype(np.float32), d, 0)
        acc.update(v)
        m1, s1 = acc.finalize()
        m2, s2 = acc.finalize()
        assert torch.equal(m1, m2) and torch.equal(s1, s2) and torch.isfinite(s1).all()


def test_stats_update_parts_checks_like_update(dev):
    """update_parts makes update()'s checks: a wrong width, dtype or a host tensor is refused before any launch and the
    buffer stays untouched."""
    from tise_toolbox_amd import _lib, device
    acc = device.StatsAccumulator(64, dev)
    for bad in (torch.ones((10, 65), device=dev), torch.ones((10, 64), dtype=torch.float64, device=dev),
                torch.ones((10, 8, 8), device=dev)):
        for kw in ({}, {"cov": False}, {"col_sum": False}):
            with pytest.raises(ValueError):
                acc.update_parts(bad, **kw)
    with pytest.raises(_lib.TiseLibraryError):
        acc.update_parts(torch.ones((10, 64)))
    assert not acc.buffer().cpu().numpy().any()
    acc.update_parts(torch.ones((10, 64), device=dev).t().contiguous().t())    # column-strided: made contiguous first
    S, s, n, _ = _read(acc)
    assert n == 10 and (s == 10).all() and (S == 10).all()


# ------------------------------------------------------------------------------------------- grouped updates
def _sizes(n_groups, seed):
    """Group sizes: empty first, in the middle and last; 1, 63, 64, 65 among them; the rest 0..70."""
    rng = np.random.default_rng(seed)
    sz = list(rng.integers(0, 71, n_groups))
    fixed = [0, 1, 63, 64, 65]
    for i, v in enumerate(fixed[:n_groups]):
        sz[i] = v
    if n_groups >= 3:
        sz[n_groups // 2] = 0
        sz[-1] = 0
    return [int(v) for v in sz]


GROUPED = [(64, 1, 0, 0), (64, 128, 0, 0), (64, 129, 0, 0), (64, 257, 0, 0), (128, 129, 4, 4), (2048, 80, 0, 0),
           (100, 20, 0, 0), (128, 40, 0, 1), (128, 30, 1, 0)]


@pytest.mark.parametrize("d,ng,ldx,off", GROUPED, ids=[f"d{c[0]}-g{c[1]}-ld+{c[2]}-off{c[3]}" for c in GROUPED])
def test_stats_grouped_exact(dev, d, ng, ldx, off):
    """Bound: 0.  stats_update_grouped folds group g's rows into accs[g] only: every group's S, s, n equal the exact
    sums of what it held before (every third group is pre-loaded through update()) plus its own rows, bit for bit.
    More than 128 groups take several launches of 128; d = 100, an odd ld or a 4-byte aligned base take the
    group-by-group fallback.  Empty groups, groups of 1, 63, 64 and 65 rows; accumulators not passed keep their buffers
    bit for bit."""
    from tise_toolbox_amd import device
    sizes = _sizes(ng, d + ng)
    if ng == 1:
        sizes = [129]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    k = _ints(int(offs[-1]), d, ng, signed=d != 64)
    x = (k / 64.0).astype(np.float32)
    pre_k = _ints(65, d, ng + 1, signed=True)
    accs = [device.StatsAccumulator(d, dev) for _ in range(ng)]
    bystanders = [device.StatsAccumulator(d, dev) for _ in range(2)]
    _, pv = _backed(dev, (pre_k / 64.0).astype(np.float32), d, 0)
    for g in range(0, ng, 3):
        accs[g].update(pv)
    for b in bystanders:
        b.update(pv)
    before = [b.buffer().clone() for b in bystanders]
    _, v = _backed(dev, x, d + ldx, off)
    device.stats_update_grouped(accs, v, offs)
    pS, ps = _exact_ref(pre_k)
    for g in range(ng):
        kg = k[offs[g]:offs[g + 1]]
        S_ref, s_ref = _exact_ref(kg) if len(kg) else (np.zeros((d, d)), np.zeros(d))
        n_ref = len(kg)
        if g % 3 == 0:
            S_ref, s_ref, n_ref = S_ref + pS, s_ref + ps, n_ref + 65
        if n_ref == 0:
            assert not accs[g].buffer().cpu().numpy().any(), f"empty group {g} written"
        else:
            _assert_exact(accs[g], S_ref, s_ref, n_ref, f"group {g} of {ng} ({sizes[g]} rows) d={d}")
    for b, was in zip(bystanders, before):
        assert torch.equal(b.buffer(), was)


def test_stats_grouped_argument_checks(dev):
    """Mismatched d across handles, decreasing offsets, a null handle and ld < d each return TISE_ERR_INVALID_ARG before
    any launch: every buffer keeps its contents bit for bit."""
    from tise_toolbox_amd import _lib, device
    lib = _lib.load()
    d = 64
    k = _ints(40, d, 1, signed=True)
    _, v = _backed(dev, (k / 64.0).astype(np.float32), d, 0)
    accs = [device.StatsAccumulator(d, dev) for _ in range(3)]
    odd = device.StatsAccumulator(128, dev)
    for a in accs:
        a.update(v[:7])
    before = [a.buffer().clone() for a in accs] + [odd.buffer().clone()]
    st = device._stream()

    def call(hs, offs, ld):
        h = (ctypes.c_void_p * len(hs))(*hs)
        o = (ctypes.c_int64 * len(offs))(*offs)
        return lib.tise_stats_update_grouped(h, len(hs), ctypes.c_void_p(v.data_ptr()), o, ld, st)

    good = [a._h for a in accs]
    assert call([accs[0]._h, odd._h, accs[2]._h], [0, 10, 20, 40], d) == _lib.TISE_ERR_INVALID_ARG
    assert call(good, [0, 10, 5, 40], d) == _lib.TISE_ERR_INVALID_ARG
    assert call([accs[0]._h, None, accs[2]._h], [0, 10, 20, 40], d) == _lib.TISE_ERR_INVALID_ARG
    assert call(good, [0, 10, 20, 40], d - 1) == _lib.TISE_ERR_INVALID_ARG
    torch.cuda.synchronize()
    for a, was in zip(accs + [odd], before):
        assert torch.equal(a.buffer(), was)


# ------------------------------------------------------------------------------------------- IS*
def _split_range(k, N, splits, rule):
    if rule == 0:
        return k * N // splits, (k + 1) * N // splits
    per = N // splits
    return k * per, (k + 1) * per


def _is_reference(x, T, N, splits, rule):
    """x: (N, Ce) float32 logits of the classes used.  -> A_ref, B_ref, dA, dB (per split / split x class), scores,
    mean, std and their bounds.

    Per row (first order; R = max_c |zz|, Z = max_c |zd|, P1 = sum_c p |zz|, P2 = sum_c p zz^2, l = log se):
      each exp argument zz is off by <= u (|zz| + Z), so each e by a relative u (|zz| + Z) + EF:
        rho_se = |dse| / se <= u (P1 + Z) + EF + gamma_C
        |dl| <= rho_se + EF l,            |dlse| <= |dl| + u |lse|
      the column kernel's p = exp(fl(zd - lse)): relative  eps = |dlse| + u (Z + R + l) + EF   (|zd - lse| <= R + l)
      sz = sum e zz:  |dsz| / se <= u (P2 + Z P1) + (EF + u + gamma_C) P1 + u (P1 + Z)
        |da| <= |dsz| / se + P1 rho_se + u P1 + |dl| + u |a|
    Per split of n_k rows (any summation order, several calls):
        |dA_k| <= sum |da_i| + gamma_{n_k} sum |a_i|
        |dB_kc| <= (max eps + gamma_{n_k}) B_kc + n_k 2^-1074        (exp results below 2^-1022 are subnormal)
      pbar = B / n_k: |dpbar| <= |dB| / n_k + u pbar
        |dH_k| <= sum_c |log pbar + 1| |dpbar| + (EF + 2u + gamma_C) sum_c |pbar log pbar| + C 2^-990
      x_k = A_k / n_k - H_k:  |dx| <= |dA| / n_k + u |A / n_k| + |dH| + u |x|;   |dscore| <= score (|dx| + EF)
    mean of K scores: |dmean| <= max |dscore| + (gamma_K + u) mean.  Population std is 1-Lipschitz in the max norm of the
    scores: |dstd| <= max |dscore| + |dmean| + gamma_{K+4} std."""
    inv_t = 1.0 / T
    zd = x.astype(np.float64) * inv_t
    Z = np.abs(zd).max(1)
    z = zd.astype(np.longdouble)
    m = z.max(1, keepdims=True)
    zz = z - m
    e = np.exp(zz)
    se = e.sum(1)
    l = np.log(se)
    p = e / se[:, None]
    a = (p * zz).sum(1) - l
    C = x.shape[1]
    gC = gamma(C)
    R = np.asarray(-zz.min(1), np.float64)
    P1 = np.asarray((p * -zz).sum(1), np.float64)
    P2 = np.asarray((p * zz * zz).sum(1), np.float64)
    lf = np.asarray(l, np.float64)
    lse = np.asarray(m[:, 0] + l, np.float64)
    rho_se = U * (P1 + Z) + EF + gC
    dl = rho_se + EF * lf
    dlse = dl + U * np.abs(lse)
    eps = dlse + U * (Z + R + lf) + EF
    dsz = U * (P2 + Z * P1) + (EF + U + gC) * P1 + U * (P1 + Z)
    da = dsz + P1 * rho_se + U * P1 + dl + U * np.abs(np.asarray(a, np.float64))
    A_ref, B_ref, dA, dB, sc, dsc = [], [], [], [], [], []
    for k in range(splits):
        r0, r1 = _split_range(k, N, splits, rule)
        nk = r1 - r0
        Ak = a[r0:r1].sum()
        Bk = p[r0:r1].sum(0)
        dAk = da[r0:r1].sum() + gamma(nk) * float(np.abs(a[r0:r1]).sum())
        Bf = np.asarray(Bk, np.float64)
        dBk = (eps[r0:r1].max() + gamma(nk)) * Bf + nk * 2.0 ** -1074
        pbar = Bk / nk
        with np.errstate(divide="ignore", invalid="ignore"):
            hl = np.where(pbar > 0, pbar * np.log(pbar), 0)
            lg = np.where(pbar > 0, np.abs(np.log(pbar) + 1), 0)
        Hk = hl.sum()
        dpbar = dBk / nk + U * np.asarray(pbar, np.float64)
        dHk = float((np.asarray(lg, np.float64) * dpbar).sum()) + (EF + 2 * U + gC) * float(np.abs(hl).sum()) + C * 2.0 ** -990
        xk = Ak / nk - Hk
        dx = dAk / nk + U * abs(float(Ak / nk)) + dHk + U * abs(float(xk))
        s = np.exp(xk)
        A_ref.append(float(Ak))
        B_ref.append(Bf)
        dA.append(dAk)
        dB.append(dBk)
        sc.append(float(s))
        dsc.append(float(s) * (dx + EF))
    sc = np.array(sc)
    dsc = np.array(dsc)
    mean = float(np.mean(sc.astype(np.longdouble)))
    std = float(np.sqrt(np.mean((sc.astype(np.longdouble) - mean) ** 2)))
    dmean = dsc.max() + (gamma(splits) + U) * mean
    dstd = dsc.max() + dmean + gamma(splits + 4) * std
    return dict(A=np.array(A_ref), B=np.stack(B_ref), dA=np.array(dA), dB=np.stack(dB), scores=sc, dscores=dsc,
                mean=mean, dmean=dmean, std=std, dstd=dstd)


def _cuts(N, splits, rule, seed, single=False):
    """Call borders: on split borders, one row beside them, and random ones; under O-IS a call lies wholly in the tail."""
    if single:
        return [0, N]
    rng = np.random.default_rng(seed)
    border = [_split_range(k, N, splits, rule)[0] for k in range(1, splits)]
    pick = rng.choice(border, size=min(4, len(border)), replace=False) if border else []
    cuts = {0, N}
    for i, b in enumerate(pick):
        cuts.add(int(b) + (i % 3) - 1)
    cuts.update(int(c) for c in rng.integers(1, N, 3))
    if rule == 1:
        cuts.add(_split_range(splits - 1, N, splits, rule)[1])
    return sorted(c for c in cuts if 0 <= c <= N)


def _logits(N, C, seed, saturate_T=None, first=0):
    rng = np.random.default_rng(seed)
    if saturate_T is None:
        return (rng.standard_normal((N, C)) * 2.5).astype(np.float32)
    # every row's winner among classes first .. first + 2, all other classes more than 800 T below it
    x = np.clip(rng.standard_normal((N, C)) * 0.5, -2.0, 2.0)
    x[np.arange(N), first + rng.integers(0, 3, N)] += 800.0 * saturate_T + 4.0
    return x.astype(np.float32)


# (C, drop_first, N, splits, rule, T, ld - C, single call, saturated)
IS_CASES = [
    (2, False, 300, 3, 0, 0.909, 1, False, False),
    (31, False, 1000, 10, 0, 0.05, 0, False, False),
    (32, False, 997, 10, 1, 0.909, 0, False, False),
    (33, False, 2500, 1, 0, 0.909, 0, True, False),
    (63, False, 1000, 100, 0, 50.0, 2, False, False),
    (64, False, 700, 64, 1, 0.909, 0, False, False),
    (65, False, 1000, 10, 0, 0.909, 3, False, False),
    (1000, False, 1000, 10, 0, 0.909, 0, False, False),
    (1008, True, 600, 10, 0, 0.909, 4, False, False),
    (81, True, 997, 10, 1, 0.05, 1, False, False),
    (100, False, 500, 10, 0, 0.909, 0, False, True),
    (100, True, 400, 5, 1, 0.05, 0, False, True),
    (65, False, 3000, 3, 0, 50.0, 0, True, False),
]


@pytest.mark.parametrize("case", IS_CASES, ids=[f"C{c[0]}{'-drop' if c[1] else ''}-N{c[2]}-s{c[3]}-{'ois' if c[4] else 'coco'}"
                                               f"-T{c[5]}{'-ld+%d' % c[6] if c[6] else ''}{'-one' if c[7] else ''}"
                                               f"{'-sat' if c[8] else ''}" for c in IS_CASES])
def test_is_per_element(dev, case):
    """A_k, B_kc, every split score, mean and std within the per-element bounds of _is_reference (docstring there).
    Column 0 is NaN under drop_first and the padding columns of a strided row are NaN: neither may be read.  Calls cut
    on and beside split borders (one call of > 1024 rows in one split where marked); under O-IS one call lies wholly in
    the dropped tail.  Saturated cases put every class but 3 more than 800 T below the winner: their pbar are exactly 0
    and the scores stay finite."""
    from tise_toolbox_amd import device
    C, drop, N, splits, rule, T, ldx, single, sat = case
    x = _logits(N, C, C * 31 + N + splits, saturate_T=T if sat else None, first=1 if drop else 0)
    if drop:
        x[:, 0] = np.nan
    ref = _is_reference(x[:, 1:] if drop else x, T, N, splits, rule)
    acc = device.InceptionScoreAccumulator(C, N, T, splits, "ois" if rule else "coco", drop, dev)
    cuts = _cuts(N, splits, rule, C + N, single)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        _, v = _backed(dev, x[lo:hi], C + ldx, 0)
        acc.update(v, lo)
    mean, std, scores = acc.finalize()
    got = acc.acc.cpu().numpy()
    Ce = C - (1 if drop else 0)
    A, B = got[:splits], got[splits:].reshape(splits, Ce)
    rA = np.abs(A - ref["A"]) / (SLACK * ref["dA"])
    rB = np.abs(B - ref["B"]) / (SLACK * ref["dB"])
    rS = np.abs(scores - ref["scores"]) / (SLACK * ref["dscores"])
    rm = abs(mean - ref["mean"]) / (SLACK * ref["dmean"])
    rs = abs(std - ref["std"]) / (SLACK * ref["dstd"])
    print(f"{case}: ratio A {rA.max():.3g} B {rB.max():.3g} scores {rS.max():.3g} mean {rm:.3g} std {rs:.3g}")
    assert np.isfinite(got).all() and np.isfinite(scores).all() and math.isfinite(mean) and math.isfinite(std)
    for name, r in (("A", rA), ("B", rB), ("scores", rS), ("mean", rm), ("std", rs)):
        assert np.max(r) <= 1.0, (name, float(np.max(r)))
    if sat:
        assert (B[:, 3:] == 0).all(), "saturated classes must have pbar exactly 0"
