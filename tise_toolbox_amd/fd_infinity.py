"""FD-infinity on MI355X: the Frechet distance extrapolated to an infinite number of generated samples.

Chong & Forsyth 2020 ("Effectively Unbiased FID and Inception Score and where to find them"), as the `dgm-eval` package of Stein
et al. 2023 computes it (the definition is RESTATED FROM MEMORY, README).  The Frechet distance of N generated samples against
fixed reference statistics is biased upwards by a term close to linear in 1 / N; with m generated rows:

    sizes      = np.linspace(min(5000, max(m // 10, 2)), m, num_points).astype(int32)          (num_points = 15)
    FD_N       = the Frechet distance of a random subset of N generated rows, drawn without replacement, against the statistics
                 of ALL reference rows
    FD-inf     = the intercept of the least-squares line of FD_N over 1 / N

dgm-eval draws the subsets unseeded, so its number changes from run to run; this module draws them from
``np.random.default_rng(seed)`` (one generator, the sizes in ascending order) and the result is reproducible.

The reference side is factored ONCE (FrechetSolver.prefactor) and every subset is one distance_prefactored; a subset's statistics
come from gathering its rows on the device into a StatsAccumulator.  When the solver flags non-finite values the subset's distance
is recomputed by fid_score.calculate_frechet_distance (its eps rescue), as fid_score does.
"""
import numpy as np
import torch

from . import _lib, device
from .engine import frechet_solver, require_gpu
from .feature_space import rows_f32


def fd_infinity_sizes(m, num_points=15):
    """The subset sizes for m generated rows.  Host."""
    m, num_points = int(m), int(num_points)
    if m < 2:
        raise ValueError(f"FD-infinity needs at least 2 generated rows (got {m})")
    if num_points < 2:
        raise ValueError(f"a line needs at least 2 points (got num_points = {num_points})")
    return np.linspace(min(5000, max(m // 10, 2)), m, num_points).astype(np.int32)


def fd_infinity_subsets(m, num_points, seed):
    """One index array (int64, in drawing order, no repeats) per size of ``fd_infinity_sizes``, from one seeded generator.  Host."""
    rng = np.random.default_rng(seed)
    return [rng.choice(int(m), size=int(s), replace=False).astype(np.int64) for s in fd_infinity_sizes(m, num_points)]


def fit_intercept(sizes, fds):
    """The intercept of the least-squares line of ``fds`` over 1 / ``sizes`` (closed form, fp64).  Host."""
    x, y = 1.0 / np.asarray(sizes, dtype=np.float64), np.asarray(fds, dtype=np.float64)
    xm, ym = x.mean(), y.mean()
    sxx = float(np.sum((x - xm) ** 2))
    if sxx == 0.0:
        raise ValueError("every subset has the same size: there is no line to fit")
    return float(ym - np.sum((x - xm) * (y - ym)) / sxx * xm)


def fd_infinity_from_features(ref, gen, num_points=15, seed=0):
    """``ref`` (n, dims), ``gen`` (m, dims): device tensors or numpy arrays -> dict(fd_infinity=float, sizes=int32 array,
    fds=fp64 array of FD_N)."""
    from . import fid_score
    for f in (ref, gen):
        if len(tuple(f.shape)) != 2:
            raise ValueError("features must be (rows, dims)")
    if ref.shape[1] != gen.shape[1]:
        raise ValueError(f"feature widths differ: {ref.shape[1]} and {gen.shape[1]}")
    if ref.shape[0] < 2:
        raise ValueError(f"FD-infinity needs at least 2 reference rows (got {ref.shape[0]})")
    subsets = fd_infinity_subsets(gen.shape[0], num_points, seed)
    if len({len(s) for s in subsets}) < 2:
        raise ValueError(f"{gen.shape[0]} generated rows give one subset size only: there is no line to fit")
    require_gpu()
    dev = ref.device if isinstance(ref, torch.Tensor) and ref.is_cuda else torch.device("cuda", torch.cuda.current_device())
    R, G = rows_f32(ref, dev), rows_f32(gen, dev)
    d = R.shape[1]
    with torch.cuda.device(dev):
        stats = device.StatsAccumulator(d, dev)
        stats.update(R)
        mu_r, sigma_r = stats.finalize()
        solver = frechet_solver(d, dev)
        solver.prefactor(sigma_r)
        fds = []
        for index in subsets:
            stats.reset()
            stats.update(G.index_select(0, torch.from_numpy(index).to(dev)))
            mu, sigma = stats.finalize()
            try:
                res = solver.distance_prefactored(mu_r, mu, sigma)
                fallback = bool(res["flags"] & _lib.TISE_FLAG_NONFINITE)
            except _lib.TiseStatusError:                                   # the process-wide solver served someone else in between
                fallback = True
            if fallback:
                fds.append(float(fid_score.calculate_frechet_distance(mu_r, sigma_r, mu, sigma)))
                solver.prefactor(sigma_r)                                  # the one-call form factors in the same solver
            else:
                fds.append(float(res["fid"]))
        stats.close()
    sizes = np.array([len(s) for s in subsets], dtype=np.int32)
    fds = np.array(fds, dtype=np.float64)
    return dict(fd_infinity=fit_intercept(sizes, fds), sizes=sizes, fds=fds)
