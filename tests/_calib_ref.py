"""Shared reference for the calibration kernel's tests (helper, no tests): the fp64 numpy oracle of csrc/calibrate.hip with
its per-row error bounds, the seeded logits, the NaN-filled embedding, and an mpmath restatement that checks the oracle.

Rounding analysis of calibrate.hip (u = 2^-53), per row with C classes, X = max_c |d_c| / T:
  d_c = z_c - m is exact; x_c = fl(d_c * fl(1/T)) = (d_c / T)(1 + 2u); ocml exp is within 1 ulp, so
  e_c = exp(d_c / T)(1 + eps), |eps| <= (2 + 2 X) u.  s = sum e_c and sd = sum d_c e_c carry another gamma_C relative to
  sum |.|, so with K = C + 2 X + 8:
    |nll err| <= u (K + |nll| + 2 |z_y - m| / T)                   (log within 1 ulp, the product, the subtraction)
    |g err|   <= u (K + 4) (|z_y - m| + sum |d| e / s) / T^2      (sd / s, the two products by 1/T)
  and the fold over N rows adds gamma_N sum |.|.  The oracle evaluates the same formulas in fp64 with numpy (its own
  error has the same bound: tests/test_calibration_host.py checks that against mpmath), so a comparison of the kernel
  with the oracle allows twice the bound."""
import numpy as np
import torch

U = 2.0 ** -53


def gamma(n):
    return n * U / (1.0 - n * U)


def calib_shape(C):
    """(G lanes per row, K values per lane; K = 0: the streaming form) -- csrc/calibrate.hip, calib_shape."""
    if C <= 64:
        return 4, 16
    if C <= 128:
        return 8, 16
    if C <= 256:
        return 16, 16
    if C <= 1024:
        return 64, 16
    if C <= 2048:
        return 64, 32
    return 64, 0


def instance_of(C):
    g, k = calib_shape(C)
    return f"<{g},{k}>"


def rows_per_block(C):
    """Rows one block takes per grid step (csrc/calibrate.hip, calib_shape): 4 waves x 64 / G rows."""
    g = 4 if C <= 64 else 8 if C <= 128 else 16 if C <= 256 else 64
    return 4 * (64 // g)


def make_logits(rows, C, T, seed, ties=True):
    """fp32 logits with |z - m| / T up to ~700, some rows with exactly tied maxima, and rows whose confidence is exactly
    1 / k (k tied maxima, every other logit 1e4 below: exp underflows to 0) -- 1/2, 1/4, 1/5 ... sit on bin edges."""
    rng = np.random.default_rng(seed)
    spread = rng.uniform(0.05, 1.0, size=(rows, 1)) * 700.0 * T / 4.0
    z = (rng.standard_normal((rows, C)) * spread).astype(np.float32)
    labels = rng.integers(0, C, size=rows)
    if ties and C >= 2:
        for i in range(0, rows, 7):                          # tied maxima: the first index must win
            k = min(C, int(rng.integers(2, 6)))
            cols = np.sort(rng.choice(C, size=k, replace=False))
            z[i, cols] = z[i].max() + 1.0
            labels[i] = cols[i % 2]                          # the first tied column or the second
        for i in range(3, rows, 11):                         # exact confidences 1/k
            k = [1, 2, 4, 5, 10, 15][i % 6]
            if k > C:
                continue
            z[i] = -1e4
            z[i, rng.choice(C, size=k, replace=False)] = 0.0
    return z, labels.astype(np.int64)


def embed(z, c0, extra_cols, dev):
    """Put (rows, C) logits at column c0 of a NaN-filled (rows + 1, c0 + C + extra_cols) device buffer."""
    rows, C = z.shape
    ld = c0 + C + extra_cols
    buf = torch.full((rows + 1, ld), float("nan"), dtype=torch.float32, device=dev)
    buf[:rows, c0:c0 + C] = torch.from_numpy(z).to(dev)
    return buf[:rows], ld


def oracle_rows(z, labels, T):
    """Per row, in fp64: nll, g, their bounds b_nll / b_g (module docstring, not doubled), conf = fl32(1 / s), the first
    argmax, and s."""
    x = z.astype(np.float64)
    n, C = x.shape
    m = x.max(axis=1)
    d = x - m[:, None]
    e = np.exp(d * (1.0 / T))
    s = e.sum(axis=1)
    sd = (d * e).sum(axis=1)
    dy = x[np.arange(n), labels] - m
    nll = np.log(s) - dy * (1.0 / T)
    g = (dy - sd / s) / T / T
    X = np.abs(d).max(axis=1) / T
    K = C + 2 * X + 8
    b_nll = U * (K + np.abs(nll) + 2 * np.abs(dy) / T)
    b_g = U * (K + 4) * (np.abs(dy) + (np.abs(d) * e).sum(axis=1) / s) / T ** 2
    conf = (1.0 / s).astype(np.float32)
    pred = np.argmax(z, axis=1)                              # first maximum
    return {"nll": nll, "g": g, "b_nll": b_nll, "b_g": b_g, "conf": conf, "pred": pred, "s": s}


def bin_rows(conf, correct, edges):
    """count / sum conf / sum correct per bin (edges[b], edges[b + 1]] for fp32 confidences."""
    n_bins = len(edges) - 1
    cnt, csum, cor = np.zeros(n_bins), np.zeros(n_bins), np.zeros(n_bins)
    for b in range(n_bins):
        inb = (conf > edges[b]) & (conf <= edges[b + 1])
        cnt[b] = inb.sum()
        csum[b] = conf[inb].astype(np.float64).sum()
        cor[b] = correct[inb].sum()
    return cnt, csum, cor


def oracle(z, labels, T, n_bins, edges=None):
    """fp64 numpy restatement of the kernel's formulas, plus per-row error bounds (module docstring).  edges: the
    ascending fp32 bin edges (default: the reference's torch.linspace(0, 1, n_bins + 1))."""
    r = oracle_rows(z, labels, T)
    n = z.shape[0]
    nll, g = r["nll"], r["g"]
    if edges is None:
        edges = torch.linspace(0, 1, n_bins + 1).numpy()
    cnt, csum, cor = bin_rows(r["conf"], r["pred"] == labels, edges)
    return {"nll": nll.sum(), "g": g.sum(), "b_nll": 2 * (r["b_nll"].sum() + gamma(n) * np.abs(nll).sum()),
            "b_g": 2 * (r["b_g"].sum() + gamma(n) * np.abs(g).sum()), "count": cnt, "conf": csum, "correct": cor}


# ---- mpmath: what the oracle is checked against ------------------------------------------------------------------------------
def mp_row(z_row, label, T, dps=60):
    """One row at dps digits -> (nll, g, 1 / s) as mpmath numbers; z_row fp32 and T fp64 enter exactly."""
    import mpmath
    with mpmath.workdps(dps):
        zz = [mpmath.mpf(float(v)) for v in z_row]
        t = mpmath.mpf(float(T))
        m = max(zz)
        d = [v - m for v in zz]
        e = [mpmath.exp(v / t) for v in d]
        s = mpmath.fsum(e)
        sd = mpmath.fsum(a * b for a, b in zip(d, e))
        dy = zz[int(label)] - m
        return +(mpmath.log(s) - dy / t), +((dy - sd / s) / t / t), +(1 / s)


def mp_abs_err(x, ref, dps=60):
    """|x - ref| for an fp64 x and an mpmath ref, subtracted at dps digits (not at mpmath's default 53 bits)."""
    import mpmath
    with mpmath.workdps(dps):
        return float(abs(mpmath.mpf(float(x)) - ref))


def fp32_midpoint_distance(inv_s, dps=60):
    """Relative distance of the mpmath number inv_s to the nearest midpoint of two neighbouring fp32 values: how far 1 / s
    is from the places where fl32 changes its mind."""
    import mpmath
    with mpmath.workdps(dps):
        c = np.float32(float(inv_s))
        best = None
        for other in (np.nextafter(c, np.float32(0)), np.nextafter(c, np.float32(2))):
            mid = (mpmath.mpf(float(c)) + mpmath.mpf(float(other))) / 2
            dist = abs(inv_s - mid) / inv_s
            best = dist if best is None or dist < best else best
        return float(best)
