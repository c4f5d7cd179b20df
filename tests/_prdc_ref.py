"""Plain numpy restatement of improved precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al.
2020), written from the published definitions as the ``prdc`` package states them.  Test infrastructure only: the product
never imports it.

    d2(a, b) = max(0, |a|^2 + |b|^2 - 2 a.b)           radius r2(i) = the (k + 1)-th smallest d2 of row i's own set INCLUDING itself
    cnt(i) = #{ j : d2(R_i, F_j) < r2_R(i) }    rec(i) = any_j d2(R_i, F_j) < r2_F(j)    prec(j) = any_i d2(R_i, F_j) < r2_R(i)
    precision = mean prec    recall = mean rec    density = sum cnt / (k m)    coverage = mean [cnt > 0]

All comparisons strict, on squared values.  ``d2_expansion`` is the fp64 form the kernels implement; ``d2_direct`` forms the
differences themselves in np.longdouble and sizes the tolerances."""
from collections import OrderedDict

import numpy as np


def d2_expansion(a, b, dtype=np.float64):
    a, b = np.asarray(a).astype(dtype), np.asarray(b).astype(dtype)
    na, nb = (a * a).sum(axis=1, dtype=dtype), (b * b).sum(axis=1, dtype=dtype)
    return np.maximum(dtype(0), (na[:, None] + nb[None, :]) - dtype(2) * (a @ b.T))


def d2_direct(a, b, dtype=np.longdouble):
    """sum_c (a_c - b_c)^2 in ``dtype``, row block by row block (no expansion, no cancellation)."""
    a, b = np.asarray(a).astype(dtype), np.asarray(b).astype(dtype)
    out = np.empty((a.shape[0], b.shape[0]), dtype=dtype)
    for i in range(a.shape[0]):
        diff = b - a[i]
        out[i] = (diff * diff).sum(axis=1, dtype=dtype)
    return out


def radii2(d2_self, k):
    """(k + 1)-th smallest of every row of a set's own distance matrix, the row's own entry included (as the packages do): the
    k-th smallest over the OTHER rows, a row's entry with itself being the smallest of its row (0, or the expansion's residue)."""
    return np.sort(d2_self, axis=1)[:, k]


def prdc(real, fake, k, d2=d2_expansion):
    """-> OrderedDict precision, recall, density, coverage (Python floats) and cnt (int64), rec, prec (bool), r2_real, r2_fake,
    cross (the n x m matrix of d2(R_i, F_j))."""
    real, fake = np.asarray(real), np.asarray(fake)
    n, m = len(real), len(fake)
    assert n >= k + 1 and m >= k + 1
    r2r, r2f = radii2(d2(real, real), k), radii2(d2(fake, fake), k)
    cross = d2(real, fake)
    inside_r = cross < r2r[:, None]
    cnt = inside_r.sum(axis=1).astype(np.int64)
    prec = inside_r.any(axis=0)
    rec = (cross < r2f[None, :]).any(axis=1)
    out = OrderedDict([("precision", int(prec.sum()) / m), ("recall", int(rec.sum()) / n), ("density", int(cnt.sum()) / (k * m)),
                       ("coverage", int((cnt > 0).sum()) / n)])
    out.update(cnt=cnt, rec=rec, prec=prec, r2_real=r2r, r2_fake=r2f, cross=cross)
    return out


def prdc_direct(real, fake, k):
    """The same from direct differences in np.longdouble."""
    return prdc(real, fake, k, d2_direct)


def smallest_margin(ref):
    """Smallest relative margin |d2 - r2| / r2 over every decision of a prdc() result (both radii against every cross pair)."""
    cross = ref["cross"].astype(np.float64)
    a = np.abs(cross - ref["r2_real"][:, None].astype(np.float64)) / ref["r2_real"][:, None].astype(np.float64)
    b = np.abs(cross - ref["r2_fake"][None, :].astype(np.float64)) / ref["r2_fake"][None, :].astype(np.float64)
    return float(min(a.min(), b.min()))


def nonfinite_rows(a):
    """Indices of the rows that hold a NaN or an infinity."""
    return np.flatnonzero(~np.isfinite(np.asarray(a, dtype=np.float64)).all(axis=1))


def prdc_dropping_nonfinite(real, fake, k, d2=d2_expansion):
    """The kernels' rule for rows that hold a NaN or an infinity (include/tise_hip.h), stated through the clean definition: such
    a row is nobody's neighbour and lies in no ball, so every other row's r2, cnt, rec and prec are those of ``prdc`` on the sets
    WITHOUT these rows; the row itself gets r2 = NaN, cnt = 0, rec = False, prec = False.  -> dict of full-size cnt, rec, prec,
    r2_real, r2_fake and the clean sub-problem's result under "clean".  (For a NaN -- not for an infinity -- plain ``prdc`` on the
    dirty input gives the same arrays: np.maximum keeps a NaN, np.sort puts it last and every comparison with it is False.)"""
    real, fake = np.asarray(real), np.asarray(fake)
    bad_r, bad_f = nonfinite_rows(real), nonfinite_rows(fake)
    keep_r, keep_f = np.setdiff1d(np.arange(len(real)), bad_r), np.setdiff1d(np.arange(len(fake)), bad_f)
    clean = prdc(real[keep_r], fake[keep_f], k, d2)
    out = dict(cnt=np.zeros(len(real), np.int64), rec=np.zeros(len(real), bool), prec=np.zeros(len(fake), bool),
               r2_real=np.full(len(real), np.nan), r2_fake=np.full(len(fake), np.nan), clean=clean)
    out["cnt"][keep_r], out["rec"][keep_r], out["r2_real"][keep_r] = clean["cnt"], clean["rec"], clean["r2_real"]
    out["prec"][keep_f], out["r2_fake"][keep_f] = clean["prec"], clean["r2_fake"]
    return out
