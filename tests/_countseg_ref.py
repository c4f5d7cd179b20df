"""The numpy fp64 restatement of the CountSeg head (include/tise_hip.h, tise_countseg_head) by the neighbour rule, the margin its
decisions rest on, and the host arithmetic of CA: what the CountSeg tests hold the module, the kernel and the route against."""
import numpy as np


def head_maps(T, w_cls, b_cls, w_den, b_den):
    """T (n, h, w, 2P) fp32 -> (M, D), each (n, C, h, w) fp64: b + sum_k W[c, k] T_k with k ascending, one term at a time (every
    product of two fp32 values is exact in fp64)."""
    T = np.asarray(T, dtype=np.float32).astype(np.float64)
    P = w_cls.shape[1]
    out = []
    for wgt, b, t in ((w_cls, b_cls, T[..., :P]), (w_den, b_den, T[..., P:2 * P])):
        wgt = np.asarray(wgt, dtype=np.float32).astype(np.float64)
        acc = np.broadcast_to(np.asarray(b, dtype=np.float32).astype(np.float64), t.shape[:3] + (wgt.shape[0],)).copy()
        for k in range(P):
            acc += t[..., k, None] * wgt[None, None, None, :, k]
        out.append(np.ascontiguousarray(acc.transpose(0, 3, 1, 2)))
    return out[0], out[1]


def map_bound(T, w_cls, b_cls, w_den, b_den):
    """|b| + sum_k |W||T| per element, (n, 2C, h w): the scale of the derived bound (P + 2) 2^-53 of a map value."""
    T = np.abs(np.asarray(T, dtype=np.float64))
    P = w_cls.shape[1]
    n, h, w, _ = T.shape
    a = np.abs(b_cls.astype(np.float64))[None, :, None] + np.einsum("npk,ck->ncp", T[..., :P].reshape(n, h * w, P), np.abs(w_cls.astype(np.float64)))
    b = np.abs(b_den.astype(np.float64))[None, :, None] + np.einsum("npk,ck->ncp", T[..., P:2 * P].reshape(n, h * w, P), np.abs(w_den.astype(np.float64)))
    return np.concatenate([a, b], 1)


def _neighbour_views(m):
    """(..., h, w) -> for each of the 8 offsets (values of that neighbour, whether it lies inside the map, whether it precedes the
    pixel in row-major order)."""
    h, w = m.shape[-2:]
    pad = np.full(m.shape[:-2] + (h + 2, w + 2), -np.inf)
    pad[..., 1:-1, 1:-1] = m
    inside = np.zeros((h + 2, w + 2), dtype=bool)
    inside[1:-1, 1:-1] = True
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                yield (pad[..., 1 + dy:1 + dy + h, 1 + dx:1 + dx + w], inside[1 + dy:1 + dy + h, 1 + dx:1 + dx + w],
                       dy < 0 or (dy == 0 and dx < 0))


def local_maxima(m):
    """(..., h, w) -> bool: p is a local maximum iff every neighbour inside the map before it (row-major) is smaller and none after
    it is larger."""
    out = np.ones(m.shape, dtype=bool)
    for nb, inside, before in _neighbour_views(m):
        out &= ~inside | ((nb < m) if before else (nb <= m))
    return out


def peak_stimulation(M):
    """(n, C, h, w) fp64 -> (conf (n, C) fp64, peaks (n, C) int32): the mean, added in row-major order, of the local maxima that
    reach the lower median (ascending rank (hw - 1) // 2); a map holding a NaN: conf NaN, 0 peaks."""
    n, c, h, w = M.shape
    conf = np.zeros((n, c), dtype=np.float64)
    peaks = np.zeros((n, c), dtype=np.int32)
    for i in range(n):
        for j in range(c):
            m = M[i, j]
            if np.isnan(m).any():
                conf[i, j] = np.nan
                continue
            med = np.sort(m.reshape(-1))[(h * w - 1) // 2]
            sel = local_maxima(m) & (m >= med)
            s = 0.0
            for v in m[sel]:                                            # boolean indexing walks in row-major order
                s += v
            peaks[i, j] = int(sel.sum())
            with np.errstate(invalid="ignore", divide="ignore"):
                conf[i, j] = s / peaks[i, j]
    return conf, peaks


def density_mean(D):
    """(n, C, h, w) fp64 -> (n, C): the row-major sum over the pixels / hw."""
    n, c, h, w = D.shape
    flat = D.reshape(n, c, h * w)
    s = np.zeros((n, c), dtype=np.float64)
    for p in range(h * w):
        s += flat[:, :, p]
    return s / float(h * w)


def head(T, w_cls, b_cls, w_den, b_den):
    """-> (conf, den, peaks, maps (n, 2C, hw)) of tise_countseg_head on T = fp32(mix + b_mix)."""
    M, D = head_maps(T, w_cls, b_cls, w_den, b_den)
    conf, peaks = peak_stimulation(M)
    n, c, h, w = M.shape
    return conf, density_mean(D), peaks, np.concatenate([M.reshape(n, c, h * w), D.reshape(n, c, h * w)], 1)


def decision_margin(maps, conf, den):
    """The smallest gap any decision of an image rests on, per image (n,): a local maximum against each of its neighbours; a local
    maximum against the median, unless it is the median element itself; conf against 0; den against the nearest half-integer.
    ``maps``: the class maps (n, C, h, w); conf, den: (n, C).  A pixel that is no local maximum is kept out by its largest neighbour:
    that gap is its margin."""
    n, c, h, w = maps.shape
    out = np.full(n, np.inf)
    lm = local_maxima(maps)
    best = np.full(maps.shape, -np.inf)                                  # the largest neighbour inside the map
    for nb, inside, _ in _neighbour_views(maps):
        best = np.maximum(best, np.where(inside, nb, -np.inf))
    flat = maps.reshape(n, c, h * w)
    order = np.argsort(flat, axis=2, kind="stable")
    med_at = order[:, :, (h * w - 1) // 2]
    med = np.take_along_axis(flat, med_at[..., None], 2)[..., 0]
    is_med = np.zeros((n, c, h * w), dtype=bool)
    np.put_along_axis(is_med, med_at[..., None], True, 2)
    with np.errstate(invalid="ignore"):
        nb_gap = np.where(np.isfinite(best), np.abs(maps - best), np.inf)        # a maximum leads by it, any other pixel trails by it
        med_gap = np.where(lm & ~is_med.reshape(maps.shape), np.abs(maps - med[..., None, None]), np.inf)
    for i in range(n):
        out[i] = min(float(nb_gap[i].min()), float(med_gap[i].min()), float(np.abs(conf[i]).min()),
                     float(np.abs(den[i] - (np.floor(den[i]) + 0.5)).min()))
    return out


# ---- the host arithmetic of CA (counting_alignment/CA.py:150-187) ---------------------------------------------------------------
def counts(conf, den):
    """np.round((conf > 0) * den): half-to-even, may be negative."""
    return np.round((np.asarray(conf) > 0).astype(np.float64) * np.asarray(den, dtype=np.float64))


def item_rmse(counting_info, count_row, names):
    gt, pred = [], []
    for name, k in counting_info.items():
        gt.append(float(k))
        pred.append(float(count_row[names.index(name)]) if name in names and count_row[names.index(name)] != 0 else 0.0)
    return float(np.sqrt(np.mean((np.asarray(gt) - np.asarray(pred)) ** 2)))


# ---- integer maps with ties: name -> (map, the peaks' (y, x) in row-major order, confidence) worked out by hand -------------------
def _pocket():
    m = np.full((5, 5), 10.0)
    m[1:4, 1:4] = 0.0
    m[2, 2] = 1.0                      # a local maximum, below the median (16 tens against 9 low values): excluded
    return m


TIE_MAPS = {
    "constant": (np.full((3, 4), 2.0), [(0, 0)], 2.0),                               # only pixel 0 is a peak
    "adjacent": (np.array([[0, 0, 0], [0, 5, 5], [0, 0, 0]], dtype=np.float64), [(1, 1)], 5.0),      # the first of two equal maxima wins
    "apart": (np.array([[0, 0, 0, 0, 0], [0, 5, 0, 5, 0], [0, 0, 0, 0, 0]], dtype=np.float64), [(1, 1), (1, 3)], 5.0),
    "below_median": (_pocket(), [(0, 0)], 10.0),
    "median_duplicates": (np.array([[2, 0, 2, 0, 2, 0, 2]], dtype=np.float64), [(0, 0), (0, 2), (0, 4), (0, 6)], 2.0),
    "negative": (np.array([[-5, -1, -5], [-5, -5, -3]], dtype=np.float64), [(0, 1)], -1.0),
    "1x1": (np.array([[7.0]]), [(0, 0)], 7.0),
    "1x5": (np.array([[1, 3, 2, 3, 0]], dtype=np.float64), [(0, 1), (0, 3)], 3.0),
    "5x1": (np.array([[1], [3], [2], [3], [0]], dtype=np.float64), [(1, 0), (3, 0)], 3.0),
}


def images(n, h, w, seed):
    """Smooth seeded images plus noise, (n, h, w, 3) uint8 (uniform bytes give flat maps): per channel a product of two waves, as the
    LPIPS tests make them, plus N(0, 8) noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for _ in range(n):
        chans = [127.0 + 100.0 * np.sin(xx / (3.0 + c) + rng.uniform(0, 6)) * np.cos(yy / (4.0 + c) + rng.uniform(0, 6)) for c in range(3)]
        a = np.stack(chans, -1)
        out.append(np.clip(np.rint(a + rng.normal(0.0, 8.0, a.shape)), 0, 255).astype(np.uint8))
    return np.stack(out)
