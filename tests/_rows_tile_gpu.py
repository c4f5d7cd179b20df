"""GPU side of the gathered-row tile's width sweep and non-finite-row tests: the uploads, the raw C ABI calls and the checks that
tests/test_gpu_kid.py, tests/test_gpu_cmmd.py and tests/test_gpu_prdc.py share (inputs: tests/_rows_tile_cases.py).

Two kinds of upload.  ``nan_padded`` is the C ABI route: ld = d rounded up to 4, plus 4, every padding column NaN and one NaN row
after the last real one, inside the same allocation -- a read at or past column d, or past the last row, turns the result into
NaN, and the launch is a legal input all the same.  ``copy_forcing_layouts`` are three tensors device._rows_side has to re-lay;
their results must equal the C ABI route's bit for bit."""
import ctypes

import numpy as np

from tests import _rows_tile_cases as tc

NAN = float("nan")


def nan_padded(a, dev):
    """-> ((rows + 1, ld) tensor, ld): ``a`` in its top left corner, NaN everywhere else."""
    import torch
    n, d = a.shape
    ld = (d + 3) // 4 * 4 + 4
    buf = torch.full((n + 1, ld), NAN, dtype=torch.float32, device=dev)
    buf[:n, :d] = torch.as_tensor(np.ascontiguousarray(a), device=dev)
    assert buf.data_ptr() % 16 == 0 and ld % 4 == 0 and ld >= d + 4
    return buf, ld


def copy_forcing_layouts(a, dev):
    """-> [(name, (rows, d) tensor)]: contiguous (re-laid when d % 4 != 0), a view whose base is 4 bytes off 16-byte alignment, a
    view with column stride 2.  What lies between and around the elements is NaN."""
    import torch
    from tise_toolbox_amd import device
    t = torch.as_tensor(np.ascontiguousarray(a), device=dev)
    n, d = t.shape
    flat = torch.full((n * d + 8,), NAN, dtype=torch.float32, device=dev)
    flat[1:1 + n * d] = t.reshape(-1)
    off = flat[1:1 + n * d].view(n, d)
    wide = torch.full((n, 2 * d), NAN, dtype=torch.float32, device=dev)
    wide[:, ::2] = t
    strided = wide[:, ::2]
    assert t.is_contiguous() and off.data_ptr() % 16 == 4 and strided.stride(1) == 2
    out = [("contiguous", t), ("base 4 bytes off", off), ("column stride 2", strided)]
    for name, v in out:
        laid = device._rows_side(v, name)
        copied = laid.data_ptr() != v.data_ptr()
        assert copied == (name != "contiguous" or d % 4 != 0), (name, d)
        assert laid.stride(1) == 1 and laid.stride(0) % 4 == 0 and laid.data_ptr() % 16 == 0
        assert torch.equal(laid.view(torch.int32), t.view(torch.int32))            # bits: the rows may hold a NaN
    return out


def _i64(a):
    a = np.ascontiguousarray(a, dtype=np.int64)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


def sized_and_filled(dev, size_fn, size_args, outputs, fill):
    """The workspace, sized through the library (``size_fn(*size_args, &bytes)``), and the outputs ``[(shape, dtype)]`` pre-filled
    with ``fill`` -- an element nobody wrote shows.  -> (workspace, its size in bytes, [output tensors])"""
    import torch
    from tise_toolbox_amd import _lib
    nb = ctypes.c_size_t()
    _lib.call(size_fn, *size_args, ctypes.byref(nb))
    ws = torch.empty(max(256, nb.value), dtype=torch.uint8, device=dev)
    return ws, nb.value, [torch.full(shape, fill, dtype=dtype, device=dev) for shape, dtype in outputs]


def mmd_cabi(fn, X, Y, ox, oy, dev, ix=None, iy=None, gamma=None):
    """tise_mmd_{poly3,rbf}_grouped on NaN-padded uploads of X and Y (``fn``: "tise_mmd_poly3" or "tise_mmd_rbf") -> (n_groups, 3)
    numpy array.  The output is pre-filled with -1: a sum nobody wrote shows."""
    import torch
    from tise_toolbox_amd import _lib
    d = X.shape[1]
    (xb, ldx), (yb, ldy) = nan_padded(X, dev), nan_padded(Y, dev)
    (ox, pox), (oy, poy) = _i64(ox), _i64(oy)
    ng = len(ox) - 1
    ixd = torch.as_tensor(np.ascontiguousarray(ix, dtype=np.int64), device=dev) if ix is not None else None
    iyd = torch.as_tensor(np.ascontiguousarray(iy, dtype=np.int64), device=dev) if iy is not None else None
    ws, nb, (out,) = sized_and_filled(dev, fn + "_workspace_bytes", (pox, poy, ng), [((ng, 3), torch.float64)], -1.0)
    extra = () if gamma is None else (ctypes.c_double(gamma),)
    _lib.call(fn + "_grouped", xb.data_ptr(), X.shape[0], ldx, ixd.data_ptr() if ixd is not None else None, len(ix) if ix is not None else 0,
              pox, yb.data_ptr(), Y.shape[0], ldy, iyd.data_ptr() if iyd is not None else None, len(iy) if iy is not None else 0, poy,
              ng, d, *extra, out.data_ptr(), ws.data_ptr(), nb, None)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def relative_error(name, got, want):
    """Largest relative error over the sums; a reference sum that is exactly 0 must be met exactly."""
    worst = 0.0
    assert got.shape == want.shape and np.all(np.isfinite(got)), (name, got)
    for g in range(want.shape[0]):
        for k in range(3):
            if want[g, k] == 0:
                assert got[g, k] == 0, (name, g, k, got[g, k])
            else:
                worst = max(worst, abs(got[g, k] - want[g, k]) / abs(want[g, k]))
    return float(worst)


def check_mmd_width(fn, mmd, X, Y, want, tol, dev, gamma=None, label=""):
    """One width of the sweep through one kernel: the C ABI route against ``want`` within ``tol``; the gathered route (the same
    groups from shuffled rows) and the three re-laid tensors through ``mmd.sums`` bit for bit equal to it.  -> the error."""
    d = X.shape[1]
    got = mmd_cabi(fn, X, Y, tc.MMD_OX, tc.MMD_OY, dev, gamma=gamma)
    worst = relative_error(f"{label} d = {d}", got, want)
    print(f"{label} d = {d}: largest relative error of a sum {worst:.3e} (bound {tol:.3e})")
    (Xs, ix), (Ys, iy) = tc.shuffled(X, 11 + d), tc.shuffled(Y, 12 + d)
    gathered = mmd_cabi(fn, Xs, Ys, tc.MMD_OX, tc.MMD_OY, dev, ix, iy, gamma)
    assert gathered.tobytes() == got.tobytes(), ("gathered route", d, gathered, got)
    for (name, xt), (_, yt) in zip(copy_forcing_layouts(X, dev), copy_forcing_layouts(Y, dev)):
        via = mmd.sums(xt, yt, tc.MMD_OX, tc.MMD_OY).cpu().numpy()
        assert via.tobytes() == got.tobytes(), (name, d, via, got)
    assert worst <= tol, (label, d, worst, tol)
    return worst


def check_mask_census(fn, dev, d, zero_features, gamma=None):
    """A kernel that is 1 for every pair: every group's sums are exactly n (n - 1), m (m - 1), n m -- tile enumeration, diagonal
    masking and the double count of the strictly-upper tiles, with no tolerance at all."""
    ox = np.concatenate([[0], np.cumsum(tc.CENSUS_SIZES_X)])
    oy = np.concatenate([[0], np.cumsum(tc.CENSUS_SIZES_Y)])
    if zero_features:
        X, Y = np.zeros((ox[-1], d), np.float32), np.zeros((oy[-1], d), np.float32)
    else:
        X, Y = tc.pool3_like(ox[-1], d, 31 + d), tc.pool3_like(oy[-1], d, 32 + d)
    got = mmd_cabi(fn, X, Y, ox, oy, dev, gamma=gamma)
    assert np.array_equal(got, tc.census_expected()), (d, got)
    ix, iy = np.random.default_rng(d).permutation(ox[-1]), np.random.default_rng(d + 1).permutation(oy[-1])
    assert np.array_equal(mmd_cabi(fn, X, Y, ox, oy, dev, ix, iy, gamma), tc.census_expected()), d


def check_mmd_bad_rows(fn, dev, d, value, family, gamma=None):
    """One non-finite element in one row, at every place of tc.mmd_bad_rows(), contiguous and gathered: the two sums of the row's
    group that involve the row are non-finite; the group's third sum and EVERY other group of the launch keep the bits of the
    launch on the clean matrix (one bad row must not spread: --per-class, the KID subsets)."""
    X, Y = tc.mmd_rows(d, family)
    (Xs, ix), (Ys, iy) = tc.shuffled(X, 21 + d), tc.shuffled(Y, 22 + d)
    clean = mmd_cabi(fn, X, Y, tc.MMD_OX, tc.MMD_OY, dev, gamma=gamma)
    assert np.all(np.isfinite(clean))
    assert mmd_cabi(fn, Xs, Ys, tc.MMD_OX, tc.MMD_OY, dev, ix, iy, gamma).tobytes() == clean.tobytes()
    for side, g, pos in tc.mmd_bad_rows():
        row = int((tc.MMD_OX if side == "x" else tc.MMD_OY)[g]) + pos
        hit = np.zeros(clean.shape, bool)
        hit[g, [0, 2] if side == "x" else [1, 2]] = True
        for gathered in (False, True):
            if gathered:                                    # the group position ``row`` is row index[row] of the shuffled matrix
                Xb = tc.with_bad_row(Xs, ix[row], value) if side == "x" else Xs
                Yb = tc.with_bad_row(Ys, iy[row], value) if side == "y" else Ys
                got = mmd_cabi(fn, Xb, Yb, tc.MMD_OX, tc.MMD_OY, dev, ix, iy, gamma)
            else:
                Xb = tc.with_bad_row(X, row, value) if side == "x" else X
                Yb = tc.with_bad_row(Y, row, value) if side == "y" else Y
                got = mmd_cabi(fn, Xb, Yb, tc.MMD_OX, tc.MMD_OY, dev, gamma=gamma)
            where = (side, g, pos, "gathered" if gathered else "contiguous", value)
            assert not np.any(np.isfinite(got[hit])), (where, got)
            assert got[~hit].tobytes() == clean[~hit].tobytes(), (where, got, clean)


# ---- the k-NN kernels ---------------------------------------------------------------------------------------------------------
def knn_cabi(R, F, k, splits, dev):
    """tise_knn_radius2 on both sides and tise_prdc_counts, all on NaN-padded uploads -> (r2_real, r2_fake, cnt, rec, prec) numpy
    arrays (rec, prec as the int32 the kernel writes).  Every output is pre-filled: an element nobody wrote shows."""
    import torch
    from tise_toolbox_amd import _lib
    d = R.shape[1]
    sides, r2 = [nan_padded(R, dev), nan_padded(F, dev)], []
    for (buf, ld), rows in zip(sides, (len(R), len(F))):
        ws, nb, (out,) = sized_and_filled(dev, "tise_knn_workspace_bytes", (rows, k, splits), [((rows,), torch.float64)], -1.0)
        _lib.call("tise_knn_radius2", buf.data_ptr(), rows, ld, d, k, splits, out.data_ptr(), ws.data_ptr(), nb, None)
        r2.append(out)
    n, m = len(R), len(F)
    cnt, rec, prec = (torch.full((rows,), -1, dtype=torch.int32, device=dev) for rows in (n, n, m))
    ws = torch.empty(8 * (n + m), dtype=torch.uint8, device=dev)
    _lib.call("tise_prdc_counts", sides[0][0].data_ptr(), n, sides[0][1], r2[0].data_ptr(), sides[1][0].data_ptr(), m, sides[1][1],
              r2[1].data_ptr(), d, splits, cnt.data_ptr(), rec.data_ptr(), prec.data_ptr(), ws.data_ptr(), ws.numel(), None)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (r2[0], r2[1], cnt, rec, prec))


def knn_device(R, F, k, splits, dev):
    """The same through device.KnnManifold on (rows, d) tensors of any layout -> the same five arrays."""
    from tise_toolbox_amd import device
    knn = device.KnnManifold(dev)
    r2r, r2f = knn.radius2(R, k, splits), knn.radius2(F, k, splits)
    cnt, rec, prec = knn.counts(R, r2r, F, r2f, splits)
    return tuple(t.cpu().numpy() for t in (r2r, r2f, cnt, rec.int(), prec.int()))


def same_bits(a, b):
    return all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def check_knn_against(got, ref, exact, rel_tol, where):
    """(r2_real, r2_fake, cnt, rec, prec) against a reference dict.  The counts always equal it; r2 equals it (``exact``) or lies
    within ``rel_tol``; a NaN of the reference's r2 (a non-finite row) must be a NaN.  -> the largest relative error of an r2."""
    r2r, r2f, cnt, rec, prec = got
    worst = 0.0
    for name, g, w in (("r2_real", r2r, ref["r2_real"]), ("r2_fake", r2f, ref["r2_fake"])):
        w = np.asarray(w, dtype=np.float64)
        nan = np.isnan(w)
        assert g.dtype == np.float64 and np.array_equal(np.isnan(g), nan), (where, name, g, w)
        if exact:
            assert np.array_equal(g[~nan], w[~nan]), (where, name, int(np.sum(g[~nan] != w[~nan])))
        else:
            assert np.all(w[~nan] > 0)
            worst = max(worst, float(np.max(np.abs(g[~nan] - w[~nan]) / w[~nan])))
    assert worst <= rel_tol, (where, worst, rel_tol)
    assert cnt.dtype == np.int32 and np.array_equal(cnt, ref["cnt"]), (where, "cnt", int(np.sum(cnt != ref["cnt"])))
    assert np.array_equal(rec, ref["rec"].astype(np.int32)), (where, "rec", int(np.sum(rec != ref["rec"])))
    assert np.array_equal(prec, ref["prec"].astype(np.int32)), (where, "prec", int(np.sum(prec != ref["prec"])))
    return worst
