"""GPU: the nearest-row search (nn_argmin_kernel / nn_merge_kernel, csrc/knn.hip) through the C ABI and
device.KnnManifold.nearest.

idx carries no tolerance: tests/test_nn_host.py asserts, from the reference alone, that the best and the second-best d2 of every
row of every float case lie a relative MIN_MARGIN (1e-9) apart, six orders of magnitude above the arithmetic's error, so idx must
EQUAL the reference's with zero exclusions.  d2 is held within tests/test_gpu_prdc.py's REL_TOL: the same expansion, the same
tile, the same bound (8 x the measured spread between the fp64 expansion and longdouble differences).  The integer-valued cases
are exact in any order: d2 equals the int64 value and every tie goes to the smallest index."""
import ctypes

import numpy as np
import pytest

from tests import _nn_cases as cases
from tests import _nn_ref
from tests import _prdc_cases as pc
from tests.test_gpu_prdc import REL_TOL


def _dev(a, dev, pad=cases.PAD, fill=7.0):
    import torch
    t = torch.as_tensor(np.asarray(a), device=dev)
    if pad:
        wide = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=t.dtype, device=dev)     # the padding must never be read
        wide[:, :t.shape[1]] = t
        t = wide[:, :t.shape[1]]
        assert t.stride(0) == a.shape[1] + pad
    return t


def _bits(pair):
    return pair[0].cpu().numpy().tobytes() + pair[1].cpu().numpy().tobytes()


def _host(pair):
    d2, idx = pair[0].cpu().numpy(), pair[1].cpu().numpy()
    assert d2.dtype == np.float64 and idx.dtype == np.int32
    return d2, idx


def _check(got, want_d2, want_idx, what):
    d2, idx = _host(got)
    assert d2.shape == want_d2.shape and idx.shape == want_idx.shape
    assert np.array_equal(idx, want_idx), (what, int(np.sum(idx != want_idx)))
    rel = float(np.max(np.abs(d2 - want_d2) / want_d2))
    assert rel <= REL_TOL, (what, rel)
    return rel


@pytest.mark.gpu
@pytest.mark.parametrize("shape", cases.SHAPES, ids=cases.shape_id)
def test_nearest_matches_the_reference_and_does_not_depend_on_the_splits(cuda_device, shape):
    """Both passes of every case: idx equal, d2 within REL_TOL, and the bits of every col_splits and of a second call the same."""
    from tise_toolbox_amd import device
    Q, B, ref = cases.float_case(*shape)
    knn = device.KnnManifold(cuda_device)
    qd, bd = _dev(Q, cuda_device), _dev(B, cuda_device)
    first = knn.nearest(qd, bd)
    worst = _check(first, ref["d2"], ref["idx"], ("cross", shape))
    for splits in cases.SPLITS:
        assert _bits(knn.nearest(qd, bd, col_splits=splits)) == _bits(first), ("cross", shape, splits)
    if shape[1] >= 2:
        own = knn.nearest(bd, bd, exclude_diagonal=True)
        worst = max(worst, _check(own, ref["d2_self"], ref["idx_self"], ("within", shape)))
        for splits in cases.SPLITS:
            assert _bits(knn.nearest(bd, bd.clone(), True, splits)) == _bits(own), ("within", shape, splits)
    else:
        d2, idx = _host(knn.nearest(bd, bd, exclude_diagonal=True))       # one row and nobody else: no candidate
        assert d2.tolist() == [np.inf] and idx.tolist() == [-1]
    assert _bits(device.KnnManifold(cuda_device).nearest(qd, bd)) == _bits(first)
    print(f"{shape}: largest relative error of a d2 {worst:.3e} (bound {REL_TOL:.3e})")


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1])
def test_integer_cases_are_exact_and_ties_go_to_the_smallest_index(cuda_device, which):
    from tise_toolbox_amd import device
    Q, B, cross, own = cases.integer_case(which)
    knn = device.KnnManifold(cuda_device)
    qd, bd = _dev(Q, cuda_device), _dev(B, cuda_device)
    want = cases.exact_nearest(cross)
    want_own = cases.exact_nearest(own, exclude_diagonal=True)
    for splits in cases.SPLITS:
        d2, idx = _host(knn.nearest(qd, bd, col_splits=splits))
        assert np.array_equal(d2, want[0].astype(np.float64)) and np.array_equal(idx, want[1]), ("cross", which, splits)
        d2, idx = _host(knn.nearest(bd, bd, True, splits))
        assert np.array_equal(d2, want_own[0].astype(np.float64)) and np.array_equal(idx, want_own[1]), ("within", which, splits)
    if which == 0:
        d2, idx = _host(knn.nearest(qd, bd, col_splits=2))
        assert (d2[3], idx[3], d2[71], idx[71], d2[10], idx[10]) == (0.0, 5, 1.0, 5, 0.0, 100)


@pytest.mark.gpu
@pytest.mark.parametrize("d", cases.CONTRACT_D)
def test_the_within_set_pass_has_the_bits_of_radius2_at_k_1(cuda_device, d):
    """The contract with the parent: the same pairs, the same d2 bits, the same minimum."""
    from tise_toolbox_amd import device
    knn = device.KnnManifold(cuda_device)
    for n in pc.radii_rows(1):
        X, _ = pc.radii_set(n, d)
        xd = _dev(X, cuda_device)
        want = knn.radius2(xd, 1).cpu().numpy()
        for splits in (0, 3):
            got = knn.nearest(xd, xd, True, splits)[0].cpu().numpy()
            assert got.tobytes() == want.tobytes(), (n, d, splits)


@pytest.mark.gpu
def test_padding_columns_are_never_read(cuda_device):
    """NaN in the padding (a read would poison d2) and the contiguous upload give the same bits, at a width that is no multiple
    of 4, one that is no multiple of 64 and one that is."""
    from tise_toolbox_amd import device
    knn = device.KnnManifold(cuda_device)
    for shape in ((64, 63, 100), (129, 65, 68), (63, 64, 64), (300, 260, 1)):
        Q, B, ref = cases.float_case(*shape)
        want = knn.nearest(_dev(Q, cuda_device, pad=0), _dev(B, cuda_device, pad=0))
        _check(want, ref["d2"], ref["idx"], shape)
        for pad, fill in ((cases.PAD, float("nan")), (4, float("inf")), (cases.PAD, 7.0)):
            got = knn.nearest(_dev(Q, cuda_device, pad, fill), _dev(B, cuda_device, pad, fill))
            assert _bits(got) == _bits(want), (shape, pad, fill)


def _without(idx, row):
    """Indices of a call without base row ``row`` moved to the numbering of the call with it."""
    return np.where(idx >= row, idx + 1, idx).astype(np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "-inf"])
def test_non_finite_rows(cuda_device, value):
    from tise_toolbox_amd import device
    knn = device.KnnManifold(cuda_device)
    Q, B, ref = cases.float_case(129, 65, 68)
    qd = _dev(Q, cuda_device)
    # a query row: (NaN, -1) for it, every other row untouched
    for row in (0, 64, 128):
        Qb = Q.copy()
        Qb[row, 67 if row else 0] = value
        d2, idx = _host(knn.nearest(_dev(Qb, cuda_device), _dev(B, cuda_device)))
        clean = _host(knn.nearest(qd, _dev(B, cuda_device)))
        assert np.isnan(d2[row]) and idx[row] == -1
        keep = np.arange(len(Q)) != row
        assert d2[keep].tobytes() == clean[0][keep].tobytes() and np.array_equal(idx[keep], clean[1][keep])
    # a base row: nobody's nearest row; every query row has the bits of the call without that row, indices shifted.  The rows
    # chosen include the nearest row of some query row (else the test would test nothing)
    for row in (int(ref["idx"][0]), 0, 64):
        Bb = B.copy()
        Bb[row, 3] = value
        rest = np.delete(B, row, axis=0)
        for splits in (0, 2):
            d2, idx = _host(knn.nearest(qd, _dev(Bb, cuda_device), col_splits=splits))
            want = _host(knn.nearest(qd, _dev(rest, cuda_device), col_splits=splits))
            assert d2.tobytes() == want[0].tobytes() and np.array_equal(idx, _without(want[1], row)), (row, splits)
            assert not np.any(idx == row)
        r_d2, r_idx, _ = _nn_ref.nearest(Q, Bb)
        assert np.array_equal(idx, r_idx) and float(np.max(np.abs(d2 - r_d2) / r_d2)) <= REL_TOL
        # the within-set pass: the bad row is a query row too
        d2, idx = _host(knn.nearest(_dev(Bb, cuda_device), _dev(Bb, cuda_device), True))
        want = _host(knn.nearest(_dev(rest, cuda_device), _dev(rest, cuda_device), True))
        keep = np.arange(len(B)) != row
        assert np.isnan(d2[row]) and idx[row] == -1
        assert d2[keep].tobytes() == want[0].tobytes() and np.array_equal(idx[keep], _without(want[1], row))
    # every base row non-finite: no candidate anywhere
    Bb = B.copy()
    Bb[:, 5] = value
    d2, idx = _host(knn.nearest(qd, _dev(Bb, cuda_device)))
    assert np.all(np.isposinf(d2)) and np.all(idx == -1)


@pytest.mark.gpu
def test_c_abi_call_with_a_workspace_sized_by_the_library_and_the_wrapper_refusals(cuda_device):
    import torch
    from tise_toolbox_amd import _lib, device
    Q, B, ref = cases.float_case(193, 257, 100)
    qd, bd = torch.as_tensor(Q, device=cuda_device), torch.as_tensor(B, device=cuda_device)
    nb = ctypes.c_size_t()
    _lib.call("tise_nn_workspace_bytes", 193, 257, 3, ctypes.byref(nb))
    assert nb.value == 8 * (193 + 257) + 12 * 193 * 3
    ws = torch.empty(nb.value, dtype=torch.uint8, device=cuda_device)
    d2 = torch.full((193,), -1.0, dtype=torch.float64, device=cuda_device)
    idx = torch.full((193,), -7, dtype=torch.int32, device=cuda_device)
    _lib.call("tise_nn_argmin", qd.data_ptr(), 193, 100, bd.data_ptr(), 257, 100, 100, 0, 3, d2.data_ptr(), idx.data_ptr(),
              ws.data_ptr(), nb.value, None)
    torch.cuda.synchronize()
    _check((d2, idx), ref["d2"], ref["idx"], "c abi")
    assert _bits((d2, idx)) == _bits(device.KnnManifold(cuda_device).nearest(qd, bd))
    knn = device.KnnManifold(cuda_device)
    with pytest.raises(ValueError, match="row counts must agree"):
        knn.nearest(qd, bd, exclude_diagonal=True)
    with pytest.raises(ValueError, match="same, positive number of columns"):
        knn.nearest(qd, bd[:, :64])
    with pytest.raises(ValueError, match="need rows"):
        knn.nearest(qd[:0], bd)
    with pytest.raises(_lib.TiseStatusError):
        knn.nearest(qd, bd, col_splits=1025)
