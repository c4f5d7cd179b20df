"""CPU: the host side of CMMD / CLIP-FID -- the two estimators of cmmd.cmmd_from_sums against the textbook forms, argument
errors, the feature file and its refusals, the CLI's defaults, and the C ABI declarations and argument checks of tise_mmd_rbf_*."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import _cmmd_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"tise_mmd_rbf_workspace_bytes": 4, "tise_mmd_rbf_grouped": 19}


def unit_rows(n, d, seed, shift=0.0):
    a = np.random.default_rng(seed).standard_normal((n, d)) + shift
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)


def test_header_and_signatures_carry_the_new_symbols_with_the_same_argument_counts():
    from tise_toolbox_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tise_hip.h")).read(), flags=re.S)
    for name, nargs in NEW.items():
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text)
        assert m is not None and name in _lib.SIGNATURES, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
    # the polynomial entry's arguments, one for one, plus gamma after d
    poly, rbf = _lib.SIGNATURES["tise_mmd_poly3_grouped"][1], _lib.SIGNATURES["tise_mmd_rbf_grouped"][1]
    assert rbf[:14] == poly[:14] and rbf[14] is ctypes.c_double and rbf[15:] == poly[14:]
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name)


@pytest.mark.parametrize("n,m", [(7, 5), (1, 6), (4, 1), (33, 40)])
def test_cmmd_from_sums_equals_the_textbook_forms(n, m):
    from tise_toolbox_amd import cmmd
    assert cmmd.SIGMA == 10.0 and cmmd.GAMMA == 1 / 200 and cmmd.SCALE == 1000.0
    x, y = unit_rows(n, 48, 10 + n), unit_rows(m, 48, 20 + m, shift=0.3)
    sums = _cmmd_ref.rbf_sums(x, y, cmmd.GAMMA)
    v = cmmd.cmmd_from_sums(sums, n, m)
    assert isinstance(v, float) and abs(v - _cmmd_ref.cmmd_v(x, y)) <= 1e-12
    assert v > 0                                               # a V-statistic of two different sets
    if n >= 2 and m >= 2:
        assert abs(cmmd.cmmd_from_sums(sums, n, m, unbiased=True) - _cmmd_ref.cmmd_u(x, y)) <= 1e-12
    else:
        with pytest.raises(ValueError):
            cmmd.cmmd_from_sums(sums, n, m, unbiased=True)


def test_identical_sets_give_zero():
    from tise_toolbox_amd import cmmd
    x = unit_rows(21, 64, 3)
    assert abs(cmmd.cmmd_from_sums(_cmmd_ref.rbf_sums(x, x, cmmd.GAMMA), 21, 21)) <= 1e-12
    assert abs(_cmmd_ref.cmmd_v(x, x)) <= 1e-12


def test_value_errors():
    from tise_toolbox_amd import cmmd
    for n, m, unbiased in ((0, 5, False), (5, 0, False), (1, 5, True), (5, 1, True)):
        with pytest.raises(ValueError):
            cmmd.cmmd_from_sums((0.0, 0.0, 0.0), n, m, unbiased)
    with pytest.raises(ValueError, match="widths differ"):    # before anything asks for a GPU
        cmmd.cmmd_from_features(np.zeros((3, 512), np.float32), np.zeros((3, 768), np.float32))
    with pytest.raises(ValueError):
        cmmd.cmmd_from_features(np.zeros(512, np.float32), np.zeros((3, 512), np.float32))


def test_feature_file_round_trip_and_refusals(tmp_path):
    from tise_toolbox_amd import cmmd, fid_score
    feats = np.random.default_rng(0).standard_normal((9, 512)).astype(np.float32)
    mu, sigma = feats.astype(np.float64).mean(0), np.cov(feats.astype(np.float64), rowvar=False)
    good = str(tmp_path / "good.npz")
    cmmd.save_features_npz(good, feats, mu, sigma)
    with np.load(good) as f:
        assert sorted(f.files) == ["features", "mu", "network", "sigma"] and str(f["network"]) == "clip-vit-b32"
        assert f["features"].dtype == np.float32
    f2, m2, s2 = cmmd.load_features_npz(good)
    assert f2.dtype == np.float32 and np.array_equal(f2, feats) and np.array_equal(m2, mu) and np.array_equal(s2, sigma)
    other, untagged, rowless = str(tmp_path / "other.npz"), str(tmp_path / "untagged.npz"), str(tmp_path / "rowless.npz")
    fid_score.save_stats_npz(other, mu, sigma, "inception-2015", feats)
    fid_score.save_stats_npz(untagged, mu, sigma, "torchvision", feats)
    fid_score.save_stats_npz(rowless, mu, sigma, cmmd.NETWORK)
    with pytest.raises(RuntimeError, match="inception-2015"):
        cmmd.load_features_npz(other)
    with pytest.raises(RuntimeError, match="no network tag"):
        cmmd.load_features_npz(untagged)
    with pytest.raises(RuntimeError, match="no 'features' array"):
        cmmd.load_features_npz(rowless)
    # and the Inception side refuses a CLIP file
    with pytest.raises(RuntimeError, match="clip-vit-b32"):
        fid_score.check_stats_network(good, "clip-vit-b32", "torchvision")


def test_cli_defaults():
    from tise_toolbox_amd import cmmd
    a = cmmd.parse_args(["--path1", "ref", "--path2", "gen"])
    assert (a.path1, a.path2, a.batch_size, a.weights, a.synthetic_weights, a.seed) == ("ref", "gen", 50, None, False, 0)
    assert (a.clip_fid, a.unbiased, a.save_features, a.saved_file, a.png_feed, a.num_workers, a.gpu) == (False, False, "", "", "ring", 0, "0")
    b = cmmd.parse_args(["--path1", "r.npz", "--path2", "g", "--clip-fid", "--unbiased", "--save-features", "o.npz", "--saved_file", "f.txt",
                         "--png-feed", "dataloader", "--num-workers", "3", "--gpu", "2", "--synthetic-weights", "--seed", "4"])
    assert (b.clip_fid, b.unbiased, b.save_features, b.saved_file, b.png_feed, b.num_workers, b.gpu, b.seed) == \
        (True, True, "o.npz", "f.txt", "dataloader", 3, "2", 4)
    with pytest.raises(SystemExit):
        cmmd.parse_args(["--path1", "ref"])


def test_no_gpu_means_a_library_error(monkeypatch):
    import torch
    from tise_toolbox_amd import _lib, cmmd
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_lib.TiseLibraryError):
        cmmd.main(["--path1", "a", "--path2", "b", "--synthetic-weights"])
    with pytest.raises(_lib.TiseLibraryError):
        cmmd.cmmd_from_features(np.ones((3, 8), np.float32), np.ones((2, 8), np.float32))


def _offs(*v):
    a = np.asarray(v, dtype=np.int64)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


def test_workspace_is_the_polynomial_one_plus_a_double_per_row_used():
    from tise_toolbox_amd import _lib
    lib = _lib.load()
    nb, nb3 = ctypes.c_size_t(), ctypes.c_size_t()
    (_, ox), (_, oy) = _offs(5, 1005, 1045, 1045), _offs(0, 1000, 1048, 1100)
    assert lib.tise_mmd_poly3_workspace_bytes(ox, oy, 3, ctypes.byref(nb3)) == _lib.TISE_OK
    assert lib.tise_mmd_rbf_workspace_bytes(ox, oy, 3, ctypes.byref(nb)) == _lib.TISE_OK
    assert nb3.value == 512 + 8 * (528 + 3 + 1) and nb.value == nb3.value + 8 * (1040 + 1100)
    assert lib.tise_mmd_rbf_workspace_bytes(ox, oy, 0, ctypes.byref(nb)) == _lib.TISE_OK and nb.value == 0
    bad = _lib.TISE_ERR_INVALID_ARG
    assert lib.tise_mmd_rbf_workspace_bytes(None, oy, 3, ctypes.byref(nb)) == bad
    assert lib.tise_mmd_rbf_workspace_bytes(ox, oy, 3, None) == bad
    assert lib.tise_mmd_rbf_workspace_bytes(_offs(0, 5, 4)[1], _offs(0, 5, 6)[1], 2, ctypes.byref(nb)) == bad
    big = _offs(0, (1 << 24) + 1)[1]
    assert lib.tise_mmd_rbf_workspace_bytes(big, big, 1, ctypes.byref(nb)) == _lib.TISE_ERR_UNSUPPORTED


def rbf_call(lib, keep, x, rows_x, ld_x, ix, nix, ox, y, rows_y, ld_y, iy, niy, oy, ng, d, gamma, out, ws, ws_bytes):
    pox = poy = None
    if ox is not None:
        a, pox = _offs(*ox)
        keep.append(a)
    if oy is not None:
        a, poy = _offs(*oy)
        keep.append(a)
    return lib.tise_mmd_rbf_grouped(x, rows_x, ld_x, ix, nix, pox, y, rows_y, ld_y, iy, niy, poy, ng, d, gamma, out, ws, ws_bytes, None)


DEFECTS = [dict(x=None), dict(y=None), dict(out=None), dict(ws=None), dict(ox=None), dict(oy=None), dict(d=0), dict(ld_x=60),
           dict(ld_y=32), dict(ld_x=66), dict(ld_y=70), dict(x="misaligned"), dict(y="misaligned"), dict(rows_x=-1), dict(ng=-1),
           dict(ox=(0, 120, 100)), dict(oy=(-1, 50, 150)), dict(ox=(0, 100, 201)), dict(oy=(0, 50, 151)), dict(ix="index", nix=199),
           dict(iy="index", niy=149), dict(ws="misaligned"), dict(ws_bytes=0), dict(ws_bytes="one short"),
           dict(gamma=float("nan")), dict(gamma=-1e-300), dict(gamma=-1.0), dict(gamma=float("inf")), dict(gamma=float("-inf"))]


def check_rejections(lib, status_bad, status_ok, X, Y, IX, OUT, WS):
    """Every call has exactly one defect and must come back TISE_ERR_INVALID_ARG before any HIP call (shared with the GPU test,
    which passes real device addresses: a defect that slipped through would launch there)."""
    keep = []
    base = dict(x=X, rows_x=200, ld_x=64, ix=None, nix=0, ox=(0, 100, 200), y=Y, rows_y=150, ld_y=68, iy=None, niy=0, oy=(0, 50, 150),
                ng=2, d=64, gamma=1 / 200, out=OUT, ws=WS, ws_bytes=1 << 20)
    nb = ctypes.c_size_t()
    assert lib.tise_mmd_rbf_workspace_bytes(_offs(0, 100, 200)[1], _offs(0, 50, 150)[1], 2, ctypes.byref(nb)) == status_ok
    assert nb.value == 512 + 8 * 16 + 8 * (200 + 150)
    assert rbf_call(lib, keep, **{**base, "ng": 0, "ox": (0,), "oy": (0,)}) == status_ok          # no groups: accepted, no launch
    assert rbf_call(lib, keep, **{**base, "ng": 0, "ox": (0,), "oy": (0,), "gamma": -1.0}) == status_bad
    for kw in DEFECTS:
        kw = dict(kw)
        for k, v in kw.items():
            if v == "misaligned":
                kw[k] = base[k] + 4
            elif v == "index":
                kw[k] = IX
            elif v == "one short":
                kw[k] = nb.value - 1
        assert rbf_call(lib, keep, **{**base, **kw}) == status_bad, kw


def test_grouped_entry_rejects_every_single_defect_without_a_gpu():
    from tise_toolbox_amd import _lib
    check_rejections(_lib.load(), _lib.TISE_ERR_INVALID_ARG, _lib.TISE_OK, 0x7f0000000000, 0x7f0000100000, 0x7f0000200000,
                     0x7f0000400000, 0x7f0000500000)


def test_gaussian_mmd_refuses_a_host_device_and_a_bad_gamma():
    from tise_toolbox_amd import _lib, device
    with pytest.raises(_lib.TiseLibraryError, match="GaussianMMD needs a HIP device"):
        device.GaussianMMD("cpu", 0.005)
    for g in (None, float("nan"), -0.5, float("inf")):
        with pytest.raises(ValueError):
            device.GaussianMMD("cuda", g)


# ---- the gathered-row tile's width sweep and the non-finite rule: the oracle's side, checked without a GPU ----------------------
def test_recorded_spread_covers_the_width_sweep():
    from tests import test_gpu_cmmd
    worst = test_gpu_cmmd.measure_spread(test_gpu_cmmd.sweep_cases())
    assert list(worst) == ["the rest"] and worst["the rest"][1] <= test_gpu_cmmd.REL_SPREAD
    assert test_gpu_cmmd.REL_TOL == 8 * test_gpu_cmmd.REL_SPREAD


def test_reference_sums_at_gamma_zero_count_the_pairs():
    from tests import _rows_tile_cases as tc
    want = tc.census_expected()
    for g, (n, m) in enumerate(zip(tc.CENSUS_SIZES_X, tc.CENSUS_SIZES_Y)):
        assert list(_cmmd_ref.rbf_sums(tc.pool3_like(n, 3, 1), tc.pool3_like(m, 3, 2), 0.0)) == list(want[g])


@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
def test_reference_is_nan_for_a_non_finite_row_and_only_where_the_row_enters(value):
    """numpy's semantics (np.maximum keeps a NaN where fmax drops it), which the kernel has to match; the textbook forms on full
    kernel matrices -- the published implementation's arithmetic -- return NaN as well."""
    from tests import _rows_tile_cases as tc
    X, Y = tc.mmd_rows(67, "unit")
    sums = lambda xs, ys: _cmmd_ref.rbf_sums(xs, ys, 1 / 200)
    clean = tc.group_sums(sums, X, Y)
    for side, g, pos in tc.mmd_bad_rows():
        row = int((tc.MMD_OX if side == "x" else tc.MMD_OY)[g]) + pos
        Xb = tc.with_bad_row(X, row, value) if side == "x" else X
        Yb = tc.with_bad_row(Y, row, value) if side == "y" else Y
        with np.errstate(invalid="ignore"):
            got = tc.group_sums(sums, Xb, Yb)
        hit = np.zeros(clean.shape, bool)
        hit[g, [0, 2] if side == "x" else [1, 2]] = True
        assert not np.any(np.isfinite(got[hit])) and got[~hit].tobytes() == clean[~hit].tobytes(), (side, g, pos)
        with np.errstate(invalid="ignore"):
            assert np.isnan(_cmmd_ref.cmmd_v(Xb, Yb)) and np.isnan(_cmmd_ref.cmmd_u(Xb, Yb))


def test_an_all_zero_row_becomes_nan_in_normalize_rows_and_in_the_value():
    import torch
    from tise_toolbox_amd import cmmd
    x = torch.ones((3, 4))
    x[1] = 0
    n = cmmd.normalize_rows(x)
    assert bool(torch.isnan(n[1]).all()) and bool(torch.isfinite(n[[0, 2]]).all())
    assert np.isnan(cmmd.cmmd_from_sums((float("nan"), 1.0, float("nan")), 3, 3))
