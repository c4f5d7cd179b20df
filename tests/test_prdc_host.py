"""CPU: the host side of precision / recall / density / coverage -- C ABI declarations, argument checks and the workspace formula
of tise_knn_* / tise_prdc_counts, the numpy reference against its extended-precision restatement and against sklearn, the
--prdc flags, and the refusal to run without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import _prdc_cases as cases
from tests import _prdc_ref
from tests import _rows_tile_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tise_knn_workspace_bytes", "tise_knn_radius2", "tise_prdc_counts")
VALUES = ("precision", "recall", "density", "coverage")


def test_header_signatures_and_sources_declare_the_new_pieces():
    from tise_toolbox_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tise_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tise_[a-z0-9_]+)\s*\(", text))
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES, name
    assert "knn.hip" in build.SOURCES
    build.build(force=False, verbose=False)
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name)
    assert "tise_knn_radius2" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


X, F, R2, R2F, OUT, CNT, REC, PREC, WS = (0x7f0000000000 + i * 0x10000000 for i in range(9))


def test_every_single_defect_is_refused_without_a_gpu():
    """Fake aligned device addresses; every call has exactly one defect and must come back TISE_ERR_INVALID_ARG or
    TISE_ERR_UNSUPPORTED before any HIP call (a launch would need a device this test does not have)."""
    from tise_toolbox_amd import _lib
    lib = _lib.load()
    refused = (_lib.TISE_ERR_INVALID_ARG, _lib.TISE_ERR_UNSUPPORTED)

    def radius2(x=X, rows=200, ld=68, d=64, k=5, splits=0, out=OUT, ws=WS, ws_bytes=1 << 30):
        return lib.tise_knn_radius2(x, rows, ld, d, k, splits, out, ws, ws_bytes, None)

    def counts(r=X, rows_r=200, ld_r=68, r2r=R2, f=F, rows_f=150, ld_f=64, r2f=R2F, d=64, splits=0, cnt=CNT, rec=REC, prec=PREC,
               ws=WS, ws_bytes=1 << 30):
        return lib.tise_prdc_counts(r, rows_r, ld_r, r2r, f, rows_f, ld_f, r2f, d, splits, cnt, rec, prec, ws, ws_bytes, None)

    nb = ctypes.c_size_t()
    assert lib.tise_knn_workspace_bytes(200, 5, 0, ctypes.byref(nb)) == _lib.TISE_OK
    for kw in (dict(k=0), dict(k=17), dict(rows=5), dict(k=16, rows=16), dict(ld=60), dict(ld=66), dict(x=X + 8), dict(x=None),
               dict(out=None), dict(ws=None), dict(ws_bytes=nb.value - 1), dict(d=0), dict(splits=-1), dict(splits=1025),
               dict(rows=(1 << 24) + 1)):
        assert radius2(**kw) in refused, kw
    for kw in (dict(ld_r=60), dict(ld_f=32), dict(ld_r=66), dict(ld_f=70), dict(r=X + 8), dict(f=F + 8), dict(r=None), dict(f=None),
               dict(r2r=None), dict(r2f=None), dict(cnt=None), dict(rec=None), dict(prec=None), dict(ws=None),
               dict(ws_bytes=8 * 350 - 1), dict(rows_r=0), dict(rows_f=0), dict(d=0), dict(splits=-1), dict(rows_f=(1 << 24) + 1)):
        assert counts(**kw) in refused, kw
    for kw in (dict(k=0), dict(k=17), dict(rows=5), dict(splits=-1), dict(rows=(1 << 24) + 1)):
        a = dict(rows=200, k=5, splits=0)
        a.update(kw)
        assert lib.tise_knn_workspace_bytes(a["rows"], a["k"], a["splits"], ctypes.byref(nb)) in refused, kw
    assert lib.tise_knn_workspace_bytes(200, 5, 0, None) in refused


def test_workspace_bytes_equal_the_documented_formula():
    """8 * rows * (S * k + 1): k candidates per row and split, and the norms.  S = col_splits, or ceil(1024 / row tiles) for 0;
    either capped at the number of column tiles."""
    from tise_toolbox_amd import _lib
    lib = _lib.load()
    nb = ctypes.c_size_t()
    for rows, k, splits, S in ((30000, 5, 0, 3), (1000, 3, 0, 16), (1000, 3, 7, 7), (130, 16, 7, 3), (6, 5, 0, 1)):
        tiles = (rows + 63) // 64
        assert S == min(splits or -(-1024 // tiles), tiles)
        assert lib.tise_knn_workspace_bytes(rows, k, splits, ctypes.byref(nb)) == _lib.TISE_OK
        assert nb.value == 8 * rows * (S * k + 1), (rows, k, splits)


@pytest.mark.parametrize("shape", [s for s in cases.COUNT_SHAPES if s[0] <= 300], ids=lambda s: "n%d-m%d-d%d-k%d" % s[:4])
def test_reference_agrees_with_its_longdouble_restatement(shape):
    R, F, ref = cases.count_case(*shape)
    direct = _prdc_ref.prdc_direct(R, F, shape[3])
    for name in ("cnt", "rec", "prec"):
        assert np.array_equal(ref[name], direct[name]), name
    assert [ref[v] for v in VALUES] == [direct[v] for v in VALUES]
    assert _prdc_ref.smallest_margin(ref) >= cases.MIN_MARGIN
    for name in ("r2_real", "r2_fake"):
        assert np.max(np.abs(ref[name] - direct[name].astype(np.float64)) / ref[name]) <= 1e-13


def test_integer_cases_are_exact_and_hold_ties():
    for which in (0, 1):
        R, F, k, ref = cases.integer_case(which)
        direct = _prdc_ref.prdc_direct(R, F, k)
        for name in ("cnt", "rec", "prec", "r2_real", "r2_fake", "cross"):
            assert np.array_equal(ref[name], direct[name]), (which, name)
        assert np.sum(ref["cross"] == ref["r2_real"][:, None]) > 0 and np.sum(ref["cross"] == ref["r2_fake"][None, :]) > 0


def test_reference_equals_the_prdc_package_restated_on_sklearn():
    """prdc.compute_prdc (Naeem et al.), restated line by line on sklearn's pairwise_distances."""
    metrics = pytest.importorskip("sklearn.metrics")
    R, F, ref = cases.count_case(*cases.COUNT_SHAPES[0])
    k = cases.COUNT_SHAPES[0][3]
    R64, F64 = R.astype(np.float64), F.astype(np.float64)

    def kth_values(x):
        return np.sort(metrics.pairwise_distances(x, x, metric="euclidean"), axis=-1)[:, k]
    real_radii, fake_radii = kth_values(R64), kth_values(F64)
    dist = metrics.pairwise_distances(R64, F64, metric="euclidean")
    precision = (dist < real_radii[:, None]).any(axis=0).mean()
    recall = (dist < fake_radii[None, :]).any(axis=1).mean()
    density = (1.0 / float(k)) * (dist < real_radii[:, None]).sum(axis=0).mean()
    coverage = (dist.min(axis=1) < real_radii).mean()
    got = [ref[v] for v in VALUES]
    assert np.allclose(got, [precision, recall, density, coverage], rtol=1e-12, atol=0), (got, precision, recall, density, coverage)
    assert got[0] == precision and got[1] == recall and got[3] == coverage     # means of the same booleans over the same counts


def test_prdc_flags_parse_with_their_defaults_and_per_class_is_refused(capsys):
    from tise_toolbox_amd import fid_score
    p = fid_score._build_parser()
    a = p.parse_args(["--path2", "x"])
    assert (a.prdc, a.prdc_k, a.prdc_saved_file) == (False, 5, "")
    a = p.parse_args(["--path2", "x", "--prdc", "--prdc-k", "3", "--prdc-saved-file", "p.txt"])
    assert (a.prdc, a.prdc_k, a.prdc_saved_file) == (True, 3, "p.txt")
    assert "3" in [act for act in p._actions if act.dest == "prdc_k"][0].help
    with pytest.raises(SystemExit) as e:
        fid_score.main(["--path1", "a", "--path2", "b", "--per-class", "--prdc", "--synthetic-weights"])
    assert e.value.code == 2 and "--per-class --prdc" in capsys.readouterr().err


def test_feature_file_rule_names_the_flag(tmp_path):
    from tise_toolbox_amd import fid_score
    plain, full = str(tmp_path / "plain.npz"), str(tmp_path / "full.npz")
    fid_score.save_stats_npz(plain, np.zeros(4), np.eye(4))
    fid_score.save_stats_npz(full, np.zeros(4), np.eye(4), "torchvision", np.ones((7, 4)))
    with pytest.raises(RuntimeError, match=r"plain\.npz.*--prdc needs the feature rows"):
        fid_score.calculate_prdc_given_paths([plain, full], 8, True, 4)
    with pytest.raises(RuntimeError, match=r"plain\.npz.*--prdc needs the feature rows"):
        fid_score.main(["--path1", full, "--path2", plain, "--prdc", "--synthetic-weights"])


def test_prdc_from_features_checks_its_arguments_and_has_no_cpu_path():
    import torch
    from tise_toolbox_amd import _lib, prdc
    x, y = cases.pool3_like(20, 8, 1), cases.pool3_like(12, 8, 2)
    with pytest.raises(ValueError, match="widths"):
        prdc.prdc_from_features(x, y[:, :6])
    with pytest.raises(ValueError, match="at least 6"):
        prdc.prdc_from_features(x, y[:5])
    with pytest.raises(ValueError):
        prdc.prdc_from_features(x, y, 17)
    if not torch.cuda.is_available():
        with pytest.raises(_lib.TiseLibraryError):
            prdc.prdc_from_features(x, y)


# ---- the gathered-row tile's width sweep and the non-finite rule: what the GPU tests rely on, checked without a GPU -------------
@pytest.mark.parametrize("d", tc.WIDTHS)
def test_width_sweep_inputs_have_the_properties_the_gpu_test_relies_on(d):
    """Integer widths: the reference is exact (it equals its longdouble restatement) and meets exact ties d2 == r2 on both sides.
    Float widths: the seeds give every decision MIN_MARGIN, and the fp64 r2 lies within the recorded spread of the longdouble one."""
    from tests import test_gpu_prdc
    R, F = tc.prdc_rows(d)
    assert R.shape == (70, d) and F.shape == (65, d) and R.dtype == np.float32
    for k in tc.PRDC_K:
        tc.check_prdc_case_properties(d, k)
        ref, direct = tc.prdc_reference(d, k), _prdc_ref.prdc_direct(R, F, k)
        for name in ("cnt", "rec", "prec"):
            assert np.array_equal(ref[name], direct[name]), (d, k, name)
        if tc.prdc_is_exact(d):
            assert np.all(np.abs(R) <= 4) and np.array_equal(R, np.round(R))
            for name in ("r2_real", "r2_fake", "cross"):
                assert np.array_equal(ref[name], direct[name]), (d, k, name)
        else:
            for name in ("r2_real", "r2_fake"):
                assert np.max(np.abs(ref[name] - direct[name]) / direct[name]) <= test_gpu_prdc.REL_SPREAD, (d, k, name)


def test_recorded_spread_covers_the_width_sweep(capsys):
    from tests import test_gpu_prdc
    assert test_gpu_prdc.measure_sweep_spread() <= test_gpu_prdc.REL_SPREAD
    assert test_gpu_prdc.REL_TOL == 8 * test_gpu_prdc.REL_SPREAD


@pytest.mark.parametrize("d", [7, 67])
def test_reference_rule_for_non_finite_rows(d):
    """prdc_dropping_nonfinite states the kernels' rule through the clean definition.  For a NaN, plain numpy on the dirty input
    says the same (np.maximum keeps a NaN, np.sort puts it last, comparisons with it are False); for an infinity it does not
    (inf - inf and inf + inf mix), which is why the rule is stated by dropping the rows."""
    R, F = tc.prdc_rows(d)
    for k in tc.PRDC_K:
        clean = tc.prdc_reference(d, k)
        for side, row in tc.prdc_bad_rows():
            for value in tc.BAD_VALUES:
                Rb = tc.with_bad_row(R, row, value) if side == "real" else R
                Fb = tc.with_bad_row(F, row, value) if side == "fake" else F
                assert list(_prdc_ref.nonfinite_rows(Rb)) == ([row] if side == "real" else [])
                assert list(_prdc_ref.nonfinite_rows(Fb)) == ([row] if side == "fake" else [])
                ref = _prdc_ref.prdc_dropping_nonfinite(Rb, Fb, k)
                mine = "r2_real" if side == "real" else "r2_fake"
                assert np.isnan(ref[mine][row]) and int(np.isnan(ref["r2_real"]).sum() + np.isnan(ref["r2_fake"]).sum()) == 1
                if side == "real":
                    assert ref["cnt"][row] == 0 and not ref["rec"][row]
                    assert np.array_equal(ref["prec"], ref["clean"]["prec"]) and len(ref["clean"]["cnt"]) == len(R) - 1
                    assert np.array_equal(ref["r2_fake"], clean["r2_fake"])        # the other side's radii do not move
                else:
                    assert not ref["prec"][row] and np.array_equal(ref["cnt"], ref["clean"]["cnt"])
                    assert np.array_equal(ref["r2_real"], clean["r2_real"])
                if np.isnan(value):
                    with np.errstate(invalid="ignore"):
                        plain = _prdc_ref.prdc(Rb, Fb, k)
                    for name in ("cnt", "rec", "prec"):
                        assert np.array_equal(plain[name], ref[name]), (d, k, side, row, name)
                    for name in ("r2_real", "r2_fake"):
                        assert np.array_equal(plain[name], ref[name], equal_nan=True), (d, k, side, row, name)
    # what fmax(0, NaN) = 0 did: the NaN row of the generated side sits at distance 0 from every row, inside every ball of
    # positive radius -- one more hit for every real row (so coverage is exactly 1), and the row itself counts as precise
    Fb = tc.with_bad_row(F, 0, float("nan"))
    with np.errstate(invalid="ignore"):
        wrong = _prdc_ref.prdc(R, Fb, 5, d2=lambda a, b: np.fmax(0.0, _prdc_ref.d2_expansion(a, b)))
    right = _prdc_ref.prdc_dropping_nonfinite(R, Fb, 5)
    assert np.all(right["r2_real"] > 0) and np.array_equal(wrong["cnt"], right["cnt"] + 1) and wrong["coverage"] == 1.0
    assert wrong["prec"][0] and not right["prec"][0] and wrong["r2_fake"][0] == 0


def test_refusal_of_non_finite_rows_names_side_count_and_first_row():
    """The host half of prdc_from_features' refusal (the device half -- NaN radii counted into its one host copy -- is in
    tests/test_gpu_prdc.py): nothing for clean sides, else ValueError for the first side that has such rows."""
    from tise_toolbox_amd import prdc
    assert prdc.refuse_nonfinite_rows((("real", 0, 70), ("fake", 0, 65))) is None
    with pytest.raises(ValueError, match=r"the real side has 2 feature rows with a NaN or an infinity \(the first is row 12\)"):
        prdc.refuse_nonfinite_rows((("real", 2, 12), ("fake", 0, 65)))
    with pytest.raises(ValueError, match=r"the fake side has 1 feature row with a NaN or an infinity \(the first is row 64\)"):
        prdc.refuse_nonfinite_rows((("real", 0, 70), ("fake", 1, 64)))
    with pytest.raises(ValueError, match=r"the real side has 1 feature row .*row 0\)"):
        prdc.refuse_nonfinite_rows((("real", 1, 0), ("fake", 1, 3)))
