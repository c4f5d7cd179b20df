"""CPU: what the nearest-row search, AuthPct, Vendi and FD-infinity promise without a GPU -- the margins of the float cases (from
the reference alone), the reference's own known answers, the host halves of the new modules, the parser and the refusals."""
import numpy as np
import pytest

from tests import _nn_cases as cases
from tests import _nn_ref


@pytest.mark.parametrize("shape", cases.SHAPES, ids=cases.shape_id)
def test_every_decision_of_a_float_case_has_a_margin(shape):
    """Best against second-best d2 in both passes and the authenticity comparison itself: a relative gap of MIN_MARGIN is six
    orders of magnitude above the arithmetic's error, so idx and the authentic flags must EQUAL the reference's, no case excluded."""
    Q, B, ref = cases.float_case(*shape)
    margin = cases.smallest_margin(ref)
    print(f"{shape}: smallest relative gap of a decision {margin:.3e}")
    assert margin >= cases.MIN_MARGIN
    assert ref["idx"].min() >= 0 and np.all(np.isfinite(ref["d2"])) and np.all(ref["d2"] > 0)
    if shape[1] >= 2:
        share = ref["auth"]["authentic"].mean()
        print(f"{shape}: authentic share {share:.3f}")
        if shape[0] >= 60:                                             # both outcomes of the comparison occur, and often (one
            assert 0.30 <= share <= 0.90                               # and six query rows give 0 and 1: too few for a share)


def test_the_integer_cases_hold_the_ties_they_are_for():
    Q, B, cross, own = cases.integer_case(0)
    d2, idx = cases.exact_nearest(cross)
    assert d2[3] == 0 and idx[3] == 5 and d2[71] == 1 and idx[71] == 5 and d2[10] == 0 and idx[10] == 100
    for row in (3, 71):                                                 # the minimum is attained at all seven copies, in every tile
        assert set(np.flatnonzero(cross[row] == d2[row])) == set(cases.DUPLICATES_0)
    assert {j // 64 for j in cases.DUPLICATES_0} == {0, 1, 2, 3}
    d2s, idxs = cases.exact_nearest(own, exclude_diagonal=True)
    assert idxs[5] == 6 and idxs[6] == 5 and idxs[199] == 5 and idxs[100] == 150 and idxs[150] == 100 and d2s[5] == 0
    # the float64 reference reproduces the int64 values exactly, ties included
    got = _nn_ref.nearest(Q, B)
    assert np.array_equal(got[0], d2.astype(np.float64)) and np.array_equal(got[1], idx)
    Q, B, cross, own = cases.integer_case(1)
    d2, idx = cases.exact_nearest(cross)
    tied = (cross == d2[:, None]).sum(axis=1)
    tiles = [len({j // 64 for j in np.flatnonzero(cross[i] == d2[i])}) for i in range(len(cross))]
    print(f"integer case 1: rows whose minimum is attained more than once: {(tied > 1).sum()} of {len(tied)}; in more than one tile: {sum(t > 1 for t in tiles)}")
    assert (tied > 1).sum() >= len(tied) // 4 and sum(t > 1 for t in tiles) >= 5


def test_the_reference_search_on_known_answers():
    B = np.array([[0, 0], [3, 0], [0, 4], [3, 0]], dtype=np.float32)
    Q = np.array([[3, 0], [0, 3], [10, 10]], dtype=np.float32)
    d2, idx, _ = _nn_ref.nearest(Q, B)
    assert d2.tolist() == [0.0, 1.0, 136.0] and idx.tolist() == [1, 2, 2]                  # the tie 1 / 3 goes to the smaller index
    d2, idx, _ = _nn_ref.nearest(B, B, exclude_diagonal=True)
    assert d2.tolist() == [9.0, 0.0, 16.0, 0.0] and idx.tolist() == [1, 3, 0, 1]
    # non-finite rows: a NaN base row is nobody's nearest, a NaN query row gets (NaN, -1), no candidate gives (+inf, -1)
    Bn = B.copy()
    Bn[1, 0] = np.nan
    d2, idx, _ = _nn_ref.nearest(Q, Bn)
    assert d2.tolist() == [0.0, 1.0, 136.0] and idx.tolist() == [3, 2, 2]
    Qn = Q.copy()
    Qn[2, 1] = np.inf
    d2, idx, _ = _nn_ref.nearest(Qn, B)
    assert np.isnan(d2[2]) and idx.tolist() == [1, 2, -1]
    d2, idx, _ = _nn_ref.nearest(B[:1], B[:1], exclude_diagonal=True)
    assert d2.tolist() == [np.inf] and idx.tolist() == [-1]
    # authenticity: a copy of a training row is not authentic; a sample far from everything is
    a = _nn_ref.authentic(B[:3], np.array([[3, 0], [100, 100]], dtype=np.float32))
    assert a["authentic"].tolist() == [False, True] and a["authpct"] == 50.0


def test_vendi_host_half_and_reference_known_answers():
    from tise_toolbox_amd import vendi
    for fn in (vendi.vendi_from_eigenvalues, _nn_ref.vendi_from_eigenvalues):
        assert fn([1.0, 0.0, -1e-18]) == 1.0
        assert abs(fn([0.25] * 4) - 4.0) < 1e-12 and abs(fn([0.25] * 4, q=2.0) - 4.0) < 1e-12 and abs(fn([0.25] * 4, q=np.inf) - 4.0) < 1e-12
        assert abs(fn([0.5, 0.25, 0.25], q=np.inf) - 2.0) < 1e-12
        assert abs(fn([0.5, 0.25, 0.25]) - np.exp(1.5 * np.log(2.0))) < 1e-12
        assert abs(fn([0.5, 0.25, 0.25], q=2.0) - 1 / 0.375) < 1e-12
        assert abs(fn([0.5, 0.25, 0.25], q=0.0) - 3.0) < 1e-12
    with pytest.raises(ValueError, match="order q"):
        vendi.vendi_from_eigenvalues([1.0], q=-1)
    with pytest.raises(ValueError, match="no positive eigenvalue"):
        vendi.vendi_from_eigenvalues([0.0, -1.0])
    assert vendi.gram_route(40, 64) == "rows" and vendi.gram_route(200, 64) == "cols" and vendi.gram_route(64, 64) == "rows"
    assert vendi.gram_route(200, 64, "rows") == "rows"
    with pytest.raises(ValueError, match="route"):
        vendi.gram_route(4, 4, "both")
    with pytest.raises(ValueError, match="order q"):
        vendi.vendi_from_features(np.ones((4, 4), np.float32), q=float("nan"))
    with pytest.raises(ValueError, match=r"\(rows, dims\)"):
        vendi.vendi_from_features(np.ones(4, np.float32))
    # the reference: n rows spread evenly over m orthogonal axes give m, identical rows give 1, and the two routes agree
    X = np.zeros((12, 7), np.float32)
    X[np.arange(12), np.arange(12) % 3] = np.arange(1, 13)
    for route in ("rows", "cols"):
        assert abs(_nn_ref.vendi(X, route=route) - 3.0) < 1e-6
        assert abs(_nn_ref.vendi(np.tile(cases.vendi_rows(40, 64)[:1], (9, 1)), route=route) - 1.0) < 1e-6
    for n, d in cases.VENDI_SHAPES:
        a, b = _nn_ref.vendi(cases.vendi_rows(n, d), route="rows"), _nn_ref.vendi(cases.vendi_rows(n, d), route="cols")
        print(f"({n}, {d}): numpy Vendi, n x n route {a!r}, d x d route {b!r}, relative gap {abs(a - b) / a:.3e}")
        assert 1.5 < a < min(n, d) and abs(a - b) / a < 1e-9


def test_fd_infinity_host_half():
    from tise_toolbox_amd import fd_infinity
    for m in cases.FDINF_M:
        got = fd_infinity.fd_infinity_sizes(m)
        want = np.linspace(min(5000, max(m // 10, 2)), m, 15).astype(np.int32)
        assert got.dtype == np.int32 and np.array_equal(got, want) and np.array_equal(got, _nn_ref.fd_infinity_sizes(m))
        assert got[0] == {20: 2, 400: 40, 60000: 5000}[m] and got[-1] == m and np.all(np.diff(got) > 0)
    assert len(fd_infinity.fd_infinity_sizes(400, 4)) == 4
    a, b = fd_infinity.fd_infinity_subsets(400, 15, 3), fd_infinity.fd_infinity_subsets(400, 15, 3)
    assert [len(s) for s in a] == fd_infinity.fd_infinity_sizes(400).tolist()
    assert all(np.array_equal(x, y) for x, y in zip(a, b))                                # reproducible from the seed
    assert not all(np.array_equal(x, y) for x, y in zip(a, fd_infinity.fd_infinity_subsets(400, 15, 4)))
    for s in a:
        assert s.dtype == np.int64 and len(np.unique(s)) == len(s) and s.min() >= 0 and s.max() < 400      # without replacement
    assert sorted(a[-1].tolist()) == list(range(400))
    # the line: y = 2 + 30 / N exactly -> intercept 2; against np.polyfit on noisy values
    sizes = fd_infinity.fd_infinity_sizes(60000)
    assert abs(fd_infinity.fit_intercept(sizes, 2.0 + 30.0 / sizes) - 2.0) < 1e-12
    y = 2.0 + 30.0 / sizes + np.random.default_rng(0).standard_normal(15) * 1e-3
    assert abs(fd_infinity.fit_intercept(sizes, y) - np.polyfit(1.0 / sizes, y, 1)[1]) < 1e-12
    for bad in (dict(m=1), dict(m=0), dict(m=100, num_points=1)):
        with pytest.raises(ValueError):
            fd_infinity.fd_infinity_sizes(**bad)
    R = np.ones((4, 3), np.float32)
    with pytest.raises(ValueError, match="widths differ"):
        fd_infinity.fd_infinity_from_features(R, np.ones((4, 5), np.float32))
    with pytest.raises(ValueError, match="at least 2 reference rows"):
        fd_infinity.fd_infinity_from_features(R[:1], R)
    with pytest.raises(ValueError, match="one subset size only"):
        fd_infinity.fd_infinity_from_features(R, R[:2])


def test_authenticity_refusals_that_need_no_gpu():
    from tise_toolbox_amd import authenticity
    T = np.ones((5, 8), np.float32)
    for fn in (authenticity.authpct_from_features, authenticity.nearest_train):
        with pytest.raises(ValueError, match="at least 2"):
            fn(T[:1], T)
        with pytest.raises(ValueError, match="widths differ: 8 and 6"):
            fn(T, T[:, :6])
        with pytest.raises(ValueError, match=r"\(rows, dims\)"):
            fn(T, T[0])
        with pytest.raises(ValueError, match="no rows"):
            fn(T, T[:0])
    with pytest.raises(ValueError, match=r"the generated side has 2 feature rows with a NaN or an infinity \(the first is row 7\)"):
        authenticity.refuse_nonfinite_rows((("training", 0, 9), ("generated", 2, 7)))
    authenticity.refuse_nonfinite_rows((("training", 0, 9), ("generated", 0, 4)))
    assert authenticity.authpct_from_counts(3, 4) == 75.0


def test_parser_and_cli_refusals(tmp_path):
    from tise_toolbox_amd import fd_dinov2
    base = ["--path1", "a", "--path2", "b"]
    args = fd_dinov2.parse_args(base)
    assert (args.train, args.authpct, args.nearest_train, args.vendi, args.fd_infinity, args.fd_infinity_seed) == ("", False, "", False, False, 0)
    args = fd_dinov2.parse_args(base + ["--train", "t", "--authpct", "--nearest-train", "o.csv", "--vendi", "--fd-infinity", "--fd-infinity-seed", "5"])
    assert (args.train, args.authpct, args.nearest_train, args.vendi, args.fd_infinity, args.fd_infinity_seed) == ("t", True, "o.csv", True, True, 5)
    for extra in (["--authpct"], ["--nearest-train", "o.csv"]):
        with pytest.raises(SystemExit):                                  # refused by the parser: before any GPU work
            fd_dinov2.parse_args(base + extra)
        with pytest.raises(SystemExit):
            fd_dinov2.main(base + extra)
    with pytest.raises(ValueError, match="need the training set"):
        fd_dinov2.calculate_fd_dinov2_given_paths([str(tmp_path), str(tmp_path)], authpct=True)
    with pytest.raises(RuntimeError, match="Invalid path"):
        fd_dinov2.calculate_fd_dinov2_given_paths([str(tmp_path), str(tmp_path)], authpct=True, train=str(tmp_path / "none"))
    # the result lines: the old ones are what they were, the new ones follow them, each only when its key is there
    res = dict(fd=1.5, kd=None, prdc=None)
    assert fd_dinov2.result_lines(res, "vitl14") == ["FD-DINOv2 (vitl14): 1.5"]
    res.update(authpct=62.5, vendi=3.25, vendi_reference=4.5, fd_infinity=dict(fd_infinity=1.25))
    assert fd_dinov2.result_lines(res, "vits14", " [x]") == [
        "FD-DINOv2 (vits14): 1.5 [x]", "AuthPct-DINOv2 (vits14): 62.5 [x]", "Vendi-DINOv2 (vits14): 3.25 [x]",
        "Vendi-DINOv2 reference (vits14): 4.5 [x]", "FD-infinity-DINOv2 (vits14): 1.25 [x]"]
