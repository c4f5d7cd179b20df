"""GPU: AuthPct (authenticity.py), the Vendi score (vendi.py) and FD-infinity (fd_infinity.py) against tests/_nn_ref.py, and
fd_dinov2's new flags end to end.

AuthPct is a count: tests/test_nn_host.py asserts from the reference alone that every decision of every float case -- nearest
against second-nearest row, and d2_train[j*] against d2_gen -- has a relative margin of 1e-9, so idx, the flags and the
percentage must EQUAL the reference's.

VENDI's bound.  delta = the relative gap between numpy's own two routes to the same number (eigvalsh of the n x n and of the d x d
Gram matrix, both LAPACK, both fp64): what two correct fp64 evaluations differ by.  The device value is held within
max(4 delta, the bisection bound) of either.  The bisection bound: tise_eigvalsh returns every eigenvalue of a matrix of norm
|G| <= 1 (the trace is 1) within K eps |G| absolutely, eps = 2^-52, with K = 64 k covering the tridiagonalisation's backward
error (a modest multiple of k eps |G|) and the bisection's final interval; an absolute error e in each of k eigenvalues moves the
entropy H = -sum l ln l by at most k e (1 + |ln e|) (the derivative -(1 + ln l) is largest where l is smallest, and a
perturbation of size e of an eigenvalue below e contributes at most e |ln e|), and the score exp(H) relatively by the same:
    bound = k * (64 k eps) * (1 + |ln(64 k eps)|),        k = the size of the route's Gram matrix (n, d, or the smaller).
The reference's two routes start from the unit rows the product itself forms in fp32 (cmmd.normalize_rows; held against numpy's
fp32 normalisation to 2 ulps): with numpy's own unit rows the score differs by 1.3e-9 to 2.3e-9 -- the last fp32 bit of the
norms, a difference of the input, not of the eigenvalue routine.  Measured gaps are printed; the README quotes them.

Figures of the first run on an MI355X: Vendi, device against numpy 8.0e-15 / 2.9e-14 .. 3.0e-14 / 3.8e-14 .. 7.5e-14 relative at
(40, 64) / (200, 64) / (100, 1024) with delta 8.0e-15 / 2.8e-14 / 7.0e-14 (bounds 6.6e-10 .. 3.9e-7); FD_N against the oracle at
most 2.1e-8 apart, FD-infinity 0.22120297734 against the oracle's line 0.22120297369."""
import csv
import os

import numpy as np
import pytest

from tests import _nn_cases as cases
from tests import _nn_ref

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52


def bisection_bound(k):
    e = 64 * k * EPS
    return k * e * (1 + abs(np.log(e)))


@pytest.mark.parametrize("shape", [s for s in cases.SHAPES if s[1] >= 2], ids=cases.shape_id)
def test_authpct_equals_the_reference_exactly(cuda_device, shape):
    """The base rows are the training side, the query rows the generated side."""
    import torch
    from tise_toolbox_amd import authenticity
    Q, B, ref = cases.float_case(*shape)
    want = ref["auth"]
    got = authenticity.nearest_train(B, torch.as_tensor(Q, device=cuda_device))
    assert got["idx"].dtype == np.int32 and got["authentic"].dtype == np.bool_ and got["d2_gen"].dtype == got["d2_train"].dtype == np.float64
    assert got["d2_train"].shape == (shape[1],) and got["d2_gen"].shape == (shape[0],)
    assert np.array_equal(got["idx"], want["idx"]) and np.array_equal(got["authentic"], want["authentic"])
    pct = authenticity.authpct_from_features(B, Q)
    print(f"{shape}: AuthPct {pct!r} (reference {want['authpct']!r})")
    assert type(pct) is float and pct == want["authpct"]


def test_authpct_on_integer_rows_with_exact_ties_and_its_refusals(cuda_device):
    """Query row 3 of integer case 0 IS training row 5, whose own nearest neighbour (a duplicate) is at 0 too: 0 < 0 is false, the
    copy is not authentic.  Every sum is exact, so the whole flag vector equals the int64 evaluation."""
    from tise_toolbox_amd import authenticity
    Q, B, cross, own = cases.integer_case(0)
    d1, j = cases.exact_nearest(cross)
    d2t, _ = cases.exact_nearest(own, exclude_diagonal=True)
    want = d2t[j] < d1
    got = authenticity.nearest_train(B, Q)
    assert np.array_equal(got["idx"], j) and np.array_equal(got["authentic"], want) and not got["authentic"][3]
    assert np.array_equal(got["d2_gen"], d1.astype(np.float64)) and np.array_equal(got["d2_train"], d2t.astype(np.float64))
    assert int((d2t[j] == d1).sum()) >= 1                                 # the strict comparison meets an exact tie
    assert authenticity.authpct_from_features(B, Q) == 100.0 * int(want.sum()) / len(want)
    Qb, Bb = Q.copy(), B.copy()
    Qb[[7, 90], 2] = np.nan
    Bb[150, 0] = np.inf
    with pytest.raises(ValueError, match=r"the generated side has 2 feature rows with a NaN or an infinity \(the first is row 7\)"):
        authenticity.authpct_from_features(B, Qb)
    with pytest.raises(ValueError, match=r"the training side has 1 feature row with a NaN or an infinity \(the first is row 150\)"):
        authenticity.nearest_train(Bb, Qb)


def test_vendi_known_answers(cuda_device):
    """Answers that need no numpy: n rows spread evenly over m orthogonal axes give m; identical rows give 1; the eigenvalues
    sum to 1 (the trace of the Gram matrix of unit rows, / n) -- within 2 (d / 2 + 2) 2^-24, the fp32 normalisation's worst-case
    error in a squared row norm."""
    from tise_toolbox_amd import vendi
    for n, d, m in ((12, 7, 3), (96, 40, 8), (30, 200, 5)):
        X = np.zeros((n, d), np.float32)
        X[np.arange(n), (np.arange(n) % m) * (d // m)] = 1.0 + np.arange(n) % 4                   # lengths differ, directions do not
        for route in ("rows", "cols", None):
            for q in (1.0, 2.0, float("inf")):
                v = vendi.vendi_from_features(X, q, route)
                assert type(v) is float and abs(v - m) <= 1e-9 * m, (n, d, m, route, q, v)
    row = cases.vendi_rows(40, 64)[:1]
    for route in ("rows", "cols"):
        v = vendi.vendi_from_features(np.tile(row, (50, 1)), route=route)
        assert abs(v - 1.0) <= 2 * 2 * (64 / 2 + 2) * 2.0 ** -24, (route, v)     # the one eigenvalue is |u|^2 = 1 + e: exp(-(1 + e) ln(1 + e))
    assert abs(vendi.vendi_from_features(row) - 1.0) <= 2 * 2 * (64 / 2 + 2) * 2.0 ** -24                  # the 1 x 1 Gram matrices
    assert vendi.vendi_from_features(np.ones((5, 1), np.float32)) == 1.0
    for n, d in cases.VENDI_SHAPES:
        for route in ("rows", "cols"):
            lam = vendi.vendi_eigenvalues(cases.vendi_rows(n, d), route)
            assert lam.shape == ((n,) if route == "rows" else (d,))
            assert abs(lam.sum() - 1.0) <= 2 * (d / 2 + 2) * 2.0 ** -24, (n, d, route, lam.sum())
    bad = np.array(cases.vendi_rows(40, 64))
    bad[3] = 0.0
    bad[9, 1] = np.nan
    with pytest.raises(ValueError, match=r"2 feature rows cannot be normalised.*\(the first is row 3\)"):
        vendi.vendi_from_features(bad)


@pytest.mark.parametrize("shape", cases.VENDI_SHAPES, ids=lambda s: "n%d-d%d" % s)
def test_vendi_seeded_cases_on_both_gram_routes(cuda_device, shape):
    import torch
    from tise_toolbox_amd import cmmd, vendi
    n, d = shape
    X = cases.vendi_rows(n, d)
    # the unit rows the product forms (cmmd.normalize_rows, fp32 on the device): numpy's fp32 norm sums in another order, its unit
    # rows differ in the last fp32 bit and the score with them by 1e-9 -- a difference of the INPUT, larger than the bound below.
    # Both routes of the reference therefore start from the device's unit rows, which are held against numpy's to 2 fp32 ulps
    U = cmmd.normalize_rows(torch.as_tensor(X, device=cuda_device)).cpu().numpy()
    assert U.dtype == np.float32 and np.all(np.abs(U - _nn_ref.normalize_rows_f32(X)) <= 2 * np.spacing(np.abs(U)))
    a, b = _nn_ref.vendi(U, route="rows", normalized=True), _nn_ref.vendi(U, route="cols", normalized=True)
    delta = abs(a - b) / a
    print(f"({n}, {d}): numpy n x n {a!r}, d x d {b!r}, delta {delta:.3e}")
    for route in ("rows", "cols", None):
        k = {"rows": n, "cols": d, None: min(n, d)}[route]
        bound = max(4 * delta, bisection_bound(k))
        v = vendi.vendi_from_features(torch.as_tensor(X, device=cuda_device), route=route)
        gap = max(abs(v - a) / a, abs(v - b) / b)
        print(f"({n}, {d}) route {route}: device {v!r}, relative gap to numpy {gap:.3e} (bound {bound:.3e}, {k} x {k} matrix)")
        assert gap <= bound, (route, v, a, b)


def test_fd_infinity_against_the_oracle(cuda_device):
    """(400 + 400 rows, d = 64): every FD_N within the 1e-3 of the project's FID tests of oracle.fid_oracle on the same rows; the
    intercept within 1e-9 of np.polyfit on the device's own FD_N and within 1e-3 of the oracle's line; reproducible from the seed."""
    from oracle import fid_oracle
    from tise_toolbox_amd import fd_infinity
    R, G = cases.fdinf_rows()
    got = fd_infinity.fd_infinity_from_features(R, G, seed=3)
    subsets = fd_infinity.fd_infinity_subsets(len(G), 15, 3)
    assert sorted(got) == ["fd_infinity", "fds", "sizes"] and type(got["fd_infinity"]) is float
    assert np.array_equal(got["sizes"], _nn_ref.fd_infinity_sizes(len(G))) and got["sizes"].dtype == np.int32
    assert got["sizes"].tolist() == [len(s) for s in subsets]
    want, want_fds = _nn_ref.fd_infinity(R, G, subsets, fid_oracle.calculate_frechet_distance)
    err = np.abs(got["fds"] - want_fds)
    print(f"FD_N: device {got['fds'].tolist()}\n      oracle {want_fds.tolist()}\n      largest |difference| {err.max():.3e}")
    print(f"FD-infinity: device {got['fd_infinity']!r}, oracle {want!r}, FD of all rows {got['fds'][-1]!r}")
    assert np.all(err <= 1e-3)
    own = float(np.polyfit(1.0 / got["sizes"].astype(np.float64), got["fds"], 1)[1])
    assert abs(got["fd_infinity"] - own) <= 1e-9 * max(1.0, abs(own))
    assert abs(got["fd_infinity"] - want) <= 1e-3
    assert got["fd_infinity"] < got["fds"][-1] < got["fds"][0]             # the bias falls with N; the intercept lies below FD of all rows
    again = fd_infinity.fd_infinity_from_features(R, G, seed=3)
    assert again["fd_infinity"] == got["fd_infinity"] and np.array_equal(again["fds"], got["fds"])
    assert fd_infinity.fd_infinity_from_features(R, G, seed=4)["fd_infinity"] != got["fd_infinity"]


TINY84 = dict(width=128, layers=2, heads=2, patch=14, resolution=84)
TINY_NAME = "tiny-mem14"
OLD = ("FD-DINOv2 (", "KD-DINOv2 (", "Precision-DINOv2 (", "Recall-DINOv2 (", "Density-DINOv2 (", "Coverage-DINOv2 (")
NEW = ("AuthPct-DINOv2 (", "Vendi-DINOv2 (", "Vendi-DINOv2 reference (", "FD-infinity-DINOv2 (")


def _png_dir(path, n, seed):
    from PIL import Image
    from tests import _cases
    os.makedirs(path)
    pool = _cases.smooth_images(12, 64, 64, seed=seed)
    for k in range(n):
        Image.fromarray(np.ascontiguousarray(np.roll(pool[k % 12], 3 * k + seed, axis=1))).save(os.path.join(path, f"{k:04d}.png"))
    return str(path)


@pytest.mark.timeout(300)
def test_cli_new_flags_end_to_end_under_a_registered_tiny_tower(cuda_device, tmp_path, capfd, monkeypatch):
    """Three directories of seeded 64 x 64 PNGs under a tiny tower: every new line equals the Python function on the
    --save-features rows, the CSV names the files, the old lines are what they are without the new flags, the three feature
    files give the same lines, and --authpct without --train is refused."""
    from tise_toolbox_amd import authenticity, dinov2_model, fd_dinov2, fd_infinity, img_data, vendi
    from tise_toolbox_amd.weights import SYNTHETIC_TAG
    monkeypatch.setitem(dinov2_model.CONFIGS, TINY_NAME, TINY84)
    monkeypatch.delenv("TISE_DINO", raising=False)
    dirs = dict(ref=_png_dir(tmp_path / "ref", 12, 3), gen=_png_dir(tmp_path / "gen", 14, 4), train=_png_dir(tmp_path / "train", 13, 5))
    npz = {k: str(tmp_path / f"{k}.npz") for k in dirs}
    common = ["--batch-size", "5", "--num-workers", "2", "--synthetic-weights", "--arch", TINY_NAME]

    def run(extra):
        capfd.readouterr()
        res = fd_dinov2.main(extra + common)
        return res, [ln for ln in capfd.readouterr().out.splitlines() if ln.startswith(OLD + NEW)]
    # the feature rows of the three sides (--save-features writes --path1's), and the old lines
    res_old, old = run(["--path1", dirs["ref"], "--path2", dirs["gen"], "--prdc", "--save-features", npz["ref"]])
    run(["--path1", dirs["gen"], "--path2", dirs["ref"], "--save-features", npz["gen"]])
    run(["--path1", dirs["train"], "--path2", dirs["ref"], "--save-features", npz["train"]])
    assert sorted(res_old) == ["fd", "kd", "prdc"] and len(old) == 5 and not any(ln.startswith(NEW) for ln in old)
    rows = {k: fd_dinov2.load_features_npz(npz[k], TINY_NAME)[0] for k in dirs}
    assert [len(rows[k]) for k in ("ref", "gen", "train")] == [12, 14, 13]
    out_csv = str(tmp_path / "near.csv")
    flags = ["--prdc", "--train", dirs["train"], "--authpct", "--nearest-train", out_csv, "--vendi", "--fd-infinity", "--fd-infinity-seed", "2"]
    res, lines = run(["--path1", dirs["ref"], "--path2", dirs["gen"]] + flags)
    assert lines[:5] == old and sorted(res) == ["authpct", "fd", "fd_infinity", "kd", "prdc", "vendi", "vendi_reference"]
    assert res["fd"] == res_old["fd"] and dict(res["prdc"]) == dict(res_old["prdc"])
    near = authenticity.nearest_train(rows["train"], rows["gen"])
    want_inf = fd_infinity.fd_infinity_from_features(rows["ref"], rows["gen"], seed=2)
    want = [f"AuthPct-DINOv2 ({TINY_NAME}): {authenticity.authpct_from_features(rows['train'], rows['gen'])}{SYNTHETIC_TAG}",
            f"Vendi-DINOv2 ({TINY_NAME}): {vendi.vendi_from_features(rows['gen'])}{SYNTHETIC_TAG}",
            f"Vendi-DINOv2 reference ({TINY_NAME}): {vendi.vendi_from_features(rows['ref'])}{SYNTHETIC_TAG}",
            f"FD-infinity-DINOv2 ({TINY_NAME}): {want_inf['fd_infinity']}{SYNTHETIC_TAG}"]
    print("\n".join(lines[5:]))
    assert lines[5:] == want
    assert np.array_equal(res["fd_infinity"]["fds"], want_inf["fds"])
    # the CSV: a header, then one line per generated row with both file names
    with open(out_csv, newline="") as f:
        table = list(csv.reader(f))
    gen_files, train_files = img_data.get_filenames(dirs["gen"]), img_data.get_filenames(dirs["train"])
    assert tuple(table[0]) == fd_dinov2.NEAREST_TRAIN_COLUMNS and len(table) == 1 + 14
    for g, line in enumerate(table[1:]):
        t = int(near["idx"][g])
        assert line == [str(g), str(t), repr(float(near["d2_gen"][g])), str(int(near["authentic"][g])), gen_files[g], train_files[t]]
    # the three feature files: the same lines, and a table without file names
    _, lines_npz = run(["--path1", npz["ref"], "--path2", npz["gen"]] + [npz["train"] if a == dirs["train"] else a for a in flags])
    assert lines_npz == lines
    with open(out_csv, newline="") as f:
        table_npz = list(csv.reader(f))
    assert [ln[:4] for ln in table_npz] == [ln[:4] for ln in table] and all(ln[4:] == ["", ""] for ln in table_npz[1:])
    # --nearest-train alone writes the table and adds no line; --authpct without --train is refused before any GPU work
    os.remove(out_csv)
    res_only, lines_only = run(["--path1", npz["ref"], "--path2", npz["gen"], "--train", npz["train"], "--nearest-train", out_csv])
    assert sorted(res_only) == ["fd", "kd", "prdc"] and lines_only == old[:1] and os.path.exists(out_csv)
    with pytest.raises(SystemExit):
        fd_dinov2.main(["--path1", npz["ref"], "--path2", npz["gen"], "--authpct"] + common)
    with pytest.raises(ValueError, match="need the training set"):
        fd_dinov2.calculate_fd_dinov2_given_paths([npz["ref"], npz["gen"]], arch=TINY_NAME, authpct=True)
