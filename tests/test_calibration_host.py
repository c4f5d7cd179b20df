"""CPU: IS* temperature calibration (tise_toolbox_amd/calibration.py) without a GPU.

The fixtures tests/golden/calib_*.npz hold what the reference's temperature_scaling.py fitted on seeded logits
(make_golden_calibration.py).  A test-local fp64 numpy restatement of the loss / gradient / ECE, driven through
torch.optim.LBFGS with the reference's never-zeroed gradient, reproduces every fixture's T to 1 fp32 ulp; without the
accumulation it does not -- which pins the quirk.  The product's own LBFGS driver (calibration.fit_temperature) is run
on the same numpy evaluator."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from tise_toolbox_amd import calibration

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "calib_*.npz")))


def load_fixture(path):
    f = dict(np.load(path))
    f["logits"] = f["q"].astype(np.float32) * np.float32(f["scale"])
    f["c0"] = int(f["c0"])
    return f


def np_terms(logits, labels, T):
    """mean NLL and mean d NLL / dT of softmax(z / T) in fp64 (the quantities csrc/calibrate.hip sums)."""
    z = logits.astype(np.float64)
    m = z.max(axis=1)
    d = z - m[:, None]
    e = np.exp(d / T)
    s = e.sum(axis=1)
    sd = (d * e).sum(axis=1)
    dy = z[np.arange(z.shape[0]), labels] - m
    return float(np.mean(np.log(s) - dy / T)), float(np.mean((dy - sd / s) / T ** 2))


def np_ece(logits, labels, T, n_bins=15):
    z = logits.astype(np.float64) / T
    z -= z.max(axis=1, keepdims=True)
    conf = (1.0 / np.exp(z).sum(axis=1)).astype(np.float32)
    pred = np.argmax(logits, axis=1)
    edges = torch.linspace(0, 1, n_bins + 1).numpy()
    ece = 0.0
    for lo, hi in zip(edges[:-1], edges[1:]):
        inb = (conf > lo) & (conf <= hi)
        if inb.any():
            ece += abs(conf[inb].astype(np.float64).mean() - (pred[inb] == labels[inb]).mean()) * inb.mean()
    return ece


def lbfgs_local(evaluate, init_temp, lr, max_iter, accumulate=True):
    t = torch.nn.Parameter(torch.ones(1) * init_temp)
    opt = torch.optim.LBFGS([t], lr=lr, max_iter=max_iter)

    def closure():
        loss, grad = evaluate(float(t.detach()[0]))
        g = torch.tensor([grad], dtype=torch.float32)
        t.grad = g if (t.grad is None or not accumulate) else t.grad + g
        return torch.tensor(loss, dtype=torch.float32)
    opt.step(closure)
    return float(t.detach()[0])


def ulps32(a, b):
    a32, b32 = np.float32(a), np.float32(b)
    return abs(int(a32.view(np.int32)) - int(b32.view(np.int32)))


def _case(path):
    f = load_fixture(path)
    x = np.ascontiguousarray(f["logits"][:, f["c0"]:])
    return f, x, f["labels"].astype(np.int64)


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p) for p in FIXTURES])
def test_restatement_reproduces_reference_temperature(path):
    f, x, y = _case(path)
    ev = lambda t: np_terms(x, y, t)                                     # noqa: E731
    args = (float(f["init_temp"]), float(f["lr"]), int(f["max_iter"]))
    t = lbfgs_local(ev, *args)
    assert ulps32(t, f["T"]) <= 1, (t, float(f["T"]))
    assert ulps32(calibration.fit_temperature(ev, *args), f["T"]) <= 1
    # without the reference's gradient accumulation the fit lands elsewhere
    t_plain = lbfgs_local(ev, *args, accumulate=False)
    assert abs(t_plain - f["T"]) > 1e-3 * f["T"], (t_plain, float(f["T"]))
    # NLL / ECE before (T = 1) and after, against the reference's fp32 evaluation
    assert abs(np_terms(x, y, 1.0)[0] - f["nll_before"]) <= 1e-5 * max(1.0, f["nll_before"])
    assert abs(np_terms(x, y, f["T"])[0] - f["nll_after"]) <= 1e-5 * max(1.0, f["nll_after"])
    assert abs(np_ece(x, y, 1.0) - f["ece_before"]) <= 1e-6
    assert abs(np_ece(x, y, f["T"]) - f["ece_after"]) <= 1e-6


def test_fixtures_are_there_and_small():
    names = sorted(os.path.basename(p) for p in FIXTURES)
    assert names == ["calib_bird51.npz", "calib_c1000.npz", "calib_c1008.npz", "calib_c50.npz", "calib_c80.npz"]
    assert sum(os.path.getsize(p) for p in FIXTURES) < 3 * 2 ** 20
    widths = {int(load_fixture(p)["logits"].shape[1]) - load_fixture(p)["c0"] for p in FIXTURES}
    assert widths == {50, 80, 1000, 1008}


def test_ece_from_bins():
    assert calibration.ece_from_bins([0, 0], [0.0, 0.0], [0.0, 0.0], 5) == 0.0
    # bin 0: 2 rows, mean conf 0.3, accuracy 0.5; bin 1: 3 rows, mean conf 0.9, accuracy 1
    got = calibration.ece_from_bins([2, 3], [0.6, 2.7], [1.0, 3.0], 5)
    assert got == pytest.approx(0.2 * 0.4 + 0.1 * 0.6, abs=1e-15)


# ---- the GPU tests' oracle against mpmath ------------------------------------------------------------------------------------
def _oracle_cases(C):
    """(z, labels, T): seeded rows with |d| / T up to ~700 and tied maxima (make_logits), then hand-built rows: two, three
    and C tied maxima with the label on and off the tie, X = max|d| / T at 690 .. 705, a row of equal logits."""
    from tests import _calib_ref as R
    out = []
    for T, seed in ((0.05, 1), (0.598, 2), (10.0, 3)):
        z, y = R.make_logits(8, C, T, seed=100 * C + seed)
        out.append((z, y, T))
    for T in (0.2188, 1.0):
        rng = np.random.default_rng(C)
        z = (rng.standard_normal((7, C)) * T).astype(np.float32)
        y = rng.integers(0, C, size=7)
        z[0, [0, C - 1]] = z[0].max() + 1.0                   # two tied maxima, label on the second
        y[0] = C - 1
        z[1, :min(3, C)] = z[1].max() + 0.5                   # three (C = 2: two), label off the tie where there is room
        y[1] = C - 1
        z[2] = 1.25                                          # all equal: s = C, nll = log C, g = 0
        for i, X in ((3, 690.0), (4, 700.0), (5, 705.0)):
            z[i, y[i]] = z[i].max() + 1.0                    # label on the maximum ...
            z[i, (y[i] + 1) % C] = z[i].max() - np.float32(X * T)          # ... and one logit X T below it
        z[6, (y[6] + 1) % C] = z[6].max() + np.float32(700.0 * T)          # the label 700 T below the maximum
        out.append((z, y, T))
    return out


@pytest.mark.parametrize("C", [2, 129, 1025, 2049])
def test_oracle_is_within_its_own_bound_of_mpmath(C):
    """The fp64 oracle the GPU tests compare the kernel with (tests/_calib_ref.oracle_rows) lies, row by row, within the
    undoubled bound b_nll / b_g of the same formulas at 60 digits; fl32(1 / s) and the first argmax agree wherever
    1 / s is clear of an fp32 rounding boundary.  That is what entitles the GPU tests to allow twice the bound."""
    from tests import _calib_ref as R
    worst = [0.0, 0.0]
    for z, y, T in _oracle_cases(C):
        o = R.oracle_rows(z, y, T)
        for i in range(z.shape[0]):
            nll, g, inv_s = R.mp_row(z[i], y[i], T)
            e_nll, e_g = R.mp_abs_err(o["nll"][i], nll), R.mp_abs_err(o["g"][i], g)
            assert e_nll <= o["b_nll"][i], (C, T, i, e_nll, o["b_nll"][i])
            assert e_g <= o["b_g"][i], (C, T, i, e_g, o["b_g"][i])
            worst = [max(worst[0], e_nll / o["b_nll"][i]), max(worst[1], e_g / o["b_g"][i] if o["b_g"][i] else 0.0)]
            if R.fp32_midpoint_distance(inv_s) > 1e-10:
                assert o["conf"][i] == np.float32(float(inv_s)), (C, T, i)
            assert o["pred"][i] == int(np.flatnonzero(z[i] == z[i].max())[0])
    print(f"C={C}: worst oracle error / bound  nll {worst[0]:.3f}  g {worst[1]:.3f}")


# ---- labels ------------------------------------------------------------------------------------------------------------------
def _touch(p):
    os.makedirs(os.path.dirname(p), exist_ok=True)
    open(p, "wb").close()


def test_labels_from_sorted_subdirs(tmp_path):
    for rel in ("zebra/a.png", "apple/x/b.png", "apple/a.png", "mango/c.jpg", "mango/notes.txt"):
        _touch(str(tmp_path / rel))
    files, labels, classes = calibration.labels_from_subdirs(str(tmp_path))
    assert classes == ["apple", "mango", "zebra"]
    rel = [os.path.relpath(f, tmp_path) for f in files]
    assert rel == ["apple/a.png", "apple/x/b.png", "mango/c.jpg", "zebra/a.png"]
    assert labels.tolist() == [0, 0, 1, 2]
    with pytest.raises(ValueError):
        calibration.labels_from_subdirs(str(tmp_path / "apple" / "x"))


def test_labels_from_file(tmp_path):
    for rel in ("a.png", "d/b.png"):
        _touch(str(tmp_path / rel))
    lf = tmp_path / "labels.txt"
    lf.write_text("a.png\t3\n\nd/b.png\t0\n")
    files, labels = calibration.labels_from_file(str(tmp_path), str(lf), num_classes=4)
    assert [os.path.relpath(f, tmp_path) for f in files] == ["a.png", "d/b.png"] and labels.tolist() == [3, 0]
    for text, msg in (("missing.png\t1\n", "no such image"), ("a.png\t4\n", "outside"), ("a.png\t-1\n", "outside"),
                      ("a.png\tcat\n", "not an integer"), ("a.png 1\n", "expected")):
        lf.write_text(text)
        with pytest.raises(ValueError, match=msg):
            calibration.labels_from_file(str(tmp_path), str(lf), num_classes=4)


# ---- CLI ---------------------------------------------------------------------------------------------------------------------
def test_cli_parser():
    p = calibration._build_parser()
    a = p.parse_args(["--features", "x.npz"])
    assert (a.features, a.image_dir, a.init_temp, a.lr, a.max_iter, a.n_bins) == ("x.npz", None, 1.0, 0.01, 50, 15)
    assert (a.rule, a.fc_bias, a.labels, a.drop_first_class, a.synthetic_weights) == ("coco", "auto", "subdirs", False, False)
    a = p.parse_args(["--image_dir", "d", "--labels", "l.txt", "--rule", "bird", "--drop-first-class", "--fc-bias", "off",
                      "--synthetic-weights", "--num-classes", "1008", "--seed", "3", "--init-temp", "0.23", "--lr", "0.02",
                      "--max-iter", "20", "--n-bins", "10", "--save-features", "f.npz", "--saved_file", "r.txt"])
    assert (a.image_dir, a.labels, a.rule, a.drop_first_class, a.fc_bias, a.num_classes, a.seed) == \
        ("d", "l.txt", "bird", True, "off", 1008, 3)
    assert (a.init_temp, a.lr, a.max_iter, a.n_bins, a.save_features, a.saved_file) == (0.23, 0.02, 20, 10, "f.npz", "r.txt")
    for bad in ([], ["--features", "x", "--image_dir", "d"], ["--features", "x", "--rule", "cub"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)


def test_cli_refuses_several_processes(monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(SystemExit, match="one process"):
        calibration.main(["--features", "x.npz"])


# ---- C ABI -------------------------------------------------------------------------------------------------------------------
def test_calib_eval_rejects_bad_arguments_without_a_gpu():
    """tise_calib_eval checks its arguments before any HIP call: fake device addresses, one defect per call."""
    from tise_toolbox_amd import _lib, build
    build.build(force=False, verbose=False)
    lib = _lib.load()
    bad = _lib.TISE_ERR_INVALID_ARG
    Z, Y, E, O, W = 0x7f0000000000, 0x7f0000100000, 0x7f0000200000, 0x7f0000300000, 0x7f0000400000
    need = ctypes.c_size_t()
    assert lib.tise_calib_workspace_bytes(1000, 1000, 15, ctypes.byref(need)) == _lib.TISE_OK
    assert need.value >= (4 + 3 * 15) * 8
    for args in ((-1, 10, 15), (10, 0, 15), (10, 10, 0), (10, 10, 65)):
        assert lib.tise_calib_workspace_bytes(*args, ctypes.byref(need)) == bad, args
    assert lib.tise_calib_workspace_bytes(10, 10, 15, None) == bad

    def call(z=Z, rows=100, ld=50, c0=0, C=50, y=Y, T=1.0, e=E, nb=15, o=O, w=W, wb=1 << 20):
        return lib.tise_calib_eval(z, rows, ld, c0, C, y, T, e, nb, o, w, wb, None)
    for kw in (dict(z=None), dict(y=None), dict(e=None), dict(o=None), dict(w=None), dict(rows=-1), dict(C=0),
               dict(c0=-1), dict(ld=49), dict(c0=1, ld=50), dict(nb=0), dict(nb=65), dict(T=0.0), dict(T=-1.0),
               dict(T=float("inf")), dict(T=float("nan")), dict(wb=8),
               # outside the domain of the arithmetic: 1 / T is not finite; the -FLT_MAX padding needs T <= 2^100
               dict(T=5e-324), dict(T=1e-310), dict(T=2.0 ** 101), dict(T=np.nextafter(2.0 ** 100, np.inf))):
        assert call(**kw) == bad, kw


def test_entry_points_raise_without_a_gpu(monkeypatch):
    """No CPU fallback: with no HIP device visible every device entry point raises TiseLibraryError."""
    from tise_toolbox_amd import _lib
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    x = np.zeros((4, 3), np.float32)
    y = np.zeros(4, np.int64)
    with pytest.raises(_lib.TiseLibraryError):
        calibration.set_temperature_from_logits(x, y, verbose=False)
    with pytest.raises(_lib.TiseLibraryError):
        calibration.expected_calibration_error(x, y)
    with pytest.raises(_lib.TiseLibraryError):
        calibration.collect_logits(["a.png"], weights=None)
