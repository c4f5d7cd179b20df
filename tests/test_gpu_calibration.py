"""GPU: IS* temperature calibration -- csrc/calibrate.hip against an fp64 oracle at every kernel instance and grid edge,
the fitted T against the reference's (tests/golden/calib_*.npz), and the labelled-image path against IS*'s own logits.

Rounding analysis of calibrate.hip (u = 2^-53), per row with C classes, X = max_c |d_c| / T:
  d_c = z_c - m is exact; x_c = fl(d_c * fl(1/T)) = (d_c / T)(1 + 2u); ocml exp is within 1 ulp, so
  e_c = exp(d_c / T)(1 + eps), |eps| <= (2 + 2 X) u.  s = sum e_c and sd = sum d_c e_c carry another gamma_C relative to
  sum |.|, so with K = C + 2 X + 8:
    |nll err| <= u (K + |nll| + 2 |z_y - m| / T)                   (log within 1 ulp, the product, the subtraction)
    |g err|   <= u (K + 4) (|z_y - m| + sum |d| e / s) / T^2      (sd / s, the two products by 1/T)
  and the fold over N rows adds gamma_N sum |.|.  The oracle evaluates the same formulas in fp64 with numpy (its own
  error has the same bound), so the test allows twice the sum (oracle()).  conf = fl32(1 / s): the
  kernel's and the oracle's s agree to ~1e-13, far closer than the 6e-8 spacing of fp32, so bin membership, the
  counts and the correct-prediction counts are compared EXACTLY (rows built to sit on a bin edge are exact on both
  sides: s is an integer there); the per-bin confidence sums within 2 gamma_N of their size.

Memory hygiene: every logits matrix lives inside a NaN-filled allocation (the column before c0, the columns past
c0 + C in a strided row, one row past the last), so a kernel that reads any of it counts a non-finite row.  Every
launch is a legal input; nothing is read out of bounds."""
import ctypes
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests._calib_ref import U, embed, gamma, make_logits, oracle, rows_per_block  # noqa: F401
from tise_toolbox_amd import _lib, calibration, device

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "calib_*.npz")))
TEMPS = (0.05, 0.2188, 0.598, 1.0, 10.0)


@pytest.fixture(scope="module")
def dev(cuda_device):
    torch.cuda.set_device(cuda_device)
    return cuda_device


def check_case(dev, rows, C, T, seed, c0=0, extra_cols=0, n_bins=15):
    z, y = make_logits(rows, C, T, seed)
    buf, ld = embed(z, c0, extra_cols, dev)
    ev = device.CalibrationEvaluator(buf, torch.from_numpy(y), c0=c0, num_classes=C, n_bins=n_bins)
    r = ev(T)
    o = oracle(z, y, T, n_bins)
    what = (rows, C, T, c0, ld)
    assert abs(r["nll_sum"] - o["nll"]) <= o["b_nll"], (what, r["nll_sum"], o["nll"], o["b_nll"])
    assert abs(r["grad_sum"] - o["g"]) <= o["b_g"], (what, r["grad_sum"], o["g"], o["b_g"])
    assert np.array_equal(r["count"], o["count"]), (what, r["count"], o["count"])
    assert np.array_equal(r["correct_sum"], o["correct"]), what
    # (a row whose 1 / s lies within ~1e-13 of an fp32 rounding boundary may round the other way: 2 such rows allowed)
    assert np.all(np.abs(r["conf_sum"] - o["conf"]) <= 2 * gamma(rows) * o["conf"] + 2 * 2.0 ** -24), what
    assert r["count"].sum() == rows
    return r


CLASS_CASES = [(1, 0), (2, 0), (50, 0), (50, 1), (63, 0), (64, 0), (65, 0), (80, 0), (1000, 0), (1008, 0), (2048, 0),
               (3000, 0)]


@pytest.mark.parametrize("C,c0", CLASS_CASES, ids=[f"C{c}_c0{o}" for c, o in CLASS_CASES])
def test_kernel_against_fp64_oracle(dev, C, c0):
    rpb = rows_per_block(C)
    row_counts = [1, 3, 64, 65, 5 * rpb - 1, 5 * rpb + 1]
    for i, rows in enumerate(row_counts):
        check_case(dev, rows, C, TEMPS[i % len(TEMPS)], seed=1000 * C + rows, c0=c0)
    for i, T in enumerate(TEMPS):                                      # every temperature, strided rows
        check_case(dev, 257, C, T, seed=7 * C + i, c0=c0, extra_cols=3)


def test_kernel_grid_edges_and_full_size(dev):
    # the grid is capped at 2048 blocks: one grid step +- 1 row, then the 50 000 x 1000 calibration size
    for rows in (2048 * rows_per_block(50) - 1, 2048 * rows_per_block(50) + 1):
        check_case(dev, rows, 50, 0.598, seed=rows)
    check_case(dev, 50000, 1000, 0.598, seed=5)
    check_case(dev, 20000, 80, 0.2188, seed=6, n_bins=64)
    check_case(dev, 3000, 10, 1.0, seed=8, n_bins=1)


def test_bin_edges_are_lower_open_upper_closed(dev):
    """Confidences exactly 1/2 and 1/4 with 4 bins (edges 0, .25, .5, .75, 1): 1/2 belongs to (.25, .5], 1/4 to (0, .25],
    1 to (.75, 1]."""
    C = 8
    z = np.full((3, C), -1e4, np.float32)
    z[0, :2] = 0.0                                   # conf 1/2
    z[1, :4] = 0.0                                   # conf 1/4
    z[2, 5] = 0.0                                    # conf 1
    y = np.array([1, 0, 5])
    buf, _ = embed(z, 0, 0, dev)
    r = device.CalibrationEvaluator(buf, torch.from_numpy(y), n_bins=4)(1.0)
    assert r["count"].tolist() == [1, 1, 0, 1]
    assert r["conf_sum"].tolist() == [0.25, 0.5, 0.0, 1.0]
    assert r["correct_sum"].tolist() == [1, 0, 0, 1]                 # row 0: label 1, first maximum is column 0


def test_bitwise_deterministic(dev):
    z, y = make_logits(50000, 1000, 0.598, seed=11)
    buf, _ = embed(z, 0, 0, dev)
    ev = device.CalibrationEvaluator(buf, torch.from_numpy(y))
    first = ev.raw(0.598)
    for _ in range(3):
        assert np.array_equal(ev.raw(0.598), first)


def test_bad_input_raises_and_is_counted(dev):
    z, y = make_logits(300, 50, 1.0, seed=3, ties=False)
    buf, _ = embed(z, 0, 0, dev)
    y_bad = y.copy()
    y_bad[[5, 17]] = [50, -1]
    ev = device.CalibrationEvaluator(buf, torch.from_numpy(y_bad))
    raw = ev.raw(1.0)
    assert raw[2] == 0 and raw[3] == 2 and raw[4:4 + 15].sum() == 298
    with pytest.raises(ValueError, match="label"):
        ev(1.0)
    buf[9, 4] = float("nan")
    buf[20, 0] = float("inf")
    ev = device.CalibrationEvaluator(buf, torch.from_numpy(y))
    assert ev.raw(1.0)[2] == 2
    with pytest.raises(ValueError, match="non-finite"):
        ev(1.0)
    with pytest.raises(ValueError):
        calibration.set_temperature_from_logits(buf, y, verbose=False)
    with pytest.raises(_lib.TiseStatusError):
        ev(0.0)


def _ulps32(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


def _numbers(line):
    import re
    return [float(v) for v in re.findall(r"[-+]?\d+\.\d+(?:e[-+]?\d+)?", line)]


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p) for p in FIXTURES])
def test_fixtures_end_to_end(dev, path, capsys):
    f = np.load(path)
    logits = f["q"].astype(np.float32) * np.float32(f["scale"])
    res = calibration.set_temperature_from_logits(logits, f["labels"], float(f["init_temp"]), float(f["lr"]),
                                                  int(f["max_iter"]), c0=int(f["c0"]))
    assert _ulps32(res["temperature"], f["T"]) <= 2, (res["temperature"], float(f["T"]))
    assert abs(res["after"]["nll"] - f["nll_after"]) <= 1e-6
    assert abs(res["after"]["ece"] - f["ece_after"]) <= 1e-6
    assert abs(res["before"]["nll"] - f["nll_before"]) <= 1e-6 and abs(res["before"]["ece"] - f["ece_before"]) <= 1e-6
    printed = capsys.readouterr().out.strip().split("\n")[-3:]
    want = [str(s) for s in f["printed"]]
    assert printed == res["lines"]
    assert printed[0] == want[0]
    assert printed[1].split(":")[0] == want[1].split(":")[0] and printed[2].split("-")[0] == want[2].split("-")[0]
    assert _ulps32(_numbers(printed[1])[0], _numbers(want[1])[0]) <= 2
    assert np.allclose(_numbers(printed[2]), _numbers(want[2]), rtol=0, atol=2e-6)
    assert sum(b[2] for b in res["after"]["bins"]) == logits.shape[0]
    assert abs(calibration.expected_calibration_error(logits, f["labels"], res["temperature"], c0=int(f["c0"]))
               - res["after"]["ece"]) == 0.0


# ---- labelled images -> the logits IS* forms ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def image_tree(tmp_path_factory):
    from PIL import Image
    root = tmp_path_factory.mktemp("calib_images")
    rng = np.random.default_rng(9)
    for cls, n in (("cat", 3), ("ant", 5), ("dog", 2)):             # uneven counts, unsorted creation order
        os.makedirs(root / cls)
        for i in range(n):
            Image.fromarray(rng.integers(0, 256, (96, 96, 3), dtype=np.uint8)).save(root / cls / f"{i}.png")
    return str(root)


@pytest.mark.parametrize("rule,num_classes,drop", [("coco", 1000, False), ("bird", 1008, True)])
def test_collected_logits_are_the_is_star_logits(dev, image_tree, rule, num_classes, drop, monkeypatch):
    from tise_toolbox_amd import inception_score as isc
    files, labels, classes = calibration.labels_from_subdirs(image_tree)
    assert classes == ["ant", "cat", "dog"] and labels.tolist() == [0] * 5 + [1] * 3 + [2] * 2
    logits, c0 = calibration.collect_logits(files, rule=rule, drop_first_class=drop, num_classes=num_classes, seed=0)
    assert c0 == (1 if drop else 0) and tuple(logits.shape) == (10, num_classes)
    seen = []
    orig = device.InceptionScoreAccumulator.update

    def spy(self, lg, idx_base):
        seen.append((int(idx_base), lg.detach().clone()))
        return orig(self, lg, idx_base)
    monkeypatch.setattr(device.InceptionScoreAccumulator, "update", spy)
    isc.configure(weights=None, num_classes=num_classes, seed=0, rule=rule, drop_first_class=drop, fc_bias="auto",
                  batch_size=50)
    isc.get_inception_score(files, splits=2)
    got = torch.empty_like(logits)
    for base, lg in seen:
        got[base:base + lg.shape[0]] = lg
    assert sum(lg.shape[0] for _, lg in seen) == 10
    assert torch.equal(got, logits), "calibration logits differ from the logits IS* reduces"
    res = calibration.set_temperature_from_logits(logits, labels, c0=c0, verbose=False)
    assert np.isfinite(res["temperature"]) and res["temperature"] > 0


def test_cli_image_dir_save_features_round_trip(dev, image_tree, tmp_path):
    from tise_toolbox_amd.weights import SYNTHETIC_TAG
    npz, out1, out2 = str(tmp_path / "f.npz"), str(tmp_path / "r1.txt"), str(tmp_path / "r2.txt")
    r1 = calibration.main(["--image_dir", image_tree, "--labels", "subdirs", "--synthetic-weights", "--save-features", npz,
                           "--saved_file", out1])
    text = open(out1).read()
    assert text.startswith("Before temperature - NLL: ") and SYNTHETIC_TAG in text
    with np.load(npz) as f:
        assert f["features"].shape == (10, 1000) and f["labels"].tolist() == [0] * 5 + [1] * 3 + [2] * 2
    r2 = calibration.main(["--features", npz])
    assert r2["temperature"] == r1["temperature"]
    # a separate process (the module's CLI) writes its result file
    p = subprocess.run([sys.executable, "-m", "tise_toolbox_amd.calibration", "--features", npz, "--saved_file", out2],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = open(out2).read().strip().split("\n")
    assert lines == r2["lines"] and p.stdout.strip().split("\n")[-3:] == r2["lines"]
