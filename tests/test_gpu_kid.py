"""GPU: the KID kernel (csrc/mmd.hip) through the C ABI and device.PolynomialMMD, kid.py on top of it, and the CLI.

TOLERANCE OF THE SUMS (relative to each sum).  Sized on the CPU, not from the kernel: ``python -m tests.test_gpu_kid`` runs
tests/_kid_ref.py in fp64 and in np.longdouble on exactly the inputs of ``sum_cases()`` below and prints the largest relative
difference between the two over all groups and all three sums:

    largest relative spread, fp64 numpy against longdouble numpy:  SPREAD = 6.875e-16   (contiguous-d768; REL_SPREAD)
    bound used for the GPU:                                        8 x SPREAD = 5.5e-15 (REL_TOL)
    the width sweep's cases (sweep_cases(): 140 rows, d = 1 .. 191): 2.185e-16 (sweep-d127) -- smaller, the constant stays

The factor 8 covers a different but equally valid summation order and the MFMA's accumulation.  A kernel that needs more is
wrong.  For the estimator (kid_from_features: mean and std over the subsets) the same relative bound is carried through the
formula MMD^2 = Sxx / (n (n - 1)) + Syy / (m (m - 1)) - 2 Sxy / (n m): an error of REL_TOL in each sum moves a subset's value by
at most REL_TOL x (|Sxx| / (n (n - 1)) + |Syy| / (m (m - 1)) + 2 |Sxy| / (n m)) =: REL_TOL x scale, the mean by at most the
largest such amount and the standard deviation (1-Lipschitz in the max norm of the perturbation) by the same; the fp64 reference
carries an error of the same kind (SPREAD x scale), so the comparison allows (REL_TOL + REL_SPREAD) x scale.
"""
import functools
import os

import numpy as np
import pytest

from tests import _kid_ref
from tests import _rows_tile_cases as tc

REL_SPREAD = 6.875e-16
REL_TOL = 8 * REL_SPREAD

SIZES_X = [1, 2, 63, 64, 65, 127, 128, 129, 1000, 0, 5, 70]
SIZES_Y = [2, 1, 64, 65, 63, 129, 127, 128, 1000, 7, 0, 70]
DIMS = [64, 100, 192, 768, 2048]


def pool3_like(rows, d, seed, shift=0.0):
    """Seeded, non-negative, pool3-scaled rows."""
    return (np.abs(np.random.default_rng(seed).standard_normal((rows, d))) * 0.5 + shift).astype(np.float32)


def sum_cases():
    """(name, X, Y, offsets_x, offsets_y, index_x | None, index_y | None, pad): group sizes straddle every tile edge, n != m,
    empty groups; contiguous rows with ld > d (``pad`` extra columns) and gathered rows; one all-equal-rows case."""
    out = []
    for d in DIMS:
        ox = np.concatenate([[0], np.cumsum(SIZES_X)])
        oy = np.concatenate([[0], np.cumsum(SIZES_Y)])
        X, Y = pool3_like(ox[-1], d, 100 + d), pool3_like(oy[-1], d, 200 + d, shift=0.02)
        out.append((f"contiguous-d{d}", X, Y, ox, oy, None, None, 12))
        rng = np.random.default_rng(300 + d)
        Xp, Yp = pool3_like(1300, d, 400 + d), pool3_like(1100, d, 500 + d, shift=0.02)
        ix = np.concatenate([rng.choice(1300, n, replace=False) for n in SIZES_X if n] + [np.zeros(0, np.int64)]).astype(np.int64)
        iy = np.concatenate([rng.choice(1100, n, replace=False) for n in SIZES_Y if n] + [np.zeros(0, np.int64)]).astype(np.int64)
        out.append((f"indexed-d{d}", Xp, Yp, ox, oy, ix, iy, 0))
    row = pool3_like(1, 192, 7)
    out.append(("all-equal-rows", np.repeat(row, 70, 0), np.repeat(row, 65, 0), np.array([0, 70]), np.array([0, 65]), None, None, 0))
    return out


def reference_sums(case, dtype=np.float64):
    _, X, Y, ox, oy, ix, iy, _ = case
    rows = []
    for g in range(len(ox) - 1):
        xs = X[ix[ox[g]:ox[g + 1]]] if ix is not None else X[ox[g]:ox[g + 1]]
        ys = Y[iy[oy[g]:oy[g + 1]]] if iy is not None else Y[oy[g]:oy[g + 1]]
        rows.append(_kid_ref.poly3_sums(xs, ys, dtype))
    return np.array(rows, dtype=dtype)


def sweep_cases(widths=tuple(tc.WIDTHS)):
    """The width sweep of the gathered-row tile (tests/_rows_tile_cases.py) in sum_cases()' form: three groups of 5, 65 and 70
    rows per side at every width."""
    return [(f"sweep-d{d}",) + tc.mmd_rows(d) + (tc.MMD_OX, tc.MMD_OY, None, None, 0) for d in widths]


@functools.lru_cache(maxsize=None)
def sweep_reference(d):
    """Computed once per width, shared, never changed."""
    a = reference_sums(sweep_cases((d,))[0])
    a.setflags(write=False)
    return a


def measure_spread(cases=None):
    worst = 0.0
    for case in (sum_cases() + sweep_cases() if cases is None else cases):
        a, b = reference_sums(case, np.float64), reference_sums(case, np.longdouble)
        nz = b != 0
        assert np.all(a[~nz] == 0)
        rel = float(np.max(np.abs(a[nz].astype(np.longdouble) - b[nz]) / np.abs(b[nz])))
        print(f"{case[0]:>20s}: fp64 vs longdouble, largest relative difference {rel:.3e}", flush=True)
        worst = max(worst, rel)
    print(f"largest relative spread {worst:.3e}; 8 x = {8 * worst:.3e}")
    return worst


def _dev(a, dev, pad=0):
    import torch
    t = torch.as_tensor(a, device=dev)
    if pad:
        wide = torch.full((t.shape[0], t.shape[1] + pad), 7.0, dtype=t.dtype, device=dev)     # the padding must never be read
        wide[:, :t.shape[1]] = t
        t = wide[:, :t.shape[1]]
        assert t.stride(0) == a.shape[1] + pad
    return t


def _check_sums(name, got, want):
    worst = 0.0
    for g in range(want.shape[0]):
        for k in range(3):
            if want[g, k] == 0:
                assert got[g, k] == 0, (name, g, k, got[g, k])
            else:
                worst = max(worst, abs(got[g, k] - want[g, k]) / abs(want[g, k]))
    print(f"{name}: largest relative error of a sum {worst:.3e} (bound {REL_TOL:.3e})")
    return worst


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_sums_match_the_numpy_reference_at_every_tile_edge(cuda_device):
    from tise_toolbox_amd import device
    mmd = device.PolynomialMMD(cuda_device)
    worst = {}
    for case in sum_cases():
        name, X, Y, ox, oy, ix, iy, pad = case
        got = mmd.sums(_dev(X, cuda_device, pad), _dev(Y, cuda_device, pad), ox, oy, ix, iy).cpu().numpy()
        assert got.shape == (len(ox) - 1, 3)
        worst[name] = _check_sums(name, got, reference_sums(case))
    assert all(w <= REL_TOL for w in worst.values()), worst


@pytest.mark.gpu
@pytest.mark.parametrize("d", tc.WIDTHS)
def test_width_sweep_of_the_row_tile(cuda_device, d):
    """Every residue of d mod 4 and both sides of the 64-column slab edge through mmd_tiles_kernel<MMD_POLY3>: NaN beyond
    column d and beyond the last row (tests/_rows_tile_gpu.py), the gathered route and the re-laid tensors bit for bit."""
    from tests import _rows_tile_gpu as tg
    from tise_toolbox_amd import device
    X, Y = tc.mmd_rows(d)
    tg.check_mmd_width("tise_mmd_poly3", device.PolynomialMMD(cuda_device), X, Y, sweep_reference(d), REL_TOL, cuda_device, label="poly3")


@pytest.mark.gpu
def test_mask_census_on_all_zero_features_is_exact(cuda_device):
    """k = (0 / d + 1)^3 = 1 for every pair: the sums are the numbers of pairs, exactly, the empty and the 1-row group included."""
    from tests import _rows_tile_gpu as tg
    for d in tc.CENSUS_WIDTHS:
        tg.check_mask_census("tise_mmd_poly3", cuda_device, d, zero_features=True)


@pytest.mark.gpu
@pytest.mark.parametrize("value", tc.BAD_VALUES, ids=tc.BAD_IDS)
def test_a_non_finite_row_poisons_its_own_sums_and_nothing_else(cuda_device, value):
    from tests import _rows_tile_gpu as tg
    for d in tc.NONFINITE_WIDTHS:
        tg.check_mmd_bad_rows("tise_mmd_poly3", cuda_device, d, value, "pool3")


@pytest.mark.gpu
@pytest.mark.parametrize("value", tc.BAD_VALUES, ids=tc.BAD_IDS)
def test_kid_from_features_is_non_finite_for_a_non_finite_row(cuda_device, value):
    """The reference code (numpy on the host) returns a non-finite value here, and so does this: nothing above the kernel hides
    the row.  Subsets of all rows, so that every subset holds the bad one; the full-set form; and the per-class form, where only
    the row's class is lost."""
    from tise_toolbox_amd import kid
    X, Y = tc.mmd_rows(67)
    for bad1, bad2 in ((tc.with_bad_row(X, 0, value), Y), (X, tc.with_bad_row(Y, tc.MMD_ROWS - 1, value))):
        want = _kid_ref.kid_from_features(bad1, bad2, 3, tc.MMD_ROWS, 1)
        got = kid.kid_from_features(bad1, bad2, 3, tc.MMD_ROWS, 1)
        assert not np.isfinite(want[0]) and not np.isfinite(got[0]), (want, got)
        assert not np.isfinite(kid.kid_from_features(bad1, bad2, subset_size=0)[0])
    names = ["a", "b", "c"]
    clean, _ = kid.per_class_kid(X, tc.MMD_OX, Y, tc.MMD_OY, names)
    got, skipped = kid.per_class_kid(tc.with_bad_row(X, int(tc.MMD_OX[1]), value), tc.MMD_OX, Y, tc.MMD_OY, names)
    assert skipped == [] and not np.isfinite(got["b"]) and got["a"] == clean["a"] and got["c"] == clean["c"], (got, clean)


@pytest.mark.gpu
def test_c_abi_call_and_mmd2_nan_for_small_groups(cuda_device):
    """The raw entry points on one small case (workspace sized by the library), and mmd2's NaN rule."""
    import ctypes
    import torch
    from tise_toolbox_amd import _lib, device
    X, Y = pool3_like(70, 64, 1), pool3_like(9, 64, 2)
    ox, oy = np.array([0, 66, 67, 70], dtype=np.int64), np.array([0, 5, 8, 9], dtype=np.int64)
    xd, yd = torch.as_tensor(X, device=cuda_device), torch.as_tensor(Y, device=cuda_device)
    pox, poy = ox.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), oy.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    nb = ctypes.c_size_t()
    _lib.call("tise_mmd_poly3_workspace_bytes", pox, poy, 3, ctypes.byref(nb))
    assert nb.value == 512 + 8 * ((3 + 1 + 2) + (1 + 1 + 1) + (1 + 1 + 1))      # 9 records of 48 bytes -> 512
    ws = torch.empty(nb.value, dtype=torch.uint8, device=cuda_device)
    out = torch.full((3, 3), -1.0, dtype=torch.float64, device=cuda_device)
    _lib.call("tise_mmd_poly3_grouped", xd.data_ptr(), 70, 64, None, 0, pox, yd.data_ptr(), 9, 64, None, 0, poy, 3, 64,
              out.data_ptr(), ws.data_ptr(), nb.value, None)
    torch.cuda.synchronize()
    want = np.array([_kid_ref.poly3_sums(X[ox[g]:ox[g + 1]], Y[oy[g]:oy[g + 1]]) for g in range(3)])
    assert _check_sums("c-abi", out.cpu().numpy(), want) <= REL_TOL
    v = device.PolynomialMMD(cuda_device).mmd2(xd, yd, ox, oy).cpu().numpy()
    assert np.isnan(v[1]) and np.isnan(v[2]) and np.isfinite(v[0])             # n = 1, and m = 1
    assert abs(v[0] - _kid_ref.mmd2(X[:66], Y[:5])) <= 1e-12


@pytest.mark.gpu
def test_the_diagonal_is_excluded(cuda_device):
    """One huge-norm row: k(x_i, x_i) ~ 1e21 would drown every other term if it entered Sxx."""
    from tise_toolbox_amd import device
    for n, at in ((130, 64), (65, 64), (5, 0), (64, 63)):
        X = pool3_like(n, 256, 11 + n)
        X[at] *= 2.0e4
        Y = pool3_like(7, 256, 12)
        got = device.PolynomialMMD(cuda_device).sums(_dev(X, cuda_device), _dev(Y, cuda_device), [0, n], [0, 7]).cpu().numpy()
        want = np.array([_kid_ref.poly3_sums(X, Y)])
        self_term = (float(X[at].astype(np.float64) @ X[at].astype(np.float64)) / 256 + 1) ** 3
        assert self_term > 1e3 * want[0, 0]
        assert _check_sums(f"huge row {at} of {n}", got, want) <= REL_TOL


@pytest.mark.gpu
def test_two_runs_give_identical_bits(cuda_device):
    import torch
    from tise_toolbox_amd import device
    case = [c for c in sum_cases() if c[0] == "indexed-d768"][0]
    _, X, Y, ox, oy, ix, iy, _ = case
    xd, yd = _dev(X, cuda_device), _dev(Y, cuda_device)
    a = device.PolynomialMMD(cuda_device).sums(xd, yd, ox, oy, ix, iy).cpu().numpy()
    torch.empty(1 << 24, device=cuda_device).normal_()                         # other work, another workspace allocation
    b = device.PolynomialMMD(cuda_device).sums(xd, yd, ox, oy, ix, iy).cpu().numpy()
    assert a.tobytes() == b.tobytes()


def _check_estimate(name, got, want_with_scale):
    mean, std, scale = want_with_scale
    bound = (REL_TOL + REL_SPREAD) * scale
    print(f"{name}: mean {got[0]!r} vs {mean!r}, std {got[1]!r} vs {std!r}; |diff| {abs(got[0] - mean):.3e} / "
          f"{(abs(got[1] - std) if not np.isnan(std) else 0.0):.3e}, bound {bound:.3e}")
    assert abs(got[0] - mean) <= bound
    if np.isnan(std):
        assert np.isnan(got[1])
    else:
        assert abs(got[1] - std) <= bound


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_kid_from_features_matches_the_reference(cuda_device):
    import torch
    from tise_toolbox_amd import kid
    f1, f2 = pool3_like(5000, 2048, 31), pool3_like(5000, 2048, 32, shift=0.03)
    got = kid.kid_from_features(torch.as_tensor(f1, device=cuda_device), f2, 100, 1000, 3)
    _check_estimate("100 x 1000 of 5000 x 2048", got, _kid_ref.kid_from_features(f1, f2, 100, 1000, 3, return_terms=True))
    full = kid.kid_from_features(f1[:3000], f2[:2500], subset_size=0)
    _check_estimate("full set 3000 vs 2500", full, _kid_ref.kid_from_features(f1[:3000], f2[:2500], subset_size=0, return_terms=True))
    # sanity ordering, not a threshold: two draws of one distribution against a shifted one
    same = kid.kid_from_features(f1, pool3_like(5000, 2048, 33), 20, 1000, 0)
    print("same distribution", same, "shifted", got)
    assert abs(same[0]) < abs(got[0])


def _class_sets(seed, absent, single):
    """80 classes, 2-48 rows each; class ``absent`` has no rows on this side, class ``single`` one row (None: neither)."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(2, 49, 80)
    if absent is not None:
        counts[absent] = 0
    if single is not None:
        counts[single] = 1
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return pool3_like(int(offsets[-1]), 2048, seed + 1, shift=0.01 * (seed % 3)), offsets


@pytest.mark.gpu
def test_per_class_kid_values_and_skipped_list(cuda_device):
    from tise_toolbox_amd import kid
    names = [f"class {i:02d}" for i in range(80)]
    f1, o1 = _class_sets(41, absent=17, single=None)
    f2, o2 = _class_sets(42, absent=None, single=60)
    assert not np.array_equal(np.diff(o1), np.diff(o2))
    want, want_skipped = _kid_ref.per_class_kid(f1, o1, f2, o2, names)
    assert want_skipped == ["class 17", "class 60"]                                # two of 80, by the reference alone
    got, skipped = kid.per_class_kid(_dev(f1, cuda_device), o1, f2, o2, names)
    assert skipped == want_skipped and list(got) == list(want) and len(got) == 78
    for i, c in enumerate(names):
        if c in want:
            x, y = f1[o1[i]:o1[i + 1]], f2[o2[i]:o2[i + 1]]
            s = _kid_ref.poly3_sums(x, y)
            n, m = len(x), len(y)
            scale = float(s[0] / (n * (n - 1)) + s[1] / (m * (m - 1)) + 2 * s[2] / (n * m))
            assert abs(got[c] - want[c]) <= (REL_TOL + REL_SPREAD) * scale, (c, got[c], want[c])


def _png_dir(path, n, seed, size=None, classes=None):
    """n PNG files; ``size`` None: every file its own size (crops).  ``classes``: crop names {stem}_{class}_{k}.png."""
    from PIL import Image
    from tests import _cases
    os.makedirs(path)
    pool = _cases.smooth_images(16, 120, 120, seed=seed)
    rng = np.random.default_rng(seed)
    for k in range(n):
        h, w = (size, size) if size else (int(rng.integers(16, 120)), int(rng.integers(16, 120)))
        im = np.roll(pool[k % 16], 5 * k + seed, axis=1)[:h, :w]
        name = f"im{seed}_{k}_{classes[k % len(classes)]}_{k}.png" if classes else f"{k:04d}.png"
        Image.fromarray(np.ascontiguousarray(im)).save(os.path.join(path, name))
    return str(path)


@pytest.mark.gpu
@pytest.mark.timeout(1500)
def test_cli_kid_beside_fid_and_the_feature_file(cuda_device, tmp_path, capfd):
    import torch
    from PIL import Image
    from tise_toolbox_amd import fid_score, img_data, kid
    ref, gen = _png_dir(tmp_path / "ref", 44, 1, size=64), _png_dir(tmp_path / "gen", 43, 2, size=64)
    base = ["--batch-size", "8", "--path1", ref, "--path2", gen, "--num-workers", "0", "--synthetic-weights"]
    kargs = ["--kid", "--kid-subsets", "10", "--kid-subset-size", "16", "--kid-seed", "5"]
    plain_file, fid_file, kid_file = tmp_path / "plain.txt", tmp_path / "fid.txt", tmp_path / "kid.txt"
    stats_plain, stats_kid = tmp_path / "plain.npz", tmp_path / "kid.npz"
    capfd.readouterr()
    fid_plain = fid_score.main(base + ["--saved_file", str(plain_file), "--save-stats", str(stats_plain)])
    out_plain = capfd.readouterr().out
    fid_kid = fid_score.main(base + kargs + ["--saved_file", str(fid_file), "--kid-saved-file", str(kid_file), "--save-stats", str(stats_kid)])
    out_kid = capfd.readouterr().out
    assert fid_plain == fid_kid and plain_file.read_bytes() == fid_file.read_bytes()
    fid_line = [ln for ln in out_plain.splitlines() if ln.startswith("FID: ")]
    assert len(fid_line) == 1 and fid_line == [ln for ln in out_kid.splitlines() if ln.startswith("FID: ")]
    assert "KID" not in out_plain
    kid_lines = [ln for ln in out_kid.splitlines() if ln.startswith("KID: ")]
    assert len(kid_lines) == 1 and kid_file.read_text() == kid_lines[0] and " +- " in kid_lines[0]
    assert out_kid.splitlines().index(kid_lines[0]) == out_kid.splitlines().index(fid_line[0]) + 1
    with np.load(stats_plain) as f:
        assert sorted(f.files) == ["mu", "sigma"]
    with np.load(stats_kid) as f:
        assert sorted(f.files) == ["features", "mu", "sigma"] and f["features"].dtype == np.float32 and f["features"].shape == (40, 2048)
        feats_file = f["features"]
    # the same files through get_activations -> kid_from_features: the same KID
    model = fid_score._build_model(2048, None, 1000, 0)

    def batches(path, n_used):
        files = img_data.get_filenames(path)[:n_used]
        return [torch.from_numpy(np.stack([np.asarray(Image.open(f).convert("RGB")) for f in files[i:i + 8]])) for i in range(0, n_used, 8)]
    a1 = fid_score.get_activations(batches(ref, 40), model, 8, 2048, verbose=False)
    a2 = fid_score.get_activations(batches(gen, 40), model, 8, 2048, verbose=False)
    assert np.array_equal(a2.astype(np.float32), feats_file)
    want = kid.kid_from_features(a1, a2, 10, 16, 5)
    print("CLI:", kid_lines[0], "| get_activations -> kid_from_features:", want)
    assert kid_lines[0].startswith(f"KID: {want[0]} +- {want[1]}")
    # the feature file as --path1: KID of gen against itself's file == KID against the directory, bit for bit
    a = fid_score.main(["--batch-size", "8", "--path1", gen, "--path2", ref, "--num-workers", "0", "--synthetic-weights"] + kargs)
    line_dir = [ln for ln in capfd.readouterr().out.splitlines() if ln.startswith("KID: ")]
    b = fid_score.main(["--batch-size", "8", "--path1", str(stats_kid), "--path2", ref, "--num-workers", "0", "--synthetic-weights"] + kargs)
    line_npz = [ln for ln in capfd.readouterr().out.splitlines() if ln.startswith("KID: ")]
    assert len(line_dir) == 1 and line_dir == line_npz and a is not None and b is not None
    # a {mu, sigma} file cannot serve --kid
    with pytest.raises(RuntimeError, match=r"plain\.npz.*--kid --save-stats"):
        fid_score.main(["--batch-size", "8", "--path1", str(stats_plain), "--path2", ref, "--num-workers", "0", "--synthetic-weights"] + kargs)
    # full-set form prints a NaN deviation
    fid_score.main(base + ["--kid", "--kid-subset-size", "0"])
    full = [ln for ln in capfd.readouterr().out.splitlines() if ln.startswith("KID: ")]
    assert len(full) == 1 and " +- nan" in full[0]


@pytest.mark.gpu
@pytest.mark.timeout(1500)
def test_cli_per_class_kid_on_ragged_crops(cuda_device, tmp_path, capfd):
    from tise_toolbox_amd import fid_score
    classes = ["dog", "traffic light", "cup"]
    ref = _png_dir(tmp_path / "ref", 41, 3, classes=classes)
    gen = _png_dir(tmp_path / "gen", 37, 4, classes=classes)
    from PIL import Image
    Image.fromarray(np.full((20, 30, 3), 90, np.uint8)).save(os.path.join(gen, "lonely_zebra_0.png"))     # one crop on one side only
    base = ["--batch-size", "8", "--path1", ref, "--path2", gen, "--label", "O-FID", "--num-classes", "80", "--num-workers", "0",
            "--synthetic-weights", "--per-class"]
    f_plain, f_fid, f_kid = tmp_path / "plain.txt", tmp_path / "fid.txt", tmp_path / "kid.txt"
    capfd.readouterr()
    pa = fid_score.main(base + ["--saved_file", str(f_plain)])
    out_plain = capfd.readouterr().out
    pb = fid_score.main(base + ["--kid", "--saved_file", str(f_fid), "--kid-saved-file", str(f_kid)])
    out_kid = capfd.readouterr().out
    assert dict(pa) == dict(pb) and f_plain.read_bytes() == f_fid.read_bytes() and "O-KID" not in out_plain
    assert f_plain.read_text() in out_kid
    lines = f_kid.read_text().splitlines()
    assert [ln.split(":")[0] for ln in lines] == ["O-KID[cup]", "O-KID[dog]", "O-KID[traffic light]", "O-KID (mean of 3 classes)",
                                                  "skipped (fewer than 2 crops on a side)"]
    assert lines[-1].endswith(": zebra") and "\n".join(lines) in out_kid
    vals = [float(ln.split(": ")[1].split(" ")[0]) for ln in lines[:4]]
    assert all(np.isfinite(vals)) and abs(vals[3] - np.mean(vals[:3])) <= 1e-15
    # the Python surface gives the same values
    kids, skipped = fid_score.calculate_per_class_kid([ref, gen], 8, "0", 2048, None, 80, 0, 0)
    assert skipped == ["zebra"] and [kids[c] for c in ("cup", "dog", "traffic light")] == vals[:3]


if __name__ == "__main__":
    measure_spread()
