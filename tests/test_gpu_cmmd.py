"""GPU: the Gaussian-kernel sums (csrc/mmd.hip, tise_mmd_rbf_grouped) through the C ABI and device.GaussianMMD, cmmd.py on top of
them (CMMD, CLIP-FID, the image loop) and the CLI.

TOLERANCE OF THE SUMS (relative to each sum).  Sized on the CPU, not from the kernel: ``python -m tests.test_gpu_cmmd`` runs
tests/_cmmd_ref.rbf_sums in fp64 and in np.longdouble on exactly the inputs of ``sum_cases()`` below and prints the largest
relative difference between the two over all groups and all three sums, per family:

    unit rows, pool3-scaled rows at gamma = 1/200, equal rows:   SPREAD = 1.097e-15   (pool3-contiguous-d768; REL_SPREAD)
    bound used for the GPU:                                      8 x SPREAD = 8.8e-15 (REL_TOL)
    the width sweep's cases (sweep_cases(): 140 rows, d = 1 .. 191):  2.502e-16 (sweep-pool3-d61) -- smaller, the constant stays
    pool3-scaled rows at gamma = 4:                              SPREAD = 8.169e-12   (pool3-g4-contiguous-d768; REL_SPREAD_G4)
    bound used for the GPU:                                      8 x SPREAD = 6.5e-11 (REL_TOL_G4)

The factor 8 is tests/test_gpu_kid.py's: it covers a different but equally valid summation order, the MFMA's accumulation and an
exp that is off by an ulp.  The gamma = 4 family has its own figure because a relative error e of d^2 (the norms are ~ d^2
themselves, so the subtraction leaves ~ 1e-16 x |a|^2 of absolute error) becomes gamma d^2 e in k = exp(-gamma d^2), and gamma d^2
reaches the hundreds there; the other families are not loosened for it.  For the estimator (cmmd_from_features) the relative bound
is carried through the formula as the KID test does: (REL_TOL + REL_SPREAD) x SCALE x ((|Sxx| + n) / n^2 + (|Syy| + m) / m^2 +
2 |Sxy| / (n m)) for the V-statistic, the i != j denominators for the unbiased one.

The tolerance of embed_image_dir against the fp32 module is the one tests/test_gpu_clip.py::test_towers_match_fp32_module
applies to encode_image -- cosine similarity >= 0.9995 against the fp32 module on the fp16-rounded parameters and the
fp16-rounded input.  That file keeps the figure inline, not as a constant that could be imported, so it is restated once below
(TOWER_COS) with this pointer.
"""
import ctypes
import os

import numpy as np
import pytest

from tests import _cmmd_ref
from tests import _rows_tile_cases as tc
from tests.test_gpu_kid import SIZES_X, SIZES_Y, _dev, pool3_like

REL_SPREAD = 1.097e-15
REL_TOL = 8 * REL_SPREAD
REL_SPREAD_G4 = 8.169e-12
REL_TOL_G4 = 8 * REL_SPREAD_G4
TOWER_COS = 0.9995                      # tests/test_gpu_clip.py::test_towers_match_fp32_module (see the docstring)

DIMS = [64, 100, 512, 768]
GAMMA = 1 / 200


def unit_rows(rows, d, seed, shift=0.0):
    a = np.random.default_rng(seed).standard_normal((rows, d)) + shift
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)


def sum_cases():
    """(name, X, Y, offsets_x, offsets_y, index_x | None, index_y | None, pad, gamma, family): tests/test_gpu_kid.py's group sizes
    (every tile edge, n != m, empty groups); contiguous rows with ld > d (``pad`` extra columns) and gathered rows.  Families:
    "unit" = unit-norm rows at the metric's gamma (k in [0.98, 1]); "pool3" = un-normalised pool3-scaled rows at gamma = 1/200, and
    "pool3-g4" the same kind at gamma = 4 with the y side shifted by 1.0 (k spans hundreds of decades within a set; across the
    sets it is ~ 1e-130 at d = 64 and underflows to exactly 0, far below the denormal range, from d = 512 on); "equal" = copies of one row (d^2 is a rounding residue clamped at 0)."""
    out = []
    ox = np.concatenate([[0], np.cumsum(SIZES_X)])
    oy = np.concatenate([[0], np.cumsum(SIZES_Y)])
    for d in DIMS:
        rng = np.random.default_rng(300 + d)
        ix = np.concatenate([rng.choice(1300, n, replace=False) for n in SIZES_X if n] + [np.zeros(0, np.int64)]).astype(np.int64)
        iy = np.concatenate([rng.choice(1100, n, replace=False) for n in SIZES_Y if n] + [np.zeros(0, np.int64)]).astype(np.int64)
        out.append((f"unit-contiguous-d{d}", unit_rows(ox[-1], d, 100 + d), unit_rows(oy[-1], d, 200 + d, 0.1), ox, oy, None, None, 12, GAMMA, "unit"))
        out.append((f"unit-indexed-d{d}", unit_rows(1300, d, 400 + d), unit_rows(1100, d, 500 + d, 0.1), ox, oy, ix, iy, 0, GAMMA, "unit"))
        X, Y = pool3_like(ox[-1], d, 600 + d), pool3_like(oy[-1], d, 700 + d, shift=0.02)
        out.append((f"pool3-contiguous-d{d}", X, Y, ox, oy, None, None, 12, GAMMA, "pool3"))
        Xp, Yp = pool3_like(1300, d, 800 + d), pool3_like(1100, d, 900 + d, shift=1.0)
        out.append((f"pool3-g4-indexed-d{d}", Xp, Yp, ox, oy, ix, iy, 0, 4.0, "pool3-g4"))
        out.append((f"pool3-g4-contiguous-d{d}", X, pool3_like(oy[-1], d, 700 + d, shift=1.0), ox, oy, None, None, 12, 4.0, "pool3-g4"))
    for name, row in (("equal-unit-rows", unit_rows(1, 512, 7)), ("equal-pool3-rows", pool3_like(1, 100, 8))):
        out.append((name, np.repeat(row, 70, 0), np.repeat(row, 65, 0), np.array([0, 70]), np.array([0, 65]), None, None, 0, GAMMA, "equal"))
    return out


_REFERENCE = {}


def reference_sums(case, dtype=np.float64):
    """Computed once per case and precision, shared by the tests that need it, never changed."""
    key = (case[0], np.dtype(dtype).name)
    if key not in _REFERENCE:
        _, X, Y, ox, oy, ix, iy, _, gamma, _ = case
        rows = []
        for g in range(len(ox) - 1):
            xs = X[ix[ox[g]:ox[g + 1]]] if ix is not None else X[ox[g]:ox[g + 1]]
            ys = Y[iy[oy[g]:oy[g + 1]]] if iy is not None else Y[oy[g]:oy[g + 1]]
            rows.append(_cmmd_ref.rbf_sums(xs, ys, gamma, dtype))
        a = np.array(rows, dtype=dtype)
        a.setflags(write=False)
        _REFERENCE[key] = a
    return _REFERENCE[key]


SWEEP_FAMILIES = ["unit", "pool3"]


def sweep_cases(widths=tuple(tc.WIDTHS)):
    """The width sweep of the gathered-row tile (tests/_rows_tile_cases.py) in sum_cases()' form: three groups of 5, 65 and 70
    rows per side at every width, unit-norm rows (the metric's input) and pool3-scaled rows, both at the metric's gamma."""
    return [(f"sweep-{family}-d{d}",) + tc.mmd_rows(d, family) + (tc.MMD_OX, tc.MMD_OY, None, None, 0, GAMMA, family)
            for d in widths for family in SWEEP_FAMILIES]


def measure_spread(cases=None):
    worst = {}
    for case in (sum_cases() + sweep_cases() if cases is None else cases):
        a, b = reference_sums(case, np.float64), reference_sums(case, np.longdouble)
        nz = a != 0                                           # a sum that is 0 in fp64: every term underflowed (longdouble reaches further down)
        assert np.all(np.abs(b[~nz]) < np.finfo(np.float64).tiny) and np.all(np.abs(a[nz]) > 1e-290)
        rel = float(np.max(np.abs(a[nz].astype(np.longdouble) - b[nz]) / np.abs(b[nz])))
        zeros = int((~nz).sum())
        print(f"{case[0]:>28s}: fp64 vs longdouble, largest relative difference {rel:.3e}; sums that are exactly 0: {zeros}", flush=True)
        fam = "gamma 4" if case[9] == "pool3-g4" else "the rest"
        if rel > worst.get(fam, ("", -1.0))[1]:
            worst[fam] = (case[0], rel)
    for fam, (name, rel) in worst.items():
        print(f"{fam}: largest relative spread {rel:.3e} ({name}); 8 x = {8 * rel:.3e}")
    return worst


def _tol(family):
    return REL_TOL_G4 if family == "pool3-g4" else REL_TOL


def _check_sums(name, got, want, tol):
    worst = 0.0
    for g in range(want.shape[0]):
        for k in range(3):
            if want[g, k] == 0:
                assert got[g, k] == 0, (name, g, k, got[g, k])
            else:
                worst = max(worst, abs(got[g, k] - want[g, k]) / abs(want[g, k]))
    print(f"{name}: largest relative error of a sum {worst:.3e} (bound {tol:.3e})")
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
def test_sums_match_the_numpy_reference_at_every_tile_edge(cuda_device, d):
    from tise_toolbox_amd import device
    worst = {}
    for case in sum_cases():
        name, X, Y, ox, oy, ix, iy, pad, gamma, family = case
        if not (name.endswith(f"-d{d}") or (family == "equal" and d == DIMS[0])):
            continue
        got = device.GaussianMMD(cuda_device, gamma).sums(_dev(X, cuda_device, pad), _dev(Y, cuda_device, pad), ox, oy, ix, iy).cpu().numpy()
        assert got.shape == (len(ox) - 1, 3)
        worst[name] = _check_sums(name, got, reference_sums(case), _tol(family)) / _tol(family)
    assert len(worst) >= 5 and all(w <= 1.0 for w in worst.values()), worst


@pytest.mark.gpu
@pytest.mark.parametrize("d", tc.WIDTHS)
def test_width_sweep_of_the_row_tile(cuda_device, d):
    """Every residue of d mod 4 and both sides of the 64-column slab edge through mmd_tiles_kernel<MMD_RBF> and its norm pre-pass:
    NaN beyond column d and beyond the last row (tests/_rows_tile_gpu.py), the gathered route and the re-laid tensors bit for bit."""
    from tests import _rows_tile_gpu as tg
    from tise_toolbox_amd import device
    for case in sweep_cases((d,)):
        name, X, Y = case[:3]
        tg.check_mmd_width("tise_mmd_rbf", device.GaussianMMD(cuda_device, GAMMA), X, Y, reference_sums(case), REL_TOL, cuda_device,
                           gamma=GAMMA, label=f"rbf {case[9]}")


@pytest.mark.gpu
def test_mask_census_at_gamma_zero_is_exact(cuda_device):
    """k = exp(-0 d2) = 1 for every pair of finite rows: the sums are the numbers of pairs, exactly, the empty and the 1-row group
    included."""
    from tests import _rows_tile_gpu as tg
    for d in tc.CENSUS_WIDTHS:
        tg.check_mask_census("tise_mmd_rbf", cuda_device, d, zero_features=False, gamma=0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("value", tc.BAD_VALUES, ids=tc.BAD_IDS)
def test_a_non_finite_row_poisons_its_own_sums_and_nothing_else(cuda_device, value):
    """fmax(0, NaN) = 0 would make such a row everybody's twin: k = exp(0) = 1 and a finite, wrong result."""
    from tests import _rows_tile_gpu as tg
    for d in tc.NONFINITE_WIDTHS:
        tg.check_mmd_bad_rows("tise_mmd_rbf", cuda_device, d, value, "unit", gamma=GAMMA)


@pytest.mark.gpu
def test_cmmd_from_features_is_nan_for_a_non_finite_or_all_zero_row(cuda_device):
    """The published implementation returns NaN for such input (NaN propagates through its kernel matrices), and so does this.
    An all-zero row becomes NaN in normalize_rows (0 / 0)."""
    import torch
    from tise_toolbox_amd import cmmd
    X, Y = tc.mmd_rows(67, "pool3")
    assert np.isfinite(cmmd.cmmd_from_features(X, Y))
    zero = np.array(X, copy=True)
    zero[tc.MMD_ROWS - 1] = 0
    assert bool(torch.isnan(cmmd.normalize_rows(torch.as_tensor(zero))[-1]).all())
    for unbiased in (False, True):
        assert np.isnan(cmmd.cmmd_from_features(zero, Y, unbiased=unbiased))
        assert np.isnan(cmmd.cmmd_from_features(X, zero, unbiased=unbiased))
        for value in tc.BAD_VALUES:
            assert np.isnan(cmmd.cmmd_from_features(tc.with_bad_row(X, 0, value), Y, unbiased=unbiased)), value
            assert np.isnan(cmmd.cmmd_from_features(torch.as_tensor(X, device=cuda_device), tc.with_bad_row(Y, 64, value), unbiased=unbiased)), value


@pytest.mark.gpu
def test_c_abi_call_on_one_small_case(cuda_device):
    """The raw entry points (workspace sized by the library, offsets that do not start at 0)."""
    import torch
    from tise_toolbox_amd import _lib
    X, Y = unit_rows(70, 64, 1), unit_rows(9, 64, 2, 0.2)
    ox, oy = np.array([3, 66, 67, 70], dtype=np.int64), np.array([1, 5, 8, 9], dtype=np.int64)
    xd, yd = torch.as_tensor(X, device=cuda_device), torch.as_tensor(Y, device=cuda_device)
    pox, poy = ox.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), oy.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    nb = ctypes.c_size_t()
    _lib.call("tise_mmd_rbf_workspace_bytes", pox, poy, 3, ctypes.byref(nb))
    assert nb.value == 512 + 8 * ((1 + 1 + 1) + (1 + 1 + 1) + (1 + 1 + 1)) + 8 * (67 + 8)
    ws = torch.empty(nb.value, dtype=torch.uint8, device=cuda_device)
    out = torch.full((3, 3), -1.0, dtype=torch.float64, device=cuda_device)
    _lib.call("tise_mmd_rbf_grouped", xd.data_ptr(), 70, 64, None, 0, pox, yd.data_ptr(), 9, 64, None, 0, poy, 3, 64, GAMMA,
              out.data_ptr(), ws.data_ptr(), nb.value, None)
    torch.cuda.synchronize()
    want = np.array([_cmmd_ref.rbf_sums(X[ox[g]:ox[g + 1]], Y[oy[g]:oy[g + 1]], GAMMA) for g in range(3)])
    assert _check_sums("c-abi", out.cpu().numpy(), want, REL_TOL) <= REL_TOL


@pytest.mark.gpu
def test_c_abi_rejections_launch_nothing(cuda_device):
    """Real device addresses: a defect that slipped through would launch.  The output keeps its fill."""
    import torch
    from tests.test_cmmd_host import check_rejections
    from tise_toolbox_amd import _lib
    x = torch.zeros((200, 64), device=cuda_device)
    y = torch.zeros((150, 68), device=cuda_device)
    index = torch.zeros(200, dtype=torch.int64, device=cuda_device)
    out = torch.full((2, 3), -7.0, dtype=torch.float64, device=cuda_device)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=cuda_device)
    check_rejections(_lib.load(), _lib.TISE_ERR_INVALID_ARG, _lib.TISE_OK, x.data_ptr(), y.data_ptr(), index.data_ptr(), out.data_ptr(),
                     ws.data_ptr())
    torch.cuda.synchronize()
    assert torch.all(out == -7.0)


@pytest.mark.gpu
def test_two_runs_give_identical_bits(cuda_device):
    import torch
    from tise_toolbox_amd import device
    for name in ("unit-indexed-d768", "unit-contiguous-d100"):
        _, X, Y, ox, oy, ix, iy, pad, gamma, _ = [c for c in sum_cases() if c[0] == name][0]
        xd, yd = _dev(X, cuda_device, pad), _dev(Y, cuda_device, pad)
        a = device.GaussianMMD(cuda_device, gamma).sums(xd, yd, ox, oy, ix, iy).cpu().numpy()
        torch.empty(1 << 22, device=cuda_device).normal_()                     # other work, another workspace allocation
        b = device.GaussianMMD(cuda_device, gamma).sums(xd, yd, ox, oy, ix, iy).cpu().numpy()
        assert a.tobytes() == b.tobytes() and np.all(a[np.diff(ox) > 1, 0] > 0), name


@pytest.mark.gpu
def test_the_diagonal_is_excluded(cuda_device):
    """k(x_i, x_i) = 1: n of them would move Sxx by far more than the bound."""
    from tise_toolbox_amd import device
    for n in (130, 65, 5, 64, 1):
        X = unit_rows(n, 256, 11 + n)
        got = device.GaussianMMD(cuda_device, GAMMA).sums(_dev(X, cuda_device), _dev(X, cuda_device), [0, n], [0, n]).cpu().numpy()
        want = np.array([_cmmd_ref.rbf_sums(X, X, GAMMA)])
        assert _check_sums(f"{n} rows against themselves", got, want, REL_TOL) <= REL_TOL
        assert abs(got[0, 0] - want[0, 0]) < 0.5 and abs(got[0, 1] - want[0, 1]) < 0.5            # not reference + n
        assert abs(got[0, 2] - (want[0, 0] + n)) <= REL_TOL * want[0, 2] + 1e-9                    # the cross sum keeps i == j


def _estimate_bound(x, y, unbiased):
    s = _cmmd_ref.rbf_sums(x, y, GAMMA)
    n, m = len(x), len(y)
    if unbiased:
        scale = abs(s[0]) / (n * (n - 1)) + abs(s[1]) / (m * (m - 1)) + 2 * abs(s[2]) / (n * m)
    else:
        scale = (abs(s[0]) + n) / (n * n) + (abs(s[1]) + m) / (m * m) + 2 * abs(s[2]) / (n * m)
    return (REL_TOL + REL_SPREAD) * _cmmd_ref.SCALE * float(scale)


@pytest.mark.gpu
def test_cmmd_from_features_matches_the_textbook_forms(cuda_device):
    import torch
    from tise_toolbox_amd import cmmd
    rng = np.random.default_rng(5)
    f1 = (rng.standard_normal((300, 512)) * 3.0 + 0.2).astype(np.float32)          # not unit-norm going in
    f2 = (rng.standard_normal((257, 512)) * 0.5 + 0.25).astype(np.float32)
    # the reference normalises in fp32 the same way: the product's own rule, on the same device, then every step in numpy
    x = cmmd.normalize_rows(torch.as_tensor(f1, device=cuda_device)).cpu().numpy()
    y = cmmd.normalize_rows(torch.as_tensor(f2, device=cuda_device)).cpu().numpy()
    for a, f in ((x, f1), (y, f2)):
        assert a.dtype == np.float32 and np.abs(np.linalg.norm(a.astype(np.float64), axis=1) - 1).max() <= 4 * np.finfo(np.float32).eps
        assert np.abs(a - f / np.linalg.norm(f, axis=1, keepdims=True)).max() <= 4 * np.finfo(np.float32).eps
    for unbiased, ref in ((False, _cmmd_ref.cmmd_v), (True, _cmmd_ref.cmmd_u)):
        got = cmmd.cmmd_from_features(torch.as_tensor(f1, device=cuda_device), f2, unbiased=unbiased)
        want, bound = ref(x, y), _estimate_bound(x, y, unbiased)
        print(f"unbiased={unbiased}: {got!r} vs {want!r}, |diff| {abs(got - want):.3e}, bound {bound:.3e}")
        assert isinstance(got, float) and abs(got - want) <= bound and got > 0
    same = cmmd.cmmd_from_features(f1, f1.copy())
    print(f"a set against itself: {same!r}, bound {_estimate_bound(x, x, False):.3e}")
    assert abs(same) <= _estimate_bound(x, x, False)
    with pytest.raises(ValueError):
        cmmd.cmmd_from_features(f1[:1], f2, unbiased=True)
    with pytest.raises(ValueError):
        cmmd.cmmd_from_features(f1, f2[:, :256])


def _png_dir(path, n, seed, sizes=((64, 64),)):
    from PIL import Image
    from tests import _cases
    os.makedirs(path)
    pool = _cases.smooth_images(16, 120, 120, seed=seed)
    for k in range(n):
        h, w = sizes[k % len(sizes)]
        im = np.roll(pool[k % 16], 5 * k + seed, axis=1)[:h, :w]
        Image.fromarray(np.ascontiguousarray(im)).save(os.path.join(path, f"{k:04d}.png"))
    return str(path)


@pytest.fixture(scope="module")
def towers(cuda_device):
    from tise_toolbox_amd import RP_coco
    return RP_coco.build_towers(None, cuda_device)[0]


@pytest.mark.gpu
def test_embed_image_dir_rows(cuda_device, towers, tmp_path):
    import torch
    from PIL import Image
    from tise_toolbox_amd import clip_model, cmmd, feeds, img_data
    path = _png_dir(tmp_path / "imgs", 70, 1)
    files = img_data.get_filenames(path)
    assert len(files) == 70
    rows = cmmd.embed_image_dir(towers, path, cuda_device, 16, workers=2, feed="ring")
    assert feeds.last.kind == "ring" and rows.shape == (70, 512) and rows.dtype == torch.float32 and rows.is_cuda
    batch = torch.from_numpy(np.stack([np.asarray(Image.open(f).convert("RGB")) for f in files])).to(cuda_device)
    with torch.no_grad():
        one = towers.encode_image(clip_model.preprocess_device(batch).half()).float()
    assert torch.equal(rows, one)                                             # every image, walk order, un-normalised, bit for bit
    assert (rows.norm(dim=-1) - 1).abs().min().item() > 1e-3
    # the fp32 torch module on the Pillow preprocess of the same files
    model_h = clip_model.build_clip(seed=0).to(cuda_device).half()
    ref = clip_model.build_clip(seed=0).to(cuda_device)
    ref.load_state_dict({k: v.float() for k, v in model_h.state_dict().items()})
    x = torch.stack([clip_model.preprocess(Image.open(f).convert("RGB")) for f in files]).to(cuda_device)
    with torch.no_grad():
        want = ref.encode_image(x.half().float())
    cos = torch.nn.functional.cosine_similarity(rows, want, dim=-1)
    print("embed_image_dir vs the fp32 module: cos min", cos.min().item())
    assert cos.min().item() >= TOWER_COS


@pytest.mark.gpu
def test_embed_image_dir_ragged_directory_takes_the_dataloader(cuda_device, towers, tmp_path):
    import torch
    from PIL import Image
    from tise_toolbox_amd import clip_model, cmmd, feeds, img_data
    path = _png_dir(tmp_path / "ragged", 11, 2, sizes=((64, 64), (48, 80)))
    files = img_data.get_filenames(path)
    rows = cmmd.embed_image_dir(towers, path, cuda_device, 4, workers=2, feed="ring")
    assert feeds.last.kind == "dataloader" and rows.shape == (11, 512)
    with torch.no_grad():
        for i, f in enumerate(files):
            x = clip_model.preprocess(Image.open(f).convert("RGB"))[None].to(cuda_device).half()
            assert torch.equal(rows[i:i + 1], towers.encode_image(x).float()), i       # the same order (towers are batch invariant)


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_cli_end_to_end(cuda_device, towers, tmp_path, capfd):
    import torch
    from oracle import fid_oracle
    from tise_toolbox_amd import cmmd, fid_score
    from tise_toolbox_amd.weights import SYNTHETIC_TAG
    ref, gen = _png_dir(tmp_path / "ref", 70, 3), _png_dir(tmp_path / "gen", 65, 4)
    out_npz, out_txt = str(tmp_path / "ref.npz"), tmp_path / "result.txt"
    tail = ["--path2", gen, "--batch-size", "16", "--num-workers", "2", "--synthetic-weights", "--clip-fid"]
    capfd.readouterr()
    value, fid = cmmd.main(["--path1", ref] + tail + ["--save-features", out_npz, "--saved_file", str(out_txt)])
    lines = [ln for ln in capfd.readouterr().out.splitlines() if ln.startswith(("CMMD (", "CLIP-FID ("))]
    r1 = cmmd.embed_image_dir(towers, ref, cuda_device, 16, workers=2)
    r2 = cmmd.embed_image_dir(towers, gen, cuda_device, 16, workers=2)
    assert r1.shape == (70, 512) and r2.shape == (65, 512)
    want_cmmd = cmmd.cmmd_from_features(r1, r2)
    (m1, s1), (m2, s2) = cmmd.clip_statistics(r1), cmmd.clip_statistics(r2)
    want_fid = float(fid_score.calculate_frechet_distance(m1, s1, m2, s2))
    assert lines == [f"CMMD (ViT-B/32): {want_cmmd}{SYNTHETIC_TAG}", f"CLIP-FID (ViT-B/32): {want_fid}{SYNTHETIC_TAG}"]
    assert (value, fid) == (want_cmmd, want_fid) and out_txt.read_text() == "\n".join(lines)
    # independently: the CPU oracle on np.mean / np.cov of the rows (N < d: the rank-deficient path)
    a1, a2 = r1.cpu().numpy().astype(np.float64), r2.cpu().numpy().astype(np.float64)
    oracle = fid_oracle.calculate_frechet_distance(a1.mean(0), np.cov(a1, rowvar=False), a2.mean(0), np.cov(a2, rowvar=False))
    print(f"measured: Frechet distance {fid!r} vs oracle {oracle!r}; MMD value {value!r}")
    assert abs(fid - oracle) <= 1e-3
    # the feature file holds the first path's rows and reproduces both lines
    with np.load(out_npz) as f:
        assert sorted(f.files) == ["features", "mu", "network", "sigma"] and str(f["network"]) == "clip-vit-b32"
        assert f["features"].dtype == np.float32 and np.array_equal(f["features"], r1.cpu().numpy())
        assert np.array_equal(f["mu"], m1) and np.array_equal(f["sigma"], s1)
    again = cmmd.main(["--path1", out_npz] + tail)
    lines_npz = [ln for ln in capfd.readouterr().out.splitlines() if ln.startswith(("CMMD (", "CLIP-FID ("))]
    assert lines_npz == lines and again == (value, fid)
    # the Python surface
    assert cmmd.calculate_cmmd_given_paths([out_npz, gen], 16, num_workers=2) == value
    assert cmmd.calculate_clip_fid_given_paths([out_npz, gen], 16, num_workers=2) == fid
    unbiased = cmmd.calculate_cmmd_given_paths([out_npz, gen], 16, num_workers=2, unbiased=True)
    assert unbiased == cmmd.cmmd_from_features(r1, r2, unbiased=True) and unbiased != value
    # a statistics file of another network is refused
    other = str(tmp_path / "inception.npz")
    fid_score.save_stats_npz(other, m1, s1, "inception-2015", r1)
    with pytest.raises(RuntimeError, match="inception-2015"):
        cmmd.main(["--path1", other] + tail)


if __name__ == "__main__":
    measure_spread()
