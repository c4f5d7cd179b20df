"""GPU: the k-nearest-neighbour kernels (csrc/knn.hip) through the C ABI and device.KnnManifold, prdc.py on top, and the CLI.

TOLERANCE OF THE RADII (relative to each r2).  Sized on the CPU, not from the kernel: ``python -m tests.test_gpu_prdc`` computes
r2 of exactly the inputs of the radii test below twice -- tests/_prdc_ref.py's fp64 expansion, and direct differences in
np.longdouble -- and prints the largest relative difference between the two over all sets, rows and k:

    largest relative spread, fp64 expansion against longdouble differences:  SPREAD = 3.426e-15  (REL_SPREAD)
        the radii test's sets:                              3.420e-15  (n = 1000, d = 192)
        the width sweep's float sets (d >= 61, 70 and 65 rows):  3.426e-15  (d = 127; measured 3.4253e-15, rounded up)
    bound used for the GPU:                                                  8 x SPREAD = 2.741e-14 (REL_TOL)

The factor 8 covers a different but equally valid summation order and the MFMA's accumulation.  A kernel that needs more is wrong.

THE COUNTS carry no tolerance.  The test asserts, from the reference alone, that every decision d2 < r2 of a float case has a
relative margin |d2 - r2| / r2 of at least 1e-9 (_prdc_cases.MIN_MARGIN) -- six orders of magnitude above the arithmetic's error --
so no decision is undecidable and cnt, rec, prec and the four values must equal the reference's exactly, with zero exclusions.
The integer-valued cases are exact in any order, ties included.
"""
import ctypes
import os

import numpy as np
import pytest

from tests import _prdc_cases as cases
from tests import _prdc_ref
from tests import _rows_tile_cases as tc

REL_SPREAD = 3.426e-15
REL_TOL = 8 * REL_SPREAD


def measure_sweep_spread():
    """The float widths of the gathered-row tile's sweep (tests/_rows_tile_cases.py): both sets, both k."""
    worst = 0.0
    for d in tc.WIDTHS:
        if tc.prdc_is_exact(d):
            continue
        rel = 0.0
        for X in tc.prdc_rows(d):
            s64, sl = np.sort(_prdc_ref.d2_expansion(X, X), axis=1), np.sort(_prdc_ref.d2_direct(X, X), axis=1)
            for k in tc.PRDC_K:
                rel = max(rel, float(np.max(np.abs(s64[:, k].astype(np.longdouble) - sl[:, k]) / sl[:, k])))
        print(f"sweep, d = {d:5d}: r2, fp64 expansion vs longdouble differences, largest relative difference {rel:.3e}", flush=True)
        worst = max(worst, rel)
    return worst


def measure_spread():
    worst = measure_sweep_spread()
    for d in cases.RADII_D:
        for n in sorted({n for k in cases.RADII_K for n in cases.radii_rows(k)}):
            X, s64 = cases.radii_set(n, d)
            sl = np.sort(_prdc_ref.d2_direct(X, X), axis=1)
            rel = 0.0
            for k in cases.RADII_K:
                if n >= k + 1:
                    rel = max(rel, float(np.max(np.abs(s64[:, k].astype(np.longdouble) - sl[:, k]) / sl[:, k])))
            print(f"n = {n:5d}, d = {d:5d}: r2, fp64 expansion vs longdouble differences, largest relative difference {rel:.3e}", flush=True)
            worst = max(worst, rel)
    print(f"largest relative spread {worst:.3e}; 8 x = {8 * worst:.3e}")
    return worst


def _dev(a, dev, pad=cases.PAD):
    import torch
    t = torch.as_tensor(np.asarray(a), device=dev)
    if pad:
        wide = torch.full((t.shape[0], t.shape[1] + pad), 7.0, dtype=t.dtype, device=dev)     # the padding must never be read
        wide[:, :t.shape[1]] = t
        t = wide[:, :t.shape[1]]
        assert t.stride(0) == a.shape[1] + pad
    return t


@pytest.mark.gpu
@pytest.mark.parametrize("d", cases.RADII_D)
def test_radii_match_the_reference_at_every_tile_and_split_edge(cuda_device, d):
    from tise_toolbox_amd import device
    knn = device.KnnManifold(cuda_device)
    worst, where = 0.0, None
    for n in sorted({n for k in cases.RADII_K for n in cases.radii_rows(k)}):
        X, s64 = cases.radii_set(n, d)
        xd = _dev(X, cuda_device)
        for k in cases.RADII_K:
            if n < k + 1:
                continue
            want = s64[:, k]
            if n == k + 1:                                     # the self-mask: with k others, r2 is the largest distance to them
                assert np.array_equal(want, s64[:, -1])
            for splits in cases.RADII_SPLITS:
                got = knn.radius2(xd, k, splits).cpu().numpy()
                assert got.shape == (n,) and got.dtype == np.float64 and np.all(np.isfinite(got))
                rel = float(np.max(np.abs(got - want) / want))
                if rel > worst:
                    worst, where = rel, (n, k, splits)
    print(f"d = {d}: largest relative error of an r2 {worst:.3e} at (n, k, splits) = {where} (bound {REL_TOL:.3e})")
    assert worst <= REL_TOL, (worst, where)


def _check_counts(knn, R, F, k, ref, splits, dev):
    rd, fd = _dev(R, dev), _dev(F, dev)
    cnt, rec, prec = knn.counts(rd, knn.radius2(rd, k, splits), fd, knn.radius2(fd, k, splits), splits)
    cnt, rec, prec = cnt.cpu().numpy(), rec.cpu().numpy(), prec.cpu().numpy()
    assert cnt.dtype == np.int32 and rec.dtype == np.bool_ and prec.dtype == np.bool_
    assert np.array_equal(cnt, ref["cnt"]), ("cnt", splits, int(np.sum(cnt != ref["cnt"])))
    assert np.array_equal(rec, ref["rec"]), ("rec", splits, int(np.sum(rec != ref["rec"])))
    assert np.array_equal(prec, ref["prec"]), ("prec", splits, int(np.sum(prec != ref["prec"])))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", cases.COUNT_SHAPES, ids=lambda s: "n%d-m%d-d%d-k%d" % s[:4])
def test_counts_equal_the_reference_exactly_on_float_inputs(cuda_device, shape):
    import torch
    from tise_toolbox_amd import device, prdc
    R, F, ref = cases.count_case(*shape)
    k = shape[3]
    margin = _prdc_ref.smallest_margin(ref)
    print(f"{shape}: smallest relative margin of a decision {margin:.3e}")
    assert margin >= cases.MIN_MARGIN                         # a property of the inputs, from the reference alone
    knn = device.KnnManifold(cuda_device)
    for splits in cases.COUNT_SPLITS:
        _check_counts(knn, R, F, k, ref, splits, cuda_device)
    got = prdc.prdc_from_features(torch.as_tensor(R, device=cuda_device), F, k)
    assert list(got) == ["precision", "recall", "density", "coverage"] and all(type(v) is float for v in got.values())
    assert all(got[name] == ref[name] for name in got), (dict(got), {name: ref[name] for name in got})


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1])
def test_counts_equal_the_reference_exactly_on_integer_inputs_with_ties(cuda_device, which):
    """Exact arithmetic in any order: equality of all arrays proves the strict `<`, the duplicate handling and the clamp."""
    from tise_toolbox_amd import device, prdc
    R, F, k, ref = cases.integer_case(which)
    ties_r = int(np.sum(ref["cross"] == ref["r2_real"][:, None])), int(np.sum(ref["cross"] == ref["r2_fake"][None, :]))
    print(f"integer case {which}: exact ties d2 == r2: {ties_r[0]} against the real radii, {ties_r[1]} against the generated ones")
    assert ties_r[0] > 0 and ties_r[1] > 0                    # the strict comparison is exercised on both sides
    if which == 1:
        assert np.all(ref["r2_real"][10:18] == 0) and np.all(ref["cross"][40:43, 0:3].diagonal() == 0)
    knn = device.KnnManifold(cuda_device)
    for side, want in ((R, ref["r2_real"]), (F, ref["r2_fake"])):
        assert np.array_equal(knn.radius2(_dev(side, cuda_device), k, 2).cpu().numpy(), want)
    for splits in cases.COUNT_SPLITS:
        _check_counts(knn, R, F, k, ref, splits, cuda_device)
    got = prdc.prdc_from_features(R, F, k)
    assert all(got[name] == ref[name] for name in got)


@pytest.mark.gpu
@pytest.mark.parametrize("d", tc.WIDTHS)
def test_width_sweep_of_the_row_tile(cuda_device, d):
    """Every residue of d mod 4 and both sides of the 64-column slab edge through knn_radius2_kernel<4> (k = 1), <8> (k = 5) and
    prdc_counts_kernel: NaN beyond column d and beyond the last row (tests/_rows_tile_gpu.py), the re-laid tensors bit for bit.
    Below 61 columns the features are integers and r2, cnt, rec, prec EQUAL the reference, exact ties on both sides included;
    from 61 on they are floats under this file's rules (REL_TOL on r2, every decision MIN_MARGIN away from its radius)."""
    from tests import _rows_tile_gpu as tg
    R, F = tc.prdc_rows(d)
    exact, worst = tc.prdc_is_exact(d), 0.0
    for k in tc.PRDC_K:
        print(f"d = {d}, k = {k}: {'ties (real, generated radii)' if exact else 'smallest margin'} {tc.check_prdc_case_properties(d, k)}")
        ref = tc.prdc_reference(d, k)
        for splits in tc.PRDC_SPLITS:
            got = tg.knn_cabi(R, F, k, splits, cuda_device)
            worst = max(worst, tg.check_knn_against(got, ref, exact, REL_TOL, (d, k, splits)))
            for (name, rt), (_, ft) in zip(tg.copy_forcing_layouts(R, cuda_device), tg.copy_forcing_layouts(F, cuda_device)):
                assert tg.same_bits(tg.knn_device(rt, ft, k, splits, cuda_device), got), (name, d, k, splits)
    print(f"d = {d}: largest relative error of an r2 {worst:.3e} (bound {0.0 if exact else REL_TOL:.3e})")


@pytest.mark.gpu
@pytest.mark.parametrize("value", tc.BAD_VALUES, ids=tc.BAD_IDS)
@pytest.mark.parametrize("d", [7, 67])
def test_a_non_finite_row_is_nobodys_neighbour_and_lies_in_no_ball(cuda_device, d, value):
    """fmax(0, NaN) = 0 would put such a row at distance 0 from every row: inside every ball of positive radius (coverage
    exactly 1), everybody's nearest neighbour.  The rule (include/tise_hip.h): the row gets r2 = NaN, cnt = rec = prec = 0 and
    every other row the results of the sets without it -- exactly on the integer inputs (d = 7), within REL_TOL and with every
    decision MIN_MARGIN away on the float ones (d = 67)."""
    from tests import _rows_tile_gpu as tg
    R, F = tc.prdc_rows(d)
    exact = tc.prdc_is_exact(d)
    for side, row in tc.prdc_bad_rows():
        Rb = tc.with_bad_row(R, row, value) if side == "real" else R
        Fb = tc.with_bad_row(F, row, value) if side == "fake" else F
        for k in tc.PRDC_K:
            ref = _prdc_ref.prdc_dropping_nonfinite(Rb, Fb, k)
            assert int(np.isnan(ref["r2_real"]).sum() + np.isnan(ref["r2_fake"]).sum()) == 1
            if not exact:
                assert _prdc_ref.smallest_margin(ref["clean"]) >= cases.MIN_MARGIN
            for splits in tc.PRDC_SPLITS:
                got = tg.knn_cabi(Rb, Fb, k, splits, cuda_device)
                tg.check_knn_against(got, ref, exact, REL_TOL, (d, value, side, row, k, splits))
            assert tg.same_bits(tg.knn_device(*(t for _, t in (tg.copy_forcing_layouts(Rb, cuda_device)[1], tg.copy_forcing_layouts(Fb, cuda_device)[2])),
                                              k, 0, cuda_device), tg.knn_cabi(Rb, Fb, k, 0, cuda_device))


@pytest.mark.gpu
def test_prdc_from_features_refuses_non_finite_rows_as_the_prdc_package_does(cuda_device, tmp_path):
    """ValueError that names the side, the number of affected rows and the first of them; through fid_score --prdc with a feature
    file as --path1 as well (its stored ``features`` go straight in)."""
    import torch
    from tise_toolbox_amd import fid_score, prdc
    R, F = tc.prdc_rows(67)
    assert all(np.isfinite(v) for v in prdc.prdc_from_features(R, F, 5).values())
    bad = tc.with_bad_row(tc.with_bad_row(R, 69, float("inf")), 12, float("nan"))
    with pytest.raises(ValueError, match=r"the real side has 2 feature rows with a NaN or an infinity \(the first is row 12\)"):
        prdc.prdc_from_features(bad, F, 5)
    with pytest.raises(ValueError, match=r"the fake side has 1 feature row with a NaN or an infinity \(the first is row 64\)"):
        prdc.prdc_from_features(torch.as_tensor(R, device=cuda_device), tc.with_bad_row(F, 64, float("-inf")), 3)
    with pytest.raises(ValueError, match=r"the real side has 1 feature row .*row 0\)"):
        prdc.prdc_from_features(tc.with_bad_row(R, 0, float("nan")), tc.with_bad_row(F, 3, float("nan")), 1)
    # the CLI: two feature files of 64-wide rows (no image is read), the first with a NaN row
    R64, F64 = tc.prdc_rows(64)
    files = []
    for name, rows in (("bad.npz", tc.with_bad_row(R64, 5, float("nan"))), ("gen.npz", F64), ("real.npz", R64)):
        a = rows[np.isfinite(rows).all(axis=1)].astype(np.float64)
        files.append(str(tmp_path / name))
        fid_score.save_stats_npz(files[-1], a.mean(0), np.cov(a, rowvar=False), "torchvision", rows)
    args = ["--path2", files[1], "--prdc", "--dims", "64", "--synthetic-weights"]
    with pytest.raises(ValueError, match=r"the real side has 1 feature row with a NaN or an infinity \(the first is row 5\)"):
        fid_score.main(["--path1", files[0]] + args)
    assert fid_score.main(["--path1", files[2]] + args) is not None


@pytest.mark.gpu
def test_a_set_against_itself_is_all_ones(cuda_device):
    """Passes only if the cross pass and the within-set pass produce the same bits for the same pair: row i's k-th neighbour j
    sits at d2 == r2 exactly (not inside, strict `<`), its k - 1 nearer neighbours and the row itself inside -> cnt = k."""
    from tise_toolbox_amd import device, prdc
    X = cases.pool3_like(257, 192, 77)
    ref = _prdc_ref.prdc(X, X, 5)
    assert [ref[name] for name in ("precision", "recall", "density", "coverage")] == [1.0, 1.0, 1.0, 1.0]
    got = prdc.prdc_from_features(X, X, 5)
    assert list(got.values()) == [1.0, 1.0, 1.0, 1.0], dict(got)
    knn = device.KnnManifold(cuda_device)
    xd = _dev(X, cuda_device)
    r2 = knn.radius2(xd, 5, 3)
    cnt, rec, prec = knn.counts(xd, r2, xd.clone(), knn.radius2(xd, 5, 1), 2)
    assert np.all(cnt.cpu().numpy() == 5) and bool(rec.all()) and bool(prec.all())


@pytest.mark.gpu
def test_two_runs_give_identical_bits(cuda_device):
    import torch
    from tise_toolbox_amd import device
    R, F, _ = cases.count_case(*cases.COUNT_SHAPES[2])
    rd, fd = _dev(R, cuda_device), _dev(F, cuda_device)

    def run():
        knn = device.KnnManifold(cuda_device)
        r2r, r2f = knn.radius2(rd, 5), knn.radius2(fd, 5)
        return b"".join(t.cpu().numpy().tobytes() for t in (r2r, r2f) + knn.counts(rd, r2r, fd, r2f))
    a = run()
    torch.empty(1 << 24, device=cuda_device).normal_()                         # other work, another workspace allocation
    assert a == run()


@pytest.mark.gpu
def test_c_abi_calls_with_a_workspace_sized_by_the_library(cuda_device):
    import torch
    from tise_toolbox_amd import _lib
    R, F, ref = cases.count_case(*cases.COUNT_SHAPES[0])
    n, m, d, k = 300, 260, 64, 5
    rd, fd = torch.as_tensor(R, device=cuda_device), torch.as_tensor(F, device=cuda_device)
    r2 = []
    for t, rows in ((rd, n), (fd, m)):
        nb = ctypes.c_size_t()
        _lib.call("tise_knn_workspace_bytes", rows, k, 2, ctypes.byref(nb))
        assert nb.value == 8 * rows * (2 * k + 1)
        ws = torch.empty(nb.value, dtype=torch.uint8, device=cuda_device)
        out = torch.full((rows,), -1.0, dtype=torch.float64, device=cuda_device)
        _lib.call("tise_knn_radius2", t.data_ptr(), rows, d, d, k, 2, out.data_ptr(), ws.data_ptr(), nb.value, None)
        torch.cuda.synchronize()
        r2.append(out)
    for got, want in zip(r2, (ref["r2_real"], ref["r2_fake"])):
        assert float(np.max(np.abs(got.cpu().numpy() - want) / want)) <= REL_TOL
    cnt = torch.full((n,), -1, dtype=torch.int32, device=cuda_device)
    rec = torch.full((n,), -1, dtype=torch.int32, device=cuda_device)
    prec = torch.full((m,), -1, dtype=torch.int32, device=cuda_device)
    ws = torch.empty(8 * (n + m), dtype=torch.uint8, device=cuda_device)
    _lib.call("tise_prdc_counts", rd.data_ptr(), n, d, r2[0].data_ptr(), fd.data_ptr(), m, d, r2[1].data_ptr(), d, 3, cnt.data_ptr(),
              rec.data_ptr(), prec.data_ptr(), ws.data_ptr(), ws.numel(), None)
    torch.cuda.synchronize()
    assert np.array_equal(cnt.cpu().numpy(), ref["cnt"])
    assert np.array_equal(rec.cpu().numpy(), ref["rec"].astype(np.int32)) and np.array_equal(prec.cpu().numpy(), ref["prec"].astype(np.int32))


def _png_dir(path, n, seed, size):
    from PIL import Image
    from tests import _cases
    os.makedirs(path)
    pool = _cases.smooth_images(16, 120, 120, seed=seed)
    for i in range(n):
        im = np.roll(pool[i % 16], 5 * i + seed, axis=1)[:size, :size]
        Image.fromarray(np.ascontiguousarray(im)).save(os.path.join(path, f"{i:04d}.png"))
    return str(path)


LABELS = ("Precision: ", "Recall: ", "Density: ", "Coverage: ")


def _four(out):
    lines = out.splitlines()
    found = [ln for ln in lines if ln.startswith(LABELS)]
    return lines, found


@pytest.mark.gpu
@pytest.mark.timeout(1500)
def test_cli_prdc_beside_fid_and_kid_and_the_feature_file(cuda_device, tmp_path, capfd):
    import torch
    from PIL import Image
    from tise_toolbox_amd import fid_score, img_data, prdc
    ref, gen = _png_dir(tmp_path / "ref", 44, 1, 64), _png_dir(tmp_path / "gen", 43, 2, 64)
    common = ["--batch-size", "8", "--num-workers", "0", "--synthetic-weights"]
    base = common + ["--path1", ref, "--path2", gen]
    pargs = ["--prdc", "--prdc-k", "3"]
    plain_file, fid_file, prdc_file = tmp_path / "plain.txt", tmp_path / "fid.txt", tmp_path / "prdc.txt"
    stats_plain, stats_full = tmp_path / "plain.npz", tmp_path / "full.npz"
    capfd.readouterr()
    fid_plain = fid_score.main(base + ["--saved_file", str(plain_file), "--save-stats", str(stats_plain)])
    out_plain = capfd.readouterr().out
    fid_both = fid_score.main(base + pargs + ["--kid", "--kid-subsets", "4", "--kid-subset-size", "16", "--saved_file", str(fid_file),
                                              "--prdc-saved-file", str(prdc_file), "--save-stats", str(stats_full)])
    out_both = capfd.readouterr().out
    # FID untouched; the plain run names none of the four
    assert fid_plain == fid_both and plain_file.read_bytes() == fid_file.read_bytes()
    assert not any(label.strip() in out_plain for label in LABELS)
    fid_line = [ln for ln in out_plain.splitlines() if ln.startswith("FID: ")]
    lines, four = _four(out_both)
    assert len(fid_line) == 1 and fid_line == [ln for ln in lines if ln.startswith("FID: ")]
    assert [ln.split(": ")[0] + ": " for ln in four] == list(LABELS)
    at = lines.index(fid_line[0])
    assert lines[at + 1].startswith("KID: ") and lines[at + 2:at + 6] == four          # after the KID line
    assert prdc_file.read_text() == "\n".join(four)
    with np.load(stats_plain) as f:
        assert sorted(f.files) == ["mu", "sigma"]
    with np.load(stats_full) as f:
        assert sorted(f.files) == ["features", "mu", "sigma"] and f["features"].dtype == np.float32 and f["features"].shape == (40, 2048)
    # the same files through get_activations -> prdc_from_features: the same four values, bit for bit
    model = fid_score._build_model(2048, None, 1000, 0)

    def batches(path, n_used):
        files = img_data.get_filenames(path)[:n_used]
        return [torch.from_numpy(np.stack([np.asarray(Image.open(f).convert("RGB")) for f in files[i:i + 8]])) for i in range(0, n_used, 8)]
    a1 = fid_score.get_activations(batches(ref, 40), model, 8, 2048, verbose=False)
    a2 = fid_score.get_activations(batches(gen, 40), model, 8, 2048, verbose=False)
    want = prdc.prdc_from_features(a1, a2, 3)
    print("CLI:", four, "| get_activations -> prdc_from_features:", dict(want))
    assert [ln.split(" ")[1] for ln in four] == [repr(v) for v in want.values()]
    # without --kid the four lines follow the FID line; the feature file as --path1 reproduces them bit for bit
    swapped = common + pargs + ["--path2", ref]
    a = fid_score.main(swapped + ["--path1", gen])
    lines_dir, four_dir = _four(capfd.readouterr().out)
    at = [i for i, ln in enumerate(lines_dir) if ln.startswith("FID: ")]
    assert len(at) == 1 and lines_dir[at[0] + 1:at[0] + 5] == four_dir and len(four_dir) == 4
    b = fid_score.main(swapped + ["--path1", str(stats_full)])
    _, four_npz = _four(capfd.readouterr().out)
    assert four_dir == four_npz and a is not None and b is not None
    # a {mu, sigma} file cannot serve --prdc, and the message names the flag
    with pytest.raises(RuntimeError, match=r"plain\.npz.*--prdc needs the feature rows"):
        fid_score.main(swapped + ["--path1", str(stats_plain)])


if __name__ == "__main__":
    measure_spread()
