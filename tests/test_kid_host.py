"""CPU: the host side of the Kernel Inception Distance -- C ABI declarations and argument checks of tise_mmd_poly3_*, the
subset sampling rule of kid.py, index validation, the --kid flags and the feature file, and dist.all_gather_rows under gloo."""
import ctypes
import os
import re
import socket
import sys

import numpy as np
import pytest

from tests import _kid_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tise_mmd_poly3_grouped", "tise_mmd_poly3_workspace_bytes")


def test_header_and_signatures_carry_the_new_symbols():
    from tise_toolbox_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tise_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tise_[a-z0-9_]+)\s*\(", text))
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES, name
    assert "mmd.hip" in build.SOURCES
    build.build(force=False, verbose=False)
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name)


def _offs(*v):
    a = np.asarray(v, dtype=np.int64)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


def test_workspace_bytes_counts_exactly_the_tiles_that_exist():
    from tise_toolbox_amd import _lib
    lib = _lib.load()
    nb = ctypes.c_size_t()
    (_, ox), (_, oy) = _offs(0, 1000, 1040, 1040), _offs(0, 1000, 1048, 1100)
    assert lib.tise_mmd_poly3_workspace_bytes(ox, oy, 3, ctypes.byref(nb)) == _lib.TISE_OK
    # 1000 rows = 16 tiles: 136 + 136 + 256; 40 vs 48 rows: 1 + 1 + 1; 0 vs 52 rows: 0 + 1 + 0.  Table: 9 x 48 bytes -> 512
    assert nb.value == 512 + 8 * (528 + 3 + 1)
    assert lib.tise_mmd_poly3_workspace_bytes(ox, oy, 0, ctypes.byref(nb)) == _lib.TISE_OK and nb.value == 0
    bad = _lib.TISE_ERR_INVALID_ARG
    assert lib.tise_mmd_poly3_workspace_bytes(None, oy, 3, ctypes.byref(nb)) == bad
    assert lib.tise_mmd_poly3_workspace_bytes(ox, oy, -1, ctypes.byref(nb)) == bad
    assert lib.tise_mmd_poly3_workspace_bytes(ox, oy, 3, None) == bad
    assert lib.tise_mmd_poly3_workspace_bytes(_offs(0, 5, 4)[1], _offs(0, 5, 6)[1], 2, ctypes.byref(nb)) == bad


def test_grouped_entry_rejects_every_single_defect_without_a_gpu():
    """Fake device addresses; every call has exactly one defect and must come back TISE_ERR_INVALID_ARG before any HIP call (a
    launch would need a device this test does not have).  The empty call (no groups) is accepted without a launch."""
    from tise_toolbox_amd import _lib
    lib = _lib.load()
    bad = _lib.TISE_ERR_INVALID_ARG
    X, Y, IX, IY, OUT, WS = 0x7f0000000000, 0x7f0000100000, 0x7f0000200000, 0x7f0000300000, 0x7f0000400000, 0x7f0000500000
    keep = []

    def call(x=X, rows_x=200, ld_x=64, ix=None, nix=0, ox=(0, 100, 200), y=Y, rows_y=150, ld_y=68, iy=None, niy=0, oy=(0, 50, 150),
             ng=2, d=64, out=OUT, ws=WS, ws_bytes=1 << 20):
        pox = poy = None
        if ox is not None:
            a, pox = _offs(*ox)
            keep.append(a)
        if oy is not None:
            a, poy = _offs(*oy)
            keep.append(a)
        return lib.tise_mmd_poly3_grouped(x, rows_x, ld_x, ix, nix, pox, y, rows_y, ld_y, iy, niy, poy, ng, d, out, ws, ws_bytes, None)

    assert call(ng=0, ox=(0,), oy=(0,)) == _lib.TISE_OK
    assert call(ng=0, ox=(0,), oy=(0,), ld_x=60) == bad                          # arguments are checked before the empty exit
    defects = [dict(x=None), dict(y=None), dict(out=None), dict(ws=None), dict(ox=None), dict(oy=None),
               dict(d=0), dict(d=-64), dict(ld_x=60), dict(ld_y=32), dict(ld_x=66), dict(ld_y=70), dict(x=X + 4), dict(y=Y + 8),
               dict(rows_x=-1), dict(rows_y=-3), dict(ng=-1), dict(nix=-1, ix=IX), dict(ox=(0, 120, 100)), dict(oy=(-1, 50, 150)),
               dict(ox=(0, 100, 201)), dict(oy=(0, 50, 151)), dict(ix=IX, nix=199), dict(iy=IY, niy=149), dict(ws=WS + 4),
               dict(ws_bytes=0)]
    for kw in defects:
        assert call(**kw) == bad, kw
    # groups of 100 / 100 rows against 50 / 100: tiles (3 + 1 + 2) + (3 + 3 + 4) = 16 -> the smallest workspace that passes the
    # size check is 512 (6 records of 48 bytes, rounded to 256) + 8 * 16 bytes; with it the call would go on to the device, so only the refusal is exercised here
    nb = ctypes.c_size_t()
    a, pox = _offs(0, 100, 200)
    b, poy = _offs(0, 50, 150)
    assert lib.tise_mmd_poly3_workspace_bytes(pox, poy, 2, ctypes.byref(nb)) == _lib.TISE_OK and nb.value == 512 + 8 * 16
    assert call(ws_bytes=nb.value - 1) == bad


@pytest.mark.parametrize("n1,n2,subsets,size,seed", [(5000, 5000, 100, 1000, 0), (300, 41, 7, 50, 3), (40, 44, 5, 1000, 9),
                                                      (17, 17, 3, 17, 1), (1003, 998, 4, 1, 2)])
def test_subset_indices_follow_the_reference_rule(n1, n2, subsets, size, seed):
    from tise_toolbox_amd import kid
    if min(size, n1, n2) < 2:
        with pytest.raises(ValueError):
            kid.subset_indices(n1, n2, subsets, size, seed)
        return
    i1, i2, m = kid.subset_indices(n1, n2, subsets, size, seed)
    r1, r2, rm = _kid_ref.subset_indices(n1, n2, subsets, size, seed)
    assert m == rm == min(size, n1, n2) and i1.dtype == i2.dtype == np.int64
    assert np.array_equal(i1, np.concatenate(r1)) and np.array_equal(i2, np.concatenate(r2))
    # the generated side is drawn first: the first draw of a fresh RandomState is side 2's first subset
    assert np.array_equal(i2[:m], np.random.RandomState(seed).choice(n2, m, replace=False))
    for s in range(subsets):
        assert len(set(i1[s * m:(s + 1) * m].tolist())) == m and i1.max() < n1 and i2.max() < n2


def test_full_set_form_draws_nothing():
    from tise_toolbox_amd import kid
    with pytest.raises(ValueError, match="full-set"):
        kid.subset_indices(100, 100, 10, 0, 0)
    x, y = np.abs(np.random.default_rng(0).standard_normal((30, 8))), np.abs(np.random.default_rng(1).standard_normal((20, 8)))
    mean, std = _kid_ref.kid_from_features(x, y, subset_size=0)
    assert np.isnan(std) and mean == _kid_ref.mmd2(x, y)
    assert abs(float(_kid_ref.mmd2(x, y, np.longdouble)) - mean) <= 1e-12


def test_index_and_offsets_are_validated_on_the_host():
    import torch
    from tise_toolbox_amd import device
    assert device.mmd_index([0, 4, 2], 5, "index_x").dtype == np.int64
    assert device.mmd_index(torch.tensor([1, 0]), 2, "index_x").tolist() == [1, 0]
    for bad in ([0, 5], [-1, 2], np.array([[0, 1]]), np.array([0.0, 1.0])):
        with pytest.raises(ValueError):
            device.mmd_index(bad, 5, "index_x")
    assert device.mmd_offsets([0, 3, 3, 9], 9, "offsets_x").tolist() == [0, 3, 3, 9]
    for bad in ([0, 4, 3], [-1, 2], [0, 10], []):
        with pytest.raises(ValueError):
            device.mmd_offsets(bad, 9, "offsets_x")


def test_kid_flags_parse_with_their_defaults():
    from tise_toolbox_amd import fid_score
    p = fid_score._build_parser()
    a = p.parse_args(["--path2", "x"])
    assert (a.kid, a.kid_subsets, a.kid_subset_size, a.kid_seed, a.kid_saved_file) == (False, 100, 1000, 0, "")
    a = p.parse_args(["--path2", "x", "--kid", "--kid-subsets", "7", "--kid-subset-size", "0", "--kid-seed", "3", "--kid-saved-file", "k.txt"])
    assert (a.kid, a.kid_subsets, a.kid_subset_size, a.kid_seed, a.kid_saved_file) == (True, 7, 0, 3, "k.txt")


def test_stats_file_without_features_is_refused_under_kid_before_any_gpu_work(tmp_path):
    from tise_toolbox_amd import fid_score
    plain, full = str(tmp_path / "plain.npz"), str(tmp_path / "full.npz")
    mu, sigma = np.zeros(4), np.eye(4)
    fid_score.save_stats_npz(plain, mu, sigma)
    with np.load(plain) as f:
        assert sorted(f.files) == ["mu", "sigma"]                                  # without --kid: exactly the old keys
    fid_score.save_stats_npz(full, mu, sigma, "inception-2015", np.ones((6, 4)))
    with np.load(full) as f:
        assert sorted(f.files) == ["features", "mu", "network", "sigma"] and f["features"].dtype == np.float32
    assert fid_score.kid_features_of_npz(full).shape == (6, 4)
    with pytest.raises(RuntimeError, match=r"plain\.npz.*--kid --save-stats"):
        fid_score.calculate_kid_given_paths([plain, full], 8, True, 4)
    with pytest.raises(RuntimeError, match=r"plain\.npz.*--kid --save-stats"):
        fid_score.main(["--path1", full, "--path2", plain, "--kid", "--synthetic-weights"])


# ---- dist.all_gather_rows under gloo ------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gather_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch
    import torch.distributed as dist
    from tise_toolbox_amd import dist as tdist
    tdist.init_from_env(backend="gloo")
    counts = {2: [5, 3], 3: [4, 0, 7]}[world]                                      # unequal shards, one of them empty
    lo = sum(counts[:rank])
    rows = torch.arange(sum(counts) * 6, dtype=torch.float32).reshape(-1, 6)       # row i = global row i
    mine = rows[lo:lo + counts[rank]].clone()
    a = tdist.all_gather_rows(mine, counts)
    b = tdist.all_gather_rows(mine)                                                # counts exchanged by the call itself
    err = None
    try:
        tdist.all_gather_rows(mine, [1] * world)
    except ValueError as e:
        err = str(e)
    q.put({"rank": rank, "a": torch.equal(a, rows), "b": torch.equal(b, rows), "dtype": str(a.dtype), "err": err is not None})
    dist.destroy_process_group()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world", [2, 3])
def test_all_gather_rows_returns_global_order_for_unequal_shards(world):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gather_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    outs = [q.get(timeout=240) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted(o["rank"] for o in outs) == list(range(world))
    assert all(o["a"] and o["b"] and o["err"] and o["dtype"] == "torch.float32" for o in outs), outs


def test_all_gather_rows_is_the_identity_for_one_process():
    import torch
    from tise_toolbox_amd import dist as tdist
    t = torch.arange(12.0).reshape(3, 4)
    assert tdist.all_gather_rows(t) is t


# ---- the gathered-row tile's width sweep and the non-finite rule: the oracle's side, checked without a GPU ----------------------
def test_recorded_spread_covers_the_width_sweep():
    from tests import test_gpu_kid
    assert test_gpu_kid.measure_spread(test_gpu_kid.sweep_cases()) <= test_gpu_kid.REL_SPREAD
    assert test_gpu_kid.REL_TOL == 8 * test_gpu_kid.REL_SPREAD


def test_reference_sums_of_a_constant_kernel_count_the_pairs():
    from tests import _rows_tile_cases as tc
    want = tc.census_expected()
    for g, (n, m) in enumerate(zip(tc.CENSUS_SIZES_X, tc.CENSUS_SIZES_Y)):
        assert list(_kid_ref.poly3_sums(np.zeros((n, 3), np.float32), np.zeros((m, 3), np.float32))) == list(want[g])


@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
def test_reference_is_non_finite_for_a_non_finite_row_and_only_where_the_row_enters(value):
    """numpy's semantics, which the kernel has to match: the sums that involve the row are non-finite, the group's third sum and
    every other group keep their bits, and the estimator built on them is non-finite."""
    from tests import _rows_tile_cases as tc
    X, Y = tc.mmd_rows(67)
    clean = tc.group_sums(_kid_ref.poly3_sums, X, Y)
    for side, g, pos in tc.mmd_bad_rows():
        row = int((tc.MMD_OX if side == "x" else tc.MMD_OY)[g]) + pos
        with np.errstate(invalid="ignore"):
            got = tc.group_sums(_kid_ref.poly3_sums, tc.with_bad_row(X, row, value) if side == "x" else X,
                                tc.with_bad_row(Y, row, value) if side == "y" else Y)
        hit = np.zeros(clean.shape, bool)
        hit[g, [0, 2] if side == "x" else [1, 2]] = True
        assert not np.any(np.isfinite(got[hit])) and got[~hit].tobytes() == clean[~hit].tobytes(), (side, g, pos)
    with np.errstate(invalid="ignore"):
        assert not np.isfinite(_kid_ref.kid_from_features(tc.with_bad_row(X, 0, value), Y, 3, tc.MMD_ROWS, 1)[0])
        assert not np.isfinite(_kid_ref.kid_from_features(X, tc.with_bad_row(Y, 139, value), subset_size=0)[0])
