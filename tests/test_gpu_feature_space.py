"""feature_space.given_paths on a stand-in space: no tower, ``embed_dir`` hands out seeded fp32 rows (9 reference, 7 generated, 11
training).  The width is 1: tise_stats_create and tise_frechet_create accept 0 < d <= 8192, so 1 is the smallest both take."""
import csv

import numpy as np
import pytest
import torch

from tise_toolbox_amd import authenticity, fd_infinity, feature_space as fs, fid_score, img_data, kid, prdc, vendi

pytestmark = pytest.mark.gpu

WIDTH = 1
COUNTS = dict(ref=9, gen=7, train=11)
NETWORK = "stand-in-net"
EVERY = ("fd", "kd", "prdc", "authpct", "vendi", "fd_infinity")


class StandIn:
    def __init__(self, root):
        rng = np.random.default_rng(23)
        self.dirs, self.rows, self.built = {}, {}, 0
        for name, n in COUNTS.items():
            (root / name).mkdir()
            self.dirs[name] = str(root / name)
            for k in range(n):                                             # one (never opened) file per row: the CSV names them
                (root / name / f"{k:03d}.png").touch()
            self.rows[name] = rng.standard_normal((n, WIDTH)).astype(np.float32)
        by_path = {self.dirs[k]: self.rows[k] for k in COUNTS}

        def build_tower(dev):
            self.built += 1
            return "the tower"

        def embed_dir(tower, path, dev, batch, workers, feed):
            assert tower == "the tower"
            return torch.from_numpy(by_path.get(path, np.zeros((0, WIDTH), np.float32))).to(dev)
        self.space = fs.Space("stand_in", NETWORK, WIDTH, build_tower, embed_dir)


@pytest.fixture
def stand_in(cuda_device, tmp_path):
    return StandIn(tmp_path)


def _same(a, b):
    """== on floats, tuples and nested dicts; np.array_equal on arrays."""
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(a, b)
    return type(a) is type(b) and a == b


def test_towers_built_feature_file_and_the_same_numbers_from_it(stand_in, tmp_path):
    s, d = stand_in, stand_in.dirs
    npz = {k: str(tmp_path / f"{k}.npz") for k in COUNTS}
    res = fs.given_paths(s.space, [d["ref"], d["gen"]], save_features=npz["ref"], train=d["train"], want=EVERY)
    assert s.built == 1                                                    # a directory, a directory and the training set: one tower
    assert sorted(res) == sorted(EVERY + ("vendi_reference",))
    fs.given_paths(s.space, [d["gen"], npz["ref"]], save_features=npz["gen"])
    assert s.built == 2                                                    # one directory: exactly one
    fs.given_paths(s.space, [d["train"], npz["ref"]], save_features=npz["train"])
    s.built = 0
    # the file holds side one's rows, mu, sigma and the tag
    mu, sigma = fs.statistics(torch.from_numpy(s.rows["ref"]).cuda())
    with np.load(npz["ref"]) as f:
        assert sorted(f.files) == ["features", "mu", "network", "sigma"] and str(f["network"]) == NETWORK
        assert f["features"].dtype == np.float32 and np.array_equal(f["features"], s.rows["ref"])
        assert np.array_equal(f["mu"], mu) and np.array_equal(f["sigma"], sigma) and f["sigma"].shape == (WIDTH, WIDTH)
    # in place of the directories: the same dict; three feature files build no tower at all
    for paths, train in (([npz["ref"], d["gen"]], d["train"]), ([npz["ref"], npz["gen"]], npz["train"])):
        before = s.built
        again = fs.given_paths(s.space, paths, train=train, want=EVERY)
        assert _same(again, res), (paths, again, res)
        assert s.built - before == (0 if train.endswith(".npz") else 1)


def test_each_number_is_the_direct_call_and_nothing_else_is_there(stand_in, tmp_path):
    s, d = stand_in, stand_in.dirs
    ref, gen, train = (torch.from_numpy(s.rows[k]).cuda() for k in ("ref", "gen", "train"))
    (m1, s1), (m2, s2) = fs.statistics(ref), fs.statistics(gen)
    near = authenticity.nearest_train(train, gen)
    direct = dict(fd=float(fid_score.calculate_frechet_distance(m1, s1, m2, s2)),
                  kd=kid.kid_from_features(ref, gen, subsets=100, subset_size=1000),
                  prdc=prdc.prdc_from_features(ref, gen, nearest_k=3),
                  authpct=authenticity.authpct_from_counts(near["authentic"].sum(), len(near["authentic"])),
                  vendi=vendi.vendi_from_features(gen), vendi_reference=vendi.vendi_from_features(ref),
                  fd_infinity=fd_infinity.fd_infinity_from_features(ref, gen, seed=4))
    assert direct["fd"] == fs.frechet_from_features(s.rows["ref"], s.rows["gen"])
    for name in EVERY:
        got = fs.given_paths(s.space, [d["ref"], d["gen"]], train=d["train"] if name == "authpct" else None, want=(name,), prdc_k=3,
                             fd_infinity_seed=4)
        want = {k: direct[k] for k in ((name, "vendi_reference") if name == "vendi" else (name,))}
        print(name, got)
        assert _same(got, want), (name, got, want)
    # the nearest-train table alone: no number, the CSV of the same 1-NN pass
    out = str(tmp_path / "near.csv")
    assert fs.given_paths(s.space, [d["ref"], d["gen"]], train=d["train"], want=(), nearest_train=out) == {}
    with open(out, newline="") as f:
        table = list(csv.reader(f))
    assert tuple(table[0]) == fs.NEAREST_TRAIN_COLUMNS and len(table) == 1 + COUNTS["gen"]
    files = {k: img_data.get_filenames(d[k]) for k in ("gen", "train")}
    assert table[1:] == [[str(g), str(int(near["idx"][g])), repr(float(near["d2_gen"][g])), str(int(near["authentic"][g])), files["gen"][g],
                          files["train"][int(near["idx"][g])]] for g in range(COUNTS["gen"])]
    with pytest.raises(ValueError, match="need the training set"):
        fs.given_paths(s.space, [d["ref"], d["gen"]], want=("authpct",))


def test_statistics_run_only_where_they_are_needed(stand_in, tmp_path, monkeypatch):
    s, d = stand_in, stand_in.dirs
    calls = []
    real = fs.statistics
    monkeypatch.setattr(fs, "statistics", lambda feats: (calls.append(feats.shape[0]), real(feats))[1])
    assert sorted(fs.given_paths(s.space, [d["ref"], d["gen"]], train=d["train"], want=("kd", "authpct"))) == ["authpct", "kd"]
    assert calls == []                                                     # no Frechet distance, no file: no statistics kernel
    fs.given_paths(s.space, [d["ref"], d["gen"]], save_features=str(tmp_path / "ref.npz"), want=("kd",))
    assert calls == [COUNTS["ref"]]                                        # the file needs side one's
    del calls[:]
    fs.given_paths(s.space, [d["ref"], d["gen"]], train=d["train"], want=("fd", "authpct"))
    assert calls == [COUNTS["ref"], COUNTS["gen"]]                         # both sides', never the training set's
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(RuntimeError, match="no images under"):
        fs.given_paths(s.space, [str(empty), d["gen"]])
