"""feature_space.py without a GPU and without the library: the feature files' refusals in the three spaces, the three parsers against
the option tables of the commit before the runner existed, the result lines, --saved_file, and the order of the refusals."""
import argparse

import numpy as np
import pytest
import torch

from tise_toolbox_amd import _lib, cmmd, dist as tdist, fd_dinov2, fd_swav, feature_space as fs, weights

# tool -> (its space, its own load_features_npz / check_feature_file wrappers bound to that space)
SPACES = {
    "cmmd": (lambda: cmmd.space("ViT-L/14@336"), lambda p: cmmd.load_features_npz(p, "ViT-L/14@336"), None),
    "fd_dinov2": (lambda: fd_dinov2.space("vits14"), lambda p: fd_dinov2.load_features_npz(p, "vits14"),
                  lambda p: fd_dinov2.check_feature_file(p, "vits14")),
    "fd_swav": (fd_swav.space, fd_swav.load_features_npz, fd_swav.check_feature_file),
}
WANT = {"cmmd": ("clip-vit-l14-336", 768), "fd_dinov2": ("dinov2-vits14", 384), "fd_swav": ("swav-resnet50", 2048)}


def _save(path, network=None, features=None):
    arrays = dict(mu=np.zeros(2), sigma=np.eye(2))
    if network is not None:
        arrays["network"] = np.asarray(network)
    if features is not None:
        arrays["features"] = features
    np.savez(path, **arrays)
    return str(path)


@pytest.mark.parametrize("tool", sorted(SPACES))
def test_space_records(tool):
    space = SPACES[tool][0]()
    assert (space.tool, space.network, space.dims) == (tool,) + WANT[tool]
    assert callable(space.build_tower) and callable(space.embed_dir)


@pytest.mark.parametrize("tool", sorted(SPACES))
def test_bad_feature_files_are_refused(tool, tmp_path, monkeypatch):
    make, load, check = SPACES[tool]
    space = make()
    rows = np.ones((3, space.dims), np.float32)
    good = _save(tmp_path / "good.npz", space.network, rows)
    untagged = _save(tmp_path / "untagged.npz", None, rows)
    foreign = _save(tmp_path / "foreign.npz", "inception-2015", rows)
    rowless = _save(tmp_path / "rowless.npz", space.network)
    narrow = _save(tmp_path / "narrow.npz", space.network, rows[:, :-1])
    # (file, what its refusal says beside the file's own name)
    cases = ((untagged, ["no network tag", space.network, f"{tool} --save-features"]),
             (foreign, ["'inception-2015'", f"--network {space.network}"]),
             (rowless, ["no 'features' array", f"{tool} --save-features"]),
             (narrow, [f"features of shape (3, {space.dims - 1})", f"expected (n, {space.dims})"]))
    for path, said in cases:
        for fn in (lambda p: fs.load_features_npz(p, space.network, space.dims, space.tool), load):
            with pytest.raises(RuntimeError) as e:
                fn(path)
            assert all(s in str(e.value) for s in [path] + said), (path, str(e.value))
    got = load(good)
    assert got[0].dtype == np.float32 and np.array_equal(got[0], rows) and got[1].shape == (2,) and got[2].shape == (2, 2)
    # the tag alone: the first two are refused with the same words, the rows of the others are not looked at -- nor read
    read = []
    real = np.lib.npyio.NpzFile.__getitem__
    monkeypatch.setattr(np.lib.npyio.NpzFile, "__getitem__", lambda self, key: (read.append(key), real(self, key))[1])
    for fn in (lambda p: fs.check_feature_file(p, space.network, space.tool),) + ((check,) if check else ()):
        for path, said in cases[:2]:
            with pytest.raises(RuntimeError) as e:
                fn(path)
            assert all(s in str(e.value) for s in [path] + said)
        for path in (good, rowless, narrow):
            fn(path)
    assert set(read) == {"network"}


# The options of the three CLIs, in --help's order, with their defaults: copied from the parsers of the commit before feature_space.py.
OPTIONS = {
    "cmmd": [("--tower", "ViT-B/32"), ("--path1", None), ("--path2", None), ("--batch-size", 50), ("--weights", None),
             ("--synthetic-weights", False), ("--seed", 0), ("--clip-fid", False), ("--unbiased", False), ("--save-features", ""),
             ("--saved_file", ""), ("--png-feed", "ring"), ("--num-workers", 0), ("--gpu", "0")],
    "fd_dinov2": [("--path1", None), ("--path2", None), ("--arch", "vitl14"), ("--kd", False), ("--prdc", False), ("--prdc-k", 5),
                  ("--train", ""), ("--authpct", False), ("--nearest-train", ""), ("--vendi", False), ("--fd-infinity", False),
                  ("--fd-infinity-seed", 0), ("--weights", None), ("--synthetic-weights", False), ("--seed", 0), ("--batch-size", 50),
                  ("--save-features", ""), ("--saved_file", ""), ("--png-feed", "ring"), ("--num-workers", 0), ("--gpu", "0")],
    "fd_swav": [("--path1", None), ("--path2", None), ("--kd", False), ("--prdc", False), ("--prdc-k", 5), ("--weights", None),
                ("--synthetic-weights", False), ("--seed", 0), ("--batch-size", 50), ("--save-features", ""), ("--saved_file", ""),
                ("--png-feed", "ring"), ("--num-workers", 0), ("--gpu_id", "0")],
}
MODULES = {"cmmd": cmmd, "fd_dinov2": fd_dinov2, "fd_swav": fd_swav}


@pytest.mark.parametrize("tool", sorted(MODULES))
def test_parsers_keep_their_options_and_defaults(tool, monkeypatch, capsys):
    seen = []
    real = argparse.ArgumentParser.parse_args
    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", lambda self, argv=None: (seen.append(self), real(self, argv))[1])
    MODULES[tool].parse_args(["--path1", "A", "--path2", "B"])
    actions = [a for a in seen[0]._actions if a.dest != "help"]
    assert [(a.option_strings, a.default) for a in actions] == [([flag], default) for flag, default in OPTIONS[tool]]
    by_flag = {a.option_strings[0]: a for a in actions}
    assert by_flag["--path1"].required and by_flag["--path2"].required and by_flag["--png-feed"].choices == ["ring", "dataloader"]
    assert by_flag["--save-features"].help == ("write --path1's embeddings (fp32, un-normalised), mu, sigma and the network tag to this .npz"
                                               if tool == "cmmd" else
                                               "write --path1's feature rows (fp32), mu, sigma and the network tag to this .npz")
    refused = [["--path1", "A"], ["--path1", "A", "--path2", "B", "--png-feed", "pipe"], ["--path1", "A", "--path2", "B", "--no-such"]]
    if tool != "cmmd":                                        # cmmd leaves --weights with --synthetic-weights to weights.resolve
        refused += [["--path1", "A", "--path2", "B"] + extra for extra in
                    (["--weights", "w", "--synthetic-weights"], ["--prdc", "--prdc-k", "0"], ["--prdc", "--prdc-k", "17"])]
    for argv in refused:
        with pytest.raises(SystemExit) as e:
            MODULES[tool].parse_args(argv)
        assert e.value.code == 2, argv
    capsys.readouterr()
    if tool == "cmmd":
        args = cmmd.parse_args(["--path1", "A", "--path2", "B", "--weights", "w", "--synthetic-weights"])
        assert args.weights == "w" and args.synthetic_weights
        with pytest.raises(RuntimeError, match="mutually exclusive"):
            weights.resolve(args.weights, args.synthetic_weights, "clip")
    else:
        assert MODULES[tool].parse_args(["--path1", "A", "--path2", "B", "--prdc-k", "17"]).prdc_k == 17      # only --prdc looks at it


FULL = dict(fd=1.5, kd=(0.25, 0.125), prdc=dict(precision=0.5, recall=0.25, density=2.0, coverage=1.0), authpct=62.5, vendi=3.25,
            vendi_reference=4.5, fd_infinity=dict(fd_infinity=1.25, slope=9.0))


@pytest.mark.parametrize("tag", ["", weights.SYNTHETIC_TAG])
def test_result_lines_are_the_strings_they_were(tag):
    assert fs.result_lines(FULL, "SwAV", tag) == [
        f"FD-SwAV: 1.5{tag}", f"KD-SwAV: 0.25 +- 0.125{tag}", f"Precision-SwAV: 0.5{tag}", f"Recall-SwAV: 0.25{tag}",
        f"Density-SwAV: 2.0{tag}", f"Coverage-SwAV: 1.0{tag}", f"AuthPct-SwAV: 62.5{tag}", f"Vendi-SwAV: 3.25{tag}",
        f"Vendi-SwAV reference: 4.5{tag}", f"FD-infinity-SwAV: 1.25{tag}"]
    dino = [f"FD-DINOv2 (vits14): 1.5{tag}", f"KD-DINOv2 (vits14): 0.25 +- 0.125{tag}", f"Precision-DINOv2 (vits14): 0.5{tag}",
            f"Recall-DINOv2 (vits14): 0.25{tag}", f"Density-DINOv2 (vits14): 2.0{tag}", f"Coverage-DINOv2 (vits14): 1.0{tag}",
            f"AuthPct-DINOv2 (vits14): 62.5{tag}", f"Vendi-DINOv2 (vits14): 3.25{tag}", f"Vendi-DINOv2 reference (vits14): 4.5{tag}",
            f"FD-infinity-DINOv2 (vits14): 1.25{tag}"]
    assert fs.result_lines(FULL, "DINOv2 (vits14)", tag) == dino == fd_dinov2.result_lines(FULL, "vits14", tag)
    plain = dict(fd=2.0, kd=None, prdc=None)
    assert fs.result_lines(plain, "SwAV", tag) == [f"FD-SwAV: 2.0{tag}"] == fd_swav.result_lines(plain, tag)
    assert fs.result_lines(dict(fd=2.0), "DINOv2 (vits14)", tag) == [f"FD-DINOv2 (vits14): 2.0{tag}"]
    assert fs.fd_result(dict(vendi=1.0, fd=2.0)) == dict(fd=2.0, kd=None, prdc=None, vendi=1.0)


def test_write_lines(tmp_path, capsys, monkeypatch):
    out = tmp_path / "out.txt"
    tdist.write_lines(["a: 1", "b: 2"], str(out))
    assert out.read_bytes() == b"a: 1\nb: 2" and capsys.readouterr().out == "a: 1\nb: 2\n"          # no trailing newline in the file
    tdist.write_lines(["c: 3"])
    assert capsys.readouterr().out == "c: 3\n" and sorted(p.name for p in tmp_path.iterdir()) == ["out.txt"]
    monkeypatch.setattr(tdist, "is_main", lambda: False)                  # another rank: no file, no line
    other = tmp_path / "other.txt"
    tdist.write_lines(["d: 4"], str(other))
    assert capsys.readouterr().out == "" and not other.exists()


RUNS = {
    "cmmd": [cmmd.calculate_cmmd_given_paths, cmmd.calculate_clip_fid_given_paths],
    "fd_dinov2": [fd_dinov2.calculate_fd_dinov2_given_paths],
    "fd_swav": [fd_swav.calculate_fd_swav_given_paths],
}


@pytest.mark.parametrize("tool", sorted(RUNS))
def test_no_gpu_is_a_library_error_after_the_refusals_that_need_none(tool, tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    d1, d2 = tmp_path / "a", tmp_path / "b"
    d1.mkdir(), d2.mkdir()
    foreign = _save(tmp_path / "foreign.npz", "inception-2015", np.ones((3, 4), np.float32))
    main = MODULES[tool].main
    with pytest.raises(_lib.TiseLibraryError, match=f"{tool} needs an MI355X"):
        main(["--path1", str(d1), "--path2", str(d2), "--synthetic-weights"])
    for argv in (["--path1", foreign, "--path2", str(d2)], ["--path1", str(d1), "--path2", foreign]):
        with pytest.raises(RuntimeError, match="statistics of network 'inception-2015'") as e:
            main(argv + ["--synthetic-weights"])
        assert not isinstance(e.value, _lib.TiseLibraryError)
    for run in RUNS[tool]:
        with pytest.raises(RuntimeError, match="Invalid path"):
            run([str(d1), str(tmp_path / "none")])
        with pytest.raises(_lib.TiseLibraryError, match=f"{tool} needs an MI355X"):
            run([str(d1), str(d2)])
        for paths in ([foreign, str(d2)], [str(d1), foreign]):
            with pytest.raises(RuntimeError, match="statistics of network 'inception-2015'") as e:
                run(paths)
            assert not isinstance(e.value, _lib.TiseLibraryError)
    if tool == "fd_dinov2":                                               # the training set's file is looked at as well
        with pytest.raises(RuntimeError, match="statistics of network 'inception-2015'"):
            main(["--path1", str(d1), "--path2", str(d2), "--train", foreign, "--authpct", "--synthetic-weights"])
        with pytest.raises(RuntimeError, match="statistics of network 'inception-2015'"):
            fd_dinov2.calculate_fd_dinov2_given_paths([str(d1), str(d2)], train=foreign, authpct=True)
