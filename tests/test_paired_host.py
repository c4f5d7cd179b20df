"""CPU: the numpy fp64 restatement of PSNR / SSIM / MS-SSIM (tests/_ssim_ref.py) against an independent scipy route and against
closed forms, and the host logic of tise_toolbox_amd.paired (stem pairing, the --self-pairs draw, the {n, sum, sum of squares}
merge, the result lines and the CSV)."""
import os

import numpy as np
import pytest

from tests import _ssim_ref as ref


def _noise_pair(h, w, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, size=(h, w, 3)).astype(np.uint8)
    y = np.clip(x.astype(np.int64) + rng.integers(-40, 41, size=x.shape), 0, 255).astype(np.uint8)
    return x, y


def _scipy_means(x, y):
    """The same definitions through scipy.ndimage.gaussian_filter: sigma 1.5 truncated at 3.5 sigma is radius 5, the same 11
    taps; the border modes only touch the 5 outer rows and columns, which the valid crop removes."""
    from scipy.ndimage import gaussian_filter

    def blur(z):
        return np.stack([gaussian_filter(z[:, :, c], 1.5, truncate=3.5)[5:-5, 5:-5] for c in range(3)], axis=2)
    x, y = x.astype(np.float64), y.astype(np.float64)
    mx, my = blur(x), blur(y)
    sxx, syy, sxy = blur(x * x) - mx * mx, blur(y * y) - my * my, blur(x * y) - mx * my
    cs = (2 * sxy + ref.C2) / (sxx + syy + ref.C2)
    s = (2 * mx * my + ref.C1) / (mx * mx + my * my + ref.C1) * cs
    return np.stack([s.mean(axis=(0, 1)), cs.mean(axis=(0, 1))], axis=1)


@pytest.mark.parametrize("shape", [(11, 11), (11, 12), (12, 11), (37, 53), (64, 64), (139, 203), (256, 256)], ids=str)
def test_restatement_agrees_with_the_scipy_route(shape):
    worst = 0.0
    for seed, (x, y) in enumerate((_noise_pair(*shape, 3), ref.smooth_pair(*shape, 4, 1), ref.smooth_pair(*shape, 25, 2))):
        worst = max(worst, float(np.max(np.abs(ref.ssim_means(x, y) - _scipy_means(x, y)))))
    assert worst <= 1e-13, worst


def test_window():
    g = ref.window()
    assert g.shape == (11,) and g.sum() == 1.0 and np.array_equal(g, g[::-1]) and np.argmax(g) == 5
    assert abs(g[4] / g[5] - np.exp(-1.0 / 4.5)) <= 1e-15
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tise_toolbox_amd", "csrc", "ssim.hip")).read()
    for v in g[:6]:                                                       # the kernel's literals are these doubles
        assert repr(float(v)) in src, v


def test_identical_images_give_exactly_one():
    for shape, seed in (((11, 11), 0), ((40, 57), 1), ((176, 176), 2), ((177, 191), 3)):
        x, _ = ref.smooth_pair(*shape, 4, seed)
        assert np.array_equal(ref.ssim_means(x, x), np.ones((3, 2)))
        assert ref.ssim(x, x) == 1.0 and ref.psnr(x, x) == float("inf")
        if min(shape) >= 176:
            assert ref.ms_ssim(x, x) == 1.0


def test_constant_images_closed_form():
    for a, b in ((0, 255), (10, 200), (255, 255), (128, 127), (0, 0)):
        x = np.full((20, 31, 3), a, dtype=np.uint8)
        y = np.full((20, 31, 3), b, dtype=np.uint8)
        want = (2.0 * a * b + ref.C1) / (a * a + b * b + ref.C1)
        assert abs(ref.ssim(x, y) - want) <= 1e-12, (a, b)
        assert np.max(np.abs(ref.ssim_means(x, y)[:, 1] - 1.0)) <= 1e-12       # no variance, no covariance: cs = C2 / C2


def test_psnr_closed_form():
    x, _ = ref.smooth_pair(13, 17, 4, 0)
    y = x.copy()
    y[5, 6, 1] = x[5, 6, 1] + 1 if x[5, 6, 1] < 255 else 254
    assert ref.sse(x, y) == 1
    want = 10.0 * np.log10(255.0 ** 2 * 3 * 13 * 17)
    assert abs(ref.psnr(x, y) - want) <= 1e-12 * want
    from tise_toolbox_amd import paired
    got = paired.psnr_from_sse(np.array([1, 0, 255 * 255 * 3 * 13 * 17]), np.array([13] * 3), np.array([17] * 3))
    assert abs(got[0] - want) <= 1e-12 * want and np.isposinf(got[1]) and abs(got[2]) <= 1e-12


def test_pooling_drops_the_last_odd_row_and_column():
    z = np.arange(5 * 7 * 3, dtype=np.float64).reshape(5, 7, 3)
    p = ref.pool2x2(z)
    assert p.shape == (2, 3, 3)
    assert p[1, 2, 0] == (z[2, 4, 0] + z[2, 5, 0] + z[3, 4, 0] + z[3, 5, 0]) / 4
    assert np.array_equal(p, ref.pool2x2(z[:4, :6]))


def test_ms_ssim_clamp_and_weights():
    from tise_toolbox_amd import paired
    assert abs(ref.MS_WEIGHTS.sum() - 1.0001) <= 1e-12 and np.array_equal(ref.MS_WEIGHTS, paired.MS_WEIGHTS)
    m = np.full((5, 3), 0.5)
    assert abs(ref.ms_from_means(m) - 0.5 ** 1.0001) <= 1e-15
    m[2, 1] = -0.2                                                        # a negative scale mean is clamped: that channel gives 0
    assert abs(ref.ms_from_means(m) - 2.0 / 3.0 * 0.5 ** 1.0001) <= 1e-15
    x, y = ref.smooth_pair(177, 191, 25, 9)
    sm = ref.ms_scale_means(x, y)
    assert abs(paired.ms_from_scale_means(sm[None])[0] - ref.ms_ssim(x, y)) <= 1e-15
    assert 0.0 < ref.ms_ssim(x, y) < 1.0


def test_small_images_are_refused_with_the_reason():
    x = np.zeros((10, 40, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match=">= 11"):
        ref.ssim(x, x)
    with pytest.raises(ValueError, match=">= 11"):
        ref.ssim(x.transpose(1, 0, 2), x.transpose(1, 0, 2))
    z = np.zeros((175, 300, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match=">= 176"):
        ref.ms_ssim(z, z)
    assert ref.ms_ssim(np.zeros((176, 176, 3)), np.zeros((176, 176, 3))) == 1.0


def _touch(path):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    open(path, "wb").close()


def test_pairing_by_stem(tmp_path):
    from tise_toolbox_amd import paired
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    for rel in ("z.png", "sub/b.png", "sub/a.jpg", "10.png", "9.png"):
        _touch(os.path.join(a, rel))
    for rel in ("z.jpg", "sub/b.jpeg", "sub/a.png", "10.png", "9.PNG", "notes.txt"):
        _touch(os.path.join(b, rel))
    f1, f2 = paired.pair_files(a, b)
    stems = ["10", "9", "sub/a", "sub/b", "z"]                             # the sorted stems
    assert [os.path.splitext(os.path.relpath(f, a))[0] for f in f1] == stems
    assert [os.path.splitext(os.path.relpath(f, b))[0] for f in f2] == stems
    assert f2[0].endswith("10.png") and f2[1].endswith("9.PNG") and f2[3].endswith(os.path.join("sub", "b.jpeg"))
    assert paired.list_files(a) == f1
    _touch(os.path.join(b, "sub", "only_here.png"))
    with pytest.raises(RuntimeError, match="only_here.png"):
        paired.pair_files(a, b)
    with pytest.raises(RuntimeError, match="only_here.png"):
        paired.pair_files(b, a)
    os.remove(os.path.join(b, "sub", "only_here.png"))
    _touch(os.path.join(a, "z.jpg"))                                       # z.png and z.jpg on one side
    with pytest.raises(RuntimeError, match="two images named 'z'"):
        paired.pair_files(a, b)
    with pytest.raises(RuntimeError, match="Invalid path"):
        paired.pair_files(str(tmp_path / "nowhere"), b)


def test_self_pairs_draw():
    from tise_toolbox_amd import paired
    p = paired.draw_self_pairs(7, 1000, seed=3)
    assert p.shape == (1000, 2) and p.dtype == np.int64
    assert np.all(p[:, 0] != p[:, 1]) and p.min() == 0 and p.max() == 6
    assert np.array_equal(p, paired.draw_self_pairs(7, 1000, seed=3))
    assert not np.array_equal(p, paired.draw_self_pairs(7, 1000, seed=4))
    assert len({(int(i), int(j)) for i, j in p}) == 42                     # every ordered pair of 7 turns up in 1000 draws
    two = paired.draw_self_pairs(2, 50, seed=0)
    assert np.all(two.sum(axis=1) == 1)
    with pytest.raises(RuntimeError, match="at least two"):
        paired.draw_self_pairs(1, 5)
    with pytest.raises(RuntimeError, match="positive"):
        paired.draw_self_pairs(5, 0)


def test_sums_merge_across_shards():
    from tise_toolbox_amd import paired
    rng = np.random.default_rng(0)
    full = {"psnr": rng.uniform(20, 40, 11), "ssim": rng.uniform(0.3, 1, 11), "ms_ssim": rng.uniform(0.3, 1, 11)}
    cut = lambda lo, hi: {k: v[lo:hi] for k, v in full.items()}
    merged = paired.metric_sums(cut(0, 4)) + paired.metric_sums(cut(4, 11)) + paired.metric_sums(cut(11, 11))
    res = paired.result_from_sums(merged)
    assert res["n"] == 11 and res["identical"] == 0
    one = paired.result_from_sums(paired.metric_sums(full))
    for k, v in full.items():
        assert abs(res[k] - v.mean()) <= 1e-13 * v.mean() and abs(res[k + "_std"] - v.std()) <= 1e-11
        assert abs(res[k] - one[k]) <= 1e-13 * v.mean() and abs(res[k + "_std"] - one[k + "_std"]) <= 1e-11
    assert paired.result_lines(res) == [f"PSNR: {res['psnr']} +- {res['psnr_std']}", f"SSIM: {res['ssim']} +- {res['ssim_std']}",
                                        f"MS-SSIM: {res['ms_ssim']} +- {res['ms_ssim_std']}"]
    # identical pairs: counted, and the PSNR mean is inf as numpy's; no MS-SSIM, no MS-SSIM line
    part = {"psnr": np.array([30.0, np.inf, np.inf]), "ssim": np.array([0.5, 1.0, 1.0])}
    res = paired.result_from_sums(paired.metric_sums(part) + paired.metric_sums({"psnr": np.array([31.0]), "ssim": np.array([0.7])}))
    assert res["n"] == 4 and res["identical"] == 2 and res["psnr"] == float("inf") and np.isnan(res["psnr_std"])
    assert "ms_ssim" not in res and abs(res["ssim"] - 0.8) <= 1e-15
    lines = paired.result_lines(res)
    assert lines[0] == "PSNR: inf +- nan" and lines[-1] == "identical pairs: 2" and len(lines) == 3
    with pytest.raises(RuntimeError, match="at least one pair"):
        paired.result_from_sums(paired.metric_sums({}))


def test_per_pair_csv():
    from tise_toolbox_amd import paired
    res = {"h": np.array([11, 12]), "w": np.array([13, 14]), "psnr": np.array([30.5, np.inf]), "ssim": np.array([0.25, 1.0])}
    text = paired.per_pair_csv(["a/x.png", "a/y.png"], ["b/x.jpg", "b/y.jpg"], res)
    assert text == "pair,file1,file2,h,w,psnr,ssim,ms_ssim\n0,a/x.png,b/x.jpg,11,13,30.5,0.25,\n1,a/y.png,b/y.jpg,12,14,inf,1.0,\n"
    res["ms_ssim"] = np.array([0.125, 1.0])
    assert paired.per_pair_csv(["p"], ["q"], res).split("\n")[1] == "0,p,q,11,13,30.5,0.25,0.125"


def test_cli_arguments():
    from tise_toolbox_amd import paired
    a = paired.parse_args(["--path1", "A", "--path2", "B"])
    assert (a.ms_ssim, a.self_pairs, a.seed, a.batch_size, a.png_feed, a.jpeg_feed, a.num_workers, a.gpu_id) == (False, 0, 0, 50, "ring", None, 0, "0")
    a = paired.parse_args(["--path1", "A", "--self-pairs", "9", "--seed", "4", "--ms-ssim"])
    assert a.self_pairs == 9 and a.seed == 4 and a.ms_ssim and a.path2 is None
    for argv in (["--path1", "A"], ["--path1", "A", "--path2", "B", "--self-pairs", "3"], ["--path2", "B"]):
        with pytest.raises(SystemExit):
            paired.parse_args(argv)
    from tise_toolbox_amd import feeds
    assert feeds.PAIRED.drop_last is False and feeds.PAIRED.kinds == feeds.IS.kinds


# the options every pair-metric CLI has: flag, default, help (None: no help text; a dict: the wording differs by tool, which
# --help has always shown -- paired prints several result lines and has no stand-in parameters to seed)
_SEED_MODEL = "seed of the --self-pairs draw and of the --synthetic-weights parameters"
COMMON_OPTIONS = {
    "path1": ("--path1", None, "folder of originals (with --self-pairs: the one folder)"),
    "path2": ("--path2", None, "folder of reconstructions, paired by relative path without extension"),
    "self_pairs": ("--self-pairs", 0, "N random pairs (i != j) of --path1 instead of two folders"),
    "seed": ("--seed", 0, {"paired": "seed of the --self-pairs draw", "lpips": _SEED_MODEL, "dists": _SEED_MODEL}),
    "per_pair": ("--per-pair", "", "write one CSV line per pair here"),
    "saved_file": ("--saved_file", "", {"paired": "write the result lines here as well", "lpips": "write the result line here as well",
                                        "dists": "write the result line here as well"}),
    "batch_size": ("--batch-size", 50, None),
    "png_feed": ("--png-feed", "ring", None),
    "jpeg_feed": ("--jpeg-feed", None, None),
    "num_workers": ("--num-workers", 0, "image decode processes per side (0 = auto)"),
    "gpu_id": ("--gpu_id", "0", None),
}
OWN_OPTIONS = {"paired": {"ms_ssim"}, "lpips": {"weights", "lpips_weights", "synthetic_weights"},
               "dists": {"weights", "dists_weights", "synthetic_weights"}}


def test_the_three_pair_parsers_agree_on_the_common_options(monkeypatch, capsys):
    import argparse
    from tise_toolbox_amd import dists, lpips, paired
    seen = []
    real = argparse.ArgumentParser.parse_args
    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", lambda self, argv=None: (seen.append(self), real(self, argv))[1])
    for name, mod in (("paired", paired), ("lpips", lpips), ("dists", dists)):
        del seen[:]
        mod.parse_args(["--path1", "A", "--path2", "B"])
        actions = {a.dest: a for a in seen[0]._actions if a.dest != "help"}
        assert set(actions) == set(COMMON_OPTIONS) | OWN_OPTIONS[name], name
        for dest, (flag, default, text) in COMMON_OPTIONS.items():
            a = actions[dest]
            want = text[name] if isinstance(text, dict) else text
            assert (a.option_strings, a.default, a.help) == ([flag], default, want), (name, dest)
        assert actions["path1"].required and actions["png_feed"].choices == ["ring", "dataloader"]
        assert actions["jpeg_feed"].choices == ["native", "pillow"]
        for argv, said in ((["--path1", "A", "--self-pairs", "3", "--path2", "X"], "--self-pairs takes --path1 only"),
                           (["--path1", "A"], "give --path2, or --self-pairs N")):
            with pytest.raises(SystemExit) as e:
                mod.parse_args(argv)
            assert e.value.code == 2 and capsys.readouterr().err.rstrip().endswith("error: " + said), (name, argv)
