"""CPU: the host side of LPIPS -- the input table, the two parameter loaders, the host mirror of the row-window launcher's
reciprocal check, closed forms of the torch module, the size refusals and the CLI surface."""
import os

import numpy as np
import pytest
import torch

from tise_toolbox_amd import conv_split, lpips, lpips_model, paired


def test_input_table_is_numpy_fp32():
    t = lpips_model.input_table()
    assert t.dtype == torch.float32 and tuple(t.shape) == (3, 256) and t.is_contiguous()
    shift, scale = (-0.030, -0.088, -0.188), (0.458, 0.448, 0.450)
    for c in range(3):
        for b in (0, 1, 127, 128, 254, 255):
            x = np.float32(b) / np.float32(127.5) - np.float32(1.0)
            want = (x - np.float32(shift[c])) / np.float32(scale[c])
            assert want.dtype == np.float32 and t[c, b].item() == float(want), (c, b)
    b = np.arange(256, dtype=np.float32)
    want = ((b / np.float32(127.5) - np.float32(1))[None] - np.float32(shift)[:, None]) / np.float32(scale)[:, None]
    assert want.dtype == np.float32 and np.array_equal(t.numpy(), want)
    assert float(t.abs().max()) < 3.0                                          # far inside the fp16 range of the split format


def _seeded_files(tmp_path, seed=3):
    g = torch.Generator().manual_seed(seed)
    trunk = {}
    for idx, (ci, co) in zip(lpips_model.CONV_INDICES, lpips_model.CONV_CHANNELS):
        trunk[f"features.{idx}.weight"] = torch.randn((co, ci, 3, 3), generator=g) * 0.05
        trunk[f"features.{idx}.bias"] = torch.randn((co,), generator=g) * 0.05
    trunk["classifier.0.weight"] = torch.zeros(2, 2)                           # torchvision's file has the classifier too: ignored
    lins = {f"lin{k}.model.1.weight": torch.rand((1, c, 1, 1), generator=g) for k, c in enumerate(lpips_model.TAP_CHANNELS)}
    p1, p2 = os.path.join(tmp_path, "vgg16.pth"), os.path.join(tmp_path, "lin_vgg.pth")
    torch.save(trunk, p1)
    torch.save(lins, p2)
    return trunk, lins, p1, p2


def test_loaders_round_trip_and_refusals(tmp_path):
    trunk, lins, p1, p2 = _seeded_files(str(tmp_path))
    m = lpips_model.build_model(p1, p2)
    assert not m.synthetic
    for k, idx in enumerate(lpips_model.CONV_INDICES):
        assert torch.equal(m.convs[k].weight, trunk[f"features.{idx}.weight"]) and torch.equal(m.convs[k].bias, trunk[f"features.{idx}.bias"])
    for k in range(5):
        assert torch.equal(m.lins[k], lins[f"lin{k}.model.1.weight"].reshape(-1))
    # another network's shapes: refused, naming both
    alex = dict(trunk)
    alex["features.0.weight"] = torch.zeros(64, 3, 11, 11)
    pa = os.path.join(str(tmp_path), "alexnet.pth")
    torch.save(alex, pa)
    with pytest.raises(ValueError, match=r"features\.0\.weight is \(64, 3, 11, 11\), VGG-16 has \(64, 3, 3, 3\).*AlexNet"):
        lpips_model.LpipsVGG16().load_trunk(pa)
    vgg11 = {k: v for k, v in trunk.items() if not k.startswith("features.2.")}
    with pytest.raises(ValueError, match=r"features\.2\.weight is missing, VGG-16 has \(64, 64, 3, 3\).*another VGG variant"):
        lpips_model.LpipsVGG16().load_trunk(vgg11)
    alex_lin = {f"lin{k}.model.1.weight": torch.zeros(1, c, 1, 1) for k, c in enumerate((64, 192, 384, 256, 256))}
    pl = os.path.join(str(tmp_path), "lin_alex.pth")
    torch.save(alex_lin, pl)
    with pytest.raises(ValueError, match=r"\[64, 192, 384, 256, 256\] channels; VGG-16 has .*\[64, 128, 256, 512, 512\].*AlexNet"):
        lpips_model.LpipsVGG16().load_lins(pl)
    sq = {f"lin{k}.model.1.weight": torch.zeros(1, c, 1, 1) for k, c in enumerate((64, 128, 256, 384, 384, 512, 512))}
    with pytest.raises(ValueError, match="SqueezeNet"):
        lpips_model.LpipsVGG16().load_lins(sq)
    # the other two networks are refused with the reason; neither file alone is enough; synthetic excludes files
    for net in ("alex", "squeeze"):
        with pytest.raises(ValueError, match="only 'vgg'"):
            lpips_model.LpipsVGG16(net)
    assert set(lpips_model.CONFIGS) == {"vgg"}
    with pytest.raises(RuntimeError, match="two files"):
        lpips_model.build_model(p1, None)
    with pytest.raises(RuntimeError, match="mutually exclusive"):
        lpips_model.build_model(p1, p2, synthetic=True)


def test_synthetic_parameters_are_seeded_scaled_and_non_negative():
    a, b, c = (lpips_model.LpipsVGG16().init_synthetic(s) for s in (0, 0, 1))
    assert a.synthetic
    for p, q, r in zip(a.parameters(), b.parameters(), c.parameters()):
        assert torch.equal(p, q) and not torch.equal(p, r)
    for conv in a.convs:
        want = (2.0 / (conv.in_channels * 9)) ** 0.5
        assert 0.8 * want < float(conv.weight.std()) < 1.2 * want
    assert all(float(lin.min()) >= 0.0 for lin in a.lins)


def _brute(ow, kw):
    for w in (ow, ow + kw - 1):
        inv = 65536 // w + 1
        for u in range(512 + ow):
            if ((u * inv) & 0xffffffff) >> 16 != u // w:
                return False
    return True


def test_rowwin_divides_is_the_launchers_check():
    for kw in range(2, 9):
        for ow in range(1, 1101):
            assert conv_split.rowwin_divides(ow, kw) == _brute(ow, kw), (ow, kw)
    assert all(conv_split.rowwin_divides(ow, 3) for ow in range(1, 124)) and conv_split.rowwin_divides(224, 3)
    assert not any(conv_split.rowwin_divides(ow, 3) for ow in (124, 125, 126, 127, 128, 256, 299, 384, 512, 1024))
    assert sum(not conv_split.rowwin_divides(ow, 3) for ow in range(1, 1025)) == 857
    assert not conv_split.rowwin_divides(0, 3)


def test_module_closed_forms():
    m = lpips_model.LpipsVGG16().init_synthetic(0)
    g = torch.Generator().manual_seed(1)
    a = torch.randint(0, 256, (2, 19, 16, 3), generator=g, dtype=torch.uint8)
    assert torch.equal(m(a, a), torch.zeros(2))                                 # identical input -> exactly 0
    assert torch.equal(m.double()(a, a), torch.zeros(2, dtype=torch.float64))
    # two one-hot features on different channels, w = 1: (1 - 0)^2 + (0 - 1)^2 = 2 per pixel (the 1e-10 in n() is below fp64's ulp of 1)
    fa, fb = torch.zeros(1, 8, 3, 5, dtype=torch.float64), torch.zeros(1, 8, 3, 5, dtype=torch.float64)
    fa[:, 2], fb[:, 5] = 1.0, 1.0
    assert lpips_model.LpipsVGG16.head(fa, fb, torch.ones(8, dtype=torch.float64)).item() == pytest.approx(2.0, abs=1e-9)
    fa[:, 2], fb[:, 5] = 7.0, 0.25                                              # the scale of a feature vector does not matter
    assert lpips_model.LpipsVGG16.head(fa, fb, torch.ones(8, dtype=torch.float64)).item() == pytest.approx(2.0, abs=1e-8)
    z = torch.zeros_like(fa)                                                    # a zero pixel on both sides contributes exactly 0
    assert lpips_model.LpipsVGG16.head(z, z, torch.ones(8, dtype=torch.float64)).item() == 0.0
    b = a.clone()
    b[0, 3, 4, 1] ^= 0x40
    v = m(a, b)
    assert v[0] > 0 and v[1] == 0                                               # a pair's number is its own


def test_size_refusals():
    m = lpips_model.LpipsVGG16().init_synthetic(0)
    for shape in ((1, 15, 16, 3), (1, 16, 15, 3), (1, 8, 300, 3)):
        with pytest.raises(ValueError, match="both sides >= 16.*four 2 x 2 floor pools"):
            m(torch.zeros(shape, dtype=torch.uint8), torch.zeros(shape, dtype=torch.uint8))
    with pytest.raises(ValueError, match="one size"):
        m(torch.zeros((1, 16, 16, 3), dtype=torch.uint8), torch.zeros((1, 16, 17, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="uint8"):
        m(torch.zeros((1, 16, 16, 3)), torch.zeros((1, 16, 16, 3)))
    assert m(torch.zeros((1, 16, 16, 3), dtype=torch.uint8), torch.full((1, 16, 16, 3), 255, dtype=torch.uint8)).shape == (1,)


def test_cli_surface_and_host_arithmetic(tmp_path):
    a = lpips.parse_args(["--path1", "A", "--path2", "B"])
    assert (a.self_pairs, a.seed, a.batch_size, a.png_feed, a.jpeg_feed, a.num_workers, a.gpu_id, a.weights, a.lpips_weights,
            a.synthetic_weights, a.per_pair, a.saved_file) == (0, 0, 50, "ring", None, 0, "0", "", "", False, "", "")
    a = lpips.parse_args(["--path1", "A", "--self-pairs", "9", "--seed", "4", "--synthetic-weights"])
    assert a.self_pairs == 9 and a.seed == 4 and a.synthetic_weights and a.path2 is None
    for argv in (["--path1", "A"], ["--path1", "A", "--path2", "B", "--self-pairs", "3"], ["--path2", "B"],
                 ["--path1", "A", "--path2", "B", "--net", "alex"],                       # no such switch: VGG-16 is the network
                 ["--path1", "A", "--path2", "B", "--synthetic-weights", "--weights", "x.pth"]):
        with pytest.raises(SystemExit):
            lpips.parse_args(argv)
    # no parameters and no --synthetic-weights: an error that names both files, never a silent stand-in
    os.environ["TORCH_HOME"], old = str(tmp_path), os.environ.get("TORCH_HOME")
    try:
        with pytest.raises(RuntimeError, match=r"--weights PATH.*vgg16-397923af\.pth.*--lpips-weights PATH"):
            lpips.resolve_model(lpips.parse_args(["--path1", "A", "--path2", "B"]))
        with pytest.raises(RuntimeError, match="Invalid path"):
            lpips.resolve_model(lpips.parse_args(["--path1", "A", "--path2", "B", "--weights", str(tmp_path / "none.pth"), "--lpips-weights", "x"]))
        assert lpips_model.default_weights_path() == os.path.join(str(tmp_path), "hub", "checkpoints", "vgg16-397923af.pth")
    finally:
        if old is None:
            del os.environ["TORCH_HOME"]
        else:
            os.environ["TORCH_HOME"] = old
    model, tag = lpips.resolve_model(lpips.parse_args(["--path1", "A", "--path2", "B", "--synthetic-weights", "--seed", "2"]))
    from tise_toolbox_amd import weights
    assert tag == weights.SYNTHETIC_TAG and model.synthetic
    assert torch.equal(model.convs[0].weight, lpips_model.LpipsVGG16().init_synthetic(2).convs[0].weight)
    # {n, sum, sum of squares} -> mean and population std; additive over shards, an empty one included
    v = np.array([0.25, 0.5, 0.0, 0.125])
    s = paired.value_sums(v[:3]) + paired.value_sums(v[3:]) + paired.value_sums([])
    res = lpips.result_from_sums(s)
    assert res["n"] == 4 and res["lpips"] == v.mean() and res["lpips_std"] == pytest.approx(v.std(), abs=1e-15)
    assert lpips.result_lines(res) == [f"LPIPS (vgg): {v.mean()} +- {res['lpips_std']}"]
    assert lpips.result_lines(res, weights.SYNTHETIC_TAG)[0].endswith(weights.SYNTHETIC_TAG)
    with pytest.raises(RuntimeError, match="at least one pair"):
        lpips.result_from_sums(paired.value_sums([]))
    text = lpips.per_pair_csv(["a/0.png", "a/1.png"], ["b/0.jpg", "b/1.jpg"], {"h": [16, 35], "w": [16, 67], "lpips": [0.0, 0.1]})
    assert text == "pair,file1,file2,h,w,lpips\n0,a/0.png,b/0.jpg,16,16,0.0\n1,a/1.png,b/1.jpg,35,67,0.1\n"


def test_chunking_by_the_byte_budget():
    from tise_toolbox_amd import vgg_pairs_hip
    assert vgg_pairs_hip.ACTIVATION_BUDGET_BYTES == 2 << 30
    assert vgg_pairs_hip.pairs_per_chunk(256, 256) == 64 and vgg_pairs_hip.pairs_per_chunk(256, 256, 1) == 1
    assert vgg_pairs_hip.pairs_per_chunk(16, 16) == 16384 and vgg_pairs_hip.pairs_per_chunk(16, 16, 1 << 62) == 32767
