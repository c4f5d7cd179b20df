"""CPU: the host side of DISTS -- the input table, the two parameter loaders, the seeded stand-ins, closed forms of the torch
module, the host arithmetic of stage 0, the size refusals and the CLI surface."""
import os

import numpy as np
import pytest
import torch

from tise_toolbox_amd import dists, dists_model, paired


def test_input_table_is_numpy_fp32():
    t = dists_model.input_table()
    assert t.dtype == torch.float32 and tuple(t.shape) == (3, 256) and t.is_contiguous()
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    for c in range(3):
        for b in (0, 1, 127, 128, 254, 255):
            x = np.float32(b) / np.float32(255.0)
            want = (x - np.float32(mean[c])) / np.float32(std[c])
            assert want.dtype == np.float32 and t[c, b].item() == float(want), (c, b)
    b = np.arange(256, dtype=np.float32)
    want = ((b / np.float32(255))[None] - np.float32(mean)[:, None]) / np.float32(std)[:, None]
    assert want.dtype == np.float32 and np.array_equal(t.numpy(), want)
    assert float(t.abs().max()) < 3.0                                          # far inside the fp16 range of the split format
    assert dists_model.STAGE_CHANNELS == (3, 64, 128, 256, 512, 512) and dists_model.N_CHANNELS == 1475


def _seeded_files(tmp_path, seed=3):
    g = torch.Generator().manual_seed(seed)
    trunk = {}
    for idx, (ci, co) in zip(dists_model.CONV_INDICES, dists_model.CONV_CHANNELS):
        trunk[f"features.{idx}.weight"] = torch.randn((co, ci, 3, 3), generator=g) * 0.05
        trunk[f"features.{idx}.bias"] = torch.randn((co,), generator=g) * 0.05
    trunk["classifier.0.weight"] = torch.zeros(2, 2)                           # torchvision's file has the classifier too: ignored
    ab = {"alpha": torch.rand((1, 1475, 1, 1), generator=g), "beta": torch.rand((1, 1475, 1, 1), generator=g)}
    p1, p2 = os.path.join(tmp_path, "vgg16.pth"), os.path.join(tmp_path, "weights.pt")
    torch.save(trunk, p1)
    torch.save(ab, p2)
    return trunk, ab, p1, p2


def test_loaders_round_trip_and_refusals(tmp_path):
    trunk, ab, p1, p2 = _seeded_files(str(tmp_path))
    m = dists_model.build_model(p1, p2)
    assert not m.synthetic
    for k, idx in enumerate(dists_model.CONV_INDICES):
        assert torch.equal(m.convs[k].weight, trunk[f"features.{idx}.weight"]) and torch.equal(m.convs[k].bias, trunk[f"features.{idx}.bias"])
    assert torch.equal(m.alpha, ab["alpha"]) and torch.equal(m.beta, ab["beta"])
    al, be = m.normalized_weights()
    assert al.dtype == torch.float64 and al.shape == (1475,) and float(al.sum() + be.sum()) == pytest.approx(1.0, abs=1e-14)
    total = ab["alpha"].double().sum() + ab["beta"].double().sum()
    assert torch.equal(al, ab["alpha"].double().reshape(-1) / total)
    # another network's shapes: the same refusals by shape as LPIPS's trunk loader, naming both
    alex = dict(trunk)
    alex["features.0.weight"] = torch.zeros(64, 3, 11, 11)
    pa = os.path.join(str(tmp_path), "alexnet.pth")
    torch.save(alex, pa)
    with pytest.raises(ValueError, match=r"features\.0\.weight is \(64, 3, 11, 11\), VGG-16 has \(64, 3, 3, 3\).*AlexNet"):
        dists_model.DistsVGG16().load_trunk(pa)
    vgg11 = {k: v for k, v in trunk.items() if not k.startswith("features.2.")}
    with pytest.raises(ValueError, match=r"features\.2\.weight is missing, VGG-16 has \(64, 64, 3, 3\).*another VGG variant"):
        dists_model.DistsVGG16().load_trunk(vgg11)
    # alpha / beta of any other shape: refused, naming both
    pw = os.path.join(str(tmp_path), "other.pt")
    torch.save({"alpha": torch.zeros(1, 1472, 1, 1), "beta": torch.zeros(1, 1475, 1, 1)}, pw)
    with pytest.raises(ValueError, match=r"alpha is \(1, 1472, 1, 1\), DISTS on VGG-16 has \(1, 1475, 1, 1\)"):
        dists_model.DistsVGG16().load_dists_weights(pw)
    with pytest.raises(ValueError, match=r"beta is \(1475,\), DISTS on VGG-16 has \(1, 1475, 1, 1\)"):
        dists_model.DistsVGG16().load_dists_weights({"alpha": torch.zeros(1, 1475, 1, 1), "beta": torch.zeros(1475)})
    with pytest.raises(ValueError, match=r"beta is missing, DISTS on VGG-16 has \(1, 1475, 1, 1\)"):
        dists_model.DistsVGG16().load_dists_weights({"alpha": torch.zeros(1, 1475, 1, 1)})
    with pytest.raises(RuntimeError, match="two files"):
        dists_model.build_model(p1, None)
    with pytest.raises(RuntimeError, match="mutually exclusive"):
        dists_model.build_model(p1, p2, synthetic=True)


def test_synthetic_parameters_are_seeded_scaled_and_non_negative():
    a, b, c = (dists_model.DistsVGG16().init_synthetic(s) for s in (0, 0, 1))
    assert a.synthetic
    for p, q, r in zip(a.parameters(), b.parameters(), c.parameters()):
        assert torch.equal(p, q) and not torch.equal(p, r)
    for conv in a.convs:
        want = (2.0 / (conv.in_channels * 9)) ** 0.5
        assert 0.8 * want < float(conv.weight.std()) < 1.2 * want
    for p in (a.alpha, a.beta):
        assert tuple(p.shape) == (1, 1475, 1, 1) and float(p.min()) >= 0.0
        assert 0.09 < float(p.mean()) < 0.11 and 0.008 < float(p.std()) < 0.012


def test_module_closed_forms():
    m = dists_model.DistsVGG16().init_synthetic(0)
    m64 = dists_model.DistsVGG16().init_synthetic(0).double()
    g = torch.Generator().manual_seed(1)
    a = torch.randint(0, 256, (2, 19, 16, 3), generator=g, dtype=torch.uint8)
    assert torch.equal(m(a, a), torch.zeros(2))                                 # identical input -> exactly 0
    assert torch.equal(m64(a, a), torch.zeros(2, dtype=torch.float64))
    # the stable form against the package's 1 - (sum alpha S1 + sum beta S2), in fp64
    b = a.clone()
    b[0, 3:9, 4:12] ^= 0x15
    b[1] = torch.randint(0, 256, (19, 16, 3), generator=g, dtype=torch.uint8)
    v, p = m64(a, b), m64.forward_package_form(a, b)
    assert (v > 1e-4).all() and float((v - p).abs().max()) <= 1e-12
    b2 = a.clone()
    b2[0, 3, 4, 1] ^= 0x40
    v = m(a, b2)
    assert v[0] > 0 and v[1] == 0                                               # a pair's number is its own
    # L2 pool: a zero map gives sqrt(1e-12) = 1e-6; the output is ceil(H/2) x ceil(W/2)
    z = dists_model.l2pool(torch.zeros(1, 4, 5, 7, dtype=torch.float64))
    assert tuple(z.shape) == (1, 4, 3, 4) and bool((z == 1e-6).all())
    for s, want in ((16, [16, 8, 4, 2, 1]), (17, [17, 9, 5, 3, 2]), (31, [31, 16, 8, 4, 2])):
        st = m.stages(torch.zeros((1, s, 16, 3), dtype=torch.uint8))
        assert [t.shape[2] for t in st] == [s] + want and [t.shape[1] for t in st] == [3, 64, 128, 256, 512, 512]
        assert dists_model.pooled_size(s) == want[1]
    # a one-pixel window at a corner: only the 2 x 2 taps inside the image count (weights 4, 2, 2, 1 of 16)
    x = torch.arange(1.0, 10.0, dtype=torch.float64).reshape(1, 1, 3, 3)
    y = dists_model.l2pool(x)
    assert float(y[0, 0, 0, 0]) == pytest.approx(np.sqrt((4 * 1 + 2 * 4 + 2 * 16 + 25) / 16 + 1e-12), abs=1e-15)
    # S1, S2 of stage_terms on a constant and an all-zero channel
    fx = torch.zeros(1, 2, 3, 5, dtype=torch.float64)
    fy = torch.zeros(1, 2, 3, 5, dtype=torch.float64)
    fx[:, 0], fy[:, 0] = 2.0, 3.0
    s1, s2 = dists_model.stage_terms(fx, fy)
    assert float(s1[0, 0]) == pytest.approx((12 + 1e-6) / (13 + 1e-6), abs=1e-15) and float(s2[0, 0]) == 1.0
    assert float(s1[0, 1]) == 1.0 and float(s2[0, 1]) == 1.0


def test_stage0_host_arithmetic():
    """dists_hip.stage0_value on exact integer sums against the module's fp64 stage 0."""
    from tise_toolbox_amd import dists_hip
    g = torch.Generator().manual_seed(5)
    h, w = 17, 19
    a = torch.randint(0, 256, (3, h, w, 3), generator=g, dtype=torch.uint8)
    b = torch.randint(0, 256, (3, h, w, 3), generator=g, dtype=torch.uint8)
    b[1] = a[1]                                                                 # an identical pair
    a[2], b[2] = 0, 255                                                         # all-0 against all-255
    x, y = a.numpy().astype(np.int64), b.numpy().astype(np.int64)
    sums = np.stack([x.sum((1, 2)), y.sum((1, 2)), (x * x).sum((1, 2)), (y * y).sum((1, 2)), (x * y).sum((1, 2))], -1)
    assert sums.shape == (3, 3, 5)
    al, be = np.array([0.2, 0.1, 0.05]), np.array([0.3, 0.15, 0.2])
    got = dists_hip.stage0_value(sums, h, w, al, be)
    s1, s2 = dists_model.stage_terms(a.permute(0, 3, 1, 2).double() / 255, b.permute(0, 3, 1, 2).double() / 255)
    want = ((torch.from_numpy(al) * (1 - s1)) + (torch.from_numpy(be) * (1 - s2))).sum(1).numpy()
    assert np.abs(got - want).max() <= 1e-14 and got[1] == 0.0 and got[0] > 1e-3
    # all-0 against all-255: mx = 0, my = 1, no variance: S1 = c1 / (1 + c1), S2 = 1
    assert got[2] == pytest.approx(al.sum() * (1 - 1e-6 / (1 + 1e-6)), abs=1e-15)
    assert dists_hip.stage0_value(sums[:, :, [1, 0, 3, 2, 4]], h, w, al, be).tobytes() == got.tobytes()      # d(y, x): the same bits


def test_size_refusals():
    m = dists_model.DistsVGG16().init_synthetic(0)
    for shape in ((1, 15, 16, 3), (1, 16, 15, 3), (1, 8, 300, 3)):
        with pytest.raises(ValueError, match="both sides >= 16.*pinned from 16 up"):
            m(torch.zeros(shape, dtype=torch.uint8), torch.zeros(shape, dtype=torch.uint8))
    with pytest.raises(ValueError, match="one size"):
        m(torch.zeros((1, 16, 16, 3), dtype=torch.uint8), torch.zeros((1, 16, 17, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="uint8"):
        m(torch.zeros((1, 16, 16, 3)), torch.zeros((1, 16, 16, 3)))
    assert m(torch.zeros((1, 16, 16, 3), dtype=torch.uint8), torch.full((1, 16, 16, 3), 255, dtype=torch.uint8)).shape == (1,)
    with pytest.raises(ValueError, match="DISTS: pair 3 needs both sides >= 16"):
        dists_model.check_size(12, 40, "DISTS: pair 3")


def test_cli_surface_and_host_arithmetic(tmp_path):
    a = dists.parse_args(["--path1", "A", "--path2", "B"])
    assert (a.self_pairs, a.seed, a.batch_size, a.png_feed, a.jpeg_feed, a.num_workers, a.gpu_id, a.weights, a.dists_weights,
            a.synthetic_weights, a.per_pair, a.saved_file) == (0, 0, 50, "ring", None, 0, "0", "", "", False, "", "")
    a = dists.parse_args(["--path1", "A", "--self-pairs", "9", "--seed", "4", "--synthetic-weights"])
    assert a.self_pairs == 9 and a.seed == 4 and a.synthetic_weights and a.path2 is None
    for argv in (["--path1", "A"], ["--path1", "A", "--path2", "B", "--self-pairs", "3"], ["--path2", "B"],
                 ["--path1", "A", "--path2", "B", "--lpips-weights", "x.pth"],             # LPIPS's switch is not this tool's
                 ["--path1", "A", "--path2", "B", "--synthetic-weights", "--dists-weights", "x.pt"],
                 ["--path1", "A", "--path2", "B", "--synthetic-weights", "--weights", "x.pth"]):
        with pytest.raises(SystemExit):
            dists.parse_args(argv)
    # no parameters and no --synthetic-weights: an error that names both files, never a silent stand-in
    os.environ["TORCH_HOME"], old = str(tmp_path), os.environ.get("TORCH_HOME")
    try:
        with pytest.raises(RuntimeError, match=r"--weights PATH.*vgg16-397923af\.pth.*--dists-weights PATH, weights\.pt"):
            dists.resolve_model(dists.parse_args(["--path1", "A", "--path2", "B"]))
        with pytest.raises(RuntimeError, match="Invalid path"):
            dists.resolve_model(dists.parse_args(["--path1", "A", "--path2", "B", "--weights", str(tmp_path / "none.pth"), "--dists-weights", "x"]))
        from tise_toolbox_amd import lpips_model
        assert dists_model.default_weights_path() == lpips_model.default_weights_path()        # --weights defaults to LPIPS's VGG path
        assert dists_model.default_weights_path() == os.path.join(str(tmp_path), "hub", "checkpoints", "vgg16-397923af.pth")
    finally:
        if old is None:
            del os.environ["TORCH_HOME"]
        else:
            os.environ["TORCH_HOME"] = old
    model, tag = dists.resolve_model(dists.parse_args(["--path1", "A", "--path2", "B", "--synthetic-weights", "--seed", "2"]))
    from tise_toolbox_amd import weights
    assert tag == weights.SYNTHETIC_TAG and model.synthetic
    assert torch.equal(model.alpha, dists_model.DistsVGG16().init_synthetic(2).alpha)
    # {n, sum, sum of squares} -> mean and population std; additive over shards, an empty one included
    v = np.array([0.25, 0.5, 0.0, 0.125])
    s = paired.value_sums(v[:3]) + paired.value_sums(v[3:]) + paired.value_sums([])
    res = dists.result_from_sums(s)
    assert res["n"] == 4 and res["dists"] == v.mean() and res["dists_std"] == pytest.approx(v.std(), abs=1e-15)
    assert dists.result_lines(res) == [f"DISTS: {v.mean()} +- {res['dists_std']}"]
    assert dists.result_lines(res, weights.SYNTHETIC_TAG)[0].endswith(weights.SYNTHETIC_TAG)
    with pytest.raises(RuntimeError, match="at least one pair"):
        dists.result_from_sums(paired.value_sums([]))
    text = dists.per_pair_csv(["a/0.png", "a/1.png"], ["b/0.jpg", "b/1.jpg"], {"h": [16, 35], "w": [16, 67], "dists": [0.0, 0.1]})
    assert text == "pair,file1,file2,h,w,dists\n0,a/0.png,b/0.jpg,16,16,0.0\n1,a/1.png,b/1.jpg,35,67,0.1\n"
