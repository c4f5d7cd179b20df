"""CPU: the ResNet-50 module of FD-SwAV (tise_toolbox_amd/resnet_model.py) -- layout, loaders, refusals, the seeded stand-ins,
BatchNorm folding, sizes -- the CLI surface of fd_swav, and the preconditions the GPU tests lean on, asserted from the fp64 module
alone."""
import os

import numpy as np
import pytest
import torch

from tise_toolbox_amd import fd_swav, resnet_model as rm, weights

SIZES = ((32, 32), (33, 47), (224, 224))


def seeded_bytes(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)


@pytest.fixture(scope="module")
def model():
    return rm.ResNet50().init_synthetic(0)


def test_layout_and_key_names(model):
    sd = model.state_dict()
    assert "table" not in sd and not any(k.startswith("fc.") for k in sd)
    assert tuple(sd["conv1.weight"].shape) == (64, 3, 7, 7) and "conv1.bias" not in sd
    assert (model.conv1.stride, model.conv1.padding) == ((2, 2), (3, 3))
    assert [len(getattr(model, f"layer{i}")) for i in (1, 2, 3, 4)] == [3, 4, 6, 3]
    inplanes = 64
    for i, planes in enumerate((64, 128, 256, 512), 1):
        for b, blk in enumerate(getattr(model, f"layer{i}")):
            stride = 2 if (b == 0 and i > 1) else 1
            assert tuple(sd[f"layer{i}.{b}.conv1.weight"].shape) == (planes, inplanes, 1, 1) and blk.conv1.stride == (1, 1)
            assert tuple(sd[f"layer{i}.{b}.conv2.weight"].shape) == (planes, planes, 3, 3)
            assert blk.conv2.stride == (stride, stride) and blk.conv2.padding == (1, 1)          # the stride sits on conv2
            assert tuple(sd[f"layer{i}.{b}.conv3.weight"].shape) == (4 * planes, planes, 1, 1)
            assert (f"layer{i}.{b}.downsample.0.weight" in sd) == (b == 0)
            if b == 0:
                assert tuple(sd[f"layer{i}.{b}.downsample.0.weight"].shape) == (4 * planes, inplanes, 1, 1)
                assert blk.downsample[0].stride == (stride, stride) and f"layer{i}.{b}.downsample.1.running_var" in sd
            for bn in ("bn1", "bn2", "bn3"):
                assert getattr(blk, bn).eps == 1e-5 and f"layer{i}.{b}.{bn}.running_mean" in sd
            inplanes = 4 * planes
    assert len(list(model.conv_bn_pairs())) == 53 and not model.training
    assert "not installed" in rm.__doc__ and "FROM MEMORY" in rm.__doc__


def test_both_checkpoint_layouts_round_trip(tmp_path, model):
    plain = {k: v.clone() for k, v in model.state_dict().items()}
    plain["fc.weight"], plain["fc.bias"] = torch.zeros(1000, 2048), torch.zeros(1000)
    p1 = str(tmp_path / "resnet50.pth")
    torch.save(plain, p1)
    swav = {"module." + k: v.clone() for k, v in model.state_dict().items()}
    swav["module.projection_head.0.weight"] = torch.zeros(2048, 2048)
    swav["module.prototypes.weight"] = torch.zeros(3000, 128)
    p2 = str(tmp_path / "swav_800ep_pretrain.pth.tar")
    torch.save(swav, p2)
    p3 = str(tmp_path / "wrapped.pth")
    torch.save({"state_dict": swav}, p3)
    for p in (p1, p2, p3):
        got = rm.load_state_dict_file(p)
        assert not got.synthetic
        for k, v in model.state_dict().items():
            assert torch.equal(got.state_dict()[k], v), (p, k)


def test_refusals_name_the_key_and_both_shapes(tmp_path, model):
    base = {k: v.clone() for k, v in model.state_dict().items()}

    def refused(sd, *needles):
        p = str(tmp_path / "other.pth")
        torch.save(sd, p)
        with pytest.raises(ValueError) as e:
            rm.load_state_dict_file(p)
        for s in needles + (p,):
            assert s in str(e.value), (s, str(e.value))
    r18 = {k: v for k, v in base.items() if ".conv3." not in k and ".bn3." not in k}             # basic blocks: no conv3
    refused(r18, "layer1.0.conv3.weight is missing", "(256, 64, 1, 1)", "ResNet-18 / 34")
    r101 = dict(base)
    for k, v in base.items():
        if k.startswith("layer3.5."):
            r101[k.replace("layer3.5.", "layer3.6.")] = v
    refused(r101, "layer3.6.", "no such entry", "ResNet-101 / 152")
    wide = dict(base)
    wide["conv1.weight"] = torch.zeros(128, 3, 7, 7)
    refused(wide, "conv1.weight is (128, 3, 7, 7)", "(64, 3, 7, 7)", "wide")
    refused({"features.0.weight": torch.zeros(64, 3, 3, 3), "features.0.bias": torch.zeros(64)}, "conv1.weight is missing",
            "(64, 3, 7, 7)", "VGG")
    refused({"Conv2d_1a_3x3.conv.weight": torch.zeros(32, 3, 3, 3)}, "conv1.weight is missing", "(64, 3, 7, 7)", "InceptionV3")


def test_init_synthetic_is_seeded(model):
    again, other = rm.ResNet50().init_synthetic(0), rm.ResNet50().init_synthetic(1)
    assert model.synthetic and again.synthetic
    for k, v in model.state_dict().items():
        if k.endswith("num_batches_tracked"):
            continue
        assert torch.equal(again.state_dict()[k], v), k
        assert not torch.equal(other.state_dict()[k], v), k
    # the recipe: g = 0.25 on every bn3 and 1 elsewhere (the downsample BatchNorm included), running_var in [0.5, 1.5)
    sd = model.state_dict()
    assert abs(float(sd["layer3.2.bn3.weight"].mean()) - 0.25) < 0.01 and abs(float(sd["layer3.2.bn2.weight"].mean()) - 1) < 0.04
    assert abs(float(sd["layer3.0.downsample.1.weight"].mean()) - 1) < 0.02
    assert 0.5 <= float(sd["layer4.0.bn1.running_var"].min()) and float(sd["layer4.0.bn1.running_var"].max()) < 1.5
    w = sd["layer2.1.conv2.weight"].double()
    assert abs(float(w.var()) * (128 * 9) / 2 - 1) < 0.02                                          # N(0, 2 / fan_in)


def test_folded_against_conv_then_batchnorm_fp64(model):
    m64 = rm.ResNet50().init_synthetic(0).double()
    folded = m64.folded()
    assert list(folded) == [name for name, _, _ in m64.conv_bn_pairs()] and len(folded) == 53
    g = torch.Generator().manual_seed(5)
    for name, conv, bn in m64.conv_bn_pairs():
        if name not in ("conv1", "layer1.0.conv2", "layer2.0.downsample.0", "layer3.0.conv2", "layer4.2.conv3"):
            continue
        x = torch.randn((2, conv.in_channels, 9, 7), generator=g, dtype=torch.float64)
        want = bn(conv(x))
        # the fp64 fold itself (what folded() rounds once to fp32) within 1e-12 relative ...
        s = bn.weight / torch.sqrt(bn.running_var + bn.eps)
        w64, b64 = conv.weight * s.view(-1, 1, 1, 1), bn.bias - bn.running_mean * s
        got = torch.nn.functional.conv2d(x, w64, b64, conv.stride, conv.padding)
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), name
        # ... and folded() is that, rounded once
        w, b = folded[name]
        assert w.dtype == torch.float32 and b.dtype == torch.float32
        assert torch.equal(w, w64.float()) and torch.equal(b, b64.float()), name


def test_output_sizes():
    assert rm.output_hw(32, 32) == (1, 1) and rm.output_hw(33, 47) == (2, 2) and rm.output_hw(224, 224) == (7, 7)
    m = rm.ResNet50().init_synthetic(0)
    seen = []
    hook = m.layer4[2].register_forward_hook(lambda mod, i, o: seen.append(tuple(o.shape[2:])))
    for h, w in ((32, 32), (33, 47)):
        out = m(seeded_bytes(1, h, w, 1))
        assert out.shape == (1, 2048) and out.dtype == torch.float32
    hook.remove()
    assert seen == [(1, 1), (2, 2)]


def test_size_and_dtype_refusals(model):
    for h, w in ((31, 64), (64, 31), (16, 16)):
        with pytest.raises(ValueError, match="five halvings must leave one pixel"):
            model(torch.zeros((1, h, w, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="uint8"):
        model(torch.zeros((1, 32, 32, 3), dtype=torch.float32))
    with pytest.raises(ValueError, match="uint8"):
        model(torch.zeros((1, 3, 32, 32), dtype=torch.uint8))
    with pytest.raises(ValueError, match="uint8"):
        model(torch.zeros((32, 32, 3), dtype=torch.uint8))


def test_cli_surface(tmp_path):
    a = fd_swav.parse_args(["--path1", "a", "--path2", "b"])
    assert (a.batch_size, a.kd, a.prdc, a.prdc_k, a.png_feed, a.num_workers, a.gpu_id, a.weights, a.synthetic_weights, a.save_features,
            a.saved_file) == (50, False, False, 5, "ring", 0, "0", None, False, "", "")
    a = fd_swav.parse_args(["--path1", "a", "--path2", "b", "--kd", "--prdc", "--prdc-k", "3", "--save-features", "o.npz", "--saved_file",
                            "o.txt", "--batch-size", "10", "--synthetic-weights", "--png-feed", "dataloader", "--num-workers", "2",
                            "--gpu_id", "1"])
    assert (a.kd, a.prdc, a.prdc_k, a.save_features, a.saved_file, a.batch_size, a.png_feed, a.num_workers, a.gpu_id) == \
        (True, True, 3, "o.npz", "o.txt", 10, "dataloader", 2, "1")
    for bad in (["--weights", "w", "--synthetic-weights"], ["--prdc", "--prdc-k", "17"], ["--authpct"], ["--vendi"], ["--fd-infinity"]):
        with pytest.raises(SystemExit):
            fd_swav.parse_args(["--path1", "a", "--path2", "b"] + bad)
    tag = weights.SYNTHETIC_TAG
    res = dict(fd=1.5, kd=(0.25, 0.125), prdc=dict(precision=0.5, recall=0.25, density=2.0, coverage=1.0))
    assert fd_swav.result_lines(res, tag) == [f"FD-SwAV: 1.5{tag}", f"KD-SwAV: 0.25 +- 0.125{tag}", f"Precision-SwAV: 0.5{tag}",
                                              f"Recall-SwAV: 0.25{tag}", f"Density-SwAV: 2.0{tag}", f"Coverage-SwAV: 1.0{tag}"]
    assert fd_swav.result_lines(dict(fd=2.0, kd=None, prdc=None)) == ["FD-SwAV: 2.0"]
    # a feature file of another network is refused on its tag alone, without a GPU; one of this network passes
    other, own = str(tmp_path / "dino.npz"), str(tmp_path / "swav.npz")
    np.savez(other, mu=np.zeros(4), sigma=np.eye(4), network=np.asarray("dinov2-vitl14"), features=np.zeros((3, 4), np.float32))
    np.savez(own, mu=np.zeros(2048), sigma=np.eye(2048), network=np.asarray("swav-resnet50"), features=np.zeros((3, 2048), np.float32))
    with pytest.raises(RuntimeError, match="dinov2-vitl14"):
        fd_swav.check_feature_file(other)
    with pytest.raises(RuntimeError, match="dinov2-vitl14"):
        fd_swav.main(["--path1", other, "--path2", own, "--synthetic-weights"])
    fd_swav.check_feature_file(own)
    assert fd_swav.load_features_npz(own)[0].shape == (3, 2048)
    assert rm.NETWORK == "swav-resnet50" == fd_swav.KIND


def test_kinds_path(monkeypatch, tmp_path):
    monkeypatch.setenv("TORCH_HOME", str(tmp_path))
    what, paths = weights._KINDS["swav-resnet50"]
    assert paths() == [os.path.join(str(tmp_path), "hub", "checkpoints", "swav_800ep_pretrain.pth.tar")] and "SwAV" in what
    with pytest.raises(RuntimeError, match="swav_800ep_pretrain.pth.tar"):
        weights.resolve(None, False, "swav-resnet50")
    assert weights.resolve(None, True, "swav-resnet50") == (None, weights.SYNTHETIC_TAG)


def test_input_table_against_numpy_fp32(model):
    x = np.arange(256, dtype=np.float32) / np.float32(255)
    want = np.stack([(x - np.float32(m)) / np.float32(s) for m, s in zip((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))]).astype(np.float32)
    assert np.array_equal(rm.input_table().numpy(), want) and model.table.dtype == torch.float32
    img = seeded_bytes(1, 32, 33, 9)
    got = model.double().network_input(img)
    model.float()
    assert got.dtype == torch.float64
    assert np.array_equal(got[0].numpy(), np.stack([want[c][img[0, :, :, c].numpy()] for c in range(3)]).astype(np.float64))


@pytest.mark.parametrize("h,w", SIZES)
def test_gpu_test_preconditions_from_the_fp64_module(h, w):
    """What tests/test_gpu_resnet.py leans on: on seeded bytes the stand-ins' largest fp64 activation stays below 65504 / 16, so the
    split format has its full 22 bits everywhere, and the features are not degenerate."""
    m64 = rm.ResNet50().init_synthetic(0).double()
    amax = []
    f = m64(seeded_bytes(1, h, w, 1000 * h + w), amax)
    assert len(amax) == 1 + 16 * 4 + 4 and max(amax) < 65504 / 16, max(amax)
    assert bool(torch.isfinite(f).all()) and float((f == 0).double().mean()) < 0.5 and 1.0 < float(f.mean()) < 10.0
