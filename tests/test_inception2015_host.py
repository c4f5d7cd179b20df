"""CPU: the --network inception-2015 option (TensorFlow Inception-2015 graph, pytorch-fid's weight file) without a GPU:
strict weight loading in both directions, the default network left as it was, the input table, the CLI surface, the
.npz network tag and the default weight path."""
import os

import numpy as np
import pytest
import torch

from tests import _inception2015_ref as ref


def _save(tmp_path, sd, name):
    p = tmp_path / name
    torch.save(sd, p)
    return str(p)


def test_pytorch_fid_state_dict_loads_strictly_into_the_variant(tmp_path):
    from tise_toolbox_amd.inception import InceptionV3, build_inception3
    sd = ref.random_state_dict(1)
    net = build_inception3(_save(tmp_path, sd, "pt_inception.pth"), network="inception-2015")
    assert net.network == "inception-2015" and not hasattr(net, "AuxLogits")
    got = net.state_dict()
    assert set(got) == set(sd)
    assert all(torch.equal(got[k], sd[k]) for k in sd)
    assert net.fc.out_features == 1008
    pools = {n: getattr(net, n).pool for n in ("Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6b", "Mixed_6c", "Mixed_6d",
                                               "Mixed_6e", "Mixed_7b", "Mixed_7c")}
    assert pools == dict({n: "avg_excl" for n in pools}, Mixed_7c="max")
    m = InceptionV3([3], weights=_save(tmp_path, sd, "w2.pth"), network="inception-2015")
    assert m.network == "inception-2015" and m.fc.weight.shape == (1008, 2048)


def test_wrong_file_for_either_network_fails_loudly(tmp_path):
    from tise_toolbox_amd.inception import build_inception3
    fid_file = _save(tmp_path, ref.random_state_dict(2), "pt_inception.pth")
    with pytest.raises(RuntimeError, match="Missing key|Unexpected key|size mismatch"):
        build_inception3(fid_file)                                  # pytorch-fid's file into the torchvision tree
    with pytest.raises(RuntimeError, match="Missing key|Unexpected key|size mismatch"):
        build_inception3(fid_file, num_classes=1000, network="inception-2015")      # head width mismatch
    from tise_toolbox_amd.inception import Inception3
    tv = {k: torch.zeros_like(v, device="cpu") for k, v in Inception3().state_dict().items()}
    tv_file = _save(tmp_path, tv, "inception_v3_google.pth")
    with pytest.raises(RuntimeError, match="Unexpected key|size mismatch"):
        build_inception3(tv_file, network="inception-2015")          # torchvision's file into the variant
    with pytest.raises(ValueError, match="network"):
        build_inception3(tv_file, network="inception-2016")


def test_default_network_keys_and_input_table_unchanged():
    from tise_toolbox_amd import device
    from tise_toolbox_amd.inception import Inception3
    net = Inception3()
    assert net.network == "torchvision" and net.fc.out_features == 1000 and hasattr(net, "AuxLogits")
    keys = sorted(net.state_dict())
    assert len(keys) == 580
    fid_shapes = ref.pytorch_fid_shapes()
    assert all(tuple(net.state_dict()[k].shape) == fid_shapes[k] for k in keys if k in fid_shapes and not k.startswith("fc."))
    # the torchvision tree minus AuxLogits and with a 1000-class fc is exactly pytorch-fid's key set
    tv_only = {k for k in keys if k.startswith("AuxLogits.")}
    assert set(keys) - tv_only == set(ref.pytorch_fid_shapes())
    assert all(getattr(net, n).pool == "avg" for n in ("Mixed_5b", "Mixed_6e", "Mixed_7b", "Mixed_7c"))
    # the torchvision table: ToTensor then the inception.py:120-124 affine, fp32, in the reference's op order
    v = np.arange(256, dtype=np.float32) / np.float32(255.0)
    want = np.stack([v * np.float32(s / 0.5) + np.float32((m - 0.5) / 0.5)
                     for s, m in ((0.229, 0.485), (0.224, 0.456), (0.225, 0.406))])
    for lut in (device.make_lut(), device.make_lut(True), device.make_lut(network="torchvision")):
        assert lut.dtype == np.float32 and lut.tobytes() == want.tobytes()
    assert device.make_lut(scale_pm1=True).tobytes() == np.tile((v - np.float32(0.5)) / np.float32(0.5), (3, 1)).tobytes()


def test_variant_input_table_and_preprocess():
    from tise_toolbox_amd import device
    from tise_toolbox_amd.inception import INCEPTION_2015_INPUT_DIV, INCEPTION_2015_INPUT_SUB
    assert (INCEPTION_2015_INPUT_SUB, INCEPTION_2015_INPUT_DIV) == (128.0, 128.0)
    lut = device.make_lut(network="inception-2015")
    want = (np.arange(256, dtype=np.float64) - 128.0) / 128.0
    assert lut.shape == (3, 256) and lut.dtype == np.float32
    for c in range(3):
        assert np.array_equal(lut[c].astype(np.float64), want)
    assert lut[:, 0].tolist() == [-1.0] * 3 and lut[:, 128].tolist() == [0.0] * 3
    with pytest.raises(ValueError):
        device.make_lut(network="tf")


def test_network_parsing_and_num_classes_default():
    from tise_toolbox_amd import calibration, fid_score, inception_score
    from tise_toolbox_amd.inception import NETWORK_CLASSES
    assert NETWORK_CLASSES == {"torchvision": 1000, "inception-2015": 1008}
    for parser, base in ((inception_score._build_parser(), ["--image_folder", "d"]),
                         (fid_score._build_parser(), ["--path1", "a", "--path2", "b"]),
                         (calibration._build_parser(), ["--features", "x.npz"])):
        a = parser.parse_args(base)
        assert a.network == "torchvision"
        a = parser.parse_args(base + ["--network", "inception-2015"])
        assert a.network == "inception-2015" and a.num_classes is None
        a = parser.parse_args(base + ["--network", "inception-2015", "--num-classes", "1001"])
        assert a.num_classes == 1001
        with pytest.raises(SystemExit):
            parser.parse_args(base + ["--network", "inception-v4"])


def test_cli_num_classes_default_reaches_the_model(monkeypatch, tmp_path):
    """main() resolves --num-classes from --network before building anything: 1008 for inception-2015, 1000 else."""
    from tise_toolbox_amd import inception_score
    seen = {}

    def fake_configure(**kw):
        seen.update(kw)
        raise SystemExit(0)
    monkeypatch.setattr(inception_score, "configure", fake_configure)
    monkeypatch.setenv("TORCH_HOME", str(tmp_path))
    if "HIP_VISIBLE_DEVICES" not in os.environ:                      # main() sets it by default: leave the process as it was
        monkeypatch.setenv("HIP_VISIBLE_DEVICES", "0")
        monkeypatch.delenv("HIP_VISIBLE_DEVICES")
    for net, n in (("inception-2015", 1008), ("torchvision", 1000)):
        with pytest.raises(SystemExit):
            inception_score.main(["--image_folder", str(tmp_path), "--synthetic-weights", "--network", net])
        assert (seen["network"], seen["num_classes"]) == (net, n)


def test_stats_npz_network_tag(tmp_path):
    from tise_toolbox_amd import fid_score
    mu, sigma = np.arange(4.0), np.eye(4)
    p15, ptv = str(tmp_path / "s15.npz"), str(tmp_path / "stv.npz")
    fid_score.save_stats_npz(p15, mu, sigma, "inception-2015")
    fid_score.save_stats_npz(ptv, mu, sigma, "torchvision")
    with np.load(p15) as f:
        assert sorted(f.files) == ["mu", "network", "sigma"] and str(f["network"]) == "inception-2015"
    with np.load(ptv) as f:
        assert sorted(f.files) == ["mu", "sigma"]                         # the default network's files stay {mu, sigma}

    class M:
        network = "torchvision"
    m15 = M()
    m15.network = "inception-2015"
    # tagged file, matching network: loads; mismatching: refused; untagged: loads on either network
    m, s = fid_score._compute_statistics_of_path(p15, m15, 50, 2048, True)
    assert np.array_equal(m, mu) and np.array_equal(s, sigma)
    with pytest.raises(RuntimeError, match="inception-2015"):
        fid_score._compute_statistics_of_path(p15, M(), 50, 2048, True)
    for model in (M(), m15):
        m, s = fid_score._compute_statistics_of_path(ptv, model, 50, 2048, True)
        assert np.array_equal(m, mu)
    ptag = str(tmp_path / "tagged_tv.npz")
    np.savez(ptag, mu=mu, sigma=sigma, network=np.asarray("torchvision"))
    with pytest.raises(RuntimeError, match="torchvision"):
        fid_score._compute_statistics_of_path(ptag, m15, 50, 2048, True)


def test_default_weight_path_resolution(tmp_path, monkeypatch):
    from tise_toolbox_amd import weights as tw
    monkeypatch.setenv("TORCH_HOME", str(tmp_path))
    assert tw.inception_kind("inception-2015") == "inception2015"
    assert tw.inception_kind("inception-2015", True) == "inception2015"
    assert tw.inception_kind("torchvision") == "inception" and tw.inception_kind("torchvision", True) == "inception80"
    with pytest.raises(RuntimeError, match="pt_inception-2015-12-05-6726825d.pth"):
        tw.resolve(None, False, "inception2015")
    # a torchvision file in the cache does not stand in for the 2015 graph
    ck = tmp_path / "hub" / "checkpoints"
    ck.mkdir(parents=True)
    (ck / "inception_v3_google-1a9a5a14.pth").write_bytes(b"x")
    with pytest.raises(RuntimeError):
        tw.resolve(None, False, "inception2015")
    want = ck / "pt_inception-2015-12-05-6726825d.pth"
    want.write_bytes(b"x")
    assert tw.resolve(None, False, "inception2015") == (str(want), "")
    other = tmp_path / "mine.pth"
    other.write_bytes(b"x")
    assert tw.resolve(str(other), False, "inception2015") == (str(other), "")
    path, tag = tw.resolve(None, True, "inception2015")
    assert path is None and tag == tw.SYNTHETIC_TAG


def test_standin_cache_key_includes_the_network(tmp_path, monkeypatch):
    from tise_toolbox_amd import inception
    monkeypatch.setenv("TISE_STANDIN_CACHE", str(tmp_path))
    p_tv = inception._standin_cache_path((0, 1000, "fid"))
    p_15 = inception._standin_cache_path((0, 1008, "fid", "inception-2015"))
    p_15b = inception._standin_cache_path((0, 1000, "fid", "inception-2015"))
    assert len({p_tv, p_15, p_15b}) == 3 and "inception-2015" in os.path.basename(p_15)


def test_variant_cpu_forward_matches_fp64_reference(tmp_path):
    """The module tree's own forward (the CPU path of InceptionV3) with the variant's pools and input map against the
    independent fp64 restatement, on random weights of pytorch-fid's shapes; and it differs from the torchvision forward."""
    from tise_toolbox_amd.inception import InceptionV3
    g = torch.Generator().manual_seed(5)
    sd = ref.random_state_dict(3)
    for k, v in sd.items():                                           # a stable, image-dependent random network
        if k.endswith("conv.weight"):
            fan = v[0].numel()
            sd[k] = torch.randn(v.shape, generator=g) * (2.0 / fan) ** 0.5
        elif k.endswith("running_var") or k.endswith("bn.weight"):
            sd[k] = torch.ones_like(v)
        elif k.endswith("running_mean") or k.endswith("bn.bias"):
            sd[k] = torch.zeros_like(v)
        elif k.startswith("fc."):
            sd[k] = torch.randn(v.shape, generator=g) * 0.05
    path = _save(tmp_path, sd, "w.pth")
    m = InceptionV3([3], weights=path, network="inception-2015").eval()
    u8 = torch.randint(0, 256, (2, 299, 299, 3), generator=g, dtype=torch.uint8).numpy()
    x = torch.from_numpy(u8).permute(0, 3, 1, 2).float() / 255.0
    with torch.no_grad():
        got = m(x)[0].flatten(1).double()
    want = ref.pool3(sd, ref.to_input(u8))
    assert (got - want).abs().max().item() <= 1e-4 * want.abs().max().item()
    # the same weights through torchvision's pools: a different function
    for mod in m.modules():
        if hasattr(mod, "pool"):
            mod.pool = "avg"
    with torch.no_grad():
        other = m(x)[0].flatten(1).double()
    assert (other - want).abs().max().item() > 1e-2 * want.abs().max().item()
