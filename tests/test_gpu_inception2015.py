"""GPU: --network inception-2015 (the TensorFlow Inception-2015 graph of the reference's IS* for COCO) on the MI355X.

Kernels: the exclude-padding average pools (split and fp32 forms) and the 3x3 / stride 1 max pools against fp64 / exact
references at the network's sizes and channel slices and at all-border sizes.  Trunks: SplitTrunk and FusedTrunk pool3
features and 1008-class logits against the independent fp64 restatement (tests/_inception2015_ref.py).  End to end: the
IS* and FID CLIs against the CPU path on the same files and stand-in weights."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import fid_oracle, is_oracle, resize_oracle
from tests import _cases
from tests import _inception2015_ref as ref
from tise_toolbox_amd.weights import SYNTHETIC_TAG

pytestmark = pytest.mark.gpu

NET = "inception-2015"
SIZES = [(2, 35, 35), (2, 17, 17), (3, 8, 8), (2, 1, 1), (2, 2, 2), (2, 3, 5)]
# (C, raw row stride, raw channel offset, output channels, output offset): the pool slices of Mixed_5b, 5c, 6b and 7b
SLICES = [(32, 208, 176, 256, 224), (64, 240, 176, 288, 224), (192, 640, 448, 768, 576), (192, 1344, 1152, 2048, 1856)]


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _excl_ref(raw64, bias64):
    """fp64: relu(avg_pool2d(count_include_pad=False) + bias), NHWC in and out."""
    y = F.avg_pool2d(raw64.permute(0, 3, 1, 2), 3, 1, 1, count_include_pad=False) + bias64.view(1, -1, 1, 1)
    return torch.relu(y).permute(0, 2, 3, 1)


# ------------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("size", SIZES)
def test_exclude_padding_avgpool_fp32_vs_fp64(cuda_device, size):
    from tise_toolbox_amd.trunk import FusedTrunk
    n, h, w = size
    g = torch.Generator().manual_seed(h * 100 + w)
    for C, ld, off, out_ld, out_off in SLICES:
        raw = torch.randn((n, h, w, ld), generator=g).to(cuda_device)
        bias = torch.randn(C, generator=g).to(cuda_device)
        out = torch.full((n, h, w, out_ld), -5.0, device=cuda_device)
        FusedTrunk._avgpool_bias_relu(raw, bias, off, C, out, out_off, excl=True)
        want = _excl_ref(raw[..., off:off + C].double(), bias.double())
        assert (out[..., out_off:out_off + C].double() - want).abs().max().item() <= 1e-6 * max(1.0, want.abs().max().item()), (size, C)
        rest = torch.cat([out[..., :out_off], out[..., out_off + C:]], -1)
        assert bool((rest == -5.0).all())                                   # nothing outside the slice touched
        if h > 1 and w > 1:                                                 # the corner divisor is 4, not 9
            corner = raw[0, :2, :2, off:off + C].double().sum((0, 1)) / 4 + bias.double()
            assert torch.allclose(out[0, 0, 0, out_off:out_off + C].double(), corner.clamp_min(0), atol=1e-6)


@pytest.mark.parametrize("size", SIZES)
def test_exclude_padding_avgpool_split_vs_fp64(cuda_device, size):
    from tise_toolbox_amd import _lib
    from tise_toolbox_amd.conv_split import merge
    from tise_toolbox_amd.trunk import SplitTrunk
    n, h, w = size
    g = torch.Generator().manual_seed(7 + h * 100 + w)
    for C, ld, off, out_ld, out_off in SLICES:
        raw = torch.randn((n, h, w, ld), generator=g).to(cuda_device)
        bias = torch.randn(C, generator=g).to(cuda_device)
        out = torch.zeros((n, h, w, 2 * out_ld), dtype=torch.float16, device=cuda_device)
        # a raw slice inside a wider row (the entry point's stride / offset) ...
        _lib.call("tise_avgpool3_excl_bias_relu_split_nhwc", _p(raw), ld, off, n, h, w, C, _p(bias), _p(out), out_ld,
                  out_off, _s())
        want = _excl_ref(raw[..., off:off + C].double(), bias.double())
        got = merge(out).double()
        tol = 2e-6 * max(1.0, want.abs().max().item())
        assert (got[..., out_off:out_off + C] - want).abs().max().item() <= tol, (size, C)
        assert not torch.cat([got[..., :out_off], got[..., out_off + C:]], -1).any()
        # ... and the packed raw tensor the trunk hands over
        packed = raw[..., off:off + C].contiguous()
        out2 = torch.zeros_like(out)
        SplitTrunk._avgpool_split(packed, bias, out2, out_off, excl=True)
        assert torch.equal(out2, out)
        # the default network's kernel on the same data is the count_include_pad average
        out3 = torch.zeros_like(out)
        SplitTrunk._avgpool_split(packed, bias, out3, out_off)
        inc = torch.relu(F.avg_pool2d(packed.double().permute(0, 3, 1, 2), 3, 1, 1) + bias.double().view(1, -1, 1, 1)).permute(0, 2, 3, 1)
        assert (merge(out3).double()[..., out_off:out_off + C] - inc).abs().max().item() <= tol


@pytest.mark.parametrize("size", SIZES)
def test_maxpool_s1p1_negative_inputs(cuda_device, size):
    """All-negative inputs: a pool that padded with zeros would return 0 on the border."""
    from tise_toolbox_amd import _lib
    from tise_toolbox_amd.conv_split import merge, split
    from tise_toolbox_amd.trunk import FusedTrunk, SplitTrunk
    n, h, w = size
    g = torch.Generator().manual_seed(11 + h * 100 + w)
    for C in (2048, 192, 64):
        x = (-1.0 - torch.rand((n, h, w, C), generator=g) * 4.0).to(cuda_device)
        want = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 1, 1).permute(0, 2, 3, 1).contiguous()
        assert bool((want < 0).all())
        got = FusedTrunk._maxpool_s1(x)
        assert torch.equal(got, want)
        xs = split(x)
        gs = SplitTrunk._maxpool_s1_split(xs)
        assert torch.equal(merge(gs), F.max_pool2d(merge(xs).permute(0, 3, 1, 2), 3, 1, 1).permute(0, 2, 3, 1).contiguous())
        # channel slices: fp32 and split, input slice at an offset, output slice at an offset
        wide = torch.cat([torch.randn((n, h, w, 32), generator=g).to(cuda_device), x], -1).contiguous()
        o = torch.full((n, h, w, C + 64), 3.0, device=cuda_device)
        _lib.call("tise_maxpool3s1p1_nhwc", _p(wide), C + 32, 32, n, h, w, C, _p(o), C + 64, 16, _s())
        assert torch.equal(o[..., 16:16 + C], want) and bool((o[..., :16] == 3).all()) and bool((o[..., 16 + C:] == 3).all())
        ws = split(wide)
        os_ = torch.zeros((n, h, w, 2 * (C + 64)), dtype=torch.float16, device=cuda_device)
        _lib.call("tise_maxpool3s1p1_split_nhwc", _p(ws), C + 32, 32, n, h, w, C, _p(os_), C + 64, 32, _s())
        m = merge(os_)
        assert torch.equal(m[..., 32:32 + C], merge(gs)) and not m[..., :32].any() and not m[..., 32 + C:].any()


def test_split_maxpool_then_conv_is_pool_then_conv(cuda_device):
    """Mixed_7c's pool branch on the split path (max pool of the split tensor, then the 1x1 split conv) equals the 1x1
    conv of the fp64 max pool of the same values to the conv's own accuracy."""
    from tise_toolbox_amd.conv_split import SplitConv, merge, split
    from tise_toolbox_amd.trunk import SplitTrunk
    g = torch.Generator().manual_seed(3)
    x = (torch.randn((4, 8, 8, 2048), generator=g) - 0.5).to(cuda_device)
    wt = (torch.randn((192, 2048, 1, 1), generator=g) * (2.0 / 2048) ** 0.5).to(cuda_device)
    b = (torch.randn(192, generator=g) * 0.2).to(cuda_device)
    conv = SplitConv(wt, b, (1, 1), (0, 0), cuda_device)
    xs = split(x)
    out = torch.zeros((4, 8, 8, 2 * 2048), dtype=torch.float16, device=cuda_device)
    conv(SplitTrunk._maxpool_s1_split(xs), [(0, 192, out, 1856, 0)])
    pooled = F.max_pool2d(merge(xs).double().permute(0, 3, 1, 2), 3, 1, 1)
    want = torch.relu(F.conv2d(pooled, wt.double(), b.double())).permute(0, 2, 3, 1)
    got = merge(out)[..., 1856:].double()
    assert (got - want).abs().max().item() <= 4e-6 * want.abs().max().item()


# ------------------------------------------------------------------------------------------------------- trunks
@pytest.fixture(scope="module")
def net2015(cuda_device):
    from tise_toolbox_amd.inception import build_inception3
    torch.set_num_threads(min(16, torch.get_num_threads()))
    sd = {k: v.float() for k, v in build_inception3(seed=0, network=NET).state_dict().items()}
    u8 = np.stack([resize_oracle.resize_bilinear_u8(im, 299, 299) for im in _cases.smooth_images(4, 256, 256, seed=5)])
    feats, logits = ref.features_of_u8(sd, u8, torch.float64, chunk=4)
    return dict(sd=sd, u8=u8, feats=feats, logits=logits)


@pytest.mark.parametrize("conv", ["split", "miopen"])
def test_trunk_features_and_logits_vs_fp64(cuda_device, net2015, conv, monkeypatch):
    from tise_toolbox_amd.engine import RealismEngine
    from tise_toolbox_amd.trunk import FusedTrunk, SplitTrunk
    monkeypatch.setenv("TISE_CONV", conv)
    torch.backends.cudnn.benchmark = False
    eng = RealismEngine(dims=2048, seed=0, with_logits=True, network=NET)
    assert type(eng.fused) is (SplitTrunk if conv == "split" else FusedTrunk) and eng.fused.avg_excl
    assert eng.model.fc.out_features == 1008
    feats, logits = eng.features_from_u8(torch.as_tensor(net2015["u8"], device=cuda_device))
    f, want = feats.double().cpu().numpy(), net2015["feats"]
    print(conv, "pool3 max abs err", np.abs(f - want).max(), "scale", np.abs(want).max())
    assert np.abs(f - want).max() <= 2e-4 * np.abs(want).max()
    lg, lw = logits.double().cpu().numpy(), net2015["logits"]
    assert lg.shape == (4, 1008)
    assert np.abs(lg - lw).max() <= 2e-3 * max(1.0, np.abs(lw).max())


def test_variant_switch_is_wired(cuda_device, net2015):
    """The same weights through the torchvision pools give different features: the switch reaches the kernels."""
    from tise_toolbox_amd.inception import InceptionV3
    from tise_toolbox_amd.trunk import SplitTrunk
    m = InceptionV3([3], seed=0, network=NET).to(cuda_device).eval()
    x = torch.as_tensor(net2015["u8"], device=cuda_device)
    from tise_toolbox_amd import device
    lut = torch.from_numpy(device.make_lut(network=NET).reshape(-1)).to(cuda_device)
    a = SplitTrunk(m, cuda_device).forward_u8(x, lut).flatten(1).clone()
    m.network = "torchvision"
    for mod in m.modules():
        if hasattr(mod, "pool"):
            mod.pool = "avg"
    b = SplitTrunk(m, cuda_device).forward_u8(x, lut).flatten(1)
    assert np.abs(a.double().cpu().numpy() - net2015["feats"]).max() <= 2e-4 * np.abs(net2015["feats"]).max()
    assert (a - b).abs().max().item() > 1e-2 * a.abs().max().item()


# ----------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def images(cuda_device):
    gen = _cases.smooth_images(130, 96, 112, seed=21)
    ref_imgs = _cases.smooth_images(18, 96, 112, seed=22, shift=0.15)
    return gen, ref_imgs


def _write(d, imgs):
    from PIL import Image
    d.mkdir(parents=True)
    for i, im in enumerate(imgs):
        Image.fromarray(im).save(d / f"{i:05d}.png")


def _cpu_features(sd, files):
    from PIL import Image
    u8 = np.stack([resize_oracle.resize_bilinear_u8(np.asarray(Image.open(f).convert("RGB")), 299, 299) for f in files])
    return ref.features_of_u8(sd, u8, torch.float32, chunk=16)


def test_is_cli_inception2015_vs_cpu(cuda_device, net2015, images, tmp_path, capsys, monkeypatch):
    from tise_toolbox_amd import img_data, inception_score as isc
    monkeypatch.setenv("TISE_CONV", "split")
    d = tmp_path / "imgs"
    _write(d, images[0])
    out = tmp_path / "is.txt"
    try:
        _is_cli_checks(isc, img_data, d, out, net2015, capsys, monkeypatch)
    finally:
        isc.configure(network="torchvision")


def _is_cli_checks(isc, img_data, d, out, net2015, capsys, monkeypatch):
    mean, std = isc.main(["--image_folder", str(d), "--saved_file", str(out), "--batch-size", "7", "--synthetic-weights",
                          "--network", NET])
    assert out.read_text() == "[Inception Score] mean: {:.5f} std: {:.5f}".format(mean, std) + SYNTHETIC_TAG
    assert "[Inception Score] mean: {:.2f} std: {:.2f}".format(mean, std) + SYNTHETIC_TAG in capsys.readouterr().out
    assert isc._ENGINE.model.fc.out_features == 1008 and isc._ENGINE.model.network == NET
    _, lg = _cpu_features(net2015["sd"], img_data.get_filenames(str(d)))
    want = is_oracle.inception_score_from_logits(lg, is_oracle.T_COCO, 10, "coco", dtype=np.float64)
    print("IS* inception-2015 device", mean, std, "cpu", want)
    assert abs(mean - want[0]) <= 1e-4 and abs(std - want[1]) <= 1e-4
    # the exact-fp32 convolution path agrees with the split path
    monkeypatch.setenv("TISE_CONV", "miopen")
    m2, s2 = isc.main(["--image_folder", str(d), "--batch-size", "7", "--synthetic-weights", "--network", NET])
    assert abs(m2 - mean) <= 1e-4 and abs(s2 - std) <= 1e-4
    # the default network's result is what it was: --network torchvision is the default, bit for bit
    monkeypatch.setenv("TISE_CONV", "split")
    d0 = isc.main(["--image_folder", str(d), "--batch-size", "7", "--synthetic-weights"])
    d1 = isc.main(["--image_folder", str(d), "--batch-size", "7", "--synthetic-weights", "--network", "torchvision"])
    assert d0 == d1 and isc._ENGINE.model.fc.out_features == 1000 and d0 != (mean, std)


def test_fid_cli_inception2015_vs_cpu(cuda_device, net2015, images, tmp_path, monkeypatch):
    from tise_toolbox_amd import fid_score, img_data
    monkeypatch.setenv("TISE_CONV", "split")
    gdir, rdir = tmp_path / "gen", tmp_path / "ref"
    _write(gdir, images[0][:21])
    _write(rdir, images[1])
    stats = tmp_path / "gen_stats.npz"
    argv = ["--batch-size", "5", "--path1", str(rdir), "--path2", str(gdir), "--num-workers", "0", "--synthetic-weights",
            "--network", NET]
    v = fid_score.main(argv + ["--save-stats", str(stats)])

    def cpu_stats(root):
        files = img_data.get_filenames(str(root))
        files = files[:fid_oracle.n_used_images(len(files), 5)]
        f, _ = _cpu_features(net2015["sd"], files)
        return fid_oracle.calculate_activation_statistics(f.astype(np.float64))
    want = fid_oracle.calculate_frechet_distance(*cpu_stats(rdir), *cpu_stats(gdir))
    print("FID inception-2015 device", v, "cpu", want)
    assert abs(v - want) <= 1e-3
    with np.load(stats) as f:
        assert str(f["network"]) == NET
    # the tagged statistics serve a run on the same network and are refused by the default one
    v2 = fid_score.main(["--batch-size", "5", "--path1", str(stats), "--path2", str(rdir), "--num-workers", "0",
                         "--synthetic-weights", "--network", NET])
    assert abs(v2 - v) <= 1e-6 * max(1.0, abs(v))
    with pytest.raises(RuntimeError, match="statistics of network"):
        fid_score.main(["--batch-size", "5", "--path1", str(stats), "--path2", str(rdir), "--num-workers", "0",
                        "--synthetic-weights"])
    # --conv exact agrees with the split path
    v3 = fid_score.main(argv + ["--conv", "exact"])
    assert abs(v3 - v) <= 1e-3
