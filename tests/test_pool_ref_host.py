"""CPU: (1) the numpy emulations of tests/_pool_ref.py against torch's fp64 ops, at the bound the older GPU tests allow the
kernels themselves (2e-6 of the output scale) -- the expected values of tests/test_gpu_pool_kernels.py are shown right by
something other than the kernels -- and the numpy split layout against conv_split's; (2) non-finite parameters are refused
where the trunks take their weights: one case per loader that ends in the trunk, the folded parameters, SplitConv, the
classifier layer (the fused ReLUs would turn a NaN into 0 silently: csrc/common.h)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _pool_ref as pr

TOL = 2e-6


def _nchw(x):
    return torch.from_numpy(np.asarray(x)).double().permute(0, 3, 1, 2)


def _close(got, want, what):
    want = want.permute(0, 2, 3, 1).numpy()
    scale = max(float(np.abs(want).max()), 1e-30)
    err = float(np.abs(got.astype(np.float64) - want).max())
    assert got.dtype == np.float32 and got.shape == want.shape and err <= TOL * scale, (what, err, scale)


@pytest.mark.parametrize("hw", pr.MAPS_S1)
def test_stride1_emulations_match_fp64(hw):
    h, w = hw
    g = np.random.default_rng(h * 100 + w)
    x = g.standard_normal((3, h, w, 8)).astype(np.float32)
    b = g.standard_normal(8).astype(np.float32)
    bb = torch.from_numpy(b).double().view(1, -1, 1, 1)
    for excl in (False, True):
        want = torch.relu(F.avg_pool2d(_nchw(x), 3, 1, 1, count_include_pad=not excl) + bb)
        _close(pr.avgpool_per_output(x, b, excl), want, ("per-output", excl))
        _close(pr.avgpool_colwalk(x, b, excl), want, ("colwalk", excl))
    _close(pr.maxpool3s1p1(x), F.max_pool2d(_nchw(x), 3, 1, 1), "maxpool s1")
    assert np.array_equal(pr.maxpool3s1p1(x), F.max_pool2d(_nchw(x), 3, 1, 1).permute(0, 2, 3, 1).numpy().astype(np.float32))
    _close(pr.bias_relu(x, b), torch.relu(_nchw(x) + bb), "bias_relu")


@pytest.mark.parametrize("hw", pr.MAPS_S2)
def test_stride2_emulations_match_fp64(hw):
    h, w = hw
    g = np.random.default_rng(h * 100 + w)
    x = g.standard_normal((3, h, w, 8)).astype(np.float32)
    b = g.standard_normal(8).astype(np.float32)
    bb = torch.from_numpy(b).double().view(1, -1, 1, 1)
    want = F.max_pool2d(_nchw(x), 3, 2)
    assert np.array_equal(pr.maxpool3s2(x), want.permute(0, 2, 3, 1).numpy().astype(np.float32))
    _close(pr.maxpool3s2(x, b), F.max_pool2d(torch.relu(_nchw(x) + bb), 3, 2), "maxpool s2 + bias")      # ReLU and max commute
    xs = (g.random((3, h, w, 3)) * 2.4 - 1.2).astype(np.float32)
    wt = (g.standard_normal((3, 3, 3, 32)) * (2.0 / 27) ** 0.5).astype(np.float32)
    b32 = (g.standard_normal(32) * 0.2).astype(np.float32)
    want = torch.relu(torch.conv2d(_nchw(xs), torch.from_numpy(wt).double().permute(3, 2, 0, 1), torch.from_numpy(b32).double(), 2))
    _close(pr.stem_fma(xs, wt, b32), want, "stem")


def test_split_layout_matches_conv_split():
    from tise_toolbox_amd import conv_split as cs
    g = np.random.default_rng(7)
    for C in (16, 32, 48, 80, 112):
        v = (g.random((2, 3, C)) * 5).astype(np.float32)
        t = np.zeros((2, 3, 2 * C), dtype=np.float16)
        pr.pack_split(t, v, 0)
        assert np.array_equal(pr.bits(t), pr.bits(cs.split(torch.from_numpy(v)).numpy())), C
        hi, lo = pr.unpack_split(t)
        assert np.array_equal(pr.merge_value(hi, lo), cs.merge(torch.from_numpy(t)).numpy())
        assert np.array_equal(pr.merge_value(hi, lo).astype(np.float64), hi.astype(np.float64) + lo.astype(np.float64) / 2048)   # exact
        m = pr.slice_mask(C, 8, 8)
        assert m.sum() == 16
    # a slice write touches its own positions only
    t = np.full((1, 2 * 80), 7.0, dtype=np.float16)
    pr.pack_split(t, np.ones((1, 8), np.float32), 72)
    assert np.all(t[:, ~pr.slice_mask(80, 72, 8)] == 7.0) and np.all(pr.unpack_split(t, 72, 8)[0] == 1.0)


# ------------------------------------------------------------------------------------- non-finite parameters are refused
def _plant(sd, key, value):
    sd = {k: v.clone() for k, v in sd.items()}
    sd[key].view(-1)[sd[key].numel() // 2] = value
    return sd


@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
def test_torchvision_checkpoint_with_a_nonfinite_tensor_is_refused(tmp_path, value):
    from tise_toolbox_amd.inception import Inception3, build_inception3
    g = torch.Generator().manual_seed(0)
    sd = {k: (torch.rand(v.shape, generator=g) + 0.5 if v.is_floating_point() else torch.zeros_like(v, device="cpu"))
          for k, v in Inception3().state_dict().items()}
    torch.save(sd, tmp_path / "ok.pth")
    build_inception3(str(tmp_path / "ok.pth"))                                          # the finite file loads
    for key in ("Mixed_6c.branch7x7_2.bn.running_var", "Conv2d_1a_3x3.conv.weight", "fc.weight"):
        torch.save(_plant(sd, key, value), tmp_path / "bad.pth")
        with pytest.raises(ValueError, match=key.rsplit(".", 1)[0].replace(".", r"\.")):
            build_inception3(str(tmp_path / "bad.pth"))
    torch.save(_plant(sd, "AuxLogits.fc.weight", value), tmp_path / "aux.pth")          # not evaluated: not refused
    build_inception3(str(tmp_path / "aux.pth"))


@pytest.mark.parametrize("value", [float("nan"), float("inf")])
def test_inception2015_checkpoint_with_a_nonfinite_tensor_is_refused(tmp_path, value):
    from tests import _inception2015_ref as ref
    from tise_toolbox_amd.inception import InceptionV3
    sd = ref.random_state_dict(3)
    torch.save(_plant(sd, "Mixed_7c.branch_pool.bn.bias", value), tmp_path / "bad.pth")
    with pytest.raises(ValueError, match=r"Mixed_7c\.branch_pool\.bn"):
        InceptionV3([3], weights=str(tmp_path / "bad.pth"), network="inception-2015")


@pytest.mark.parametrize("value", [float("nan"), float("inf")])
def test_slim_checkpoint_with_a_nonfinite_tensor_is_refused(tmp_path, value):
    from tests._tf_ckpt_writer import write_slim_checkpoint
    from tests.test_slim_bird_host import _random_slim_state
    from tise_toolbox_amd.inception import build_inception3
    sd = _plant(_random_slim_state(4), "Mixed_5d.branch5x5_2.conv.weight", value)
    path = write_slim_checkpoint(str(tmp_path / "model.ckpt"), sd, block_size=65536)
    with pytest.raises(ValueError, match=r"Mixed_5d\.branch5x5_2\.conv"):
        build_inception3(weights=path, network="slim")


def _tiny_trunk_model():
    """An InceptionV3 wrapper with finite random parameters, built without the stand-in calibration."""
    from tests import _inception2015_ref as ref
    from tise_toolbox_amd.inception import InceptionV3
    import os
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "w.pth")
        torch.save(ref.random_state_dict(5), p)
        return InceptionV3([3], weights=p, network="inception-2015")


def test_trunk_refuses_nonfinite_folded_parameters_naming_the_layer():
    """What no file check can see: finite tensors whose FOLD is not (a negative running variance: sqrt -> NaN; a variance
    of -eps: 1 / 0 -> Inf), and a model handed over in memory.  FusedTrunk (the base of SplitTrunk) checks the folded
    weight, scale and bias of every layer and the classifier layer, and names the first bad layer."""
    from tise_toolbox_amd.trunk import FusedTrunk
    m = _tiny_trunk_model()
    FusedTrunk(m, torch.device("cpu"))                                                  # finite: accepted
    bn = m.blocks[2][4].branch7x7_3.bn                                                  # Mixed_6b
    keep = bn.running_var.clone()
    with torch.no_grad():
        bn.running_var[5] = -1.0
    with pytest.raises(ValueError, match=r"blocks\.2\.4\.branch7x7_3"):
        FusedTrunk(m, torch.device("cpu"))
    with torch.no_grad():
        bn.running_var.copy_(keep)
        bn.running_var[5] = -bn.eps
    with pytest.raises(ValueError, match=r"blocks\.2\.4\.branch7x7_3"):
        FusedTrunk(m, torch.device("cpu"))
    with torch.no_grad():
        bn.running_var.copy_(keep)
        m.blocks[0][0].conv.weight[3, 1, 2, 0] = float("nan")                           # the stem layer's table
    with pytest.raises(ValueError, match=r"blocks\.0\.0"):
        FusedTrunk(m, torch.device("cpu"))
    with torch.no_grad():
        m.blocks[0][0].conv.weight[3, 1, 2, 0] = 0.5
        m.fc.bias[7] = float("inf")
    with pytest.raises(ValueError, match=r"layer fc"):
        FusedTrunk(m, torch.device("cpu"))


@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
def test_split_conv_refuses_nonfinite_weights_and_bias(value):
    from tise_toolbox_amd.conv_split import SplitConv
    w = torch.full((64, 32, 1, 1), 0.25)
    b = torch.zeros(64)
    SplitConv(w, b, (1, 1), (0, 0), "cpu", name="ok")
    wb = w.clone()
    wb[9, 4, 0, 0] = value
    with pytest.raises(ValueError, match="SplitConv Mixed_x"):
        SplitConv(wb, b, (1, 1), (0, 0), "cpu", name="Mixed_x")
    bb = b.clone()
    bb[63] = value
    with pytest.raises(ValueError, match="bias"):
        SplitConv(w, bb, (1, 1), (0, 0), "cpu")
