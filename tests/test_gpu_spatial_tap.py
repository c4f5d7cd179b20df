"""GPU: the spatial tap of the split trunk -- tise_split_tap_rows (csrc/trunk_ops.hip), SplitTrunk(spatial=True) and
RealismEngine(resize="tf1", spatial=True).

Kernel: a channel slice of a split tensor as fp32 rows against conv_split.merge, bit for bit, across a 32-channel block
boundary and into the 16-wide tail.  Trunk: the rows after Mixed_6d against a forward hook on the fp64 module.  Engine: the tap
changes nothing else, the tf1 route feeds the trunk the restatement's bits, and an engine built without the new arguments
launches what it launched before."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _cases
from tests import _tf1_resize_ref as tf1

pytestmark = pytest.mark.gpu

NET = "inception-2015"
# (n, h, w, C, c0, nc, ld)
TAP_CASES = [(2, 17, 17, 192, 0, 7, 2048),      # sFID's tap: 2023 values, 25 padding columns
             (1, 3, 5, 48, 28, 7, 108),         # crosses from the 32-block into the 16-wide tail
             (3, 1, 1, 32, 25, 7, 7),           # no padding
             (1, 2, 2, 64, 30, 4, 16)]          # crosses a 32-block boundary


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("n,h,w,C,c0,nc,ld", TAP_CASES, ids=lambda v: str(v))
def test_tap_kernel_matches_merge_bit_for_bit(cuda_device, n, h, w, C, c0, nc, ld):
    import ctypes
    from tise_toolbox_amd import _lib, device
    from tise_toolbox_amd.conv_split import merge, split
    g = torch.Generator().manual_seed(100 * C + c0)
    # a split tensor as the trunk writes it (lo below half an ulp of hi) ...
    t = split(torch.randn((n, h, w, C), generator=g) * 3.0).to(cuda_device)
    # ... and one of unrelated halves, whose sum is NOT exact in fp32: one rounding, as merge's
    r = torch.randn((n, h, w, 2 * C), generator=g).half().to(cuda_device)
    for x in (t, r):
        want = merge(x)[..., c0:c0 + nc].reshape(n, -1)
        out = torch.full((n, ld), float("nan"), dtype=torch.float32, device=cuda_device)
        _lib.call("tise_split_tap_rows", ctypes.c_void_p(x.data_ptr()), n, h * w, C, c0, nc, ctypes.c_void_p(out.data_ptr()), ld,
                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        used = h * w * nc
        assert torch.equal(_bits(out[:, :used]), _bits(want))
        assert out[:, used:].numel() == n * (ld - used) and bool((_bits(out[:, used:]) == 0).all())      # padding is +0.0
        assert torch.equal(_bits(device.split_tap_rows(x, c0, nc, ld)), _bits(out))


def test_tap_refusals(cuda_device):
    from tise_toolbox_amd import device
    t = torch.zeros((1, 2, 2, 128), dtype=torch.float16, device=cuda_device)
    for c0, nc, ld in ((0, 7, 27), (-1, 7, 64), (60, 7, 64), (0, 0, 64), (64, 1, 64)):
        with pytest.raises(ValueError):
            device.split_tap_rows(t, c0, nc, ld)
    with pytest.raises(ValueError):
        device.split_tap_rows(t.float(), 0, 7, 64)


# ------------------------------------------------------------------------------------------------------- trunk and engine
@pytest.fixture(scope="module")
def split_conv():
    old = os.environ.get("TISE_CONV")
    os.environ["TISE_CONV"] = "split"
    yield
    if old is None:
        os.environ.pop("TISE_CONV", None)
    else:
        os.environ["TISE_CONV"] = old


@pytest.fixture(scope="module")
def images():
    u8 = _cases.smooth_images(4, 64, 72, seed=31)
    x = tf1.network_input_tf1(u8, (299, 299))                          # (4, 299, 299, 3) fp32, the restatement's bits
    u8.setflags(write=False)
    x.setflags(write=False)
    return u8, x


@pytest.fixture(scope="module")
def engines(cuda_device, split_conv):
    from tise_toolbox_amd.engine import RealismEngine
    torch.set_num_threads(min(16, torch.get_num_threads()))
    kw = dict(dims=2048, seed=0, network=NET, with_logits=True)
    return dict(spatial=RealismEngine(resize="tf1", spatial=True, **kw), tf1=RealismEngine(resize="tf1", **kw), default=RealismEngine(**kw))


def _mixed_6d_rows(x_nhwc, dtype):
    """The first 7 channels of Mixed_6d's branch1x1 output (after ReLU) in h, w, c order, from a forward hook on the CPU module
    in ``dtype`` (seeded Inception-2015 parameters, built as the net2015 fixture of tests/test_gpu_inception2015.py builds them)."""
    from tise_toolbox_amd.inception import build_inception3
    net = build_inception3(seed=0, network=NET).to(dtype).eval()
    got = []
    hook = net.Mixed_6d.branch1x1.register_forward_hook(lambda m, i, o: got.append(o.detach().clone()))
    with torch.no_grad():
        x = torch.as_tensor(np.ascontiguousarray(x_nhwc)).to(dtype).permute(0, 3, 1, 2)
        x = net.Conv2d_2b_3x3(net.Conv2d_2a_3x3(net.Conv2d_1a_3x3(x)))
        x = F.max_pool2d(x, kernel_size=3, stride=2)
        x = net.Conv2d_4a_3x3(net.Conv2d_3b_1x1(x))
        x = F.max_pool2d(x, kernel_size=3, stride=2)
        for name in ("Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d"):
            x = getattr(net, name)(x)
    hook.remove()
    assert len(got) == 1 and tuple(got[0].shape[1:]) == (192, 17, 17)
    return got[0][:, :7].permute(0, 2, 3, 1).reshape(got[0].shape[0], -1).numpy()


def test_trunk_rows_vs_fp64_hook(cuda_device, engines, images):
    _, x = images
    e = engines["spatial"]
    xin = torch.as_tensor(np.array(x), device=cuda_device).permute(0, 3, 1, 2)             # NCHW view, channels_last storage
    e._trunk(xin, prenormalized=True)
    rows = e.spatial_rows()
    assert tuple(rows.shape) == (4, 2048) and rows.dtype == torch.float32
    rows = rows.cpu().numpy()
    want = _mixed_6d_rows(x, torch.float64)
    assert want.shape == (4, 2023) and np.abs(want).max() > 0
    err = np.abs(rows[:, :2023].astype(np.float64) - want).max()
    print("Mixed_6d tap max abs err", err, "scale", np.abs(want).max())
    assert err <= 2e-4 * np.abs(want).max()
    assert not rows[:, 2023:].any() and not np.signbit(rows[:, 2023:]).any()                 # exactly +0


def test_spatial_engine_changes_nothing_else(cuda_device, engines, images):
    u8 = torch.as_tensor(np.array(images[0]), device=cuda_device)
    fa, la = engines["spatial"].features_from_u8(u8)
    fb, lb = engines["tf1"].features_from_u8(u8)
    assert tuple(fa.shape) == (4, 2048) and tuple(la.shape) == (4, 1008)
    assert torch.equal(_bits(fa), _bits(fb)) and torch.equal(_bits(la), _bits(lb))
    assert engines["tf1"].fused._spatial_rows is None and not engines["tf1"].spatial


def test_tf1_route_feeds_the_restatements_bits(cuda_device, engines, images):
    u8, x = images
    e = engines["tf1"]
    got, lg = e.features_from_u8(torch.as_tensor(np.array(u8), device=cuda_device))
    xin = torch.as_tensor(np.array(x), device=cuda_device).permute(0, 3, 1, 2)
    want, lw = e._trunk(xin, prenormalized=True)
    assert torch.equal(_bits(got), _bits(want)) and torch.equal(_bits(lg), _bits(lw))
    # and it is another route than the uint8 one
    other, _ = engines["default"].features_from_u8(torch.as_tensor(np.array(u8), device=cuda_device))
    assert not torch.equal(got, other)


def test_default_engine_is_todays(cuda_device, engines, images):
    """Without the new arguments: the uint8 resize, the uint8 stem and the same trunk launches as before, no tap."""
    from tise_toolbox_amd import device
    from tise_toolbox_amd.trunk import SplitTrunk
    e = engines["default"]
    assert e.resize == "reference" and e.spatial is False and isinstance(e.fused, SplitTrunk) and e.fused.spatial is False
    u8 = torch.as_tensor(np.array(images[0]), device=cuda_device)
    got, lg = e.features_from_u8(u8)
    trunk = SplitTrunk(e.model, cuda_device)                           # built as before this feature: no keyword
    want = trunk.forward_u8(device.resize_u8_only(u8, (299, 299)), e.lut_dev).flatten(1)
    assert torch.equal(_bits(got), _bits(want))
    assert torch.equal(_bits(lg), _bits(trunk.fc_logits(4, bias=False)))
    assert e.fused._spatial_rows is None and trunk._spatial_rows is None
    e.begin(n_total=4)
    assert e.stats_spatial is None
    e.step_u8(u8)
    with pytest.raises(ValueError):
        e.statistics_spatial()
    with pytest.raises(ValueError):
        e.spatial_rows()


def test_spatial_statistics_follow_the_rows(cuda_device, engines, images):
    e = engines["spatial"]
    u8 = torch.as_tensor(np.array(images[0]), device=cuda_device)
    e.features_from_u8(u8)
    rows = e.spatial_rows().double().cpu().numpy()[:, :2023]
    e.begin(n_total=4, temperature=1.0, splits=1)
    e.step_u8(u8[:3], 0)
    e.step_u8(u8[3:], 3)
    e.reduce()
    mu, sigma = e.statistics_spatial()
    assert tuple(mu.shape) == (2023,) and tuple(sigma.shape) == (2023, 2023)
    scale = np.abs(rows).max()
    assert np.abs(mu.cpu().numpy() - rows.mean(0)).max() <= 1e-12 * scale
    assert np.abs(sigma.cpu().numpy() - np.cov(rows, rowvar=False)).max() <= 1e-12 * scale * scale


def test_refusals(cuda_device, split_conv, monkeypatch):
    from tise_toolbox_amd.engine import RealismEngine
    with pytest.raises(ValueError, match="inception-2015"):
        RealismEngine(resize="tf1")                                    # the default network
    with pytest.raises(ValueError):
        RealismEngine(resize="tf2", network=NET)
    with pytest.raises(ValueError):
        RealismEngine(dims=768, network=NET, spatial=True)             # the tap sits behind Mixed_6d of the whole trunk
    monkeypatch.setenv("TISE_CONV", "miopen")
    with pytest.raises(ValueError, match="split"):
        RealismEngine(network=NET, spatial=True)
