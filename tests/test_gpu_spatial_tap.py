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


# The launch caps its grid at 16 384 workgroups of 256 threads: n * ld above TAP_STRIDE goes round the grid-stride loop.
TAP_STRIDE = 16384 * 256
# (n, h, w, C, c0, nc, ld), each just past the cap
TAP_PAST_THE_CAP = [(2049, 17, 17, 16, 0, 7, 2048),     # the first n at which sFID's rows (ld = 2048) stride; C = 16: all tail
                    (2071, 17, 17, 16, 0, 7, 2027),     # odd ld: n * ld is odd, a partial last workgroup, rows shift per round
                    (32515, 1, 3, 48, 28, 7, 129),      # crosses from the 32-block into the 16-wide tail, odd total
                    (32515, 2, 2, 64, 30, 4, 129)]      # crosses a 32-block boundary, odd total


@pytest.mark.parametrize("n,h,w,C,c0,nc,ld", TAP_PAST_THE_CAP, ids=lambda v: str(v))
def test_tap_kernel_past_the_grid_cap(cuda_device, n, h, w, C, c0, nc, ld):
    """More output values than the capped grid has threads: the second round of the loop writes the tail.  Every value is
    bit-equal to conv_split.merge's slice in h, w, c order, the padding is exactly +0 and the source's bits are unchanged."""
    import ctypes
    from tise_toolbox_amd import _lib
    from tise_toolbox_amd.conv_split import merge, split
    total = n * ld
    assert TAP_STRIDE < total < 2 * TAP_STRIDE and (ld == 2048 or total % 256)
    g = torch.Generator(device=cuda_device).manual_seed(100 * C + c0)
    t = split(torch.randn((n, h, w, C), generator=g, device=cuda_device) * 3.0).contiguous()
    before = t.clone()
    want = merge(t)[..., c0:c0 + nc].reshape(n, -1)
    out = torch.full((n, ld), float("nan"), dtype=torch.float32, device=cuda_device)
    _lib.call("tise_split_tap_rows", ctypes.c_void_p(t.data_ptr()), n, h * w, C, c0, nc, ctypes.c_void_p(out.data_ptr()), ld,
              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    used = h * w * nc
    assert used < ld
    rows = torch.nonzero((_bits(out[:, :used]) != _bits(want)).any(dim=1)).flatten().tolist()
    assert not rows, f"{len(rows)} of {n} rows differ from merge: first {rows[0]}, last {rows[-1]}"
    pad = _bits(out[:, used:])
    assert pad.numel() == n * (ld - used) and bool((pad == 0).all())                                  # +0.0: no sign bit, no NaN left
    assert not bool(torch.signbit(out[:, used:]).any())
    assert torch.equal(t.view(torch.int16), before.view(torch.int16))


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


def test_spatial_engine_changes_nothing_else_on_the_clean_route(cuda_device, split_conv, images):
    """The other float route: resize="clean" with and without the tap gives the same pool3 and logits, bit for bit, and the
    tap's rows there are the tap of the SAME trunk -- the rows a resize="tf1" engine's trunk gives on the clean input."""
    from tise_toolbox_amd import device
    from tise_toolbox_amd.engine import RealismEngine
    kw = dict(dims=2048, seed=0, network=NET, with_logits=True, resize="clean")
    u8 = torch.as_tensor(np.array(images[0]), device=cuda_device)
    with_tap, without = RealismEngine(spatial=True, **kw), RealismEngine(**kw)
    fa, la = with_tap.features_from_u8(u8)
    fa, la = fa.clone(), la.clone()
    rows = with_tap.spatial_rows().clone()
    fb, lb = without.features_from_u8(u8)
    assert tuple(fa.shape) == (4, 2048) and tuple(la.shape) == (4, 1008) and tuple(rows.shape) == (4, 2048)
    assert torch.equal(_bits(fa), _bits(fb)) and torch.equal(_bits(la), _bits(lb))
    assert without.fused._spatial_rows is None and not without.spatial
    assert bool((_bits(rows[:, 2023:]) == 0).all()) and bool(rows[:, :2023].any(1).all())
    x = device.resize_f32(u8, (299, 299))                               # the clean input, through the tf1 engine's trunk
    tf1_eng = RealismEngine(dims=2048, seed=0, network=NET, with_logits=True, resize="tf1", spatial=True)
    fc, lc = tf1_eng._trunk(x, prenormalized=True)
    assert torch.equal(_bits(fc), _bits(fa)) and torch.equal(_bits(lc), _bits(la))
    assert torch.equal(_bits(tf1_eng.spatial_rows()), _bits(rows))


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
