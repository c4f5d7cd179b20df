"""GPU: non-finite and out-of-range values at every fused ReLU and every writer of a split tensor.

The contract (``holds``): against torch on the CPU -- the same op in fp32, relu included, which propagates NaN -- the
kernel's output is non-finite wherever the reference's is, OR the range guard of the split format is raised after the
launch.  A finite output with a clear flag where the reference is non-finite is the failure: a silent wrong number.

What reading the kernels predicts, and these tests pin: every ReLU is fmaxf(v, 0) and every running maximum fmaxf(vmax, v),
and fmaxf returns the operand that is not NaN -- so a NaN leaves a ReLU as 0 and a max-pool drops a NaN tap, without a flag.
Only split_mean propagates it.  A split tensor cannot even hold +-Inf (hi = +-inf, lo = NaN: the pair merges to NaN), so
an Inf planted in a split INPUT behaves like a NaN.  The hazard is closed on the host: non-finite parameters are refused
(ValueError naming the layer; trunk.py, conv_split.py, inception.py), the network input is a table look-up of a byte, and
with finite operands the first non-finite value of a pass is an fp32 result beyond the fp16 range, which raises the guard
where it is stored.  So here:
  * weight / bias / scale cases: ValueError at construction;
  * activation cases with +-Inf or 7e4 in an fp32 input, and every case of split_mean: the contract;
  * activation cases with no legal origin once the parameters are finite -- a NaN planted directly, an Inf planted in a
    split input -- are kept as a RECORD of what the kernels do (0 out / tap dropped, no flag) in tests named so: a kernel
    change that makes the ReLU propagate NaN has to touch them knowingly.
Each launch is also run on the untouched input (flag clear, finite output), and the flag is read-and-clear.

Found by these tests: split_mean's NaN-catching maximum, (|v| <= vmax) ? vmax : |v|, caught a NaN only in the LAST of a thread's
eight channels -- the next finite value fails the comparison against a NaN maximum as well and replaced it.  The fp32 row
carried the NaN either way, so the contract held through the output; the maximum now keeps a NaN and the flag is asserted.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _avgpool_child as child
from tests import _pool_ref as pr
from tests.test_gpu_pool_kernels import P, call, dv, run_child, st

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
VALUES = {"nan": NAN, "+inf": INF, "-inf": -INF, "7e4": 7e4}
N, H, W = 2, 9, 9
WHERE = {"interior": (0, 4, 4, 3), "border": (1, 0, 8, 5)}


@pytest.fixture(scope="module")
def dev(cuda_device):
    return cuda_device


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).permute(0, 3, 1, 2)


def _np(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def base_input(C, seed=0):
    """A legal activation tensor: non-negative (post-ReLU like), no zeros, moderate, and exactly representable as a split
    pair, so that the sites with a split input see the values the reference sees."""
    return pr.merge_value(*pr.split_value((np.random.default_rng(seed).random((N, H, W, C)) + 0.25).astype(np.float32)))


def _bias(C):
    return (np.random.default_rng(9).standard_normal(C) * 0.2).astype(np.float32)


# ---- the activation sites: name -> (channels, run(x, dev) -> fp32 numpy output, ref(x) -> fp32 numpy, split INPUT?) ---------
def _f32_site(fn, ref, s2=False, bias=True):
    def run(x, dev):
        C = x.shape[-1]
        oh, ow = ((H - 3) // 2 + 1, (W - 3) // 2 + 1) if s2 else (H, W)
        out = torch.zeros((N, oh, ow, C), dtype=torch.float32, device=dev)
        b, xd = dv(_bias(C), dev), dv(x, dev)
        if fn == "tise_bias_relu_nhwc":
            call(fn, P(xd), C, 0, N * H * W, C, P(b), P(out), C, 0, st())
        elif fn == "tise_maxpool3s1p1_nhwc":
            call(fn, P(xd), C, 0, N, H, W, C, P(out), C, 0, st())
        else:
            call(fn, P(xd), C, 0, N, H, W, C, P(b) if bias else None, P(out), C, 0, st())
        return out.cpu().numpy()
    return (8, run, ref, False)


def _bv(C):
    return torch.from_numpy(_bias(C)).view(1, -1, 1, 1)


def _avg_split_site(excl):
    def run(x, dev):
        c = dict(x=x, bias=_bias(8), n=N, h=H, w=W, C=8, x_ld=8, x_off=0, out_C=16, out_off=8, excl=excl)
        out, _ = child.run_cases([c], dev, read_flag=False)[0]
        return pr.merge_value(*pr.unpack_split(out, 8, 8))
    return (8, run, lambda x: _np(torch.relu(F.avg_pool2d(_t(x), 3, 1, 1, count_include_pad=not excl) + _bv(8))), False)


def _maxpool_split_site(fn, s2):
    def run(x, dev):
        oh, ow = ((H - 3) // 2 + 1, (W - 3) // 2 + 1) if s2 else (H, W)
        xs = dv(pr.pack_split(np.zeros((N, H, W, 32), dtype=np.float16), x, 0), dev)
        out = torch.zeros((N, oh, ow, 32), dtype=torch.float16, device=dev)
        call(fn, P(xs), 16, 0, N, H, W, 16, P(out), 16, 0, st())
        return pr.merge_value(*pr.unpack_split(out.cpu().numpy()))
    return (16, run, (lambda x: _np(F.max_pool2d(_t(x), 3, 2))) if s2 else (lambda x: _np(F.max_pool2d(_t(x), 3, 1, 1))), True)


def _mean_site(both):
    def run(x, dev):
        xs = dv(pr.pack_split(np.zeros((N, H, W, 64), dtype=np.float16), x, 0), dev)
        out = torch.zeros((N, 32), dtype=torch.float32, device=dev)
        if both:
            sp = torch.zeros((N, 64), dtype=torch.float16, device=dev)
            call("tise_split_mean_both_nhwc", P(xs), N, H * W, 32, P(out), P(sp), st())
        else:
            call("tise_split_mean_nhwc", P(xs), N, H * W, 32, P(out), st())
        return out.cpu().numpy()
    return (32, run, lambda x: torch.from_numpy(x).mean((1, 2)).numpy(), True)


def _conv_params(variant):
    if variant == "pipe":
        return torch.full((32, 32, 3, 3), 0.125), torch.zeros(32), (1, 1), dict(variant="pipe", pipe_cfg=34)
    return torch.full((64, 32, 1, 1), 0.125), torch.zeros(64), (0, 0), (dict(variant="glds") if variant == "glds" else {})


def _run_conv(conv, x, dev):
    xs = pr.pack_split(np.zeros((N, H, W, 64), dtype=np.float16), x, 0)
    out = torch.zeros((N, H, W, 2 * conv.cout), dtype=torch.float16, device=dev)
    conv(dv(xs, dev), [(0, conv.cout, out, 0, 0)])
    return pr.merge_value(*pr.unpack_split(out.cpu().numpy()))


def _conv_site(variant):
    w, b, pad, kw = _conv_params(variant)

    def run(x, dev):
        from tise_toolbox_amd.conv_split import SplitConv
        return _run_conv(SplitConv(w, b, (1, 1), pad, dev, **kw), x, dev)
    return (32, run, lambda x: _np(torch.relu(torch.conv2d(_t(x), w, b, 1, pad))), True)


SITES = {
    "bias_relu": _f32_site("tise_bias_relu_nhwc", lambda x: _np(torch.relu(_t(x) + _bv(8)))),
    "avgpool": _f32_site("tise_avgpool3_bias_relu_nhwc", lambda x: _np(torch.relu(F.avg_pool2d(_t(x), 3, 1, 1) + _bv(8)))),
    "avgpool_excl": _f32_site("tise_avgpool3_excl_bias_relu_nhwc",
                              lambda x: _np(torch.relu(F.avg_pool2d(_t(x), 3, 1, 1, count_include_pad=False) + _bv(8)))),
    "maxpool3s2_bias": _f32_site("tise_maxpool3s2_nhwc", lambda x: _np(F.max_pool2d(torch.relu(_t(x) + _bv(8)), 3, 2)), s2=True),
    "maxpool3s2": _f32_site("tise_maxpool3s2_nhwc", lambda x: _np(F.max_pool2d(_t(x), 3, 2)), s2=True, bias=False),
    "maxpool3s1p1": _f32_site("tise_maxpool3s1p1_nhwc", lambda x: _np(F.max_pool2d(_t(x), 3, 1, 1))),
    "avgpool_split": _avg_split_site(False),
    "avgpool_excl_split": _avg_split_site(True),
    "maxpool3s2_split": _maxpool_split_site("tise_maxpool3s2_split_nhwc", True),
    "maxpool3s1p1_split": _maxpool_split_site("tise_maxpool3s1p1_split_nhwc", False),
    "split_mean": _mean_site(False),
    "split_mean_both": _mean_site(True),
    "conv_default": _conv_site("default"),
    "conv_glds": _conv_site("glds"),
    "conv_pipe": _conv_site("pipe"),
}
# fp32 output, no split tensor written: the guard is not involved, the output itself must carry the non-finite value
SPLIT_WRITERS = {"avgpool_split", "avgpool_excl_split", "maxpool3s2_split", "maxpool3s1p1_split", "split_mean_both",
                 "conv_default", "conv_glds", "conv_pipe"}


def no_legal_origin(site, value):
    """The activation cases the kernels are only RECORDED on: a NaN planted directly (every site but split_mean, which
    propagates it), and an Inf planted in a split input (it cannot be represented: the pair merges to NaN)."""
    if site.startswith("split_mean"):
        return False
    return value == "nan" or (SITES[site][3] and value in ("+inf", "-inf"))


def observe(site, value, where, dev):
    """-> (reference, output on the planted input, flag after it, flag read again, output on the clean input, flag after it)."""
    from tise_toolbox_amd import device
    C, run, ref, _ = SITES[site]
    x0 = base_input(C)
    device.read_split_overflow()
    clean = run(x0, dev)
    clean_flag = device.read_split_overflow()
    x = x0.copy()
    n, h, w, c = WHERE[where]
    x[n, h, w, c] = VALUES[value]
    got = run(x, dev)
    flag = device.read_split_overflow()
    again = device.read_split_overflow()
    with np.errstate(all="ignore"):
        want = ref(x)
    assert want.shape == got.shape, (want.shape, got.shape)
    return want, got, flag, again, clean, clean_flag, ref(x0)


def holds(want, got, flag):
    bad = ~np.isfinite(want)
    return bool(flag) or not np.isfinite(got[bad]).any()


CASES = [(s, v, w) for s in SITES for v in VALUES for w in WHERE]


@pytest.mark.parametrize("site,value,where", [c for c in CASES if not no_legal_origin(c[0], c[1])])
def test_nonfinite_activation_is_visible_in_the_output_or_raises_the_guard(dev, site, value, where):
    want, got, flag, again, clean, clean_flag, want_clean = observe(site, value, where, dev)
    print(f"{site} {value} {where}: reference non-finite at {int((~np.isfinite(want)).sum())}, output non-finite at "
          f"{int((~np.isfinite(got)).sum())}, flag {flag}")
    assert not clean_flag and np.isfinite(clean).all(), "the untouched input must pass silently"
    assert np.abs(clean - want_clean).max() <= 1e-5 * np.abs(want_clean).max(), "the site computes the reference's op"
    assert not again, "the flag is read-and-clear"
    assert holds(want, got, flag), f"finite output and a clear flag where the reference is non-finite ({site}, {value}, {where})"
    if site not in SPLIT_WRITERS:
        assert not flag
    if site in ("avgpool_split", "avgpool_excl_split") and value == "+inf":
        assert flag, "an fp32 +Inf stored into a split tensor is beyond the fp16 range: the guard must fire"
    if site == "split_mean_both" and value != "7e4":
        # the planted channels (3 and 5 of a thread's 8) are not the thread's last: the running maximum must KEEP a NaN
        assert flag, "split_mean's NaN-catching maximum lost the NaN"


@pytest.mark.parametrize("site,value,where", [c for c in CASES if no_legal_origin(c[0], c[1])])
def test_record_kernel_turns_nan_into_zero_or_drops_the_tap_without_a_flag(dev, site, value, where):
    """NOT a contract: the kernels' behaviour on inputs that have no legal origin once the parameters are finite.  The
    ReLU sites store 0 where the reference is NaN; the max pools store the maximum of the other taps; no flag is raised."""
    want, got, flag, again, clean, clean_flag, _ = observe(site, value, where, dev)
    assert not clean_flag and np.isfinite(clean).all()
    bad = np.isnan(want) | np.isinf(want)
    assert np.isfinite(got).all() and not flag and not again, (site, value, where, flag)
    if "maxpool" in site:                                   # the tap is dropped: the pool of the map with -inf in its place
        C, _, ref, _ = SITES[site]
        x = base_input(C)
        x[WHERE[where]] = -INF
        assert np.array_equal(got, ref(x).astype(np.float32))
    elif bad.any():
        assert (got[bad] == 0.0).all()
        assert np.abs(got[~bad] - want[~bad]).max() <= 1e-5 * np.abs(want[~bad]).max()


def test_per_output_average_pool_in_a_child_process(dev, tmp_path):
    """The same planted inputs through the per-output split average-pool kernel (TISE_AVGPOOL_PER_OUTPUT: a fresh process,
    one child for all cases): the contract for +-Inf and 7e4, the record for NaN, flag clear on the untouched input."""
    cases, meta = [], []
    for excl in (False, True):
        for value in [None] + list(VALUES):
            for where in (WHERE if value else ["interior"]):
                x = base_input(8)
                if value:
                    x[WHERE[where]] = VALUES[value]
                cases.append(dict(x=x, bias=_bias(8), n=N, h=H, w=W, C=8, x_ld=8, x_off=0, out_C=16, out_off=8, excl=excl))
                meta.append((excl, value, where))
    res = run_child(cases, tmp_path, "nonfinite")
    for c, (excl, value, where), (out, flag) in zip(cases, meta, res):
        got = pr.merge_value(*pr.unpack_split(out, 8, 8))
        with np.errstate(all="ignore"):
            want = SITES["avgpool_excl_split" if excl else "avgpool_split"][2](c["x"])
        if value is None:
            assert not flag and np.isfinite(got).all()
        elif value == "nan":
            assert not flag and np.isfinite(got).all() and (got[np.isnan(want)] == 0.0).all(), (excl, value, where)
        else:
            assert holds(want, got, flag), (excl, value, where)


# ------------------------------------------------------------------------------------------------- parameters
@pytest.mark.parametrize("variant", ["default", "glds", "pipe"])
@pytest.mark.parametrize("value", ["nan", "+inf", "-inf"])
def test_split_conv_refuses_a_nonfinite_weight_or_bias(dev, variant, value):
    from tise_toolbox_amd.conv_split import SplitConv
    w, b, pad, kw = _conv_params(variant)
    w2 = w.clone()
    w2[5, 7, 0, 0] = VALUES[value]
    with pytest.raises(ValueError, match="non-finite"):
        SplitConv(w2.to(dev), b.to(dev), (1, 1), pad, dev, **kw)
    b2 = b.clone()
    b2[11] = VALUES[value]
    with pytest.raises(ValueError, match="non-finite"):
        SplitConv(w.to(dev), b2.to(dev), (1, 1), pad, dev, **kw)


@pytest.mark.parametrize("variant", ["default", "glds", "pipe"])
def test_split_conv_7e4_weight_overflows_into_the_guard(dev, variant):
    """A finite weight of 7e4 is legal; the results beyond the fp16 range raise the guard."""
    from tise_toolbox_amd import device
    from tise_toolbox_amd.conv_split import SplitConv
    w, b, pad, kw = _conv_params(variant)
    w2 = w.clone()
    w2[5, 7, 0, 0] = 7e4
    device.read_split_overflow()
    got = _run_conv(SplitConv(w2.to(dev), b.to(dev), (1, 1), pad, dev, **kw), base_input(32), dev)
    want = _np(torch.relu(torch.conv2d(_t(base_input(32)), w2, b, 1, pad)))
    assert want[..., 5].max() > 65504 and device.read_split_overflow() and not device.read_split_overflow()
    keep = [c for c in range(want.shape[-1]) if c != 5]
    assert np.abs(got[..., keep] - want[..., keep]).max() <= 1e-5 * want[..., keep].max()


@pytest.mark.parametrize("variant", ["default", "glds", "pipe"])
def test_record_conv_epilogue_turns_a_nan_weight_into_zero_without_a_flag(dev, variant):
    """NOT a contract: what the kernels do with the NaN weight SplitConv now refuses (``check=False`` is the trunks' switch
    for parameters they have checked themselves): the cout's results leave the epilogue's ReLU as 0, no flag."""
    from tise_toolbox_amd import device
    from tise_toolbox_amd.conv_split import SplitConv
    w, b, pad, kw = _conv_params(variant)
    w2 = w.clone()
    w2[5, 7, 0, 0] = NAN
    device.read_split_overflow()
    got = _run_conv(SplitConv(w2.to(dev), b.to(dev), (1, 1), pad, dev, check=False, **kw), base_input(32), dev)
    assert np.isfinite(got).all() and (got[..., 5] == 0.0).all() and not device.read_split_overflow()


def _stem_module(plant, value):
    from tise_toolbox_amd.inception import BasicConv2d
    g = torch.Generator().manual_seed(2)
    m = BasicConv2d(3, 32, kernel_size=3, stride=2)
    with torch.no_grad():
        m.conv.weight.copy_(torch.randn(m.conv.weight.shape, generator=g) * (2.0 / 27) ** 0.5)
        m.bn.weight.copy_(1.0 + 0.1 * torch.randn(32, generator=g))
        m.bn.bias.copy_(0.1 * torch.randn(32, generator=g))
        m.bn.running_mean.zero_()
        m.bn.running_var.fill_(1.0)
        if plant == "weight":
            m.conv.weight[6, 1, 2, 0] = value
        elif plant == "bias":
            m.bn.bias[6] = value
        elif plant == "scale":
            m.bn.weight[6] = value
    return m.eval()


@torch.no_grad()
def _run_stems(c, dev):
    """The three stem entry points on the folded parameters of a trunk._Conv -> ({name: merged fp32 output}, {name: guard
    flag after that launch}, the fp32 reference)."""
    from tise_toolbox_amd import device
    from tise_toolbox_amd.trunk import pack_stem_mfma
    g = np.random.default_rng(4)
    n, h, w = 2, 9, 11
    u8 = g.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    lut = (g.random((3, 256)) * 2.4 - 1.2).astype(np.float32)
    x = np.stack([lut[ch][u8[..., ch]] for ch in range(3)], -1).astype(np.float32)
    wt = c.w.permute(2, 3, 1, 0).contiguous().float()
    wsp, scale = pack_stem_mfma(c.w, dev)
    xd, ud, ld, bd = dv(x, dev), dv(u8, dev), dv(lut.reshape(-1), dev), c.b.contiguous()
    outs, flags = {}, {}
    device.read_split_overflow()
    for name in ("fp32", "u8", "mfma"):
        out = torch.zeros((n, 4, 5, 64), dtype=torch.float16, device=dev)
        if name == "fp32":
            call("tise_stem_conv3x3s2_split", P(xd), n, h, w, P(wt), P(bd), P(out), st())
        elif name == "u8":
            call("tise_stem_conv3x3s2_split_u8", P(ud), P(ld), n, h, w, P(wt), P(bd), P(out), st())
        else:
            call("tise_stem_conv3x3s2_split_u8_mfma", P(ud), P(ld), n, h, w, P(wsp), P(scale), P(bd), P(out), st())
        flags[name] = device.read_split_overflow()
        outs[name] = pr.merge_value(*pr.unpack_split(out.cpu().numpy()))
    want = _np(torch.relu(torch.conv2d(_t(x), c.w.cpu().float().contiguous(), c.b.cpu(), 2)))
    return outs, flags, want


@pytest.mark.parametrize("plant", ["weight", "bias", "scale"])
@pytest.mark.parametrize("value", ["nan", "+inf", "-inf"])
def test_stem_parameters_are_refused_where_the_trunk_takes_them(dev, plant, value):
    """The u8 stems cannot take a non-finite pixel; a non-finite weight, bias or BatchNorm scale (the MFMA form's ``scale``
    and every form's folded weight) is refused when the trunk folds the layer."""
    from tise_toolbox_amd.trunk import _Conv, require_finite_params
    c = _Conv([_stem_module(plant, VALUES[value]).to(dev)], dev, ["Conv2d_1a_3x3"])
    with pytest.raises(ValueError, match="Conv2d_1a_3x3"):
        require_finite_params(c.names, c.finite, dev)
    ok = _Conv([_stem_module(None, 0.0).to(dev)], dev, ["Conv2d_1a_3x3"])
    require_finite_params(ok.names, ok.finite, dev)


@pytest.mark.parametrize("plant", [None, "weight", "bias", "scale"])
def test_record_stems_turn_a_nan_parameter_into_zero_without_a_flag(dev, plant):
    """NOT a contract: the three stem kernels on the parameters the trunk now refuses -- the cout's results leave the ReLU as
    0, no flag -- and, with ``plant`` None, on finite ones: the reference's values, flag clear."""
    from tise_toolbox_amd import device
    from tise_toolbox_amd.trunk import _Conv
    with torch.no_grad():
        c = _Conv([_stem_module(plant, NAN).to(dev)], dev, ["Conv2d_1a_3x3"])
        outs, flags, want = _run_stems(c, dev)
    assert not any(flags.values()), flags
    keep = [ch for ch in range(32) if ch != 6]
    for name, got in outs.items():
        assert np.isfinite(got).all(), name
        assert np.abs(got[..., keep] - want[..., keep]).max() <= 1e-5 * np.abs(want[..., keep]).max(), name
        if plant:
            assert np.isnan(want[..., 6]).all() and (got[..., 6] == 0.0).all(), name


def test_stem_7e4_bias_overflows_into_the_guard(dev):
    from tise_toolbox_amd import device
    from tise_toolbox_amd.trunk import _Conv
    with torch.no_grad():
        c = _Conv([_stem_module("bias", 7e4).to(dev)], dev, ["Conv2d_1a_3x3"])
    outs, flags, want = _run_stems(c, dev)
    assert want[..., 6].min() > 65504 and all(flags.values()), flags
    assert not device.read_split_overflow()
