"""GPU: the three kernels of csrc/lpips.hip at every layout edge, and the split-precision convolution at LPIPS's shapes -- the
widths at which ``SplitConv`` left to "auto" has to leave the row-window kernel (conv_split.rowwin_divides).

Input kernel and pool: no tolerance, bit for bit against ``conv_split.split`` of the table look-up resp. of ``max_pool2d`` of the
merged values.  Head: against a numpy extended-precision restatement, within a derived bound (test_head_against_numpy).
Convolutions: ``tests/_trunk_audit.CONV_TOL`` of the output scale against an fp64 convolution, the project's figure for every
split convolution."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests._trunk_audit import CONV_TOL

pytestmark = pytest.mark.gpu

SENT = -7.25                                                     # exact in fp16 and fp64


@pytest.fixture(scope="module")
def dev(cuda_device):
    return cuda_device


def bits16(t):
    return t.contiguous().view(torch.int16).cpu()


def P(t, byte_offset=0):
    return ctypes.c_void_p(t.data_ptr() + byte_offset)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------------------ input kernel
@pytest.mark.parametrize("h,w", [(16, 16), (17, 19)])
def test_input_split_bit_for_bit(dev, h, w):
    from tise_toolbox_amd import conv_split, device, lpips_model
    g = torch.Generator().manual_seed(h * 100 + w)
    n = 2
    lut = lpips_model.input_table()
    xs = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8) for _ in range(n)]
    ys = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8) for _ in range(n)]
    xs[0][0, 0], ys[1][h - 1, w - 1] = torch.tensor([0, 255, 128], dtype=torch.uint8), torch.tensor([255, 0, 1], dtype=torch.uint8)
    dx, dy = [t.to(dev) for t in xs], [t.to(dev) for t in ys]
    odd = torch.zeros(h * w * 3 + 1, dtype=torch.uint8, device=dev)                    # one source at an odd byte address
    odd[1:] = dx[1].reshape(-1)
    dx[1] = odd[1:].view(h, w, 3)
    assert dx[1].data_ptr() % 2 == 1 and dx[1].is_contiguous()
    big = torch.full((2 * n + 2, h, w, 64), SENT, dtype=torch.float16, device=dev)      # canaries: an image before and one after
    out = device.lpips_input_split(dx, dy, lut.to(dev), out=big[1:1 + 2 * n])
    torch.cuda.synchronize()
    assert out.data_ptr() == big[1].data_ptr()
    assert bool((big[0] == SENT).all()) and bool((big[-1] == SENT).all())
    want32 = torch.zeros((2 * n, h, w, 32), dtype=torch.float32)
    for i, img in enumerate(xs + ys):
        for c in range(3):
            want32[i, :, :, c] = lut[c][img[:, :, c].long()]
    want = conv_split.split(want32)
    assert torch.equal(bits16(out), bits16(want))
    hi, lo = conv_split.halves(out.cpu())
    assert not bool(hi[..., 3:].view(torch.int16).any()) and not bool(lo[..., 3:].view(torch.int16).any())   # +0.0 in both halves
    assert bool((hi[..., :3] != 0).any()) and bool((lo[..., :3] != 0).any())
    fresh = device.lpips_input_split(torch.stack(dx), torch.stack(dy), lut.to(dev))     # the stacked form, a fresh destination
    assert torch.equal(bits16(fresh), bits16(want))
    with pytest.raises(ValueError, match="one size"):
        device.lpips_input_split([dx[0], dx[0][:h - 1]], [dy[0], dy[0][:h - 1]], lut.to(dev))


# ------------------------------------------------------------------------------------------------------------------ pool
@pytest.mark.parametrize("h,w", [(2, 2), (3, 5), (16, 16), (17, 31)])
@pytest.mark.parametrize("C", [64, 48])
def test_maxpool2s2_split_bit_for_bit(dev, h, w, C):
    from tise_toolbox_amd import conv_split, device
    g = torch.Generator().manual_seed(h * 1000 + w * 10 + C)
    n = 2
    x32 = torch.randn((n, h, w, C), generator=g) * 3.0
    x32[0, 0, 0, :8] = 0.0
    x = conv_split.split(x32)
    merged = conv_split.merge(x)
    want = conv_split.split(F.max_pool2d(merged.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).contiguous())
    assert want.shape == (n, h // 2, w // 2, 2 * C)
    got = device.maxpool2s2_split(x.to(dev))
    assert torch.equal(bits16(got), bits16(want))
    # a channel slice of the source into a destination slice at an offset of a wider tensor; the rest of it survives
    Cd, off, x_off, c = 96, 48, 16, 32
    dst = torch.full((n, h // 2, w // 2, 2 * Cd), SENT, dtype=torch.float16, device=dev)
    device.maxpool2s2_split(x.to(dev), out=dst, out_off=off, x_off=x_off, channels=c)
    torch.cuda.synchronize()
    hi, lo = conv_split.halves(dst.cpu())
    whi, wlo = conv_split.halves(want)
    assert torch.equal(bits16(hi[..., off:off + c]), bits16(whi[..., x_off:x_off + c]))
    assert torch.equal(bits16(lo[..., off:off + c]), bits16(wlo[..., x_off:x_off + c]))
    keep = torch.ones(Cd, dtype=torch.bool)
    keep[off:off + c] = False
    assert bool((hi[..., keep] == SENT).all()) and bool((lo[..., keep] == SENT).all())


# ------------------------------------------------------------------------------------------------------------------ head
def _features(g, n, h, w, C):
    """Post-ReLU-like split features (2n, h, w, 2C) and their exact values as float64."""
    from tise_toolbox_amd import conv_split
    v = torch.randn((2 * n, h, w, C), generator=g).abs() * torch.rand((2 * n, h, w, 1), generator=g) * 4.0
    v[torch.rand(v.shape, generator=g) < 0.3] = 0.0
    s = conv_split.split(v)
    hi, lo = conv_split.halves(s)
    return s, hi.double().numpy() + lo.double().numpy() / 2048.0


def _head_reference(val, wt, n):
    """(per-pair value, per-pair bound scale S) in extended precision: S = mean over the pixels of
    sum_c |w_c| (|a_c| / n(a) + |b_c| / n(b))^2."""
    L = np.longdouble
    a, b = val[:n].astype(L), val[n:].astype(L)
    na = np.sqrt((a * a).sum(-1, keepdims=True)) + L(1e-10)
    nb = np.sqrt((b * b).sum(-1, keepdims=True)) + L(1e-10)
    ah, bh = a / na, b / nb
    wl = wt.astype(L)
    d = (wl * (ah - bh) ** 2).sum(-1)
    s = (np.abs(wl) * (np.abs(ah) + np.abs(bh)) ** 2).sum(-1)
    return d.reshape(n, -1).mean(1), s.reshape(n, -1).mean(1)


def _run_head(dev, s, wt, n, init=0.0):
    """One tise_lpips_layer call with canaries around ``out`` and the workspace -> (n,) float64 numpy."""
    from tise_toolbox_amd import _lib, device
    h, w, C = s.shape[1], s.shape[2], s.shape[3] // 2
    need = device.lpips_workspace_bytes(n, h, w)
    assert need == 8 * n * ((h * w + 255) // 256)
    out = torch.full((n + 4,), SENT, dtype=torch.float64, device=dev)
    out[2:2 + n] = init
    ws = torch.full((need // 8 + 16,), SENT, dtype=torch.float64, device=dev)
    _lib.call("tise_lpips_layer", P(s), ctypes.c_int64(n), h, w, C, P(wt), P(out, 16), P(ws, 64), ctypes.c_size_t(need), stream())
    torch.cuda.synchronize()
    o, wsh = out.cpu().numpy(), ws.cpu().numpy()
    assert (o[:2] == SENT).all() and (o[2 + n:] == SENT).all(), "the canaries around out"
    assert (wsh[:8] == SENT).all() and (wsh[8 + need // 8:] == SENT).all(), "the canaries around the workspace"
    return o[2:2 + n].copy()


# C: VGG's 64 / 128 / 512 (512: a whole wave per pixel), 48 (a 16-channel tail block, six of eight lanes of a group), 16 (two
# lanes).  hw: 1, either side of one wave's 64 pixels at C = 64, 256 + 1 = one pixel past a workgroup's share.
HEAD_SHAPES = [(1, 1), (7, 9), (8, 8), (5, 13), (1, 257)]


@pytest.mark.parametrize("C", [64, 128, 512, 48, 16])
def test_head_against_numpy(dev, C):
    """BOUND.  u = 2^-53.  Per pixel the kernel forms sa = sum_c a_c^2 (fma chain of 8, then a butterfly: relative error <= C u / 2
    + ..., halved by the square root), n(a) (two more roundings) and a_c / n(a) (one): a relative error <= (C / 2 + 4) u on each
    normalised value, so t = a^ - b^ carries <= (C / 2 + 4) u (|a^| + |b^|) + u |t|; t^2, the product with w_c and the sum over C
    terms add (C + 2) u sum |w_c| t^2.  With |t| <= |a^| + |b^| that is <= (2 C + 10) u S per pixel, S = sum_c |w_c| (|a^_c| +
    |b^_c|)^2.  The pixel sum is a chain of at most C / 4 adds per lane group (256 pixels / (4 waves x 64 / G pixels), G <= C / 4),
    6 + 3 adds across the workgroup, ceil(slots / 64) + 6 in the finish and one division: <= (C / 4 + 16 + log2(hw)) u.  Together
    <= (2.25 C + 26 + log2 hw) u <= 4 (C + log2(hw) + 1) u for every C >= 16, relative to the mean of S over the pixels.  The
    reference is formed in extended precision (its own error is below 2^-60 of S)."""
    g = torch.Generator().manual_seed(C)
    worst = 0.0
    for k, (h, w) in enumerate(HEAD_SHAPES):
        n = 1 if k % 2 else 3
        s, val = _features(g, n, h, w, C)
        wt = torch.randn(C, generator=g)                                     # signed: the bound is in |w_c|
        want, scale = _head_reference(val, wt.numpy().astype(np.float64), n)
        got = _run_head(dev, s.to(dev), wt.to(dev), n)
        bound = 4.0 * (C + np.log2(h * w) + 1) * 2.0 ** -53 * scale.astype(np.float64)
        err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
        print(f"lpips head C={C} hw={h * w} n={n}: worst error / bound = {float((err / bound).max()):.3f}, "
              f"error / S = {float((err / scale.astype(np.float64)).max()):.3e}")
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (C, h, w, err, bound)
        again = _run_head(dev, s.to(dev), wt.to(dev), n)                     # two calls: the same bits
        assert again.tobytes() == got.tobytes()
        added = _run_head(dev, s.to(dev), wt.to(dev), n, init=0.5)           # the value is ADDED into out
        assert added.tobytes() == (0.5 + got).tobytes()
    assert worst <= 1.0


@pytest.mark.parametrize("C", [64, 48, 512])
def test_head_special_cases(dev, C):
    from tise_toolbox_amd import conv_split
    g = torch.Generator().manual_seed(1000 + C)
    n, h, w = 3, 5, 13
    s, val = _features(g, n, h, w, C)
    wt = torch.rand(C, generator=g)
    # identical features: exactly 0.0 (and -0.0 is not accepted either)
    same = torch.cat([s[:n], s[:n]], 0)
    got = _run_head(dev, same.to(dev), wt.to(dev), n)
    assert got.tobytes() == np.zeros(n).tobytes()
    # an all-zero pixel on both sides contributes exactly 0: the pair's value is the sum over the other pixels / hw
    z = s.clone()
    z[0, 2, 3], z[n, 2, 3] = 0, 0                                            # pair 0, both sides
    z[1, 0, 0] = 0                                                           # pair 1, side one only: sum_c w_c b^_c^2
    vz = val.copy()
    vz[0, 2, 3], vz[n, 2, 3], vz[1, 0, 0] = 0.0, 0.0, 0.0
    want, scale = _head_reference(vz, wt.numpy().astype(np.float64), n)
    got = _run_head(dev, z.to(dev), wt.to(dev), n)
    bound = 4.0 * (C + np.log2(h * w) + 1) * 2.0 ** -53 * scale.astype(np.float64)
    assert (np.abs(got.astype(np.longdouble) - want).astype(np.float64) <= bound).all()
    only = torch.zeros_like(s)                                               # ONE live pixel per pair, zero on side one
    only[n:, 1, 1] = s[n:, 1, 1]
    got1 = _run_head(dev, only.to(dev), wt.to(dev), n)
    v1 = np.zeros_like(val)
    v1[n:, 1, 1] = val[n:, 1, 1]
    want1, scale1 = _head_reference(v1, wt.numpy().astype(np.float64), n)
    assert (np.abs(got1.astype(np.longdouble) - want1).astype(np.float64) <= 4.0 * (C + 8) * 2.0 ** -53 * scale1.astype(np.float64)).all()
    assert (got1 > 0).all()
    # a NaN (and an inf) in pair 1's features reaches pair 1's number only
    base = _run_head(dev, s.to(dev), wt.to(dev), n)
    for poison in (float("nan"), float("inf")):
        bad = s.clone()
        hi, lo = conv_split.halves(bad)
        hi = hi.clone()
        hi[1, 4, 12, C - 1] = poison                                         # side one of pair 1, the last pixel and channel
        bad = conv_split._interleave(hi, lo.clone())
        got = _run_head(dev, bad.to(dev), wt.to(dev), n)
        assert np.isnan(got[1]) and got[[0, 2]].tobytes() == base[[0, 2]].tobytes(), (poison, got, base)


def test_head_wrapper_and_pair_independence(dev):
    """device.lpips_layer: a pair's bits do not depend on n or on its position in the launch."""
    from tise_toolbox_amd import device
    g = torch.Generator().manual_seed(77)
    n, h, w, C = 3, 1, 257, 64
    s, _ = _features(g, n, h, w, C)
    wt = torch.rand(C, generator=g).to(dev)
    sd = s.to(dev)
    full = device.lpips_layer(sd, wt, torch.zeros(n, dtype=torch.float64, device=dev)).cpu().numpy()
    for i in range(n):
        alone = device.lpips_layer(torch.stack([sd[i], sd[n + i]]), wt, torch.zeros(1, dtype=torch.float64, device=dev)).cpu().numpy()
        assert alone.tobytes() == full[i:i + 1].tobytes()
    rev = torch.cat([sd[:n].flip(0), sd[n:].flip(0)], 0)
    assert device.lpips_layer(rev, wt, torch.zeros(n, dtype=torch.float64, device=dev)).cpu().numpy()[::-1].tobytes() == full.tobytes()
    with pytest.raises(ValueError, match="at most 512 channels"):
        device.lpips_layer(torch.zeros((2, 1, 1, 2 * 528), dtype=torch.float16, device=dev), torch.zeros(528, device=dev),
                           torch.zeros(1, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError, match="float64"):
        device.lpips_layer(sd, wt, torch.zeros(n, dtype=torch.float32, device=dev))
    with pytest.raises(ValueError, match="workspace"):
        device.lpips_layer(sd, wt, torch.zeros(n, dtype=torch.float64, device=dev), workspace=torch.zeros(8, dtype=torch.uint8, device=dev))


# ---------------------------------------------------------------------------------------------- convolutions at LPIPS's shapes
# which kernel SplitConv left to "auto" takes at KW = 3 (tile widths 2..4 for all five layers): the row-window kernel where its
# window fits (OW >= 5) and its 16-bit reciprocal of the row length is exact (every OW <= 123, 224), else the default kernel.
# (OW = 7 does fit a window -- rowwin_fits is false below 5 -- so OW = 4 stands beside 2 for "no row window fits".)
CONV_KERNEL = {2: "fast", 4: "fast", 7: "rowwin", 16: "rowwin", 123: "rowwin", 124: "fast", 128: "fast", 224: "rowwin", 256: "fast",
               257: "fast"}
CONV_LAYERS = [(32, 64), (64, 64), (64, 128), (128, 256), (512, 512)]


@pytest.fixture(scope="module")
def conv_layers(dev):
    """Per layer: (SplitConv left to auto, fp64 weight, fp64 bias), built once."""
    from tise_toolbox_amd.conv_split import SplitConv
    out = {}
    for cin, cout in CONV_LAYERS:
        g = torch.Generator().manual_seed(cin * 1000 + cout)
        wt = torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (9 * min(cin, 64))) ** 0.5
        if cin == 32:
            wt[:, 3:] = 0.0                                                  # conv1_1: 29 zero weight columns
        bias = torch.randn(cout, generator=g) * 0.1
        out[(cin, cout)] = (SplitConv(wt, bias, (1, 1), (1, 1), dev), wt.double(), bias.double())
    return out


@pytest.mark.parametrize("ow", sorted(CONV_KERNEL))
@pytest.mark.parametrize("cin,cout", CONV_LAYERS)
def test_conv_at_lpips_shapes(dev, conv_layers, monkeypatch, cin, cout, ow):
    from tise_toolbox_amd import _lib, conv_split
    conv, w64, b64 = conv_layers[(cin, cout)]
    assert conv.variant == "rowwin" and conv.tn in (2, 3, 4)                 # what "auto" chose for the layer
    g = torch.Generator().manual_seed(ow)
    n, h = 1, 3
    x32 = torch.randn((n, h, ow, cin), generator=g)
    if cin == 32:
        x32[..., 3:] = 0.0
    x = conv_split.split(x32)
    xv = conv_split.halves(x)
    ref_in = (xv[0].double() + xv[1].double() / 2048.0).permute(0, 3, 1, 2)
    want = torch.relu(F.conv2d(ref_in, w64, b64, 1, 1)).permute(0, 2, 3, 1)
    scale = want.abs().max().item()
    codes = []
    real = _lib.call

    def spy(name, *args):
        if name == "tise_conv_split_f16":
            codes.append(args[1])
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", spy)
    y = torch.full((n, h, ow, 2 * cout), SENT, dtype=torch.float16, device=dev)
    assert conv(x.to(dev), [(0, cout, y, 0, 0)]) == (h, ow)
    torch.cuda.synchronize()
    assert len(codes) == 1
    took = "rowwin" if codes[0] & 64 else ("fast" if codes[0] & 128 else "other")
    assert took == CONV_KERNEL[ow], (cin, cout, ow, hex(codes[0]))
    assert took == ("rowwin" if conv_split.rowwin_fits(ow, 3) and conv_split.rowwin_divides(ow, 3) else "fast")
    hi, lo = conv_split.halves(y.cpu())
    got = hi.double() + lo.double() / 2048.0
    err = (got - want).abs().max().item()
    print(f"conv {cin}->{cout} OW={ow} {took}: error / scale = {err / scale:.3e}")
    assert err <= CONV_TOL * scale, (cin, cout, ow, err, scale)
