"""GPU: the kernels of csrc/dists.hip at every layout edge, and the split-precision convolution at the row lengths that DISTS's
ceil pools produce (9, 5, 3, 2 and 1 -- LPIPS's floor pools never made them).

L2 pool: numpy fp64 on ``merge(x)``, within the split format's own step (test_l2pool_against_numpy).  Head: numpy extended
precision within a derived bound (test_layer_against_numpy).  Stage-0 sums: numpy int64, exact.  Convolutions:
``tests/_trunk_audit.CONV_TOL`` of the output scale against an fp64 convolution, the project's figure for every split convolution."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests._trunk_audit import CONV_TOL

pytestmark = pytest.mark.gpu

SENT = -7.25                                                     # exact in fp16 and fp64
WG = 512                                                         # TISE_DISTS_WG_PIXELS


@pytest.fixture(scope="module")
def dev(cuda_device):
    return cuda_device


def bits16(t):
    return t.contiguous().view(torch.int16).cpu()


def P(t, byte_offset=0):
    return ctypes.c_void_p(t.data_ptr() + byte_offset)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------------------------- L2 pool
def _l2pool_reference(v):
    """(n, h, w, C) float64 -> (n, ceil(h/2), ceil(w/2), C) float64: the nine weighted squares in row-major tap order, zero padding."""
    n, h, w, C = v.shape
    oh, ow = (h + 1) // 2, (w + 1) // 2
    sq = np.zeros((n, 2 * oh + 1, 2 * ow + 1, C), dtype=np.float64)
    sq[:, 1:h + 1, 1:w + 1] = v * v
    acc = np.zeros((n, oh, ow, C), dtype=np.float64)
    for dh in range(3):
        for dw in range(3):
            g = (0.5 if dh == 1 else 0.25) * (0.5 if dw == 1 else 0.25)
            acc = acc + g * sq[:, dh:dh + 2 * oh:2, dw:dw + 2 * ow:2]
    return np.sqrt(acc + 1e-12)


def _check_l2pool(got, ref, what):
    """The bound of the split format, 2^-21 |ref| + 2^-35, and whether the result was bit-identical to split(float32(ref))."""
    from tise_toolbox_amd import conv_split
    m = conv_split.merge(got.cpu()).double().numpy()
    err = np.abs(m - ref)
    bound = 2.0 ** -21 * np.abs(ref) + 2.0 ** -35
    want = conv_split.split(torch.from_numpy(ref.astype(np.float32)))
    same = torch.equal(bits16(got), bits16(want))
    print(f"l2pool {what}: worst error / bound = {float((err / bound).max()):.3f}; bit-identical to split(float32(ref)): {same}")
    assert (err <= bound).all(), (what, float((err / bound).max()))
    return same


@pytest.mark.parametrize("h,w", [(1, 1), (1, 2), (2, 1), (2, 2), (3, 5), (16, 16), (17, 31)])
@pytest.mark.parametrize("C", [64, 48])
def test_l2pool_against_numpy(dev, h, w, C):
    from tise_toolbox_amd import conv_split, device
    g = torch.Generator().manual_seed(h * 1000 + w * 10 + C)
    for n in (1, 3):
        x32 = torch.randn((n, h, w, C), generator=g) * 3.0
        x32[0, 0, 0, :8] = 0.0
        x = conv_split.split(x32)
        ref = _l2pool_reference(conv_split.merge(x).double().numpy())
        oh, ow = (h + 1) // 2, (w + 1) // 2
        assert ref.shape == (n, oh, ow, C)
        # canaries: an image before and one after the destination
        big = torch.full((n + 2, oh, ow, 2 * C), SENT, dtype=torch.float16, device=dev)
        got = device.l2pool3s2_split(x.to(dev), out=big[1:1 + n])
        torch.cuda.synchronize()
        assert got.data_ptr() == big[1].data_ptr() and tuple(got.shape) == (n, oh, ow, 2 * C)
        assert bool((big[0] == SENT).all()) and bool((big[-1] == SENT).all())
        _check_l2pool(got, ref, f"{h} x {w} C={C} n={n}")
        again = device.l2pool3s2_split(x.to(dev))                                  # a second call, a fresh destination: the same bits
        assert torch.equal(bits16(again), bits16(got))
        # a channel slice of the source into a destination slice at an offset of a wider tensor; the rest of it survives
        Cd, off, x_off, c = 96, 48, 16, 32
        dst = torch.full((n, oh, ow, 2 * Cd), SENT, dtype=torch.float16, device=dev)
        device.l2pool3s2_split(x.to(dev), out=dst, out_off=off, x_off=x_off, channels=c)
        torch.cuda.synchronize()
        hi, lo = conv_split.halves(dst.cpu())
        ghi, glo = conv_split.halves(got.cpu())
        assert torch.equal(bits16(hi[..., off:off + c]), bits16(ghi[..., x_off:x_off + c]))
        assert torch.equal(bits16(lo[..., off:off + c]), bits16(glo[..., x_off:x_off + c]))
        keep = torch.ones(Cd, dtype=torch.bool)
        keep[off:off + c] = False
        assert bool((hi[..., keep] == SENT).all()) and bool((lo[..., keep] == SENT).all())


def test_l2pool_zero_map_and_border_taps(dev):
    from tise_toolbox_amd import conv_split, device
    n, h, w, C = 2, 5, 6, 64
    z = torch.zeros((n, h, w, 2 * C), dtype=torch.float16, device=dev)
    got = device.l2pool3s2_split(z)
    want = conv_split.split(torch.full((n, 3, 3, C), float(np.float32(1e-6))))
    assert torch.equal(bits16(got), bits16(want))                                  # a zero map: split(float32(1e-6)) exactly
    # values on the image border only, the four corners included: every window that reaches outside sees zeros there
    g = torch.Generator().manual_seed(9)
    x32 = torch.zeros((n, h, w, C))
    edge = torch.zeros((h, w), dtype=torch.bool)
    edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
    x32[:, edge] = torch.randn((n, int(edge.sum()), C), generator=g) * 5.0
    x = conv_split.split(x32)
    ref = _l2pool_reference(conv_split.merge(x).double().numpy())
    _check_l2pool(device.l2pool3s2_split(x.to(dev)), ref, "border values 5 x 6")
    # one corner pixel alone (bottom right; h even, w odd): it is tap (2, 1) of the last window, weight 2/16, and of no other
    one = torch.zeros((1, 4, 5, 64))
    one[0, 3, 4, :] = 8.0
    got = device.l2pool3s2_split(conv_split.split(one).to(dev))
    want32 = torch.full((1, 2, 3, 64), float(np.float32(1e-6)))
    want32[0, 1, 2] = float(np.float32(np.sqrt(64.0 * 2.0 / 16.0 + 1e-12)))
    assert torch.equal(bits16(got), bits16(conv_split.split(want32)))


# ------------------------------------------------------------------------------------------------------------------- head
def _features(g, n, h, w, C):
    """Non-negative split features (2n, h, w, 2C), a tenth of the channels zero on both sides and channel 1 constant on each
    side, and their exact values as float64."""
    from tise_toolbox_amd import conv_split
    v = torch.randn((2 * n, h, w, C), generator=g).abs() * torch.rand((2 * n, 1, 1, C), generator=g) * 4.0
    v[torch.rand(v.shape, generator=g) < 0.2] = 0.0
    v[..., ::10] = 0.0                                                       # channels 0, 10, ..: zero on both sides
    v[:n, :, :, 1], v[n:, :, :, 1] = 1.7, 0.3                                # channel 1: constant over the pixels
    s = conv_split.split(v)
    hi, lo = conv_split.halves(s)
    return s, hi.double().numpy() + lo.double().numpy() / 2048.0


def _layer_reference(val, alpha, beta, n):
    """Per-pair sum_c alpha_c (1 - S1_c) + beta_c (1 - S2_c) in extended precision."""
    L = np.longdouble
    C = val.shape[-1]
    a, b = val[:n].astype(L).reshape(n, -1, C), val[n:].astype(L).reshape(n, -1, C)
    mx, my = a.mean(1), b.mean(1)
    dx, dy = a - mx[:, None], b - my[:, None]
    vx, vy, cxy = (dx * dx).mean(1), (dy * dy).mean(1), (dx * dy).mean(1)
    c = L(1e-6)
    s1 = (2 * mx * my + c) / (mx * mx + my * my + c)
    s2 = (2 * cxy + c) / (vx + vy + c)
    return (alpha.astype(L) * (1 - s1) + beta.astype(L) * (1 - s2)).sum(1)


def _K(C, hw):
    """The factor of the bound (test_layer_against_numpy's docstring)."""
    slots = 256 // (C // 8)
    chain = min(hw, -(-WG // slots) + slots + -(-hw // WG))
    return 4 * chain + 40


def _run_layer(dev, s, alpha, beta, n, init=0.0):
    """One tise_dists_layer call with canaries around ``out`` and the workspace -> (n,) float64 numpy."""
    from tise_toolbox_amd import _lib, device
    h, w, C = s.shape[1], s.shape[2], s.shape[3] // 2
    need = device.dists_workspace_bytes(n, h, w, C)
    assert need == 8 * n * C * (7 * ((h * w + WG - 1) // WG) + 2)
    out = torch.full((n + 4,), SENT, dtype=torch.float64, device=dev)
    out[2:2 + n] = init
    ws = torch.full((need // 8 + 16,), SENT, dtype=torch.float64, device=dev)
    _lib.call("tise_dists_layer", P(s), ctypes.c_int64(n), h, w, C, P(alpha), P(beta), P(out, 16), P(ws, 64), ctypes.c_size_t(need),
              stream())
    torch.cuda.synchronize()
    o, wsh = out.cpu().numpy(), ws.cpu().numpy()
    assert (o[:2] == SENT).all() and (o[2 + n:] == SENT).all(), "the canaries around out"
    assert (wsh[:8] == SENT).all() and (wsh[8 + need // 8:] == SENT).all(), "the canaries around the workspace"
    return o[2:2 + n].copy()


# hw: 1, 2, either side of 64, 257, and 513 = one pixel past a workgroup's share, so that two partials are combined
LAYER_SHAPES = [(1, 1), (1, 2), (7, 9), (8, 8), (5, 13), (1, 257), (19, 27)]


@pytest.mark.parametrize("C", [16, 64, 128, 512, 48])
def test_layer_against_numpy(dev, C):
    """BOUND.  u = 2^-53; the features are non-negative and at most 64 (asserted).  A channel's sums are formed as a chain: a
    thread adds its share of a workgroup's 512 pixels in order (ceil(512 / P) terms, P = 256 / (C / 8) pixel slots), the P slots are
    added in order, then the ceil(hw / 512) workgroups: L = min(hw, ceil(512 / P) + P + ceil(hw / 512)) additions at most.
    Means: a sum of non-negative terms, relative error <= L u, one division: e = (L + 1) u on mx and my.  S1 = (2 mx my + c) /
    (mx^2 + my^2 + c) has only non-negative terms: the inputs move numerator and denominator by <= 2 e each, their own three
    roundings each and the division add 7 u: |dS1| <= 4 e + 7 u.  Second moments about the computed means: x - mx (u), the product
    (u), the chain (L u): every term of vx, vy is non-negative and |dx dy| <= (dx^2 + dy^2) / 2, so the absolute errors of vx + vy
    and of 2 cxy are <= (L + 3) u (vx + vy); the shift of the means by d <= e * 64 adds d^2 to each moment, and d^2 / c <= (137 u
    64)^2 / 1e-6 < u for every shape here.  With |2 cxy + c| <= vx + vy + c: |dS2| <= 2 (L + 3) u + 5 u + 2 u.  Then 1 - S (u
    each), the products with alpha and beta (u each, |1 - S1| <= 1, |1 - S2| <= 2) and the sum over the channels -- 2 additions
    in a thread, 6 in the butterfly, 3 across the waves, 1 into out: 12 u of at most 2 sum(|alpha| + |beta|).  Together
    |error| <= (4 L + 40) u sum_c (|alpha_c| + |beta_c|): K = 4 L + 40 grows like hw / 512, the serial chain over the workgroups.
    The reference is formed in extended precision (its own error is below 2^-60)."""
    g = torch.Generator().manual_seed(C)
    worst = 0.0
    for k, (h, w) in enumerate(LAYER_SHAPES):
        n = 1 if k % 2 else 3
        s, val = _features(g, n, h, w, C)
        assert 0.0 <= val.min() and val.max() <= 64.0
        alpha = torch.randn(C, generator=g, dtype=torch.float64) / C         # signed: the bound is in |alpha_c| + |beta_c|
        beta = torch.randn(C, generator=g, dtype=torch.float64) / C
        want = _layer_reference(val, alpha.numpy(), beta.numpy(), n)
        got = _run_layer(dev, s.to(dev), alpha.to(dev), beta.to(dev), n)
        bound = _K(C, h * w) * 2.0 ** -53 * float(alpha.abs().sum() + beta.abs().sum())
        err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
        print(f"dists layer C={C} hw={h * w} n={n}: K = {_K(C, h * w)}, worst error / bound = {float(err.max() / bound):.4f}")
        worst = max(worst, float(err.max() / bound))
        assert (err <= bound).all(), (C, h, w, err, bound)
        again = _run_layer(dev, s.to(dev), alpha.to(dev), beta.to(dev), n)   # two calls: the same bits
        assert again.tobytes() == got.tobytes()
        added = _run_layer(dev, s.to(dev), alpha.to(dev), beta.to(dev), n, init=0.5)     # the value is ADDED into out
        assert added.tobytes() == (0.5 + got).tobytes()
    assert worst <= 1.0


@pytest.mark.parametrize("C,h,w", [(64, 5, 13), (48, 5, 13), (512, 5, 13), (64, 19, 27)])
def test_layer_exact_cases(dev, C, h, w):
    from tise_toolbox_amd import conv_split
    g = torch.Generator().manual_seed(1000 + C + h)
    n = 3
    s, val = _features(g, n, h, w, C)
    alpha = (torch.rand(C, generator=g, dtype=torch.float64) / C).to(dev)
    beta = (torch.rand(C, generator=g, dtype=torch.float64) / C).to(dev)
    zeros = np.zeros(n).tobytes()
    # identical features: exactly 0.0 (and -0.0 is not accepted either)
    same = torch.cat([s[:n], s[:n]], 0)
    assert _run_layer(dev, same.to(dev), alpha, beta, n).tobytes() == zeros
    # channel 1 is constant on both sides (1.7 and 0.3): its variances and covariance are exactly 0, so S2 = c / c = 1 and
    # alpha = 0, beta = e_1 gives exactly 0.0; alpha = e_1 gives 1 - S1 of the two constants
    e1 = torch.zeros(C, dtype=torch.float64, device=dev)
    e1[1] = 1.0
    zero = torch.zeros(C, dtype=torch.float64, device=dev)
    assert _run_layer(dev, s.to(dev), zero, e1, n).tobytes() == zeros
    a, b = val[0, 0, 0, 1], val[n, 0, 0, 1]
    want = 1.0 - (2.0 * a * b + 1e-6) / (a * a + b * b + 1e-6)
    got = _run_layer(dev, s.to(dev), e1, zero, n)
    assert np.abs(got - want).max() <= 8 * 2.0 ** -53 and want > 0.1
    # constant on side one only: the covariance is exactly 0, S2 = c / (vy + c)
    half = s.clone()
    half[n:] = conv_split.split(torch.from_numpy(val[n:]).float() * torch.rand((n, h, w, 1), generator=g))
    hv = conv_split.merge(half).double().numpy()
    vy = hv[n:, :, :, 1].reshape(n, -1).var(1)
    got = _run_layer(dev, half.to(dev), zero, e1, n)
    assert np.abs(got - (1.0 - 1e-6 / (vy + 1e-6))).max() <= _K(C, h * w) * 2.0 ** -53 and (got > 0.5).all()
    # channels that are zero on both sides add exactly 0: only they carry weight
    z = torch.zeros(C, dtype=torch.float64, device=dev)
    z[::10] = 0.25
    assert _run_layer(dev, s.to(dev), z, z, n).tobytes() == zeros
    # a NaN (and an inf) in pair 1's features reaches pair 1's number only
    base = _run_layer(dev, s.to(dev), alpha, beta, n)
    for poison in (float("nan"), float("inf")):
        hi, lo = conv_split.halves(s.clone())
        hi = hi.clone()
        hi[1, h - 1, w - 1, C - 1] = poison                                  # side one of pair 1, the last pixel and channel
        bad = conv_split._interleave(hi, lo.clone())
        got = _run_layer(dev, bad.to(dev), alpha, beta, n)
        assert np.isnan(got[1]) and got[[0, 2]].tobytes() == base[[0, 2]].tobytes(), (poison, got, base)


def test_layer_wrapper_and_pair_independence(dev):
    """device.dists_layer: a pair's bits do not depend on n or on its position in the launch."""
    from tise_toolbox_amd import device
    g = torch.Generator().manual_seed(77)
    n, h, w, C = 3, 19, 27, 64
    s, _ = _features(g, n, h, w, C)
    alpha = (torch.rand(C, generator=g, dtype=torch.float64) / C).to(dev)
    beta = (torch.rand(C, generator=g, dtype=torch.float64) / C).to(dev)
    sd = s.to(dev)

    def run(t, m):
        return device.dists_layer(t, alpha, beta, torch.zeros(m, dtype=torch.float64, device=dev)).cpu().numpy()
    full = run(sd, n)
    assert (full > 0).all()
    for i in range(n):
        assert run(torch.stack([sd[i], sd[n + i]]), 1).tobytes() == full[i:i + 1].tobytes()
    assert run(torch.cat([sd[:n].flip(0), sd[n:].flip(0)], 0), n)[::-1].tobytes() == full.tobytes()
    assert run(torch.cat([sd[n:], sd[:n]], 0), n).tobytes() == full.tobytes()          # the two sides exchanged: the same bits
    assert run(sd, n).tobytes() == full.tobytes()                                       # a second call
    with pytest.raises(ValueError, match="at most 512 channels"):
        device.dists_layer(torch.zeros((2, 1, 1, 2 * 528), dtype=torch.float16, device=dev), torch.zeros(528, dtype=torch.float64, device=dev),
                           torch.zeros(528, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError, match="alpha must be 64 contiguous float64"):
        device.dists_layer(sd, alpha.float(), beta, torch.zeros(n, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError, match="out must be"):
        device.dists_layer(sd, alpha, beta, torch.zeros(n, dtype=torch.float32, device=dev))
    with pytest.raises(ValueError, match="workspace"):
        device.dists_layer(sd, alpha, beta, torch.zeros(n, dtype=torch.float64, device=dev), workspace=torch.zeros(8, dtype=torch.uint8, device=dev))


# ------------------------------------------------------------------------------------------------------------ stage-0 sums
def _want_sums(xs, ys):
    out = []
    for a, b in zip(xs, ys):
        x, y = a.numpy().astype(np.int64), b.numpy().astype(np.int64)
        out.append(np.stack([x.sum((0, 1)), y.sum((0, 1)), (x * x).sum((0, 1)), (y * y).sum((0, 1)), (x * y).sum((0, 1))], -1))
    return np.stack(out)


@pytest.mark.parametrize("h,w", [(16, 16), (17, 19), (65, 64)])                # 65 x 64: two workgroups per pair
def test_image_sums_exact(dev, h, w):
    from tise_toolbox_amd import device
    g = torch.Generator().manual_seed(h * 100 + w)
    n = 3
    xs = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8) for _ in range(n)]
    ys = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8) for _ in range(n)]
    xs[2], ys[2] = torch.zeros((h, w, 3), dtype=torch.uint8), torch.full((h, w, 3), 255, dtype=torch.uint8)      # all-0 against all-255
    want = _want_sums(xs, ys)
    assert want.shape == (n, 3, 5) and want.dtype == np.int64
    dx, dy = [t.to(dev) for t in xs], [t.to(dev) for t in ys]
    odd = torch.zeros(h * w * 3 + 1, dtype=torch.uint8, device=dev)                    # one source at an odd byte address
    odd[1:] = dx[1].reshape(-1)
    dx[1] = odd[1:].view(h, w, 3)
    assert dx[1].data_ptr() % 2 == 1 and dx[1].is_contiguous()
    big = torch.full((n + 2, 3, 5), -77, dtype=torch.int64, device=dev)                # canaries around the output
    got = device.dists_image_sums(dx, dy, out=big[1:1 + n])
    torch.cuda.synchronize()
    assert bool((big[0] == -77).all()) and bool((big[-1] == -77).all())
    assert np.array_equal(got.cpu().numpy(), want)                                     # all fifteen integers of every pair
    assert np.array_equal(device.dists_image_sums(torch.stack(xs).to(dev), torch.stack(ys).to(dev)).cpu().numpy(), want)
    with pytest.raises(ValueError, match="one size"):
        device.dists_image_sums([dx[0], dx[0][:h - 1]], [dy[0], dy[0][:h - 1]])


# ---------------------------------------------------------------------------------------- convolutions at DISTS's new widths
CONV_LAYERS = [(64, 128), (512, 512)]


@pytest.fixture(scope="module")
def conv_layers(dev):
    """Per layer: (SplitConv left to auto, fp64 weight, fp64 bias), built once."""
    from tise_toolbox_amd.conv_split import SplitConv
    out = {}
    for cin, cout in CONV_LAYERS:
        g = torch.Generator().manual_seed(cin * 1000 + cout)
        wt = torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (9 * min(cin, 64))) ** 0.5
        bias = torch.randn(cout, generator=g) * 0.1
        out[(cin, cout)] = (SplitConv(wt, bias, (1, 1), (1, 1), dev), wt.double(), bias.double())
    return out


@pytest.mark.parametrize("ow", [1, 2, 3, 5, 9])
@pytest.mark.parametrize("cin,cout", CONV_LAYERS)
def test_conv_at_dists_widths(dev, conv_layers, cin, cout, ow):
    from tise_toolbox_amd import conv_split
    conv, w64, b64 = conv_layers[(cin, cout)]
    g = torch.Generator().manual_seed(ow)
    n, h = 1, 3
    x = conv_split.split(torch.randn((n, h, ow, cin), generator=g))
    xv = conv_split.halves(x)
    ref_in = (xv[0].double() + xv[1].double() / 2048.0).permute(0, 3, 1, 2)
    want = torch.relu(F.conv2d(ref_in, w64, b64, 1, 1)).permute(0, 2, 3, 1)
    scale = want.abs().max().item()
    y = torch.full((n, h, ow, 2 * cout), SENT, dtype=torch.float16, device=dev)
    assert conv(x.to(dev), [(0, cout, y, 0, 0)]) == (h, ow)
    torch.cuda.synchronize()
    hi, lo = conv_split.halves(y.cpu())
    got = hi.double() + lo.double() / 2048.0
    err = (got - want).abs().max().item()
    print(f"conv {cin}->{cout} OW={ow}: error / scale = {err / scale:.3e}")
    assert err <= CONV_TOL * scale, (cin, cout, ow, err, scale)
