"""GPU: tise_countseg_head (csrc/countseg.hip) alone, on seeded fp32 ``mix``, against the numpy fp64 restatement of
tests/_countseg_ref.py -- every map size at which the kernel takes another path (one pixel, one row, one column, fewer and more
pixels than the workgroup has threads, the limit), full and partial class groups, a leading dimension with an offset -- its exact
integer tie cases, a NaN, canaries around the four outputs, its reproducibility, and the 2048 -> 240 mix convolution.

Bounds (derived, not measured): a map value is b + P products, each exact in fp64, added one at a time: at most P + 1 roundings of
the partial sums, (P + 2) 2^-53 (|b| + sum |W||T|).  A confidence or density mean adds at most hw more terms and one division:
(P + hw + 2) 2^-53 of the absolute sum."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _countseg_ref as R
from tests._trunk_audit import CONV_TOL

pytestmark = pytest.mark.gpu

SIZES = ((1, 1), (1, 2), (2, 1), (1, 5), (3, 3), (2, 7), (14, 14), (15, 17), (32, 32))
WIDTHS = ((120, 80), (8, 3), (8, 1))
U = 2.0 ** -53
PAD = 16                                                             # canary elements on either side of an output


def seeded(n, h, w, P, C, ld, off, seed):
    """-> dict of fp32 numpy arrays: mix (n, h, w, ld) with NaN outside [off, off + 2P) (the kernel must not read it into a
    result), and the head's parameters."""
    rng = np.random.default_rng(seed)
    mix = np.full((n, h, w, ld), np.nan, dtype=np.float32)
    mix[..., off:off + 2 * P] = rng.standard_normal((n, h, w, 2 * P)).astype(np.float32)
    he = np.float32((2.0 / P) ** 0.5)
    return dict(mix=mix, off=off, P=P, C=C,
                b_mix=(0.1 * rng.standard_normal(2 * P)).astype(np.float32),
                w_cls=(he * rng.standard_normal((C, P))).astype(np.float32), b_cls=rng.standard_normal(C).astype(np.float32),
                w_den=(he * rng.standard_normal((C, P))).astype(np.float32), b_den=rng.uniform(-0.5, 3.5, C).astype(np.float32))


def t_of(case):
    """T = fp32(mix + b_mix) of the case's own channels, (n, h, w, 2P)."""
    P, off = case["P"], case["off"]
    return (case["mix"][..., off:off + 2 * P] + case["b_mix"]).astype(np.float32)


def reference(case):
    with np.errstate(invalid="ignore", over="ignore"):
        return R.head(t_of(case), case["w_cls"], case["b_cls"], case["w_den"], case["b_den"])


def launch(dev, case, want_maps=True):
    """One tise_countseg_head call with canaries around the four outputs -> (conf, den, peaks, maps | None) as numpy."""
    from tise_toolbox_amd import _lib
    n, h, w, ld = case["mix"].shape
    C, P = case["C"], case["P"]
    on = {k: torch.from_numpy(np.ascontiguousarray(case[k])).to(dev) for k in ("mix", "b_mix", "w_cls", "b_cls", "w_den", "b_den")}
    sizes = {"conf": n * C, "den": n * C, "peaks": n * C, "maps": n * 2 * C * h * w}
    bufs = {k: torch.full((sizes[k] + 2 * PAD,), -777, dtype=torch.int32 if k == "peaks" else torch.float64, device=dev) for k in sizes}
    ptr = lambda t, at=0: ctypes.c_void_p(t.data_ptr() + at * t.element_size())
    _lib.call("tise_countseg_head", ptr(on["mix"]), ctypes.c_int64(ld), int(case["off"]), ptr(on["b_mix"]), ptr(on["w_cls"]),
              ptr(on["b_cls"]), ptr(on["w_den"]), ptr(on["b_den"]), ctypes.c_int64(n), h, w, P, C, ptr(bufs["conf"], PAD),
              ptr(bufs["den"], PAD), ptr(bufs["peaks"], PAD), ptr(bufs["maps"], PAD) if want_maps else ctypes.c_void_p(None),
              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    out = {}
    for k, t in bufs.items():
        a = t.cpu().numpy()
        assert (a[:PAD] == -777).all() and (a[PAD + sizes[k]:] == -777).all(), f"{k}: a canary was overwritten"
        out[k] = a[PAD:PAD + sizes[k]]
    if not want_maps:
        assert (out["maps"] == -777).all()
    return (out["conf"].reshape(n, C), out["den"].reshape(n, C), out["peaks"].reshape(n, C),
            out["maps"].reshape(n, 2 * C, h * w) if want_maps else None)


def check(dev, case):
    n, h, w, _ = case["mix"].shape
    P, C = case["P"], case["C"]
    conf, den, peaks, maps = reference(case)
    bound = R.map_bound(t_of(case), case["w_cls"], case["b_cls"], case["w_den"], case["b_den"])          # (n, 2C, hw)
    scale = float(np.abs(maps).max())
    margin = R.decision_margin(maps[:, :C].reshape(n, C, h, w), conf, den)
    assert (margin >= 1e-9 * scale).all(), f"bad fixture: margin {margin} at map scale {scale}"
    g_conf, g_den, g_peaks, g_maps = launch(dev, case)
    err = np.abs(g_maps - maps) / ((P + 2) * U * bound)
    assert err.max() <= 1.0, err.max()
    assert np.array_equal(g_peaks, peaks)
    sel = (R.local_maxima(maps[:, :C].reshape(n, C, h, w)) & (maps[:, :C].reshape(n, C, h, w) >=
                                                              np.sort(maps[:, :C], 2)[:, :, (h * w - 1) // 2, None, None])).reshape(n, C, h * w)
    conf_abs = (bound[:, :C] * sel).sum(2) / peaks
    den_abs = bound[:, C:].sum(2) / (h * w)
    tol = (P + h * w + 2) * U
    e_conf, e_den = np.abs(g_conf - conf) / (tol * conf_abs), np.abs(g_den - den) / (tol * den_abs)
    print(f"countseg head {h}x{w} P={P} C={C} n={n} ld={case['mix'].shape[3]}: maps {err.max():.3f} conf {e_conf.max():.3f} den {e_den.max():.3f} "
          f"of their bounds; peaks {peaks.min()}..{peaks.max()}; margin / scale {margin.min() / scale:.2e}")
    assert e_conf.max() <= 1.0 and e_den.max() <= 1.0
    no_maps = launch(dev, case, want_maps=False)                             # a null ``maps`` skips it and changes nothing else
    assert no_maps[0].tobytes() == g_conf.tobytes() and no_maps[1].tobytes() == g_den.tobytes() and np.array_equal(no_maps[2], g_peaks)


@pytest.mark.parametrize("P,C", WIDTHS)
@pytest.mark.parametrize("h,w", SIZES)
def test_head_against_the_restatement(cuda_device, h, w, P, C):
    seed = 1000 * h + 10 * w + C
    check(cuda_device, seeded(1, h, w, P, C, 2 * P, 0, seed))                                # n = 1, the dense leading dimension
    check(cuda_device, seeded(3, h, w, P, C, 256, 12 if P == 120 else 236, seed + 1))        # n = 3, ld 256 at an offset


def test_a_larger_map_is_refused(cuda_device):
    from tise_toolbox_amd import _lib, device
    case = seeded(1, 33, 32, 8, 3, 16, 0, 5)
    with pytest.raises(_lib.TiseStatusError) as e:
        launch(cuda_device, case)
    assert e.value.status == _lib.TISE_ERR_UNSUPPORTED
    with pytest.raises(ValueError, match="1024 pixels"):
        device.countseg_head(*(torch.from_numpy(case[k]).to(cuda_device) for k in ("mix", "b_mix", "w_cls", "b_cls", "w_den", "b_den")))


def tie_case(m):
    """Small-integer parameters that put the integer map ``m`` (and two maps made from it) into the class branch: P = 8, C = 3,
    class 0 = m, class 1 = -m, class 2 = 2 m + 1; the density maps are small integers too.  Every value is exact."""
    h, w = m.shape
    P, C = 8, 3
    rng = np.random.default_rng(h * 16 + w)
    mix = np.zeros((1, h, w, 2 * P), dtype=np.float32)
    b_mix = rng.integers(-3, 4, 2 * P).astype(np.float32)
    mix[0, :, :, 0] = m - b_mix[0]                                           # T_0 = m
    mix[0, :, :, 1:] = rng.integers(-4, 5, (h, w, 2 * P - 1)).astype(np.float32)
    w_cls = np.zeros((C, P), dtype=np.float32)
    w_cls[0, 0], w_cls[1, 0], w_cls[2, 0] = 1.0, -1.0, 2.0
    b_cls = np.array([0.0, 0.0, 1.0], dtype=np.float32)
    return dict(mix=mix, off=0, P=P, C=C, b_mix=b_mix, w_cls=w_cls, b_cls=b_cls,
                w_den=rng.integers(-2, 3, (C, P)).astype(np.float32), b_den=rng.integers(-2, 3, C).astype(np.float32))


@pytest.mark.parametrize("name", sorted(R.TIE_MAPS))
def test_integer_tie_cases_are_bit_equal(cuda_device, name):
    m, peak_at, conf0 = R.TIE_MAPS[name]
    case = tie_case(m)
    conf, den, peaks, maps = reference(case)
    assert np.array_equal(maps[0, 0].reshape(m.shape), m) and conf[0, 0] == conf0 and peaks[0, 0] == len(peak_at)
    got = launch(cuda_device, case)
    for g, r in zip(got, (conf, den, peaks, maps)):
        assert g.tobytes() == r.astype(g.dtype).tobytes(), name


def test_a_nan_stays_in_its_image_and_class(cuda_device):
    """W_cls[1][5] = inf and T_5 = 0 at one pixel of image 1: inf * 0 = NaN in class 1 of image 1 only.  (The other images' class-1
    maps are +inf everywhere by their own arithmetic: confidence inf from the one peak a constant map has.)"""
    case = seeded(3, 5, 6, 8, 3, 16, 0, 77)
    case["w_cls"][1, 5] = np.inf
    case["mix"][..., 5] = np.abs(case["mix"][..., 5]) + 1.0
    case["b_mix"][5] = 0.25
    case["mix"][1, 2, 3, 5] = -0.25
    conf, den, peaks, maps = reference(case)
    assert np.argwhere(np.isnan(conf)).tolist() == [[1, 1]] and peaks[1, 1] == 0 and np.isfinite(den).all()
    assert np.isinf(conf[0, 1]) and np.isinf(conf[2, 1]) and peaks[0, 1] == 1 and np.isfinite(conf[:, [0, 2]]).all()
    g_conf, g_den, g_peaks, g_maps = launch(cuda_device, case)
    assert np.argwhere(np.isnan(g_conf)).tolist() == [[1, 1]] and np.array_equal(g_peaks, peaks)
    keep = np.isfinite(conf)
    assert np.array_equal(np.isinf(g_conf), np.isinf(conf)) and np.allclose(g_conf[keep], conf[keep], rtol=1e-13, atol=0)
    assert np.allclose(g_den, den, rtol=1e-13, atol=1e-15) and np.array_equal(np.isnan(g_maps), np.isnan(maps))


def test_bits_do_not_depend_on_batch_position_or_call(cuda_device):
    case = seeded(4, 15, 17, 120, 80, 240, 0, 9)
    whole = launch(cuda_device, case)
    again = launch(cuda_device, case)
    rev = dict(case, mix=np.ascontiguousarray(case["mix"][::-1]))
    back = launch(cuda_device, rev)
    alone = launch(cuda_device, dict(case, mix=np.ascontiguousarray(case["mix"][2:3])))
    for k in range(4):
        assert whole[k].tobytes() == again[k].tobytes()
        assert whole[k].tobytes() == np.ascontiguousarray(back[k][::-1]).tobytes()
        assert whole[k][2:3].tobytes() == alone[k].tobytes()


def test_device_wrapper(cuda_device):
    from tise_toolbox_amd import device
    case = seeded(2, 3, 3, 8, 3, 32, 8, 21)
    on = [torch.from_numpy(case[k]).to(cuda_device) for k in ("mix", "b_mix", "w_cls", "b_cls", "w_den", "b_den")]
    conf, den, peaks, maps = device.countseg_head(*on, off=8, want_maps=True)
    want = launch(cuda_device, case)
    for g, r in zip((conf, den, peaks, maps), want):
        assert g.cpu().numpy().tobytes() == r.tobytes()
    assert len(device.countseg_head(*on, off=8)) == 3
    with pytest.raises(ValueError, match="b_cls"):
        device.countseg_head(on[0], on[1], on[2], on[3][:2], on[4], on[5], off=8)
    with pytest.raises(ValueError, match="float32"):
        device.countseg_head(on[0].double(), *on[1:])


@pytest.mark.parametrize("side", (1, 2, 14))
def test_mix_convolution_against_fp64(cuda_device, side):
    """The 2048 -> 240 SplitConv of the route, kernel choice left to auto, in mode 1 (scale * conv, no bias) at the map sizes of 32,
    64 and 448 pixel images."""
    from tise_toolbox_amd.conv_split import SplitConv, merge, split
    g = torch.Generator().manual_seed(side)
    n = 2
    x = torch.randn((n, side, side, 2048), generator=g).abs_()
    wgt = torch.randn((240, 2048, 1, 1), generator=g) * (2.0 / 2048) ** 0.5
    xs = split(x).to(cuda_device)
    conv = SplitConv(wgt, torch.randn(240, generator=g), (1, 1), (0, 0), cuda_device, name="mix")
    raw = torch.full((n, side, side, 240), float("nan"), dtype=torch.float32, device=cuda_device)
    conv(xs, [(0, 240, raw, 0, 1)])
    ref = merge(xs.cpu()).double().reshape(-1, 2048) @ wgt.double().reshape(240, 2048).T
    err = (raw.cpu().double().reshape(-1, 240) - ref).abs().max().item() / ref.abs().max().item()
    print(f"mix convolution {side}x{side}: variant {conv.variant} tn {conv.tn}, error / scale {err:.3e}")
    assert err <= CONV_TOL
