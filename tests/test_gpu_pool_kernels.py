"""GPU: the pool, bias and stem kernels of csrc/trunk_ops.hip against the fp32 emulations of tests/_pool_ref.py at every
layout edge -- one-pixel and one-row maps, maps a stride-2 window does not cover, channel slices at odd offsets of wider
tensors, split tensors with a 16-channel tail block, the grid-stride loops' second pass, the argument checks.

Tolerance: none.  Max pools, bias_relu, the FMA stems AND the average pools must equal their emulation bit for bit: the
library is built with ``-O3 --offload-arch=gfx950 -std=c++17 -fPIC`` and nothing else (tise_toolbox_amd/build.py) -- no
fast-math, no relaxed division, fp32 denormals kept -- so HIP's default holds, correctly rounded fp32 division (the kernels'
``/ div`` compiles to v_div_scale / v_rcp / v_div_fmas / v_div_fixup, the IEEE sequence), and every other step is a single
fp32 add, max or conversion.  The emulations are validated against fp64 without a GPU in tests/test_pool_ref_host.py.

Memory hygiene: everything outside the input slice is NaN (the kernels never read it), everything outside the output slice a
sentinel that must survive."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _avgpool_child as child
from tests import _pool_ref as pr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT32 = np.float32(-7.25)
SENT16 = child.SENTINEL
GRID_CAP = 16384 * 256          # grid_for: at most 16384 blocks of 256 threads; more elements take the loop's second pass


@pytest.fixture(scope="module")
def dev(cuda_device):
    return cuda_device


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def call(name, *args):
    from tise_toolbox_amd import _lib
    _lib.call(name, *args)


def status(name, *args):
    from tise_toolbox_amd import _lib
    return getattr(_lib.load(), name)(*args)


def dv(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def out_hw(kind, h, w):
    return ((h - 3) // 2 + 1, (w - 3) // 2 + 1) if kind == "s2" else (h, w)


def same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    bad = pr.bits(got) != pr.bits(want)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4], want[bad][:4])


# ------------------------------------------------------------------------------------------------- fp32 forms
def _f32_case(g, n, h, w, oh, ow, sl, dev):
    C, x_ld, x_off, out_ld, out_off = sl
    xs = g.standard_normal((n, h, w, C)).astype(np.float32)
    x = np.full((n, h, w, x_ld), np.nan, dtype=np.float32)
    x[..., x_off:x_off + C] = xs
    bias = g.standard_normal(C).astype(np.float32)
    out = torch.full((n, oh, ow, out_ld), float(SENT32), dtype=torch.float32, device=dev)
    return xs, bias, dv(x, dev), dv(bias, dev), out


def _check_f32(out, want, sl, what):
    C, _, _, _, out_off = sl
    got = out.cpu().numpy()
    same_bits(got[..., out_off:out_off + C], want, what)
    rest = np.delete(got, np.s_[out_off:out_off + C], axis=-1)
    assert (pr.bits(rest) == pr.bits(np.array(SENT32))).all(), (what, "wrote outside its output slice")


F32_KERNELS = {
    "bias_relu": ("s1", lambda xs, b: pr.bias_relu(xs, b)),
    "avgpool": ("s1", lambda xs, b: pr.avgpool_per_output(xs, b, False)),
    "avgpool_excl": ("s1", lambda xs, b: pr.avgpool_per_output(xs, b, True)),
    "maxpool3s1p1": ("s1", lambda xs, b: pr.maxpool3s1p1(xs)),
    "maxpool3s2": ("s2", lambda xs, b: pr.maxpool3s2(xs)),
    "maxpool3s2_bias": ("s2", lambda xs, b: pr.maxpool3s2(xs, b)),
}


def _launch_f32(kernel, x, bias, out, n, h, w, sl):
    C, x_ld, x_off, out_ld, out_off = sl
    if kernel == "bias_relu":
        call("tise_bias_relu_nhwc", P(x), x_ld, x_off, n * h * w, C, P(bias), P(out), out_ld, out_off, st())
    elif kernel in ("avgpool", "avgpool_excl"):
        call("tise_avgpool3_excl_bias_relu_nhwc" if kernel == "avgpool_excl" else "tise_avgpool3_bias_relu_nhwc",
             P(x), x_ld, x_off, n, h, w, C, P(bias), P(out), out_ld, out_off, st())
    elif kernel == "maxpool3s1p1":
        call("tise_maxpool3s1p1_nhwc", P(x), x_ld, x_off, n, h, w, C, P(out), out_ld, out_off, st())
    else:
        call("tise_maxpool3s2_nhwc", P(x), x_ld, x_off, n, h, w, C, P(bias) if kernel == "maxpool3s2_bias" else None, P(out),
             out_ld, out_off, st())


@pytest.mark.parametrize("kernel", list(F32_KERNELS))
def test_fp32_kernels_equal_their_emulation_at_every_map_and_slice(dev, kernel):
    kind, emu = F32_KERNELS[kernel]
    i = 0
    for (h, w) in (pr.MAPS_S2 if kind == "s2" else pr.MAPS_S1):
        for n in pr.BATCHES:
            for sl in pr.SLICES_F32:
                g = np.random.default_rng(100 + i)
                i += 1
                oh, ow = out_hw(kind, h, w)
                xs, bias, x, b, out = _f32_case(g, n, h, w, oh, ow, sl, dev)
                _launch_f32(kernel, x, b, out, n, h, w, sl)
                _check_f32(out, emu(xs, bias), sl, (kernel, n, h, w, sl))


# ------------------------------------------------------------------------------------------------- split max pools
@pytest.mark.parametrize("kernel", ["maxpool3s2_split", "maxpool3s1p1_split"])
def test_split_max_pools_equal_their_emulation_at_every_block_edge(dev, kernel):
    """Input (80 channels) and output (112 channels) both end in a 16-channel tail block; slices inside full blocks, inside
    the tail, ending at the tail boundary, 8 wide at the second half of a 32-block, and across the boundary."""
    kind = "s2" if kernel == "maxpool3s2_split" else "s1"
    pool = pr.maxpool3s2 if kind == "s2" else pr.maxpool3s1p1
    xc, oc = pr.SPLIT_X_C, pr.SPLIT_OUT_C
    i = 0
    for (h, w) in (pr.MAPS_S2 if kind == "s2" else pr.MAPS_S1):
        for n in pr.BATCHES:
            for (x_off, C, out_off) in pr.SLICES_SPLIT:
                g = np.random.default_rng(300 + i)
                i += 1
                oh, ow = out_hw(kind, h, w)
                v = (g.random((n, h, w, C)) * 5.0).astype(np.float32)
                v[g.random(v.shape) < 0.2] = 0.0                          # post-ReLU activations: exact zeros among them
                x = np.full((n, h, w, 2 * xc), np.nan, dtype=np.float16)
                pr.pack_split(x, v, x_off)
                out = torch.full((n, oh, ow, 2 * oc), float(SENT16), dtype=torch.float16, device=dev)
                xd = dv(x, dev)
                call(f"tise_{kernel}_nhwc", P(xd), xc, x_off, n, h, w, C, P(out), oc, out_off, st())
                got = out.cpu().numpy()
                whi, wlo = pr.maxpool_split(*pr.unpack_split(x, x_off, C), pool)
                ghi, glo = pr.unpack_split(got, out_off, C)
                same_bits(ghi, whi, (kernel, "hi", n, h, w, x_off, C, out_off))
                same_bits(glo, wlo, (kernel, "lo", n, h, w, x_off, C, out_off))
                assert (pr.bits(got[..., ~pr.slice_mask(oc, out_off, C)]) == pr.bits(np.array(SENT16))).all(), (kernel, "sentinel")


# ------------------------------------------------------------------------------------------------- split average pools
def _check_avg_split(cases, results, emu, what):
    for c, (got, flag) in zip(cases, results):
        xs = c["x"][..., c["x_off"]:c["x_off"] + c["C"]]
        whi, wlo = pr.split_value(emu(xs, c["bias"], c["excl"]))
        ghi, glo = pr.unpack_split(got, c["out_off"], c["C"])
        key = (what, c["n"], c["h"], c["w"], c["C"], c["x_ld"], c["x_off"], c["out_off"], c["excl"])
        same_bits(ghi, whi, key + ("hi",))
        same_bits(glo, wlo, key + ("lo",))
        assert (pr.bits(got[..., ~pr.slice_mask(c["out_C"], c["out_off"], c["C"])]) == pr.bits(np.array(SENT16))).all(), key
        assert not flag, key


def run_child(cases, tmp_path, tag):
    """Run ``cases`` through the per-output kernel: a fresh process with TISE_AVGPOOL_PER_OUTPUT=1 (one child for all cases)."""
    src, dst = str(tmp_path / f"{tag}_in.npz"), str(tmp_path / f"{tag}_out.npz")
    child.save_cases(src, cases)
    env = dict(os.environ, TISE_AVGPOOL_PER_OUTPUT="1")
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_avgpool_child.py"), src, dst], env=env, cwd=ROOT,
                           capture_output=True, text=True, timeout=240)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"avgpool child timed out; stderr:\n{e.stderr}")
    assert p.returncode == 0, f"avgpool child exit {p.returncode}; stderr:\n{p.stderr[-6000:]}"
    z = np.load(dst)
    assert bool(z["per_output"])
    return [(z[f"o{i}"], bool(z[f"f{i}"])) for i in range(len(cases))]


def test_split_average_pools_both_kernels_equal_their_emulations(dev, tmp_path):
    """The column-walking kernel (this process) and the per-output kernel (a child process: its switch is read once per
    process) on the same cases, each against the emulation of ITS summation order, bit for bit; on signed inputs the two
    orders must differ in the bits of some case, which shows that the child really ran the other kernel.  Against each other:
    on the non-negative cases of _pool_ref.avg_split_cross_cases (where the bound is derived) the values before the split lie
    within 2 fp32 ulp -- asserted on the emulations, which the kernels have just been shown to equal bit for bit -- and the
    stored values within 2 ulp + the two split roundings (half a unit of the lo half: 2^-20 each in the binade [8, 16))."""
    assert "TISE_AVGPOOL_PER_OUTPUT" not in os.environ, "this process must run the default (column-walking) kernel"
    cases = pr.avg_split_cases()
    cross = pr.avg_split_cross_cases()
    here = child.run_cases(cases + cross, dev)
    there = run_child(cases + cross, tmp_path, "avg")
    _check_avg_split(cases + cross, here, pr.avgpool_colwalk, "colwalk")
    _check_avg_split(cases + cross, there, pr.avgpool_per_output, "per-output")
    assert any(not np.array_equal(pr.bits(a[0]), pr.bits(b[0])) for a, b in zip(here[:len(cases)], there[:len(cases)]))
    worst = 0
    for c, (a, _), (b, _) in zip(cross, here[len(cases):], there[len(cases):]):
        xs = c["x"][..., c["x_off"]:c["x_off"] + c["C"]]
        ea, eb = pr.avgpool_colwalk(xs, c["bias"], c["excl"]), pr.avgpool_per_output(xs, c["bias"], c["excl"])
        assert ea.min() >= 8.0 and ea.max() < 16.0 and eb.min() >= 8.0 and eb.max() < 16.0
        worst = max(worst, int(pr.ulp_distance(ea, eb).max()))
        va = pr.merge_value(*pr.unpack_split(a, c["out_off"], c["C"])).astype(np.float64)
        vb = pr.merge_value(*pr.unpack_split(b, c["out_off"], c["C"])).astype(np.float64)
        assert np.abs(va - vb).max() <= 2 * 2.0 ** -20 + 2 * 2.0 ** -20, (c["h"], c["w"], c["excl"])
    print(f"split average pools: the two orders differ by at most {worst} fp32 ulp before the split")
    assert worst <= 2


# ------------------------------------------------------------------------------------------------- FMA stems
def _stem_inputs(g, n, h, w):
    u8 = g.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    lut = (g.random((3, 256)) * 2.4 - 1.2).astype(np.float32)
    wt = (g.standard_normal((3, 3, 3, 32)) * (2.0 / 27) ** 0.5 * np.exp2(g.integers(-3, 4, (1, 1, 1, 32)))).astype(np.float32)
    bias = (g.standard_normal(32) * 0.2).astype(np.float32)
    x = np.stack([lut[c][u8[..., c]] for c in range(3)], -1).astype(np.float32)
    return u8, lut, wt, bias, x


@pytest.mark.parametrize("form", ["fp32", "u8"])
def test_fma_stems_equal_the_fma_chain(dev, form):
    """stem_conv3x3s2_split (fp32 input) and stem_conv3x3s2_split_u8 (byte input + table; odd widths put the last window
    rows on unaligned addresses and at the end of the tensor: the byte-wise loader) against the (kh, kw, cin) FMA chain."""
    i = 0
    for (h, w) in pr.MAPS_S2:
        for n in pr.BATCHES:
            g = np.random.default_rng(700 + i)
            i += 1
            u8, lut, wt, bias, x = _stem_inputs(g, n, h, w)
            oh, ow = out_hw("s2", h, w)
            buf = torch.full((n * oh * ow * 64 + 64,), float(SENT16), dtype=torch.float16, device=dev)
            xd, ud, ld, wd, bd = dv(x, dev), dv(u8, dev), dv(lut.reshape(-1), dev), dv(wt, dev), dv(bias, dev)
            if form == "fp32":
                call("tise_stem_conv3x3s2_split", P(xd), n, h, w, P(wd), P(bd), P(buf), st())
            else:
                call("tise_stem_conv3x3s2_split_u8", P(ud), P(ld), n, h, w, P(wd), P(bd), P(buf), st())
            got = buf.cpu().numpy()
            assert (pr.bits(got[-64:]) == pr.bits(np.array(SENT16))).all(), "wrote past the output tensor"
            whi, wlo = pr.split_value(pr.stem_fma(x, wt, bias))
            ghi, glo = pr.unpack_split(got[:-64].reshape(n, oh, ow, 64))
            same_bits(ghi, whi, (form, "hi", n, h, w))
            same_bits(glo, wlo, (form, "lo", n, h, w))


# ------------------------------------------------------------------------------------------------- grid-stride wrap
def _rows(t, img, r0, r1):
    return t[img, r0:r1].cpu().numpy()[None]


@pytest.mark.parametrize("kernel", ["bias_relu", "avgpool", "maxpool3s2", "maxpool3s1p1", "stem"])
def test_grid_stride_second_pass(dev, kernel):
    """Just over 16384 x 256 elements in one launch: the grid is capped (grid_for) and the loop's second pass computes the
    rest.  The launch must equal the same kernel run on the two halves of the batch, bit for bit, and the emulation on rows
    of both images, among them the row that holds the first element of the second pass."""
    C = 32
    if kernel in ("bias_relu", "avgpool", "maxpool3s1p1"):
        n, h, w = 2, 513, 512
        oh, ow, per_pixel = h, w, C // 4
    elif kernel == "maxpool3s2":
        n, h, w = 2, 1027, 1025
        oh, ow, per_pixel = 513, 512, C // 4
    else:
        n, h, w = 2, 1027, 2049
        oh, ow, per_pixel = 513, 1024, 4
    total = n * oh * ow * per_pixel
    assert GRID_CAP < total < GRID_CAP + GRID_CAP // 64 and (n // 2) * oh * ow * per_pixel <= GRID_CAP
    first = GRID_CAP // per_pixel                                  # output pixel of the second pass's first element
    img, row = first // (oh * ow), (first % (oh * ow)) // ow
    assert img == 1 and 0 < row < oh - 1
    g = torch.Generator(device="cpu").manual_seed(11)
    bias = torch.randn(C, generator=g).to(dev)
    if kernel == "stem":
        x = (torch.rand((n, h, w, 3), device=dev) * 2.4 - 1.2)
        wt = (torch.randn((3, 3, 3, 32), generator=g) * (2.0 / 27) ** 0.5).to(dev)
        out = torch.empty((n, oh, ow, 64), dtype=torch.float16, device=dev)
        halves = torch.empty_like(out)

        def launch(xx, oo, nn):
            call("tise_stem_conv3x3s2_split", P(xx), nn, h, w, P(wt), P(bias), P(oo), st())
    else:
        x = torch.randn((n, h, w, C), device=dev)
        out = torch.empty((n, oh, ow, C), dtype=torch.float32, device=dev)
        halves = torch.empty_like(out)
        name = {"bias_relu": "bias_relu", "avgpool": "avgpool", "maxpool3s2": "maxpool3s2_bias", "maxpool3s1p1": "maxpool3s1p1"}[kernel]

        def launch(xx, oo, nn):
            _launch_f32(name, xx, bias, oo, nn, h, w, (C, C, 0, C, 0))
    launch(x, out, n)
    launch(x[:1], halves[:1], 1)
    launch(x[1:], halves[1:], 1)
    assert torch.equal(out.view(torch.int16 if kernel == "stem" else torch.int32), halves.view(torch.int16 if kernel == "stem" else torch.int32))
    b = bias.cpu().numpy()
    for (im, r0, r1) in [(0, 0, 2), (1, row - 1, row + 2), (1, oh - 2, oh)]:
        got = _rows(out, im, r0, r1)
        if kernel == "bias_relu":
            want = pr.bias_relu(_rows(x, im, r0, r1), b)
        elif kernel in ("avgpool", "maxpool3s1p1"):
            a, z = max(r0 - 1, 0), min(r1 + 1, h)                 # one row of context on each side, where the map has one: the compared rows see every tap
            full = (pr.avgpool_per_output(_rows(x, im, a, z), b) if kernel == "avgpool" else pr.maxpool3s1p1(_rows(x, im, a, z)))
            want = full[:, r0 - a:r0 - a + (r1 - r0)]
        elif kernel == "maxpool3s2":
            want = pr.maxpool3s2(_rows(x, im, 2 * r0, 2 * (r1 - 1) + 3), b)
        else:
            want = pr.stem_fma(_rows(x, im, 2 * r0, 2 * (r1 - 1) + 3), wt.cpu().numpy(), b)
        if kernel == "stem":
            whi, wlo = pr.split_value(want)
            ghi, glo = pr.unpack_split(got)
            same_bits(ghi, whi, (kernel, im, r0))
            same_bits(glo, wlo, (kernel, im, r0))
        else:
            same_bits(got, want, (kernel, im, r0))


# ------------------------------------------------------------------------------------------------- argument checks
def test_argument_checks_come_before_any_launch(dev):
    """TISE_ERR_INVALID_ARG for a misaligned offset, for x_off + C > x_ld (and the same on the output side), for C % 8 != 0 on
    the split forms; TISE_OK for n == 0.  The outputs stay untouched: nothing was launched."""
    from tise_toolbox_amd import _lib
    INV, OK = _lib.TISE_ERR_INVALID_ARG, _lib.TISE_OK
    x = torch.zeros((1, 4, 4, 32), device=dev)
    b = torch.zeros(32, device=dev)
    o = torch.full((1, 4, 4, 32), float(SENT32), device=dev)
    xs = torch.zeros((1, 4, 4, 2 * 48), dtype=torch.float16, device=dev)
    os_ = torch.full((1, 4, 4, 2 * 48), float(SENT16), dtype=torch.float16, device=dev)
    s = st()
    f32 = {
        "tise_bias_relu_nhwc": lambda x_ld, x_off, n, C, o_ld, o_off: (P(x), x_ld, x_off, n * 16, C, P(b), P(o), o_ld, o_off, s),
        "tise_avgpool3_bias_relu_nhwc": lambda x_ld, x_off, n, C, o_ld, o_off: (P(x), x_ld, x_off, n, 4, 4, C, P(b), P(o), o_ld, o_off, s),
        "tise_avgpool3_excl_bias_relu_nhwc": lambda x_ld, x_off, n, C, o_ld, o_off: (P(x), x_ld, x_off, n, 4, 4, C, P(b), P(o), o_ld, o_off, s),
        "tise_maxpool3s2_nhwc": lambda x_ld, x_off, n, C, o_ld, o_off: (P(x), x_ld, x_off, n, 4, 4, C, P(b), P(o), o_ld, o_off, s),
        "tise_maxpool3s1p1_nhwc": lambda x_ld, x_off, n, C, o_ld, o_off: (P(x), x_ld, x_off, n, 4, 4, C, P(o), o_ld, o_off, s),
    }
    for name, a in f32.items():
        assert status(name, *a(32, 0, 0, 16, 32, 0)) == OK, name                  # n == 0
        assert status(name, *a(32, 2, 1, 16, 32, 0)) == INV, name                 # misaligned input offset
        assert status(name, *a(32, 0, 1, 16, 32, 6)) == INV, name                 # misaligned output offset
        assert status(name, *a(32, 0, 1, 6, 32, 0)) == INV, name                  # C % 4
        assert status(name, *a(32, 20, 1, 16, 32, 0)) == INV, name                # x_off + C > x_ld
        assert status(name, *a(32, 0, 1, 16, 32, 20)) == INV, name                # out_off + C > out_ld
        assert status(name, *a(30, 0, 1, 16, 32, 0)) == INV, name                 # misaligned row stride
    avg = {fn: (lambda x_ld, x_off, n, C, o_ld, o_off, fn=fn: (P(x), x_ld, x_off, n, 4, 4, C, P(b), P(os_), o_ld, o_off, s))
           for fn in ("tise_avgpool3_bias_relu_split_nhwc", "tise_avgpool3_excl_bias_relu_split_nhwc")}
    for name, a in avg.items():
        assert status(name, *a(32, 0, 0, 16, 48, 0)) == OK, name
        assert status(name, *a(32, 2, 1, 16, 48, 0)) == INV, name                 # misaligned input offset
        assert status(name, *a(32, 0, 1, 16, 48, 4)) == INV, name                 # output offset not a multiple of 8
        assert status(name, *a(32, 0, 1, 12, 48, 0)) == INV, name                 # C % 8
        assert status(name, *a(32, 20, 1, 16, 48, 0)) == INV, name                # x_off + C > x_ld
        assert status(name, *a(32, 0, 1, 16, 48, 40)) == INV, name                # out_off + C > out_ld
        assert status(name, *a(32, 0, 1, 16, 40, 0)) == INV, name                 # output channel count not a multiple of 16
    for name in ("tise_maxpool3s2_split_nhwc", "tise_maxpool3s1p1_split_nhwc"):
        a = lambda x_ld, x_off, n, C, o_ld, o_off: (P(xs), x_ld, x_off, n, 4, 4, C, P(os_), o_ld, o_off, s)
        assert status(name, *a(48, 0, 0, 16, 48, 0)) == OK, name
        assert status(name, *a(48, 4, 1, 16, 48, 0)) == INV, name                 # input offset not a multiple of 8
        assert status(name, *a(48, 0, 1, 16, 48, 4)) == INV, name
        assert status(name, *a(48, 0, 1, 12, 48, 0)) == INV, name                 # C % 8
        assert status(name, *a(48, 40, 1, 16, 48, 0)) == INV, name                # x_off + C > x_ld
        assert status(name, *a(48, 0, 1, 16, 48, 40)) == INV, name
        assert status(name, *a(40, 0, 1, 16, 48, 0)) == INV, name                 # channel count not a multiple of 16
    for name, a in (("tise_stem_conv3x3s2_split", lambda n, h: (P(x), n, h, 4, P(b), P(b), P(os_), s)),
                    ("tise_stem_conv3x3s2_split_u8", lambda n, h: (P(xs), P(b), n, h, 4, P(b), P(b), P(os_), s))):
        assert status(name, *a(0, 4)) == OK, name
        assert status(name, *a(1, 2)) == INV, name                                # a map smaller than the window
    torch.cuda.synchronize()
    assert bool((o == float(SENT32)).all()) and bool((os_ == float(SENT16)).all())
