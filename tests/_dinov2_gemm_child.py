"""The GEMM case lists of tests/test_gpu_dinov2_kernels.py (``tise_gemm_f16_res32`` and ``tise_gemm_f16_act``'s ``act = 2``), their
fp64 references and bounds, and a child-process entry point, as tests/_clip_gemm_child.py is for the CLIP towers' epilogue.

The instance switches ``TISE_GEMM_SHAPE`` / ``TISE_GEMM_BIG`` are read once per process, so three of the four kernel bodies'
new epilogue code can only be reached from a fresh process: ``python tests/_dinov2_gemm_child.py`` runs every case under the
environment it was started with and prints one JSON list on stdout.  Not collected by pytest.

Extends the derivation of tests/_clip_gemm_child.py (u16 = 2^-11, eta16 = 2^-25, and u32 = 2^-24 the unit roundoff of fp32).
The fp32 pre-activation x^ = acc + bias differs from the fp64 x by at most E = 2 (K + 1) 2^-24 (sum_k |a_mk||w_nk| + |b_n|).

``tise_gemm_f16_res32``: out = fl(res + fl(scale * x^)) -- one fp32 multiply, one fp32 add, NO fp16 rounding anywhere:

    |out - ref| <= (1 + 2^-8) [ |scale| E + u32 |scale x| + u32 |ref| ],      ref = res + scale x in fp64

(without a scale the multiply and its term are absent: scale = 1 exactly).  At |res| ~ 1 this is ~1e-7; an fp16 rounding of the
update or of the sum would be ~5e-4 and fails every case.  One case needs more than fp16's 11 bits outright: res = 4096, update
2^-8 -> exactly 4096.00390625.

``act = 2`` (exact GELU), exhaustive: W is the 64 x 64 identity and A holds all 63 488 finite fp16 values, so x^ = x exactly
(E = 0) and the kernel computes h = fp16(fl(fl(0.5 x) t)), t = fl(1 + erff(fl(x c))), c = fp32(2^-1/2).  With dt the absolute
error of t,

    |h - ref| <= (1 + 2^-8) [ u16 |ref| + eta16 + 0.5 |x| dt + u32 |ref| ],      ref = 0.5 x (1 + erf(x / sqrt 2)) in fp64

dt = K_ACT 2^-24 collects the argument's two roundings (|z erf'(z)| <= 0.49, so <= 2^-24), the add's rounding (<= 2^-24) and
erff's own error.  No accuracy statement for erff ships with the ROCm device library (an installation holds its bitcode,
ocml.bc, and no document), so K_ACT is the second choice: the worst dt this very test observed on an
MI355X against fp64 -- max over the 63 488 inputs of (|h - ref| - u16 |ref| - eta16) / (0.5 |x| 2^-24) -- times 2.
First run: 0.482 on every kernel instance (K_ACT_OBSERVED), so K_ACT = 1.0: erff is well inside one unit of 2^-24 where it
matters.  The term matters only where 1 + erf cancels (x < -1); elsewhere the fp16 rounding dominates.
Non-finite inputs: +inf -> +inf, -inf -> -0 or 0, NaN -> NaN.
"""
import json
import os
import sys

U16 = 2.0 ** -11
ETA16 = 2.0 ** -25
U32 = 2.0 ** -24
C_ACC = 2.0
K_ACT_OBSERVED = 0.482               # the first run on an MI355X, the same on all four kernel instances (module docstring)
K_ACT = 1.0                          # 2 x K_ACT_OBSERVED, rounded up

SHAPES = ((130, 136, 64), (257, 264, 128), (1, 8, 64))
LARGEST = (257, 264, 128)
SENTINEL = -7.0


def res32_cases():
    cases = []
    for (m, n, k) in SHAPES:
        for scale in (True, False):
            for bias in (True, False):
                for inplace in (True, False):
                    cases.append(dict(name=f"m{m}_n{n}_k{k}{'_scale' if scale else ''}{'_bias' if bias else ''}{'_inplace' if inplace else ''}",
                                      m=m, n=n, k=k, scale=scale, bias=bias, inplace=inplace, strided=False))
    for (m, n, k) in SHAPES:                                # out32 a slice of a wider tensor, res32 another
        cases.append(dict(name=f"m{m}_n{n}_k{k}_scale_bias_strided", m=m, n=n, k=k, scale=True, bias=True, inplace=False, strided=True))
    return cases


RES32_CASES = res32_cases()


def instance_for(m, n, env=None, act=0):
    """tests/_clip_gemm_child.py's rule; under the default TISE_GEMM_BIG an act = 2 launch never takes a 256 x 256 kernel."""
    from tests._clip_gemm_child import instance_for as f
    env = dict(os.environ if env is None else env)
    if act == 2 and int(env.get("TISE_GEMM_BIG", "1")) == 1:
        env["TISE_GEMM_BIG"] = "0"
    return f(m, n, env)


L_GELU_ERF = 1.13                    # the largest |GELU'| (1.1289 at x = sqrt 2)


def check_act2(a, w, b, out):
    """(ratio, largest |x|) of an act = 2 launch on random operands against fp64: |h - ref| <= (1 + 2^-8)[u16 |ref| + eta16 + L E
    + 0.5 |x| K_ACT 2^-24 + u32 |ref|] with L = 1.13 the largest |GELU'| and E the accumulator bound (``b`` may be None).  A
    function of the operands: run_gelu_dispatch_edge and the tower audit (tests/_tower_audit.py) share it."""
    import torch
    k = a.shape[1]
    x = a.double() @ w.double().t()
    mag = a.double().abs() @ w.double().abs().t()
    if b is not None:
        x = x + b.double()
        mag = mag + b.double().abs()
    E = C_ACC * (k + 1) * 2.0 ** -24 * mag
    ref = 0.5 * x * (1 + torch.special.erf(x * 0.5 ** 0.5))
    bound = (1 + 2.0 ** -8) * (U16 * ref.abs() + ETA16 + L_GELU_ERF * E + 0.5 * x.abs() * K_ACT * 2.0 ** -24 + U32 * ref.abs())
    return float(((out.double() - ref).abs() / bound).max().item()), float(x.abs().max().item())


def run_gelu_dispatch_edge(dev):
    """act = 2 with bias at 6141 x 8184 x 64 = 768 tiles of 256 x 256, where the default rule sends every other launch to a
    256 x 256 kernel and this one not: random operands against fp64 within check_act2's bound."""
    import torch
    from tise_toolbox_amd import clip_hip
    m, n, k = 6141, 8184, 64
    g = torch.Generator(device=dev).manual_seed(768)
    a = (torch.randn((m, k), generator=g, device=dev) * 0.7).half()
    w = (torch.randn((n, k), generator=g, device=dev) * 0.4).half()
    b = (torch.randn(n, generator=g, device=dev) * 0.3).half()
    out = clip_hip.gemm(a, w, b, act=2)
    again = clip_hip.gemm(a, w, b, act=2)
    ratio, spread = check_act2(a, w, b, out)
    return dict(instance=instance_for(m, n, act=2), ratio=ratio,
                finite=bool(torch.isfinite(out).all().item()), repeat_equal=bool(torch.equal(out, again)),
                spread=spread)


def make_res32_inputs(case, dev):
    import torch
    m, n, k = case["m"], case["n"], case["k"]
    g = torch.Generator(device=dev).manual_seed(sum(map(ord, case["name"])) * 7919 + m * 31 + n)
    rn = lambda *s: torch.randn(s, generator=g, device=dev)
    a = (rn(m, k) * 0.7).half()
    w = (rn(n, k) * k ** -0.5).half()
    b = (rn(n) * 0.3).half() if case["bias"] else None
    s = (0.5 + torch.rand(n, generator=g, device=dev)) * torch.where(rn(n) < 0, -1.0, 1.0) if case["scale"] else None
    r = rn(m, n) * 3
    r[0, 0] = 3e4                                           # a large stream value beside O(1) updates
    out_wide = None
    if case["strided"]:
        aw = torch.zeros((m, k + 72), dtype=torch.float16, device=dev)
        aw[:, 8:8 + k] = a
        a = aw[:, 8:8 + k]
        rw = torch.zeros((m, n + 12), dtype=torch.float32, device=dev)
        rw[:, 4:4 + n] = r
        r = rw[:, 4:4 + n]
        out_wide = torch.full((m, n + 16), SENTINEL, dtype=torch.float32, device=dev)
        out = out_wide[:, 8:8 + n]
    elif case["inplace"]:
        out = None
    else:
        out = torch.empty((m, n), dtype=torch.float32, device=dev)
    return a, w, b, s, r, out, out_wide


def check_res32(a, w, b, s, r, out):
    """The largest |out - ref| / bound (module docstring); fp64 on the device."""
    import torch
    k = a.shape[1]
    a64, w64 = a.double(), w.double()
    x = a64 @ w64.t()
    mag = a64.abs() @ w64.abs().t()
    if b is not None:
        x += b.double()
        mag += b.double().abs()
    E = C_ACC * (k + 1) * 2.0 ** -24 * mag
    if s is not None:
        s64 = s.double()
        upd = s64 * x
        ref = r.double() + upd
        bound = s64.abs() * E + U32 * upd.abs() + U32 * ref.abs()
    else:
        ref = r.double() + x
        bound = E + U32 * ref.abs()
    bound = (1 + 2.0 ** -8) * bound + 2.0 ** -149
    return float(((out.double() - ref).abs() / bound).max().item())


def run_res32_case(case, dev):
    import torch
    from tise_toolbox_amd import dinov2_hip
    a, w, b, s, r, out, out_wide = make_res32_inputs(case, dev)
    r0 = r.clone()
    got = dinov2_hip.gemm_res32(a, w, b, s, r, out)
    torch.cuda.synchronize(dev)
    rec = dict(name=case["name"], instance=instance_for(case["m"], case["n"]), finite=bool(torch.isfinite(got).all().item()),
               ratio=check_res32(a, w, b, s, r0, got), untouched=True, res_kept=True)
    if case["inplace"]:
        rec["res_kept"] = got.data_ptr() == r.data_ptr()
    else:
        rec["res_kept"] = bool(torch.equal(r, r0))
    if out_wide is not None:
        n = case["n"]
        rec["untouched"] = bool((out_wide[:, :8] == SENTINEL).all().item() and (out_wide[:, 8 + n:] == SENTINEL).all().item())
    if (case["m"], case["n"], case["k"]) == LARGEST and not case["inplace"]:
        again = torch.empty_like(got)
        dinov2_hip.gemm_res32(a, w, b, s, r0, again)
        rec["repeat_equal"] = bool(torch.equal(again, got))
    return rec


def run_res32_exact(dev):
    """res = 4096, update 2^-8: exactly 4096.00390625 (13 + 8 = 21 significant bits: fp32 holds it, fp16 does not); and M = 0
    writes nothing."""
    import torch
    from tise_toolbox_amd import dinov2_hip
    m, n, k = 130, 136, 64
    a = torch.zeros((m, k), dtype=torch.float16, device=dev)
    a[:, 0] = 2.0 ** -8
    w = torch.zeros((n, k), dtype=torch.float16, device=dev)
    w[:, 0] = 1.0
    r = torch.full((m, n), 4096.0, dtype=torch.float32, device=dev)
    out = dinov2_hip.gemm_res32(a, w, None, None, r, torch.empty_like(r))
    exact = bool((out == 4096.00390625).all().item())
    two = torch.full((n,), 2.0, dtype=torch.float32, device=dev)      # with a scale of 2 and a bias of 2^-8: 4096 + 2 (2^-8 + 2^-8)
    b = torch.full((n,), 2.0 ** -8, dtype=torch.float16, device=dev)
    out2 = dinov2_hip.gemm_res32(a, w, b, two, r, torch.empty_like(r))
    exact2 = bool((out2 == 4096.015625).all().item())
    keep = torch.full((4, n), SENTINEL, dtype=torch.float32, device=dev)
    from tise_toolbox_amd import _lib, clip_hip                      # M = 0 with real pointers (an empty tensor has none)
    _lib.call("tise_gemm_f16_res32", clip_hip._p(a), k, clip_hip._p(w), k, None, None, clip_hip._p(keep), n, clip_hip._p(keep), n,
              0, n, k, clip_hip._stream())
    torch.cuda.synchronize(dev)
    return dict(exact=exact, exact_scaled=exact2, m0_untouched=bool((keep == SENTINEL).all().item()))


def all_finite_halves(dev):
    """The 63 488 finite fp16 values as a (992, 64) matrix (bit patterns 0x0000-0x7bff and 0x8000-0xfbff)."""
    import numpy as np
    import torch
    bits = np.concatenate([np.arange(0x0000, 0x7c00), np.arange(0x8000, 0xfc00)]).astype(np.uint16)
    h = torch.from_numpy(bits.view(np.float16).copy())
    assert h.numel() == 63488 and bool(torch.isfinite(h).all()) and h.unique().numel() == 63487      # +0 and -0 compare equal
    return h.reshape(992, 64).to(dev)


def run_gelu_exhaustive(dev):
    """-> dict(ratio: worst |h - ref| / bound, k_observed: the worst dt in units of 2^-24 (module docstring), nonfinite: ok?)."""
    import torch
    from tise_toolbox_amd import clip_hip
    a = all_finite_halves(dev)
    w = torch.eye(64, dtype=torch.float16, device=dev)
    out = clip_hip.gemm(a, w, act=2)
    torch.cuda.synchronize(dev)
    x = a.double()
    ref = 0.5 * x * (1 + torch.special.erf(x * 0.5 ** 0.5))
    err = (out.double() - ref).abs()
    bound = (1 + 2.0 ** -8) * (U16 * ref.abs() + ETA16 + 0.5 * x.abs() * K_ACT * 2.0 ** -24 + U32 * ref.abs())
    nz = x != 0
    k_obs = float((((err - U16 * ref.abs() - ETA16) / (0.5 * x.abs() * 2.0 ** -24))[nz]).max().item())
    zeros_ok = bool((out[~nz] == 0).all().item())
    # the same values through the bias instead of A (x^ = 0 + b): the other operand of the epilogue's add
    b = a[752].contiguous()                                           # -2.0 .. -2.12
    outb = clip_hip.gemm(torch.zeros((3, 64), dtype=torch.float16, device=dev), w, bias=b, act=2)
    bias_ok = bool(b[0] == -2 and torch.equal(outb[1], out[752]))
    # non-finite pre-activations, each alone in its row (inf * 0 of the identity makes the rest of that row NaN)
    nf = torch.zeros((4, 64), dtype=torch.float16, device=dev)
    nf[0, 5], nf[1, 9], nf[2, 3], nf[3, 7] = float("inf"), float("-inf"), float("nan"), 1.0
    o = clip_hip.gemm(nf, w, act=2).float().cpu()
    nonfinite = bool(o[0, 5] == float("inf") and o[1, 9] == 0 and o[2, 3] != o[2, 3] and torch.isfinite(o[3]).all()
                     and abs(float(o[3, 7]) - 0.8413) < 1e-3)
    return dict(instance=instance_for(992, 64), ratio=float((err / bound).max().item()), k_observed=k_obs, zeros_ok=zeros_ok,
                bias_ok=bias_ok, nonfinite=nonfinite, finite=bool(torch.isfinite(out).all().item()))


def run_all(dev):
    import torch
    recs = [run_res32_case(c, dev) for c in RES32_CASES]
    torch.cuda.empty_cache()
    return dict(res32=recs, exact=run_res32_exact(dev), gelu=run_gelu_exhaustive(dev))


def main():
    import torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    from tise_toolbox_amd import _lib
    assert torch.cuda.is_available(), "no HIP device"
    _lib.load()
    json.dump(run_all(torch.device("cuda", 0)), sys.stdout)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()
