"""The GEMM case list of tests/test_gpu_clip_kernels.py, its fp64 reference and bounds, and a child-process entry point.

``tise_gemm_f16`` reads ``TISE_GEMM_SHAPE`` / ``TISE_GEMM_BIG`` once per process, so the two kernel instances the
default rule never selects (``gemm_f16_kernel``, ``gemm16_f16_kernel<true>``) can only be reached from a fresh process:
``python tests/_clip_gemm_child.py`` runs every case of ``CASES`` under the environment it was started with and prints
one JSON list (one record per case: kernel instance, bound ratio, elements outside the rounding interval, digest of the
output) on stdout.  Not collected by pytest (no ``test_`` prefix); the parent test starts it, one child at a time.

Arithmetic of the kernel (csrc/clip_ops.hip, every instance): fp16 operands, exact fp16 products accumulated in fp32
on the matrix cores, ``+ bias`` in fp32, QuickGELU ``v / (1 + __expf(-1.702 v))`` in fp32, ONE rounding to fp16; with a
residual, ``fp16(float(that) + float(r))``: a second rounding.  The reference is the same statement in fp64 on the same
fp16 inputs.  Two checks per element, both derived from those rounding points (u = 2^-11, eta = 2^-25 the largest
fp16 rounding error below the normal range):

1. Rounding interval.  Pre-activation error |x^ - x| <= E = c (K + 1) 2^-24 (sum_k |a_mk||w_nk| + |b_n|), c = 2: K
   products are exact in fp32, K additions plus the bias add each round with a unit of at most 2^-23 (c = 2 allows the
   matrix core's adder to truncate instead of rounding to nearest).  The fp32 QuickGELU of x^ lies in act([x - E, x + E])
   widened by e_act |act| with e_act = 2^-20 + 2^-22 |1.702 x|: __expf's argument is rounded twice (1.702f and the
   product) and its result carries a few ulp; 1 + e, the division add a few more.  Rounding to fp32, to fp16 and the
   residual add are monotone, so the output must lie between the images of the interval's ends under exactly the
   kernel's own roundings (fp64 -> fp32 -> fp16, then fp16(fp32(h) + fp32(r))).  This pins WHERE the kernel rounds:
   adding the residual before the fp16 rounding, or a different QuickGELU constant, moves elements out.
2. Magnitude bound, the usual form: |out - ref| <= (1 + 2^-8) [u |ref| + eta + L E + e_act |v| + (u |v| + eta if res)]
   with ref = act(x) + r in fp64, v = act(x), L = 1.1 the largest |QuickGELU'| (1.0998; 1 without activation).  The
   factor 1 + 2^-8 covers the second-order products of the first-order terms (each <= 2^-10 relative).
"""
import hashlib
import json
import math
import os
import sys

U16 = 2.0 ** -11
ETA16 = 2.0 ** -25
C_ACC = 2.0
L_GELU = 1.1
X_MIN_GELU = -0.7511542554412889        # the minimum of x * sigmoid(1.702 x): 1 + t (1 - sigmoid(t)) = 0 at t = -1.27846
F_MIN_GELU = X_MIN_GELU / (1.0 + math.exp(-1.702 * X_MIN_GELU))

# name -> (M, N, K, epilogue flags, strided, inputs): bias / res / act; strided = every operand a slice of a wider tensor
_MS = (1, 127, 128, 129, 255, 257)
_NS = (8, 120, 136, 248, 264)
_KS = (192, 64, 128, 3072)                                 # 192: three K-steps, the odd tail after one double step
_EPIS = (("bias",), ("res",), ("act",), ("bias", "act"), ("bias", "res", "act"), ())


def _case_list():
    cases = []
    i = 0
    for m in _MS:
        for n in _NS:
            cases.append(dict(name=f"m{m}_n{n}_k{_KS[i % 4]}_{'+'.join(_EPIS[i % 6]) or 'plain'}{'_strided' if i % 3 == 0 else ''}",
                              m=m, n=n, k=_KS[i % 4], epi=_EPIS[i % 6], strided=i % 3 == 0, kind="randn"))
            i += 1
    for k in _KS:                                          # every K with every epilogue at one tail shape
        for j, epi in enumerate(_EPIS):
            cases.append(dict(name=f"m257_n264_k{k}_{'+'.join(epi) or 'plain'}_e{j}", m=257, n=264, k=k, epi=epi,
                              strided=j % 2 == 1, kind="randn"))
    # pre-activations at +-60: __expf(1.702 * 60) overflows fp32 (sigmoid -> 0 exactly), with and without bias
    cases.append(dict(name="pm60_act_nobias", m=129, n=136, k=64, epi=("act",), strided=False, kind="pm60"))
    cases.append(dict(name="pm60_bias_act_res", m=255, n=248, k=128, epi=("bias", "act", "res"), strided=True, kind="pm60bias"))
    # both sides of the big-kernel rule (>= 768 tiles of 256 x 256), K = 64: one K-step and no double step at all
    cases.append(dict(name="tiles767_k64", m=3300, n=15096, k=64, epi=("bias",), strided=False, kind="randn"))
    cases.append(dict(name="tiles768_k64", m=6141, n=8184, k=64, epi=("bias", "res"), strided=False, kind="randn"))
    # the big kernel with an odd K-step count and an N tail of 8 (N % 256 == 8), strided, full epilogue
    cases.append(dict(name="big_k192_ntail8", m=8193, n=5896, k=192, epi=("bias", "res", "act"), strided=True, kind="randn"))
    return cases


CASES = _case_list()
LARGEST = "big_k192_ntail8"


def instance_for(m, n, env=None):
    """The kernel instance tise_gemm_f16 launches (clip_ops.hip: the TISE_GEMM_BIG / TISE_GEMM_SHAPE rule)."""
    env = os.environ if env is None else env
    big_mode = int(env.get("TISE_GEMM_BIG", "1"))
    shape = int(env.get("TISE_GEMM_SHAPE", "0"))
    tiles_big = ((m + 255) // 256) * ((n + 255) // 256)
    big = big_mode == 2 or (big_mode == 1 and tiles_big >= 768)
    if shape == 16 or (shape == 0 and not big):
        return "gemm16_f16_kernel<true>" if big else "gemm16_f16_kernel<false>"
    return "gemm_f16_big_kernel" if big else "gemm_f16_kernel"


SENTINEL = -7.0                                            # fp16-exact marker of the columns beside a strided output


def make_inputs(case, dev):
    """fp16 inputs of a case (seeded on the device: the same in every process) and the output view to write."""
    import torch
    m, n, k, epi = case["m"], case["n"], case["k"], case["epi"]
    g = torch.Generator(device=dev).manual_seed(sum(map(ord, case["name"])) * 7919 + m * 31 + n)
    rn = lambda *s: torch.randn(s, generator=g, device=dev)
    a = (rn(m, k) * 0.7).half()
    w = (rn(n, k) * k ** -0.5).half()
    b = (rn(n) * 0.3).half() if "bias" in epi else None
    r = rn(m, n).half() if "res" in epi else None
    if case["kind"] == "pm60":                             # x = +-60 (alternating rows) + a small product
        a[:, 0] = torch.where(torch.arange(m, device=dev) % 2 == 0, 60.0, -60.0).half()
        w[:, 0] = 1.0
    elif case["kind"] == "pm60bias":                       # x = +-60 (alternating columns, from the bias) + a small product
        b = torch.where(torch.arange(n, device=dev) % 2 == 0, 60.0, -60.0).half()
    out_wide = None
    if case["strided"]:
        aw = torch.zeros((m, k + 72), dtype=torch.float16, device=dev)
        aw[:, 8:8 + k] = a
        a = aw[:, 8:8 + k]
        ww = torch.zeros((n, k + 40), dtype=torch.float16, device=dev)
        ww[:, 16:16 + k] = w
        w = ww[:, 16:16 + k]
        if r is not None:
            rw = torch.zeros((m, n + 24), dtype=torch.float16, device=dev)
            rw[:, 8:8 + n] = r
            r = rw[:, 8:8 + n]
        out_wide = torch.full((m, n + 16), SENTINEL, dtype=torch.float16, device=dev)
        out = out_wide[:, 8:8 + n]
    else:
        out = torch.empty((m, n), dtype=torch.float16, device=dev)
    return a, w, b, r, out, out_wide


def _quick_gelu(x):
    import torch
    return x * torch.sigmoid(1.702 * x)


def _h(x):
    """fp64 -> fp32 -> fp16: the kernel holds the value in fp32 before its fp16 rounding."""
    import torch
    return x.to(torch.float32).to(torch.float16)


def check(a, w, b, r, act, out):
    """(ratio, outside): the largest |out - ref| / magnitude bound and the number of elements outside the rounding
    interval (module docstring).  fp64 on the device."""
    import torch
    k = a.shape[1]
    a64, w64 = a.double(), w.double()
    x = a64 @ w64.t()
    s = a64.abs() @ w64.abs().t()
    if b is not None:
        x += b.double()
        s += b.double().abs()
    E = C_ACC * (k + 1) * 2.0 ** -24 * s
    del s
    lo, hi = x - E, x + E
    if act:
        v = _quick_gelu(x)
        flo, fhi = _quick_gelu(lo), _quick_gelu(hi)
        vmin = torch.where((lo <= X_MIN_GELU) & (hi >= X_MIN_GELU), torch.full_like(x, F_MIN_GELU),
                           torch.minimum(flo, fhi))
        vmax = torch.maximum(flo, fhi)
        e_act = 2.0 ** -20 + 2.0 ** -22 * 1.702 * torch.maximum(lo.abs(), hi.abs())
        mag = torch.maximum(vmin.abs(), vmax.abs())
        vlo, vhi = vmin - e_act * mag - 1e-38, vmax + e_act * mag + 1e-38
        dv = L_GELU * E + e_act * v.abs()
        del flo, fhi, vmin, vmax, mag, e_act
    else:
        v, vlo, vhi, dv = x, lo, hi, E
    del lo, hi
    hlo, hhi = _h(vlo), _h(vhi)
    del vlo, vhi
    if r is not None:
        rf = r.float()
        olo, ohi = (hlo.float() + rf).half(), (hhi.float() + rf).half()
        ref = v + r.double()
        bound = U16 * ref.abs() + ETA16 + dv + U16 * v.abs() + ETA16
    else:
        olo, ohi = hlo, hhi
        ref = v
        bound = U16 * ref.abs() + ETA16 + dv
    bound *= 1 + 2.0 ** -8
    outside = int(((out < olo) | (out > ohi) | ~torch.isfinite(out)).sum().item())
    ratio = float(((out.double() - ref).abs() / bound).max().item())
    return ratio, outside


def run_case(case, dev, repeat=False):
    """Launch one case through clip_hip.gemm and check it: a JSON-ready record."""
    import torch
    from tise_toolbox_amd import clip_hip
    a, w, b, r, out, out_wide = make_inputs(case, dev)
    act = 1 if "act" in case["epi"] else 0
    clip_hip.gemm(a, w, b, r, act, out=out)
    torch.cuda.synchronize(dev)
    ratio, outside = check(a, w, b, r, act, out)
    untouched = True
    if out_wide is not None:
        n = case["n"]
        untouched = bool((out_wide[:, :8] == SENTINEL).all().item() and (out_wide[:, 8 + n:] == SENTINEL).all().item())
    rec = dict(name=case["name"], instance=instance_for(case["m"], case["n"]), ratio=ratio, outside=outside,
               untouched=untouched, digest=hashlib.sha1(out.contiguous().cpu().numpy().tobytes()).hexdigest())
    if repeat:
        again = torch.empty_like(out)
        clip_hip.gemm(a, w, b, r, act, out=again)
        rec["repeat_equal"] = bool(torch.equal(again, out))
    return rec


def main():
    import torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    from tise_toolbox_amd import _lib
    assert torch.cuda.is_available(), "no HIP device"
    _lib.load()
    dev = torch.device("cuda", 0)
    recs = []
    for case in CASES:
        recs.append(run_case(case, dev))
        torch.cuda.empty_cache()
    json.dump(recs, sys.stdout)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()
