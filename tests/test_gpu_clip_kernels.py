"""GPU: every kernel of csrc/clip_ops.hip pinned to a plain fp64 statement of the arithmetic it documents ("fp16
tensors, fp32 accumulation / statistics"), per element, at every kernel instance and at the tile edges.

References are computed in float64 from the same fp16 inputs with PyTorch (never with the product kernels).  Each
bound is derived from the kernel's rounding points and written in the test's docstring; u = 2^-11 is the fp16 unit
roundoff, eta = 2^-25 the largest fp16 rounding error below the normal range.  Token assembly is pure data movement
plus one fp32 add, so it must be EXACT.  Misaligned or out-of-range calls are tested without a GPU only
(tests/test_cabi_symbols.py): nothing here launches one."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from tests import _clip_gemm_child as gc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U16, ETA16, C_ACC = gc.U16, gc.ETA16, gc.C_ACC   # c = 2: each fp32 addition rounds with a unit of at most 2^-23


# ---------------------------------------------------------------------------------------------------------------------
# GEMM: tise_gemm_f16 = fp16(act(sum_k a w + b)) [+ r, rounded again]; the case list, reference and both bounds live in
# tests/_clip_gemm_child.py (module docstring) so that a child process with another kernel selection runs the very same
# cases
_DEFAULT = {}                                   # case name -> record of this (default-selection) process


@pytest.mark.timeout(300)
@pytest.mark.parametrize("case", gc.CASES, ids=[c["name"] for c in gc.CASES])
def test_gemm_matches_fp64_per_element(cuda_device, case):
    """Per element: the output lies inside the interval the kernel's own roundings map the fp64 pre-activation +- E
    to (E = 2 (K + 1) 2^-24 (sum |a||w| + |b|)), and |out - ref| <= (1 + 2^-8)[u|ref| + eta + L E + e_act|v| + (u|v| +
    eta with a residual)] (derivation: tests/_clip_gemm_child.py).  Strided outputs leave the columns beside them
    untouched; the largest case run twice is bit-identical."""
    rec = gc.run_case(case, cuda_device, repeat=case["name"] == gc.LARGEST)
    _DEFAULT[case["name"]] = rec
    print(f"{rec['name']}: {rec['instance']} ratio {rec['ratio']:.3f} outside {rec['outside']}")
    assert rec["instance"] == gc.instance_for(case["m"], case["n"], {})
    assert rec["outside"] == 0, rec
    assert rec["ratio"] <= 1.0, rec
    assert rec["untouched"], rec
    if "repeat_equal" in rec:
        assert rec["repeat_equal"], rec


def test_gemm_m0_writes_nothing(cuda_device):
    """M = 0 returns OK and writes nothing (the output buffer keeps its sentinel).  Called through the C ABI with real
    addresses: torch reports a null data pointer for an empty tensor."""
    from tise_toolbox_amd import _lib, clip_hip
    a = torch.ones((4, 64), dtype=torch.float16, device=cuda_device)
    w = torch.ones((16, 64), dtype=torch.float16, device=cuda_device)
    out = torch.full((4, 16), gc.SENTINEL, dtype=torch.float16, device=cuda_device)
    _lib.call("tise_gemm_f16", clip_hip._p(a), 64, clip_hip._p(w), 64, None, None, 0, clip_hip._p(out), 16, 0, 16, 64, 0,
              clip_hip._stream())
    torch.cuda.synchronize()
    assert (out == gc.SENTINEL).all()


_CHILD_ENVS = ({"TISE_GEMM_SHAPE": "32"}, {"TISE_GEMM_SHAPE": "16"}, {"TISE_GEMM_BIG": "0"}, {"TISE_GEMM_BIG": "2"})


@pytest.mark.timeout(1000)
def test_gemm_every_kernel_instance_in_a_child(cuda_device):
    """The selection switches are read once per process, so the instances the default rule never takes run in child
    processes (tests/_clip_gemm_child.py), ONE AT A TIME, each under a time limit, the same cases and bounds.  No child
    is started after one fails.  Where a child selects the same instance as this process, the outputs are bit-identical
    (the switch changes the selection, never the arithmetic).  Together: all four instances ran."""
    for case in gc.CASES:                                          # the default records (computed here if run alone)
        if case["name"] not in _DEFAULT:
            _DEFAULT[case["name"]] = gc.run_case(case, cuda_device)
            torch.cuda.empty_cache()
    torch.cuda.empty_cache()
    seen = {r["instance"] for r in _DEFAULT.values()}
    for extra in _CHILD_ENVS:
        env = {k: v for k, v in os.environ.items() if k not in ("TISE_GEMM_SHAPE", "TISE_GEMM_BIG")}
        env.update(extra)
        try:
            p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_clip_gemm_child.py")], env=env, cwd=ROOT,
                               capture_output=True, text=True, timeout=240)
        except subprocess.TimeoutExpired as e:
            pytest.fail(f"child {extra} timed out; stderr:\n{e.stderr}")
        assert p.returncode == 0, f"child {extra} exit {p.returncode}; stderr:\n{p.stderr[-6000:]}"
        recs = json.loads(p.stdout.strip().splitlines()[-1])
        assert [r["name"] for r in recs] == [c["name"] for c in gc.CASES]
        for case, r in zip(gc.CASES, recs):
            assert r["instance"] == gc.instance_for(case["m"], case["n"], extra)
            assert r["outside"] == 0 and r["ratio"] <= 1.0 and r["untouched"], (extra, r)
            d = _DEFAULT[r["name"]]
            if d["instance"] == r["instance"]:
                assert d["digest"] == r["digest"], (extra, r["name"], r["instance"])
        worst = max(recs, key=lambda r: r["ratio"])
        print(f"child {extra}: instances {sorted({r['instance'] for r in recs})}, worst ratio {worst['ratio']:.3f} ({worst['name']})")
        seen |= {r["instance"] for r in recs}
    assert seen == {"gemm16_f16_kernel<false>", "gemm16_f16_kernel<true>", "gemm_f16_kernel", "gemm_f16_big_kernel"}, seen


# ---------------------------------------------------------------------------------------------------------------------
# Attention
def _attention_ref(qkv, batch, seq, heads, causal):
    """fp64 softmax(Q K^T / 8 + mask) V and the per-element bound terms."""
    q, k, v = qkv.double().view(batch, seq, 3, heads, 64).permute(2, 0, 3, 1, 4)          # (B, H, S, 64)
    s = q @ k.transpose(-1, -2) / 8
    sabs = q.abs() @ k.abs().transpose(-1, -2) / 8
    mask = torch.ones((seq, seq), dtype=torch.bool, device=qkv.device)
    if causal:
        mask = torch.tril(mask)
    s = s.masked_fill(~mask, -math.inf)
    p = torch.softmax(s, -1)
    o = p @ v
    # score error: 64 exact products summed in fp32 (c = 2), the 1/8 is exact; the exponent's argument s - m carries the
    # error of s_j and of the maximum, plus __expf's own (2^-20 + 2^-21 |s_j - m|, as in the GEMM's QuickGELU)
    err_s = (C_ACC * 65 * 2.0 ** -24 * sabs).masked_fill(~mask, 0).amax(-1, keepdim=True)
    spread = (s.amax(-1, keepdim=True) - s.masked_fill(~mask, math.inf).amin(-1, keepdim=True))
    delta = 2 * err_s + 2.0 ** -20 + 2.0 ** -21 * spread
    pv_abs = p @ v.abs()                                                                 # sum_j p_j |v_j|
    pv_dev = (p.unsqueeze(-1) * (v.unsqueeze(-3) - o.unsqueeze(-2)).abs()).sum(-2)      # sum_j p_j |v_j - o|
    vsum = mask.double() @ v.abs()                                                      # sum over unmasked j of |v_j|
    nkeys = 32 * ((seq + 31) // 32)
    theta_c = (seq + 4) * 2.0 ** -24                            # the fp32 sum of the p's, its reciprocal, the product
    inner = (U16 * pv_abs + ETA16 * vsum + C_ACC * nkeys * 2.0 ** -24 * pv_abs + theta_c * o.abs()
             + torch.expm1(2 * delta) * pv_dev)
    bound = (1 + 2.0 ** -8) * (U16 * o.abs() + ETA16 + (1 + U16) * inner)
    heads_last = lambda t: t.transpose(1, 2).reshape(batch * seq, heads * 64)
    return heads_last(o), heads_last(bound), p


def _qkv(batch, seq, heads, kind, g, dev):
    e = heads * 64
    x = torch.randn((batch, seq, 3, heads, 64), generator=g, device=dev)
    if kind == "peaked":                        # scores ~ N(0, 13^2): up to about +-40, one key takes > 0.999 mostly
        x[:, :, :2] *= 3.6
    elif kind == "uniform":                     # identical keys: every unmasked key has exactly the same score
        x[:, :, 1] = x[:, :1, 1]
    elif kind == "offset":                      # V = 1000 + N(0, 1): a large common offset
        x[:, :, 2] += 1000.0
    return x.reshape(batch * seq, 3 * e).half()


_SEQS = (1, 2, 31, 32, 33, 50, 63, 64, 65, 77, 95, 96)
_HEADS = (1, 8, 12)
_BATCHES = (3, 1, 2, 5, 7)
_ATT = [(seq, causal, _HEADS[i % 3], _BATCHES[i % 5], "randn") for i, (seq, causal) in
        enumerate((s, c) for s in _SEQS for c in (0, 1))]
_ATT += [(seq, causal, heads, batch, kind) for kind in ("peaked", "uniform", "offset")
         for (seq, causal, heads, batch) in ((32, 1, 8, 3), (33, 0, 12, 1), (77, 1, 8, 5), (96, 0, 1, 6), (2, 1, 12, 2))]


@pytest.mark.timeout(120)
def test_attention_matches_fp64_per_element(cuda_device):
    """seq 1..96 across the NT = 1 / 2 / 3 instances and their tile edges, causal or not, heads 1 / 8 / 12 with batch *
    heads both multiple and not of 4 (the last workgroup's idle waves), plus a peaked softmax (scores to ~ +-40), an
    exactly uniform one, and V with a common offset of 1000.  Per element, against fp64 softmax(QK^T/8 + mask) V:
        |o^ - o| <= (1 + 2^-8)[u|o| + eta + (1 + u)(u S_p + eta sum_j|v_j| + 2 Sp 2^-24 S_p + theta |o|
                                                      + (exp(2 D) - 1) sum_j p_j |v_j - o|)]
    S_p = sum_j p_j |v_j| (P rounded to fp16: u per term, eta below the normal range; the fp32 PV accumulation over the
    32 NT padded keys: 2 * 32 NT * 2^-24), theta = (seq + 4) 2^-24 (the fp32 sum, reciprocal and product common to the
    row), D = 2 max_j |s^_j - s_j| + 2^-20 + 2^-21 (max - min score) (64 exact products in fp32, c = 2; __expf), the
    factor 2 of D: a perturbation moves both p_j and the normalisation.  Row 0 of a causal sequence sees itself only:
    its output is V row 0 exactly."""
    from tise_toolbox_amd import clip_hip
    g = torch.Generator(device=cuda_device).manual_seed(11)
    peaked_rows = 0
    for seq, causal, heads, batch, kind in _ATT:
        qkv = _qkv(batch, seq, heads, kind, g, cuda_device)
        got = clip_hip.attention(qkv, batch, seq, heads, bool(causal))
        ref, bound, p = _attention_ref(qkv, batch, seq, heads, bool(causal))
        err = (got.double() - ref).abs()
        ratio = (err / bound).max().item()
        assert torch.isfinite(got).all() and ratio <= 1.0, (seq, causal, heads, batch, kind, ratio)
        if causal:
            e = heads * 64
            v0 = qkv.view(batch, seq, 3 * e)[:, 0, 2 * e:]
            assert torch.equal(got.view(batch, seq, e)[:, 0], v0), (seq, heads, batch, kind)
        if kind == "peaked":
            peaked_rows += int((p.amax(-1) > 0.999).sum().item())
    assert peaked_rows >= 100                                        # the peaked cases did peak


def test_attention_refuses_what_it_cannot_run(cuda_device):
    """seq = 97 and head_dim != 64: TISE_ERR_INVALID_ARG (checked before any launch)."""
    from tise_toolbox_amd import _lib, clip_hip
    lib = _lib.load()
    qkv = torch.zeros((2 * 97, 3 * 128), dtype=torch.float16, device=cuda_device)
    out = torch.zeros((2 * 97, 128), dtype=torch.float16, device=cuda_device)
    st = clip_hip._stream()
    assert lib.tise_attention_f16(qkv.data_ptr(), 2, 97, 2, 64, 0, out.data_ptr(), st) == _lib.TISE_ERR_INVALID_ARG
    assert lib.tise_attention_f16(qkv.data_ptr(), 2, 96, 4, 32, 0, out.data_ptr(), st) == _lib.TISE_ERR_INVALID_ARG
    assert lib.tise_attention_f16(qkv.data_ptr(), 2, 96, 1, 128, 0, out.data_ptr(), st) == _lib.TISE_ERR_INVALID_ARG


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm
def _ln_check(x, gamma, beta, eps, got):
    """fp64 layer_norm of the fp16 input and the bound:  mean: 16 sequential adds per lane + 6 shuffle levels + the
    division, |e_mu| <= 23 2^-24 sum|x|/C;  q = sum (x - mean)^2 = C (var + e_mu^2) (1 + th_q), |th_q| <= 27 2^-24 (the
    linear term vanishes: sum (x - mu) = 0);  rstd relative error th_r <= (th_q var + e_mu^2) / (2 (var + eps)) + 2^-22
    (+ eps rounding, rsqrt);  y^ = fl(fl(fl(d rstd) g) + b):
        |out - y| <= (1 + 2^-8)[u|y| + eta + (1 + u)(|e_mu| rstd |g| + |d rstd g| (th_r + 4 2^-24) + 2^-24 (|y| + |b|))]
    with d = x - mean, all in fp64."""
    C = x.shape[1]
    x64, g64, b64 = x.double(), gamma.double(), beta.double()
    ref = torch.nn.functional.layer_norm(x64, (C,), g64, b64, eps)
    mu = x64.mean(1, keepdim=True)
    var = ((x64 - mu) ** 2).mean(1, keepdim=True)
    e_mu = 23 * 2.0 ** -24 * x64.abs().mean(1, keepdim=True)
    th_r = (27 * 2.0 ** -24 * var + e_mu ** 2) / (2 * (var + eps)) + 2.0 ** -22
    rstd = 1 / torch.sqrt(var + eps)
    inner = e_mu * rstd * g64.abs() + ((x64 - mu) * rstd * g64).abs() * (th_r + 4 * 2.0 ** -24) + 2.0 ** -24 * (ref.abs() + b64.abs())
    bound = (1 + 2.0 ** -8) * (U16 * ref.abs() + ETA16 + (1 + U16) * inner)
    return ((got.double() - ref).abs() / bound).max().item(), ref


@pytest.mark.timeout(120)
def test_layernorm_matches_fp64_per_element(cuda_device):
    """C in {8, 64, 504, 512, 520, 768, 1016, 1024} (idle lanes, C not a multiple of 64, the second 512-column half
    partly used), rows = 1, 2, 3 (mod 4), strided input and output (ld > C, the columns beside the output untouched),
    rows with a common offset of 1000, a small-variance row (eps matters), a constant row (output = beta exactly),
    one channel at 3e4.  Bound: _ln_check."""
    from tise_toolbox_amd import clip_hip
    g = torch.Generator(device=cuda_device).manual_seed(5)
    eps = 1e-5
    for i, C in enumerate((8, 64, 504, 512, 520, 768, 1016, 1024)):
        rows = 4 * (5 + 3 * i) + 1 + i % 3
        x = torch.randn((rows, C), generator=g, device=cuda_device) * 2 + 0.5
        x[1] = 1e3 + torch.randn(C, generator=g, device=cuda_device)          # common offset 1e3, std 1
        x[2] = 3e-3 * torch.randn(C, generator=g, device=cuda_device)          # var ~ 1e-5 ~ eps
        x[3] = 0.7                                                              # constant row
        x[4] = 1 + 0.1 * torch.randn(C, generator=g, device=cuda_device)
        x[4, (7 * i) % C] = 3e4                                                 # one outlier channel
        x = x.half()
        gamma = (1 + 0.2 * torch.randn(C, generator=g, device=cuda_device)).half()
        beta = (0.3 * torch.randn(C, generator=g, device=cuda_device)).half()
        for strided in (False, True):
            if strided:
                xw = torch.zeros((rows, C + 16), dtype=torch.float16, device=cuda_device)
                xw[:, :C] = x
                xin = xw[:, :C]
                ow = torch.full((rows, C + 24), gc.SENTINEL, dtype=torch.float16, device=cuda_device)
                out = ow[:, 8:8 + C]
                clip_hip.layernorm(xin, gamma, beta, eps, out=out)
                assert (ow[:, :8] == gc.SENTINEL).all() and (ow[:, 8 + C:] == gc.SENTINEL).all(), C
            else:
                out = clip_hip.layernorm(x, gamma, beta, eps)
            ratio, _ = _ln_check(x, gamma, beta, eps, out)
            assert torch.isfinite(out).all() and ratio <= 1.0, (C, rows, strided, ratio)
            assert torch.equal(out[3], beta), C                                 # constant row: (x - mean) = 0 exactly


# ---------------------------------------------------------------------------------------------------------------------
# Token assembly: exact
@pytest.mark.timeout(120)
def test_patchify_is_exact(cuda_device):
    """Patch matrix [B G^2][3 P^2], columns (c, ky, kx) = conv1.weight.flatten(1), against unfold; batch 230 at 224 / 32
    passes the 16 384-workgroup grid cap (the grid-stride loop's second pass)."""
    from tise_toolbox_amd import _lib, clip_hip
    g = torch.Generator(device=cuda_device).manual_seed(2)
    for res, patch in ((224, 32), (64, 16), (48, 8)):
        for b in (1, 3, 230):
            img = torch.randn((b, 3, res, res), generator=g, device=cuda_device).half()
            gr = res // patch
            out = torch.empty((b * gr * gr, 3 * patch * patch), dtype=torch.float16, device=cuda_device)
            _lib.call("tise_patchify_f16", clip_hip._p(img), b, res, patch, clip_hip._p(out), clip_hip._stream())
            want = img.unfold(2, patch, patch).unfold(3, patch, patch).permute(0, 2, 3, 1, 4, 5).reshape(b * gr * gr, -1)
            assert torch.equal(out, want), (res, patch, b)


@pytest.mark.timeout(120)
def test_vit_tokens_are_exact(cuda_device):
    """x[b][0] = cls + pos[0], x[b][1 + p] = patch_out[b NP + p] + pos[1 + p]: fp32 add, one fp16 rounding -- equal to
    (cat(cls, patch_out).float() + pos.float()).half(); batch 120 x 50 tokens x 768 passes the grid cap."""
    from tise_toolbox_amd import _lib, clip_hip
    g = torch.Generator(device=cuda_device).manual_seed(3)
    W = 768
    for npch in (49, 4):
        for b in (1, 7, 120):
            pe = torch.randn((b * npch, W), generator=g, device=cuda_device).half()
            cls = torch.randn(W, generator=g, device=cuda_device).half()
            pos = torch.randn((npch + 1, W), generator=g, device=cuda_device).half()
            x = torch.empty((b * (npch + 1), W), dtype=torch.float16, device=cuda_device)
            _lib.call("tise_vit_tokens_f16", clip_hip._p(pe), clip_hip._p(cls), clip_hip._p(pos), b, npch, W, clip_hip._p(x),
                      clip_hip._stream())
            seqs = torch.cat([cls.expand(b, 1, W), pe.view(b, npch, W)], 1)
            want = (seqs.float() + pos.float()).half().view(b * (npch + 1), W)
            assert torch.equal(x, want), (npch, b)


@pytest.mark.timeout(120)
def test_text_tokens_are_exact(cuda_device):
    """x[r] = table[tok[r]] + pos[r % seq] in fp32, one fp16 rounding; ids up to 49 407; 120 x 77 rows x 512 passes the
    grid cap."""
    from tise_toolbox_amd import _lib, clip_hip
    g = torch.Generator(device=cuda_device).manual_seed(4)
    W, V = 512, 49408
    table = torch.randn((V, W), generator=g, device=cuda_device).half()
    pos = torch.randn((77, W), generator=g, device=cuda_device).half()
    for seq, b in ((1, 5), (17, 9), (77, 120)):
        tok = torch.randint(0, V, (b, seq), generator=g, device=cuda_device, dtype=torch.int32)
        tok[0, -1] = V - 1
        tok[-1, 0] = 0
        x = torch.empty((b * seq, W), dtype=torch.float16, device=cuda_device)
        _lib.call("tise_text_tokens_f16", clip_hip._p(tok), clip_hip._p(table), clip_hip._p(pos), b * seq, seq, W, clip_hip._p(x),
                  clip_hip._stream())
        want = (table[tok.long()].float() + pos[:seq].float()).half().view(b * seq, W)
        assert torch.equal(x, want), (seq, b)


@pytest.mark.timeout(60)
def test_gather_rows_is_exact(cuda_device):
    """out[i] = x[index[i]]: duplicates, the first and the last row, a descending run; a launch past the grid cap."""
    from tise_toolbox_amd import _lib, clip_hip
    g = torch.Generator(device=cuda_device).manual_seed(6)
    for rows, W, n in ((50, 768, 64), (9240, 512, 9000)):
        x = torch.randn((rows, W), generator=g, device=cuda_device).half()
        idx = torch.randint(0, rows, (n,), generator=g, device=cuda_device)
        idx[:4] = torch.tensor([0, rows - 1, 0, rows - 1])
        idx[4:20] = torch.arange(rows - 1, rows - 17, -1)
        out = torch.empty((n, W), dtype=torch.float16, device=cuda_device)
        _lib.call("tise_gather_rows_f16", clip_hip._p(x), clip_hip._p(idx), n, W, clip_hip._p(out), clip_hip._stream())
        assert torch.equal(out, x[idx]), (rows, W, n)
