"""GPU: the kernels of the DINOv2 tower's fp32 residual stream (csrc/clip_ops.hip) against fp64 references computed from the same
fp16 / fp32 inputs, never from the product kernels: tise_gemm_f16_act's act = 2 on all 63 488 finite fp16 values, tise_gemm_f16_res32
at the tile edges of every kernel instance (the other three in child processes: the instance switches are read once per
process), tise_layernorm_f32 with both output types, and the token assembly, which is exact.  Bounds: tests/_dinov2_gemm_child.py
(GEMMs) and _ln32_check below."""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import _dinov2_gemm_child as dc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _assert_all(res, where):
    for r in res["res32"]:
        assert r["finite"] and r["ratio"] <= 1.0 and r["untouched"] and r["res_kept"] and r.get("repeat_equal", True), (where, r)
    assert sum("repeat_equal" in r for r in res["res32"]) >= 1
    assert res["exact"] == dict(exact=True, exact_scaled=True, m0_untouched=True), (where, res["exact"])
    g = res["gelu"]
    print(f"{where}: act=2 on {g['instance']}: worst |h - ref| / bound {g['ratio']:.3f}, observed dt {g['k_observed']:.3f} x 2^-24 (K_ACT = {dc.K_ACT})")
    assert g["finite"] and g["zeros_ok"] and g["bias_ok"] and g["nonfinite"] and g["ratio"] <= 1.0, (where, g)


@pytest.fixture(scope="module")
def default_process(cuda_device):
    return dc.run_all(cuda_device)


def test_res32_and_exact_gelu_in_this_process(default_process):
    """Every case of tests/_dinov2_gemm_child.py under the default instance rule (gemm16_f16_kernel<false> at these sizes):
    (130, 136, 64), (257, 264, 128), (1, 8, 64) with / without scale and bias, in place and out of place, a strided out32
    whose neighbouring columns stay untouched, M = 0, the largest case twice with equal bits, 4096 + 2^-8 exactly; act = 2 on
    every finite fp16 value and on +-inf / NaN."""
    assert {r["instance"] for r in default_process["res32"]} == {"gemm16_f16_kernel<false>"}
    assert [r["name"] for r in default_process["res32"]] == [c["name"] for c in dc.RES32_CASES] and len(dc.RES32_CASES) == 27
    _assert_all(default_process, "default")


# gemm_f16_big_kernel, gemm16_f16_kernel<true> (TISE_GEMM_SHAPE=16 alone selects this process's instance again, so it goes
# together with TISE_GEMM_BIG=2) and gemm_f16_kernel
_CHILD_ENVS = (({"TISE_GEMM_BIG": "2"}, "gemm_f16_big_kernel"), ({"TISE_GEMM_SHAPE": "16", "TISE_GEMM_BIG": "2"}, "gemm16_f16_kernel<true>"),
               ({"TISE_GEMM_SHAPE": "32"}, "gemm_f16_kernel"))


@pytest.mark.timeout(400)
def test_res32_and_exact_gelu_on_every_kernel_instance_in_a_child(cuda_device, default_process):
    """The same cases and bounds in fresh child processes, ONE AT A TIME, each under a time limit; no child is started after one
    fails.  So the new epilogue of every kernel body runs at a tile edge."""
    for extra, instance in _CHILD_ENVS:
        env = {k: v for k, v in os.environ.items() if k not in ("TISE_GEMM_SHAPE", "TISE_GEMM_BIG")}
        env.update(extra)
        try:
            p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_dinov2_gemm_child.py")], env=env, cwd=ROOT,
                               capture_output=True, text=True, timeout=120)
        except subprocess.TimeoutExpired as e:
            pytest.fail(f"child {extra} timed out; stderr:\n{e.stderr}")
        assert p.returncode == 0, f"child {extra} exit {p.returncode}; stderr:\n{p.stderr[-6000:]}"
        res = json.loads(p.stdout.strip().splitlines()[-1])
        assert {r["instance"] for r in res["res32"]} == {instance} and res["gelu"]["instance"] == instance
        _assert_all(res, str(extra))


def test_exact_gelu_at_the_big_kernel_threshold(cuda_device):
    """6141 x 8184 x 64 with bias and act = 2: 768 tiles of 256 x 256, the threshold of the default instance rule, which an
    act = 2 launch does not follow (it stays on the 128 x 128 kernel); random operands against fp64, equal bits twice."""
    r = dc.run_gelu_dispatch_edge(cuda_device)
    assert r["instance"] == "gemm16_f16_kernel<false>" and dc.instance_for(6141, 8184, {}, act=1) == "gemm_f16_big_kernel"
    assert r["finite"] and r["repeat_equal"] and r["spread"] > 8 and r["ratio"] <= 1.0, r


def test_res32_refuses_what_it_cannot_run(cuda_device):
    """Real device pointers, one defect each: TISE_ERR_INVALID_ARG, and the output keeps its bits."""
    from tise_toolbox_amd import _lib, clip_hip
    lib = _lib.load()
    m, n, k = 4, 16, 64
    a = torch.zeros((m, k), dtype=torch.float16, device=cuda_device)
    w = torch.zeros((n, k), dtype=torch.float16, device=cuda_device)
    r = torch.full((m, n + 4), dc.SENTINEL, dtype=torch.float32, device=cuda_device)
    st = clip_hip._stream()
    call = lambda res, ldr, out, ldo, nn=n, kk=k: lib.tise_gemm_f16_res32(a.data_ptr(), k, w.data_ptr(), k, None, None, res, ldr, out, ldo, m, nn, kk, st)
    bad = _lib.TISE_ERR_INVALID_ARG
    assert call(r.data_ptr() + 4, n + 4, r.data_ptr(), n + 4) == bad          # misaligned res32
    assert call(r.data_ptr(), n + 4, r.data_ptr() + 8, n + 4) == bad          # misaligned out32
    assert call(r.data_ptr(), n - 4, r.data_ptr(), n + 4) == bad              # stride < n
    assert call(r.data_ptr(), n + 4, r.data_ptr(), n + 4, nn=12) == bad       # n % 8
    assert call(r.data_ptr(), n + 4, r.data_ptr(), n + 4, kk=32) == bad       # k % 64
    assert lib.tise_gemm_f16_act(a.data_ptr(), k, w.data_ptr(), k, None, None, 0, a.data_ptr(), k, m, n, k, 3, st) == bad   # act = 3
    assert lib.tise_gemm_f16(a.data_ptr(), k, w.data_ptr(), k, None, None, 0, a.data_ptr(), k, m, n, k, 2, st) == bad       # the CLIP entry: act 0, 1
    torch.cuda.synchronize()
    assert (r == dc.SENTINEL).all()


# ---------------------------------------------------------------------------------------------------------------------
def _ln32_check(x, gamma, beta, eps, got):
    """tests/test_gpu_clip_kernels.py::_ln_check for tise_layernorm_f32.  The input is fp32 itself, the statistics have the same
    shape (16 sequential adds per lane + 6 shuffle levels + the division: |e_mu| <= 23 2^-24 sum|x|/C; q = C (var + e_mu^2)(1 +
    th_q), |th_q| <= 27 2^-24; rstd = 1 / sqrt(q / C + eps): th_r <= (th_q var + e_mu^2) / (2 (var + eps)) + 2^-22), gamma and beta
    are fp32, and y^ = fl(fl(fl(d rstd) g) + b).  The statistics term is
        inner = |e_mu| rstd |g| + |d rstd g| (th_r + 4 2^-24) + 2^-24 (|y| + |b|)
    and  fp16 out: |out - y| <= (1 + 2^-8)[u16 |y| + eta16 + (1 + u16) inner];   fp32 out: |out - y| <= (1 + 2^-8) inner + 2^-149
    (the last fp32 rounding is inner's 2^-24 |y| already)."""
    C = x.shape[1]
    x64, g64, b64 = x.double(), gamma.double(), beta.double()
    ref = torch.nn.functional.layer_norm(x64, (C,), g64, b64, eps)
    mu = x64.mean(1, keepdim=True)
    var = ((x64 - mu) ** 2).mean(1, keepdim=True)
    e_mu = 23 * 2.0 ** -24 * x64.abs().mean(1, keepdim=True)
    th_r = (27 * 2.0 ** -24 * var + e_mu ** 2) / (2 * (var + eps)) + 2.0 ** -22
    rstd = 1 / torch.sqrt(var + eps)
    inner = e_mu * rstd * g64.abs() + ((x64 - mu) * rstd * g64).abs() * (th_r + 4 * 2.0 ** -24) + 2.0 ** -24 * (ref.abs() + b64.abs())
    if got.dtype == torch.float16:
        bound = (1 + 2.0 ** -8) * (dc.U16 * ref.abs() + dc.ETA16 + (1 + dc.U16) * inner)
    else:
        bound = (1 + 2.0 ** -8) * inner + 2.0 ** -149
    return ((got.double() - ref).abs() / bound).max().item()


@pytest.mark.parametrize("C", [8, 64, 384, 768, 1024])
def test_layernorm_f32_matches_fp64_per_element(cuda_device, C):
    """C = 8 (idle lanes), 64 (one lane group exactly), 384 (ViT-S: the first half partly used), 768 (ViT-B: the second half
    partly used), 1024 (both halves full); rows = 1, 4, 5 (one workgroup
    exactly, and a second one with three idle waves); fp16 and fp32 output; strided input and output with the columns beside the
    output untouched; a row with a common offset of 1000, a small-variance row (eps = 1e-6 matters), a constant row (output =
    beta exactly: the constant has 11 significant bits, so its fp32 sum over C <= 1024 columns is exact), and a row of O(1)
    entries with one at 3e4 -- the residual stream's outliers -- finite and within the bound."""
    from tise_toolbox_amd import dinov2_hip
    g = torch.Generator(device=cuda_device).manual_seed(C)
    eps = 1e-6
    rn = lambda *s: torch.randn(s, generator=g, device=cuda_device)
    gamma, beta = 1 + 0.2 * rn(C), 0.3 * rn(C)
    for rows in (1, 4, 5):
        x = rn(rows, C) * 2 + 0.5
        x[0] = 1 + 0.1 * rn(C)
        x[0, (7 * rows) % C] = 3e4                                              # one outlier among O(1) entries
        if rows >= 4:
            x[1] = 1e3 + rn(C)
            x[2] = 1e-3 * rn(C)
            x[3] = 0.7001953125                                                 # constant row (fp16-exact)
        for odt in (torch.float16, torch.float32):
            pad = 8 if odt == torch.float16 else 4
            xw = torch.zeros((rows, C + 12), dtype=torch.float32, device=cuda_device)
            xw[:, 4:4 + C] = x
            ow = torch.full((rows, C + 3 * pad), dc.SENTINEL, dtype=odt, device=cuda_device)
            outs = (dinov2_hip.layernorm32(x, gamma, beta, eps, odt),
                    dinov2_hip.layernorm32(xw[:, 4:4 + C], gamma, beta, eps, odt, out=ow[:, pad:pad + C]))
            assert (ow[:, :pad] == dc.SENTINEL).all() and (ow[:, pad + C:] == dc.SENTINEL).all(), (C, rows, odt)
            assert torch.equal(outs[0], outs[1]) and outs[0].dtype == odt
            ratio = _ln32_check(x, gamma, beta, eps, outs[0])
            assert torch.isfinite(outs[0]).all() and ratio <= 1.0, (C, rows, odt, ratio)
            if rows >= 4:
                assert torch.equal(outs[0][3], beta.to(odt)), (C, odt)          # constant row: (x - mean) = 0 exactly
    lib_bad = dinov2_hip._lib.load().tise_layernorm_f32(x.data_ptr(), 1032, gamma.data_ptr(), beta.data_ptr(), x.data_ptr(), 1032, 1, 1032,
                                                        dinov2_hip.ctypes.c_float(eps), 1, None)
    assert lib_bad == dinov2_hip._lib.TISE_ERR_INVALID_ARG                      # C > 1024


def test_token_assembly_and_class_row_gather_are_exact(cuda_device):
    """tise_vit_tokens_f32 = float(fp16 patch row) + fp32 position row, and the fp32 class row + position row 0: pure movement
    plus ONE fp32 add, so torch's fp32 add of the same operands gives the same bits; tise_gather_rows_f32 moves rows.  Width 384
    and 1024, 3 images x 122 tokens and 70 x 257 (more elements than one pass of the 16 384-workgroup grid covers at 1024)."""
    from tise_toolbox_amd import _lib, clip_hip
    g = torch.Generator(device=cuda_device).manual_seed(11)
    for b, npatch, width in ((3, 121, 384), (70, 256, 1024), (1, 1, 8)):
        pe = (torch.randn((b * npatch, width), generator=g, device=cuda_device) * 3).half()
        cls = torch.randn(width, generator=g, device=cuda_device)
        pos = torch.randn((npatch + 1, width), generator=g, device=cuda_device) * 0.02
        pos[1, 0], cls[1 % width] = 1e-30, 1e4                                  # an add that underflows into the fp16 row / a large class entry
        x = torch.full((b * (npatch + 1), width), dc.SENTINEL, dtype=torch.float32, device=cuda_device)
        _lib.call("tise_vit_tokens_f32", clip_hip._p(pe), clip_hip._p(cls), clip_hip._p(pos), b, npatch, width, clip_hip._p(x), clip_hip._stream())
        want = torch.cat([cls.expand(b, 1, width), pe.float().view(b, npatch, width)], 1) + pos
        assert torch.equal(x.view(b, npatch + 1, width), want), (b, npatch, width)
        idx = torch.arange(b, device=cuda_device, dtype=torch.int64).flip(0) * (npatch + 1)
        c = torch.empty((b, width), dtype=torch.float32, device=cuda_device)
        _lib.call("tise_gather_rows_f32", clip_hip._p(x), clip_hip._p(idx), b, width, clip_hip._p(c), clip_hip._stream())
        assert torch.equal(c, want[:, 0].flip(0)), (b, npatch, width)
