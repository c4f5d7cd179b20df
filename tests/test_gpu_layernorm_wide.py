"""GPU: tise_layernorm_wide_f16 (csrc/clip_ops.hip: layernorm_kernel with four 16-byte groups per lane, rows of up to 2048
columns; open_clip ViT-H/14 is 1280 wide) against fp64 layer_norm of the same fp16 input.

THE BOUND is tests/test_gpu_clip_kernels.py::_ln_check's, restated for up to 32 sequential adds per lane instead of 16 (the two
fp32 sums run over 4 x 8 values per lane before the six shuffle levels):
    mean:  32 adds + 6 levels + the division,  |e_mu| <= 39 2^-24 sum|x| / C              (was 23)
    q = sum (x - mean)^2 = C (var + e_mu^2)(1 + th_q),  |th_q| <= 43 2^-24                 (was 27: + 16 adds)
    rstd relative error th_r <= (th_q var + e_mu^2) / (2 (var + eps)) + 2^-22
    |out - y| <= (1 + 2^-8)[u|y| + eta + (1 + u)(|e_mu| rstd |g| + |d rstd g| (th_r + 4 2^-24) + 2^-24 (|y| + |b|))]

Measured on an MI355X: worst error / bound 0.992 (C 1280, 3 rows; the fp16 rounding of the output is nearly all of it), 0.945 at
C 8 and 0.988 at C 2048."""
import ctypes

import pytest
import torch

from tests.test_gpu_clip_kernels import ETA16, U16

pytestmark = pytest.mark.gpu

WIDTHS = (8, 1024, 1032, 1280, 2048)
ROWS = (1, 3, 4, 5, 257)
SENTINEL = 1234.0
EPS = 1e-5


def _ln_check_wide(x, gamma, beta, eps, got):
    C = x.shape[1]
    x64, g64, b64 = x.double(), gamma.double(), beta.double()
    ref = torch.nn.functional.layer_norm(x64, (C,), g64, b64, eps)
    mu = x64.mean(1, keepdim=True)
    var = ((x64 - mu) ** 2).mean(1, keepdim=True)
    e_mu = 39 * 2.0 ** -24 * x64.abs().mean(1, keepdim=True)
    th_r = (43 * 2.0 ** -24 * var + e_mu ** 2) / (2 * (var + eps)) + 2.0 ** -22
    rstd = 1 / torch.sqrt(var + eps)
    inner = e_mu * rstd * g64.abs() + ((x64 - mu) * rstd * g64).abs() * (th_r + 4 * 2.0 ** -24) + 2.0 ** -24 * (ref.abs() + b64.abs())
    bound = (1 + 2.0 ** -8) * (U16 * ref.abs() + ETA16 + (1 + U16) * inner)
    return ((got.double() - ref).abs() / bound).max().item()


def _wide(x, gamma, beta, out, eps=EPS):
    from tise_toolbox_amd import _lib, clip_hip
    return _lib.load().tise_layernorm_wide_f16(x.data_ptr(), x.stride(0), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(),
                                               out.stride(0), x.shape[0], x.shape[1], ctypes.c_float(eps), clip_hip._stream())


@pytest.mark.parametrize("C", WIDTHS)
def test_layernorm_wide_matches_fp64_per_element(cuda_device, C):
    """C in {8 (one lane), 1024 (two full groups, two idle), 1032 (the first column of the third group), 1280 (ViT-H/14), 2048 (all
    four)}, rows 1 / 3 / 4 / 5 / 257 (the last workgroup's idle waves), ldx and ldo > C with the columns beside the output
    untouched; a constant row (output = beta exactly) and a row with one value of 6e4 among small ones."""
    from tise_toolbox_amd import _lib, clip_hip
    g = torch.Generator(device=cuda_device).manual_seed(1000 + C)
    gamma = (1 + 0.2 * torch.randn(C, generator=g, device=cuda_device)).half()
    beta = (0.3 * torch.randn(C, generator=g, device=cuda_device)).half()
    worst = 0.0
    for rows in ROWS:
        x = torch.randn((rows, C), generator=g, device=cuda_device) * 2 + 0.5
        x[0] = 0.7                                                          # constant row
        if rows > 1:
            x[1] = 1 + 0.1 * torch.randn(C, generator=g, device=cuda_device)
            x[1, (7 * rows) % C] = 6e4                                      # one outlier channel, near the top of fp16
        xw = torch.zeros((rows, C + 16), dtype=torch.float16, device=cuda_device)
        xw[:, :C] = x.half()
        xin = xw[:, :C]
        ow = torch.full((rows, C + 24), SENTINEL, dtype=torch.float16, device=cuda_device)
        out = ow[:, 8:8 + C]
        assert _wide(xin, gamma, beta, out) == _lib.TISE_OK
        torch.cuda.synchronize()
        assert (ow[:, :8] == SENTINEL).all() and (ow[:, 8 + C:] == SENTINEL).all(), (C, rows)
        ratio = _ln_check_wide(xin, gamma, beta, EPS, out)
        worst = max(worst, ratio)
        print(f"C {C} rows {rows}: ratio {ratio:.3f}")
        assert torch.isfinite(out).all() and ratio <= 1.0, (C, rows, ratio)
        assert torch.equal(out[0], beta), (C, rows)                         # constant row: (x - mean) = 0 exactly
        if C <= 1024:                                                       # groups beyond C add +0: the two-group kernel's bits
            assert torch.equal(out, clip_hip.layernorm(xin.contiguous(), gamma, beta, EPS)), (C, rows)
        again = torch.empty_like(out)
        assert _wide(xin, gamma, beta, again) == _lib.TISE_OK and torch.equal(again, out), (C, rows)
    print(f"C {C}: worst ratio {worst:.3f}")


def test_layernorm_wide_refusals_on_the_device(cuda_device):
    """C = 2056 (beyond four groups), C = 12 (not a multiple of 8) and a pointer 8 bytes off: TISE_ERR_INVALID_ARG, nothing written;
    tise_layernorm_f16 still refuses 1032."""
    from tise_toolbox_amd import _lib, clip_hip
    lib = _lib.load()
    bad = _lib.TISE_ERR_INVALID_ARG
    x = torch.zeros((2, 2064), dtype=torch.float16, device=cuda_device)
    gamma = torch.ones(2064, dtype=torch.float16, device=cuda_device)
    beta = torch.zeros(2064, dtype=torch.float16, device=cuda_device)
    out = torch.full((2, 2064), SENTINEL, dtype=torch.float16, device=cuda_device)
    st = clip_hip._stream()
    eps = ctypes.c_float(EPS)
    call = lambda fn, xp, c: fn(xp, 2064, gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), 2064, 2, c, eps, st)
    assert call(lib.tise_layernorm_wide_f16, x.data_ptr(), 2056) == bad
    assert call(lib.tise_layernorm_wide_f16, x.data_ptr(), 12) == bad
    assert call(lib.tise_layernorm_wide_f16, x.data_ptr() + 8, 1280) == bad
    assert call(lib.tise_layernorm_f16, x.data_ptr(), 1032) == bad
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    assert call(lib.tise_layernorm_wide_f16, x.data_ptr(), 1032) == _lib.TISE_OK
    torch.cuda.synchronize()
    assert (out[:, :1032] == 0).all() and (out[:, 1032:] == SENTINEL).all()  # a constant row gives beta = 0
