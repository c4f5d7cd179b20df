"""GPU: tise_paired_cosine (csrc/clip_ops.hip; device.paired_cosine) against the cosine of the same rows in extended precision.

THE BOUND.  The kernel forms three sums of d exact products in fp64 (a product of two fp16 or two fp32 values is exact in fp64):
a lane adds at most ceil(d / 64) terms in turn and six butterfly levels follow, so each sum carries at most ceil(d / 64) + 6
roundings on its way, far fewer than the d of a sequential sum the issue's `(d + 16) 2^-53` allows for; the product aa * bb, the
square root and the division add three (the 16 covers them and the reference's own).  A rounding of a sum is relative to a
PARTIAL sum, which a . b's cancellation can leave far above |a . b| itself, so `relative` is relative to what the sums are
made of:

    |cos^ - cos| <= (d + 16) 2^-53 * sum_k |a_k b_k| / sqrt((a . a)(b . b))

The factor is |cos| itself for rows without cancellation (an identical pair: exactly 1) and at most 1 (Cauchy-Schwarz).

Measured on an MI355X: worst error / bound 0.065 on the fp16 tables and 0.093 on the fp32 ones."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NS = (1, 63, 64, 65)
DS = (8, 512, 1000, 1024)


def _ref(a, b):
    """np.longdouble (64-bit mantissa on x86) cosine and the bound's scale, from the tables' own values."""
    a, b = a.astype(np.longdouble), b.astype(np.longdouble)
    norm = np.sqrt((a * a).sum(1) * (b * b).sum(1))
    with np.errstate(invalid="ignore", divide="ignore"):
        return ((a * b).sum(1) / norm).astype(np.float64), (np.abs(a * b).sum(1) / norm).astype(np.float64)


def _tables(n, d, dtype, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    a = torch.randn((n, d), generator=g, device=dev)
    b = 0.5 * a + torch.randn((n, d), generator=g, device=dev)            # cos about 0.45
    if n > 2:
        b[1] = torch.randn(d, generator=g, device=dev)                    # an unrelated pair: cos near 0, heavy cancellation
        b[2] = -a[2]                                                      # cos = -1
    return a.to(dtype), b.to(dtype)


@pytest.mark.parametrize("dtype", (torch.float16, torch.float32))
def test_paired_cosine_matches_extended_precision(cuda_device, dtype):
    """n in {1, 63, 64, 65} (the last workgroup's idle waves), d in {8 (most lanes idle), 512, 1000 (a ragged last pass), 1024}, fp16
    and fp32 tables: inside the bound, and two launches give the same bits."""
    from tise_toolbox_amd import device
    worst = 0.0
    for n in NS:
        for d in DS:
            a, b = _tables(n, d, dtype, 100 * n + d, cuda_device)
            got = device.paired_cosine(a, b)
            assert got.dtype == torch.float64 and got.shape == (n,)
            ref, scale = _ref(a.cpu().numpy(), b.cpu().numpy())
            err = np.abs(got.cpu().numpy() - ref)
            ratio = float((err / ((d + 16) * 2.0 ** -53 * scale)).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (n, d, dtype, ratio)
            assert torch.equal(got, device.paired_cosine(a, b)), (n, d)
            if n > 2:
                assert abs(got[2].item() + 1.0) <= (d + 16) * 2.0 ** -53, (n, d)
    print(f"{dtype}: worst error / bound {worst:.3f}")


def test_zero_rows_identical_pairs_and_refusals(cuda_device):
    """A zero row on either side gives NaN (numpy's 0 / 0) and leaves its neighbours alone; an identical pair gives 1 within the
    bound; tables of different shapes or dtypes are refused before the launch."""
    from tise_toolbox_amd import device
    for dtype in (torch.float16, torch.float32):
        for d in DS:
            a, b = _tables(5, d, dtype, 7 + d, cuda_device)
            b[0] = a[0]
            a[3] = 0
            b[4] = 0
            got = device.paired_cosine(a, b).cpu().numpy()
            assert abs(got[0] - 1.0) <= (d + 16) * 2.0 ** -53, (dtype, d, got[0])
            assert np.isnan(got[3]) and np.isnan(got[4]) and np.isfinite(got[:3]).all(), (dtype, d, got)
    a = torch.zeros((4, 8), device=cuda_device)
    with pytest.raises(ValueError):
        device.paired_cosine(a, a[:3])
    with pytest.raises(ValueError):
        device.paired_cosine(a, a.half())
    with pytest.raises(ValueError):
        device.paired_cosine(a.double(), a.double())
    assert device.paired_cosine(a[:0], a[:0]).shape == (0,)
