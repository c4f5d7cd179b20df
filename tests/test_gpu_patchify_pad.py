"""GPU: tise_patchify_pad_f16 (csrc/clip_ops.hip) is pure data movement: the leading 3 P^2 columns of every row equal
F.unfold's reordering of the same fp16 image bit for bit, the padding columns are exactly +0 whatever the buffer held (it comes
from torch.empty: here it is pre-filled with NaN), and where tise_patchify_f16 runs too the two agree."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CASES = ((28, 14, 640), (336, 14, 640), (42, 14, 704), (48, 12, 448), (64, 32, 3072), (7, 7, 192))


def _call(img, b, res, patch, kpad, out):
    from tise_toolbox_amd import _lib, clip_hip
    return _lib.load().tise_patchify_pad_f16(img.data_ptr(), b, res, patch, kpad, out.data_ptr(), clip_hip._stream())


@pytest.mark.parametrize("res,patch,kpad", CASES)
def test_patchify_pad_is_exact_and_zero_pads(cuda_device, res, patch, kpad):
    from tise_toolbox_amd import _lib, clip_hip
    g = torch.Generator(device=cuda_device).manual_seed(res + patch)
    k = 3 * patch * patch
    for b in (1, 3):
        img = torch.randn((b, 3, res, res), generator=g, device=cuda_device).half()
        rows = b * (res // patch) ** 2
        out = torch.full((rows, kpad), float("nan"), dtype=torch.float16, device=cuda_device)
        assert _call(img, b, res, patch, kpad, out) == _lib.TISE_OK
        # unfold: (b, 3 P^2, G^2) with the channel-major (c, ky, kx) order of conv1.weight.flatten(1)
        want = F.unfold(img.float(), patch, stride=patch).transpose(1, 2).reshape(rows, k).half()
        assert torch.equal(out[:, :k], want), (res, patch, b)
        pad = out[:, k:]
        assert (pad == 0).all() and not torch.signbit(pad).any(), (res, patch, b)      # exactly +0
        if patch % 8 == 0 and kpad == k:
            old = torch.empty((rows, k), dtype=torch.float16, device=cuda_device)
            _lib.call("tise_patchify_f16", clip_hip._p(img), b, res, patch, clip_hip._p(old), clip_hip._stream())
            assert torch.equal(out, old), (res, patch, b)


def test_patchify_pad_refusals(cuda_device):
    """kpad < 3 P^2, kpad % 64 != 0, res % patch != 0: TISE_ERR_INVALID_ARG and nothing written."""
    from tise_toolbox_amd import _lib
    img = torch.zeros((1, 3, 28, 28), dtype=torch.float16, device=cuda_device)
    out = torch.full((4, 640), 7.0, dtype=torch.float16, device=cuda_device)
    bad = _lib.TISE_ERR_INVALID_ARG
    assert _call(img, 1, 28, 14, 576, out) == bad                       # 576 < 588
    assert _call(img, 1, 28, 14, 600, out) == bad                       # not a multiple of 64
    assert _call(img, 1, 28, 12, 448, out) == bad                       # 28 % 12 != 0
    torch.cuda.synchronize()
    assert (out == 7.0).all()
