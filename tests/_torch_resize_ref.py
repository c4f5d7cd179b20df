"""numpy restatement of torch's float32 bilinear interpolation, the resize of pytorch-fid -- test infrastructure.

``F.interpolate(x, size=(oh, ow), mode="bilinear", align_corners=False)`` (no antialiasing) on ``x = byte / 255`` as the CPU
build of torch computes it (aten/src/ATen/native/cpu/UpSampleKernel.cpp), restated operation by operation.  Per axis, all in
float32:

    scale = float32(in) / float32(out)
    s     = max(fma(scale, float32(o) + 0.5, -0.5), 0)          the source index is a FUSED multiply-add
    i0    = min(int(s), in - 1);  i1 = min(i0 + 1, in - 1);  l1 = s - float32(i0);  l0 = 1 - l1

and per output value, with a, b the upper and c, d the lower pair of source values p = float32(byte) / float32(255):

    top = fma(wx0, a, wx1 * b);  bot = fma(wx0, c, wx1 * d);  v = fma(hy0, top, hy1 * bot)

In each line the second product is a float32 multiply of its own and the first is fused into the add.  pytorch-fid's wrapper
then maps ``2 * v - 1``.  numpy has no fused multiply-add: ``fma`` below forms the exact product in float64 (24 + 24 bits fit
in 53), adds in float64, and repairs that add to round-to-odd from its exact error before the single rounding to float32
(53 >= 2 * 24 + 2 bits, so the two roundings equal one); tests/test_torch_resize_host.py holds it to libm's ``fmaf`` and the
whole file to the installed torch, bit for bit.  csrc/resize_torch.hip is pinned to this file."""
import numpy as np

F = np.float32


def fma(a, b, c):
    """float32 fused multiply-add, elementwise: round32(a * b + c) with ONE rounding."""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    a, b, c = np.broadcast_arrays(a, b, c)
    prod = a * b                                          # exact: two 24-bit significands
    t = prod + c
    bb = t - prod                                         # two-sum (Knuth): err is the exact error of the float64 add
    err = (prod - (t - bb)) + (c - bb)
    u = np.ascontiguousarray(t).view(np.int64).copy()
    fix = (err != 0.0) & ((u & 1) == 0)                   # inexact and even: step to the odd neighbour on the error's side
    away = (err > 0.0) == (t > 0.0)                       # the exact sum is larger in magnitude than t
    u[fix] += np.where(away, 1, -1)[fix]
    return u.view(np.float64).astype(np.float32)


def axis_taps(in_size, out_size):
    """-> (i0, i1, l0, l1) of the out_size outputs of one axis: int64 indices, float32 weights."""
    scale = F(in_size) / F(out_size)
    o = np.arange(out_size, dtype=np.float32) + F(0.5)
    s = np.maximum(fma(scale, o, F(-0.5)), F(0.0))
    i0 = np.minimum(s.astype(np.int64), in_size - 1)
    i1 = np.minimum(i0 + 1, in_size - 1)
    l1 = (s - i0.astype(np.float32)).astype(np.float32)
    l0 = (F(1.0) - l1).astype(np.float32)
    return i0, i1, l0, l1


def unit(u8):
    """ToTensor: float32(byte) / float32(255), a true float32 division."""
    return (np.asarray(u8).astype(np.float32) / F(255.0)).astype(np.float32)


def interpolate(x, out_hw):
    """(N,H,W,C) float32 -> (N,oh,ow,C) float32: torch's bilinear interpolation of every channel."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 4
    oh, ow = out_hw
    y0, y1, hy0, hy1 = axis_taps(x.shape[1], oh)
    x0, x1, wx0, wx1 = axis_taps(x.shape[2], ow)
    wx0, wx1 = wx0[None, None, :, None], wx1[None, None, :, None]
    hy0, hy1 = hy0[None, :, None, None], hy1[None, :, None, None]
    r0, r1 = x[:, y0], x[:, y1]
    top = fma(wx0, r0[:, :, x0], wx1 * r0[:, :, x1])
    bot = fma(wx0, r1[:, :, x0], wx1 * r1[:, :, x1])
    out = fma(hy0, top, hy1 * bot)
    assert out.dtype == np.float32
    return out


def interpolate_channels_last_kernel(x, out_hw):
    """torch's OTHER CPU kernel (UpSampleKernel.cpp cpu_upsample_linear_channels_last), which csrc/resize_torch.hip does NOT
    implement: the same indices and lambdas, but one weight per tap, w00 = hy0 * wx0, w01 = hy0 * wx1, w10 = hy1 * wx0,
    w11 = hy1 * wx1, and  out = fma(w11, d, fma(w10, c, fma(w00, a, w01 * b))).  Observed on torch 2.10.0 (CPU): a 3-channel
    input goes through it, whatever its memory format, when torch runs on ONE thread, and when oh + ow <= 128; every other
    call (pytorch-fid's 299 x 299 with more than one thread) goes through the kernel ``interpolate`` restates.  It is here so
    that the host test can say what torch computes at the small outputs, and how far the two kernels are apart."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 4
    oh, ow = out_hw
    y0, y1, hy0, hy1 = axis_taps(x.shape[1], oh)
    x0, x1, wx0, wx1 = axis_taps(x.shape[2], ow)
    wx0, wx1 = wx0[None, None, :, None], wx1[None, None, :, None]
    hy0, hy1 = hy0[None, :, None, None], hy1[None, :, None, None]
    r0, r1 = x[:, y0], x[:, y1]
    a, b, c, d = r0[:, :, x0], r0[:, :, x1], r1[:, :, x0], r1[:, :, x1]
    return fma(hy1 * wx1, d, fma(hy1 * wx0, c, fma(hy0 * wx0, a, (hy0 * wx1) * b)))


def resize_torch(u8, out_hw):
    """(N,H,W,C) uint8 -> (N,oh,ow,C) float32 in [0, 1]: ToTensor, then the interpolation (no affine)."""
    u8 = np.asarray(u8)
    assert u8.dtype == np.uint8 and u8.ndim == 4
    return interpolate(unit(u8), out_hw)


def network_input_torch(u8, out_hw=(299, 299), mul=2.0, sub=1.0):
    """(N,H,W,3) uint8 -> (N,oh,ow,3) float32: the resize, then v * mul - sub as two float32 operations."""
    return (resize_torch(u8, out_hw) * F(mul) - F(sub)).astype(np.float32)


def torch_interpolate(x_nhwc, out_hw, channels_last=False):
    """The same through torch itself on the CPU: (N,H,W,C) float32 -> (N,oh,ow,C) float32."""
    import torch
    import torch.nn.functional as TF
    t = torch.from_numpy(np.ascontiguousarray(x_nhwc)).permute(0, 3, 1, 2)
    t = t.contiguous(memory_format=torch.channels_last) if channels_last else t.contiguous()
    y = TF.interpolate(t, size=tuple(out_hw), mode="bilinear", align_corners=False)
    return np.ascontiguousarray(y.permute(0, 2, 3, 1).numpy())


def content(seed, n, h, w):
    """Seeded (n, h, w, 3) uint8 test images: uniform bytes."""
    return np.random.RandomState(seed).randint(0, 256, size=(n, h, w, 3)).astype(np.uint8)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
