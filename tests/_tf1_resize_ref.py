"""TensorFlow 1's legacy ResizeBilinear restated in numpy: the definition that csrc/resize_tf1.hip is pinned to, bit for bit.

tf.image.resize_bilinear(images, size, align_corners=False) of TensorFlow 1 (resize_bilinear_op.cc, LegacyScaler: no
half-pixel centres, no antialiasing), as the guided-diffusion evaluator's Inception graph applies it to its uint8 input cast to
float32, followed by the graph's Sub(128) and Mul(1/128).  Per axis, all in float32:

    scale = float32(in) / float32(out);  x = float32(o) * scale;  lo = floor(x);  hi = min(ceil(x), in - 1);  t = x - floor(x)

and per output value  top = tl + (tr - tl) * tx;  bot = bl + (br - bl) * tx;  v = top + (bot - top) * ty;  (v - sub) * mul.
numpy evaluates every float32 multiply and add as an operation of its own (no fused multiply-add): the CPU form of the
TensorFlow kernel.  TensorFlow itself is NOT what this is checked against (it is not a dependency of the project); its
documented 2 x 2 -> 4 x 4 example is (tests/test_tf1_resize_host.py).
"""
import numpy as np

F = np.float32


def axis_taps(in_size, out_size, clamp_lo=True):
    """-> (lo, hi, t) of the out_size outputs of one axis: int64 indices, float32 weights.  ``clamp_lo=False`` gives
    TensorFlow's own lower index, which it does not clamp (see unclamped_lo_max)."""
    scale = F(in_size) / F(out_size)
    x = np.arange(out_size, dtype=np.float32) * scale
    fl = np.floor(x)
    lo = fl.astype(np.int64)
    if clamp_lo:
        lo = np.minimum(lo, in_size - 1)
    hi = np.minimum(np.ceil(x).astype(np.int64), in_size - 1)
    return lo, hi, (x - fl).astype(np.float32)


def unclamped_lo_max(in_size, out_size):
    """The largest lower index TensorFlow would read on this axis (it is in bounds when <= in_size - 1)."""
    return int(axis_taps(in_size, out_size, clamp_lo=False)[0].max())


def resize_tf1(u8, out_hw):
    """(N,H,W,C) uint8 -> (N,oh,ow,C) float32, the resized image (no affine)."""
    u8 = np.asarray(u8)
    assert u8.dtype == np.uint8 and u8.ndim == 4
    oh, ow = out_hw
    y0, y1, ty = axis_taps(u8.shape[1], oh)
    x0, x1, tx = axis_taps(u8.shape[2], ow)
    src = u8.astype(np.float32)
    tx = tx[None, None, :, None]
    ty = ty[None, :, None, None]
    rows0, rows1 = src[:, y0], src[:, y1]
    tl, tr, bl, br = rows0[:, :, x0], rows0[:, :, x1], rows1[:, :, x0], rows1[:, :, x1]
    top = tl + (tr - tl) * tx
    bot = bl + (br - bl) * tx
    out = top + (bot - top) * ty
    assert out.dtype == np.float32
    return out


def network_input_tf1(u8, out_hw=(299, 299), sub=128.0, mul=2.0 ** -7):
    """(N,H,W,3) uint8 -> (N,oh,ow,3) float32: the resize, then (v - sub) * mul as two float32 operations."""
    return (resize_tf1(u8, out_hw) - F(sub)) * F(mul)
