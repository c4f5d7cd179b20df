"""GPU: tise_resize_tf1_f32 (csrc/resize_tf1.hip) against the numpy restatement of TensorFlow 1's legacy ResizeBilinear
(tests/_tf1_resize_ref.py), bit for bit: up- and downscaling, the identity, a one-pixel source, odd sizes, more than one
workgroup, and a source at an odd byte address."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import _tf1_resize_ref as ref

pytestmark = pytest.mark.gpu

# (n, h, w, oh, ow)
CASES = [(1, 2, 2, 4, 4), (2, 299, 299, 299, 299), (3, 64, 64, 299, 299), (1, 256, 256, 299, 299), (1, 512, 384, 299, 299),
         (1, 1, 1, 299, 299), (2, 300, 301, 299, 299), (1, 37, 53, 5, 7)]


@functools.lru_cache(maxsize=None)
def _source(n, h, w):
    rng = np.random.default_rng(1000 * n + 17 * h + w)
    x = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    flat = x.reshape(-1)
    flat[0] = 0                                                  # both ends of the byte range are in every source
    flat[-1] = 255
    if flat.size > 2:
        flat[1] = 255
    x.setflags(write=False)
    return x


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _same_bits(got, want, what):
    g, w = np.ascontiguousarray(got).view(np.int32), np.ascontiguousarray(want).view(np.int32)
    assert g.shape == w.shape, (g.shape, w.shape)
    bad = np.argwhere(g != w)
    assert len(bad) == 0, f"{what}: {len(bad)} of {g.size} values differ in their bits, first at {tuple(bad[0])}: " \
                          f"{got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}"


def _run(src, oh, ow, sub=128.0, mul=2.0 ** -7):
    """The C entry point on a (n, h, w, 3) uint8 device tensor, into a destination pre-filled with NaN."""
    from tise_toolbox_amd import _lib
    n, h, w, _ = src.shape
    dst = torch.full((n, oh, ow, 3), float("nan"), dtype=torch.float32, device=src.device)
    _lib.call("tise_resize_tf1_f32", ctypes.c_void_p(src.data_ptr()), n, h, w, ctypes.c_void_p(dst.data_ptr()), oh, ow, sub, mul, _stream())
    return dst.cpu().numpy()


@pytest.mark.parametrize("n,h,w,oh,ow", CASES, ids=lambda v: str(v))
def test_kernel_matches_restatement_bit_for_bit(cuda_device, n, h, w, oh, ow):
    x = _source(n, h, w)
    got = _run(torch.as_tensor(np.array(x), device=cuda_device), oh, ow)
    assert not np.isnan(got).any()                               # every output was written
    _same_bits(got, ref.network_input_tf1(x, (oh, ow)), f"{(n, h, w)} -> {(oh, ow)}")


# The launch caps its grid at GRID_CAP workgroups of 256 threads; a thread takes pixels i, i + stride, ... (csrc/resize_tf1.hip).
GRID_CAP = 16384
STRIDE = GRID_CAP * 256                                          # 4 194 304 output pixels per round of the loop

# (n, h, w, oh, ow): just past the cap.  The first is the product's output size; the second is not square, its pixel count is
# no multiple of 256 (a partial last workgroup in the second round) and ow does not divide the stride, so a thread's ox, oy and
# img all change from one iteration to the next.
PAST_THE_CAP = [(48, 8, 8, 299, 299), (94, 5, 6, 149, 301)]


@pytest.mark.parametrize("n,h,w,oh,ow", PAST_THE_CAP, ids=lambda v: str(v))
def test_past_the_grid_cap_bit_for_bit(cuda_device, n, h, w, oh, ow):
    """More output pixels than the capped grid has threads: the second iteration of the grid-stride loop writes the tail.
    Every value is held to the restatement, so a wrong stride, a loop left early or an index that wraps shows."""
    pixels = n * oh * ow
    assert STRIDE < pixels < 2 * STRIDE
    if (oh, ow) != (299, 299):
        assert pixels % 256 != 0 and STRIDE % ow != 0 and STRIDE % (oh * ow) != 0
    x = _source(n, h, w)
    got = _run(torch.as_tensor(np.array(x), device=cuda_device), oh, ow)
    assert not np.isnan(got).any()                               # every output was written
    _same_bits(got, ref.network_input_tf1(x, (oh, ow)), f"{(n, h, w)} -> {(oh, ow)}")


def test_several_rounds_of_the_grid_stride_loop(cuda_device):
    """600 images -> 299 x 299 are 53.6 M pixels, 13 rounds of the loop (a 1000-image pass of the product takes 22).  The
    sources cycle through 7 distinct images; a 7-image launch (one round, no loop) is held to the restatement on the host,
    and the 644 MB result is compared with it on the device, image i against image i mod 7, bit for bit.  Nothing of the
    big result is sampled and nothing of it is copied back."""
    n, k, h, w, oh, ow = 600, 7, 4, 4, 299, 299
    assert n * oh * ow > 12 * STRIDE
    base = _source(k, h, w)
    small_src = torch.as_tensor(np.array(base), device=cuda_device)
    small = torch.full((k, oh, ow, 3), float("nan"), dtype=torch.float32, device=cuda_device)
    from tise_toolbox_amd import _lib
    _lib.call("tise_resize_tf1_f32", ctypes.c_void_p(small_src.data_ptr()), k, h, w, ctypes.c_void_p(small.data_ptr()), oh, ow,
              128.0, 2.0 ** -7, _stream())
    _same_bits(small.cpu().numpy(), ref.network_input_tf1(base, (oh, ow)), "the 7-image launch")

    idx = torch.arange(n, device=cuda_device) % k
    src = small_src[idx].contiguous()
    dst = torch.full((n, oh, ow, 3), float("nan"), dtype=torch.float32, device=cuda_device)
    _lib.call("tise_resize_tf1_f32", ctypes.c_void_p(src.data_ptr()), n, h, w, ctypes.c_void_p(dst.data_ptr()), oh, ow,
              128.0, 2.0 ** -7, _stream())
    want = small.view(torch.int32)
    got = dst.view(torch.int32)
    full = (n // k) * k
    same = (got[:full].view(n // k, k, oh, ow, 3) == want).flatten(2).all(dim=2).flatten()
    same = torch.cat([same, (got[full:] == want[:n - full]).flatten(1).all(dim=1)])
    bad = torch.nonzero(~same).flatten().tolist()
    assert not bad, f"{len(bad)} of {n} images differ from their 7-image twin: first {bad[0]}, last {bad[-1]}"


def test_raw_values_without_the_affine(cuda_device):
    x = _source(1, 37, 53)
    got = _run(torch.as_tensor(np.array(x), device=cuda_device), 5, 7, sub=0.0, mul=1.0)
    _same_bits(got, ref.resize_tf1(x, (5, 7)), "sub 0, mul 1")


def test_batch_slice_at_an_odd_address(cuda_device):
    from tise_toolbox_amd import device
    x = _source(5, 33, 35)
    u8 = torch.as_tensor(np.array(x), device=cuda_device)
    part = u8[1:]
    assert part.data_ptr() % 2 == 1 and part.is_contiguous()     # 33 * 35 * 3 = 3465 bytes per image
    want = ref.network_input_tf1(x[1:], (299, 299))
    _same_bits(_run(part, 299, 299), want, "u8[1:]")
    # the wrapper: NCHW view of the same NHWC bits (channels_last), or a contiguous NCHW copy
    y = device.resize_tf1_f32(part, (299, 299), 128, 2.0 ** -7)
    assert tuple(y.shape) == (4, 3, 299, 299) and y.is_contiguous(memory_format=torch.channels_last)
    _same_bits(y.permute(0, 2, 3, 1).cpu().numpy(), want, "device.resize_tf1_f32")
    z = device.resize_tf1_f32(part, (299, 299), 128, 2.0 ** -7, channels_last=False)
    assert z.is_contiguous() and torch.equal(z, y)


def test_bad_arguments_are_refused_before_anything_is_enqueued(cuda_device):
    from tise_toolbox_amd import _lib, device
    lib = _lib.load()
    src = torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device=cuda_device)
    dst = torch.full((1, 2, 2, 3), float("nan"), dtype=torch.float32, device=cuda_device)
    S, D = ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr())
    bad = _lib.TISE_ERR_INVALID_ARG
    assert lib.tise_resize_tf1_f32(S, 1, 0, 4, D, 2, 2, 128.0, 2.0 ** -7, _stream()) == bad
    assert lib.tise_resize_tf1_f32(S, 1, 4, -1, D, 2, 2, 128.0, 2.0 ** -7, _stream()) == bad
    assert lib.tise_resize_tf1_f32(S, 1, 4, 4, D, 0, 2, 128.0, 2.0 ** -7, _stream()) == bad
    assert lib.tise_resize_tf1_f32(S, 1, 4, 4, D, 2, 0, 128.0, 2.0 ** -7, _stream()) == bad
    assert lib.tise_resize_tf1_f32(S, -1, 4, 4, D, 2, 2, 128.0, 2.0 ** -7, _stream()) == bad
    assert lib.tise_resize_tf1_f32(None, 1, 4, 4, D, 2, 2, 128.0, 2.0 ** -7, _stream()) == bad
    assert lib.tise_resize_tf1_f32(S, 1, 4, 4, None, 2, 2, 128.0, 2.0 ** -7, _stream()) == bad
    torch.cuda.synchronize()
    assert torch.isnan(dst).all()                                # nothing ran
    with pytest.raises(ValueError):
        device.resize_tf1_f32(src.float(), (2, 2))
    with pytest.raises(ValueError):
        device.resize_tf1_f32(src, (0, 2))
