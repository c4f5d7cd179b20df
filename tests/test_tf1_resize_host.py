"""CPU: the numpy restatement of TensorFlow 1's legacy ResizeBilinear (tests/_tf1_resize_ref.py) -- the pin of
csrc/resize_tf1.hip -- against TensorFlow's documented example, the identity, and the bound that makes the kernel's extra clamp
of the lower index dead code at every size served."""
import numpy as np

from tests import _tf1_resize_ref as ref


def test_documented_2x2_to_4x4_example():
    # the example of TF1's resize documentation for align_corners=False without half-pixel centres
    x = np.array([[1, 2], [3, 4]], dtype=np.uint8).reshape(1, 2, 2, 1)
    want = np.array([[1, 1.5, 2, 2], [2, 2.5, 3, 3], [3, 3.5, 4, 4], [3, 3.5, 4, 4]], dtype=np.float32)
    got = ref.resize_tf1(x, (4, 4))[0, :, :, 0]
    assert got.dtype == np.float32
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


def test_same_size_returns_the_bytes():
    rng = np.random.default_rng(0)
    x = rng.integers(0, 256, (2, 299, 299, 3), dtype=np.uint8)
    x[0, 0, 0], x[0, 0, 1] = 0, 255
    got = ref.resize_tf1(x, (299, 299))
    assert np.array_equal(got.view(np.int32), x.astype(np.float32).view(np.int32))


def test_unclamped_lower_index_stays_in_bounds():
    """TensorFlow does not clamp floor(o * scale) to in - 1; the kernel does.  The clamp is never active: the float32 product
    (out - 1) * (in / out) stays below in for every source size 1..4096 resized to 299, and for every pair up to 64 x 64."""
    for n_in in range(1, 4097):
        assert ref.unclamped_lo_max(n_in, 299) <= n_in - 1, n_in
    for n_out in range(1, 65):
        for n_in in range(1, 65):
            assert ref.unclamped_lo_max(n_in, n_out) <= n_in - 1, (n_in, n_out)


def test_clamped_and_unclamped_taps_agree():
    for n_in, n_out in ((1, 299), (64, 299), (256, 299), (512, 299), (300, 299), (37, 5), (53, 7)):
        a, b = ref.axis_taps(n_in, n_out, clamp_lo=True), ref.axis_taps(n_in, n_out, clamp_lo=False)
        assert all(np.array_equal(p, q) for p, q in zip(a, b))
        assert a[0].min() >= 0 and a[1].max() <= n_in - 1 and (a[1] >= a[0]).all() and (a[2] >= 0).all() and (a[2] < 1).all()


def test_affine_is_sub_then_mul():
    rng = np.random.default_rng(1)
    x = rng.integers(0, 256, (1, 5, 7, 3), dtype=np.uint8)
    v = ref.resize_tf1(x, (9, 11))
    got = ref.network_input_tf1(x, (9, 11))
    want = (v - np.float32(128)) * np.float32(2.0 ** -7)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))
    # bytes 0, 128 and 255 at their own size: -1, 0, 127 / 128
    b = np.array([0, 128, 255], dtype=np.uint8).reshape(1, 1, 1, 3)
    assert ref.network_input_tf1(b, (1, 1)).reshape(-1).tolist() == [-1.0, 0.0, 127.0 / 128.0]
    assert np.array_equal(ref.network_input_tf1(x, (9, 11), sub=0.0, mul=1.0).view(np.int32), v.view(np.int32))
