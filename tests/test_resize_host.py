"""Host half of the resize pin: what the expected values of tests/test_gpu_resize.py rest on.

1. ``oracle.resize_oracle.resize_u8`` against the INSTALLED Pillow's ``Image.resize`` itself (not a stored file), BILINEAR
   and BICUBIC, on random bytes and on images made only of 0 and 255 (the clip in clip8, bicubic overshoot), on both sides
   of ``Image.resize``'s vertical-pass-first rule (h > 100 w and the height shrinks).
2. The precondition of the kernel's 24-bit multiplies (``__mul24`` -> v_mad_i32_i24), swept through the oracle's
   coefficient tables: every coefficient fits the signed 24-bit operand and the accumulator fits ``int``.
3. The kernel's own host tables (``precompute_coeffs`` in csrc/resize_plan.h, rounded in csrc/resize.hip) are host C++ that only a launch reaches and
   there is deliberately no export for them: they are covered by OUTPUTS in tests/test_gpu_resize.py -- every output byte
   depends on every coefficient of its two windows, and those tests compare every byte with Pillow at every table shape
   (up-scale, down-scale, identity, both filters, 1-pixel axes).  What this module adds is that the oracle those tests
   also hold to Pillow has the same tables as Pillow everywhere the GPU tests look.

No GPU here: Pillow, numpy and the oracle only.
"""
import itertools

import numpy as np
import pytest
from PIL import Image

from oracle import resize_oracle

PIL_FILTER = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}
FILTERS = ("bilinear", "bicubic")
SIDES = (1, 2, 3, 7, 16, 299, 300, 640)


def _images(h, w, seed):
    """The two kinds of content: random bytes, and 0 / 255 only (saturating sums and bicubic overshoot on every edge)."""
    rng = np.random.default_rng(seed)
    return {"random": rng.integers(0, 256, (h, w, 3), dtype=np.uint8),
            "binary": (rng.integers(0, 2, (h, w, 3), dtype=np.uint8) * 255).astype(np.uint8)}


def _check(h, w, oh, ow, filt):
    for kind, img in _images(h, w, seed=h * 100003 + w * 17 + oh).items():
        want = np.asarray(Image.fromarray(img).resize((ow, oh), PIL_FILTER[filt]))
        got = resize_oracle.resize_u8(img, oh, ow, filt)
        assert want.shape == (oh, ow, 3)
        np.testing.assert_array_equal(got, want, err_msg=f"{h}x{w} -> {oh}x{ow} {filt} {kind}")


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("out", [299, 224])
def test_oracle_equals_pillow_every_pair_of_source_sides(filt, out):
    for h, w in itertools.product(SIDES, SIDES):
        _check(h, w, out, out, filt)


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("oh,ow", [(1, 1), (1, 682), (5, 682), (61, 37), (300, 298)])
def test_oracle_equals_pillow_odd_outputs(filt, oh, ow):
    for h, w in ((1, 1), (7, 5), (64, 48), (300, 700), (299, 301)):
        _check(h, w, oh, ow, filt)


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("h,w", [(2000, 1500), (4000, 3000), (16, 5000), (5000, 64)])
def test_oracle_equals_pillow_large_sources(filt, h, w):
    _check(h, w, 299, 299, filt)


# Image.resize: ``if self.size[1] > self.size[0] * 100 and size[1] < self.size[1]`` -> vertical pass first
RULE_CASES = [(480, 4, 299, 299, True), (480, 5, 299, 299, False), (1024, 8, 299, 299, True), (1000, 10, 299, 299, False),
              (5000, 48, 299, 299, True), (5000, 64, 299, 299, False), (5000, 16, 6000, 299, False)]


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("h,w,oh,ow,inside", RULE_CASES)
def test_oracle_equals_pillow_on_both_sides_of_the_vertical_first_rule(filt, h, w, oh, ow, inside):
    assert resize_oracle.pillow_vertical_first(h, w, oh) is inside
    _check(h, w, oh, ow, filt)
    if inside:
        # what the rule means, and what the device road does with it: (h, w) -> (oh, w) -> (oh, ow), each step Pillow's own
        img = _images(h, w, seed=h + w)["random"]
        two = Image.fromarray(img).resize((w, oh), PIL_FILTER[filt]).resize((ow, oh), PIL_FILTER[filt])
        np.testing.assert_array_equal(np.asarray(two), np.asarray(Image.fromarray(img).resize((ow, oh), PIL_FILTER[filt])))


def test_device_wrapper_states_the_same_rule_as_the_oracle():
    from tise_toolbox_amd import device
    for h, w, oh, _, inside in RULE_CASES:
        assert device.pillow_vertical_first(h, w, oh) is inside
    for h, w, oh in itertools.product((1, 99, 100, 101, 200, 201, 5000), (1, 2, 50), (1, 100, 101, 299, 6000)):
        assert device.pillow_vertical_first(h, w, oh) == resize_oracle.pillow_vertical_first(h, w, oh) == (h > 100 * w and oh < h)


@pytest.mark.parametrize("filt", FILTERS)
def test_coefficients_fit_the_24_bit_multiply_and_the_int_accumulator(filt):
    """resize.hip multiplies a byte by a coefficient with __mul24 (v_mad_i32_i24: both operands are taken as SIGNED 24-bit
    values, so |k| < 2**23 is required, the byte being < 2**8) and accumulates in ``int`` as Pillow does: the largest
    possible |sum| is 255 * sum|k| plus the rounding constant 2**21, which must stay below 2**31.  Both limits are derived
    from the number formats, not measured.  (For the record, the full sweep gave max|k| = 4 718 205 and a largest
    accumulator of 1 359 106 172.)  Input sizes: 1..64 and every third size up to 700 (the full 1..700 takes about a
    minute), plus the four large ones."""
    in_sizes = sorted(set(range(1, 65)) | set(range(65, 701, 3)) | {700, 1000, 2048, 4000, 5000})
    kmax, accmax = 0, 0
    for out_size in (1, 2, 3, 224, 299, 682):
        for in_size in in_sizes:
            bounds, kk = resize_oracle.precompute_coeffs(in_size, out_size, filt)
            k = kk.astype(np.int64)
            assert (k[np.arange(k.shape[1])[None, :] >= bounds[:, 1:2]] == 0).all()           # nothing behind a window's count
            kmax = max(kmax, int(np.abs(k).max()))
            accmax = max(accmax, 255 * int(np.abs(k).sum(axis=1).max()) + (1 << 21))
    assert kmax < 2 ** 23, kmax
    assert accmax < 2 ** 31, accmax
