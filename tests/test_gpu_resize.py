"""resize_bilinear_u8_kernel (csrc/resize.hip) against the installed Pillow on every branch, edge and plan path.

The kernel is integer arithmetic, so every comparison is ``assert_array_equal``.  The expected uint8 image is Pillow's own
``Image.resize``; the oracle (oracle/resize_oracle.py) must agree with it in the same test; the expected float outputs are
the 3x256 table applied to that uint8 image, exactly.  ``_check_all_products`` compares the four products of a call (float
channels-last, float planar, the uint8 next to a float output, uint8 only) with one expected image, every destination inside
a larger buffer of canary bytes that must be intact afterwards.  The kernel's host tables (precompute_coeffs in resize_plan.h)
have no export: they are covered here by outputs (tests/test_resize_host.py, point 3 of its docstring).

Every GPU step is an ordinary launch with valid arguments or a host-side refusal that returns before any launch.
"""
import ctypes
import os

import numpy as np
import pytest
import torch
from PIL import Image

from oracle import resize_oracle
from tests import _cases

pytestmark = pytest.mark.gpu

PIL_FILTER = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}
FILTERS = ("bilinear", "bicubic")


@pytest.fixture(scope="module")
def dev(cuda_device):
    return cuda_device


# ------------------------------------------------------------------- the three tests that lived in test_gpu_kernels.py
def test_resize_golden_bit_exact(dev, golden_dir):
    from tise_toolbox_amd import device
    g = np.load(os.path.join(golden_dir, "pil_resize_299.npz"))
    names = [k[3:] for k in g.files if k.startswith("in_")]
    lut = device.make_lut(True)
    for k in names:
        src = torch.as_tensor(g["in_" + k], device=dev).unsqueeze(0)
        for cl in (True, False):
            out, u8 = device.resize_bilinear_u8(src, (299, 299), lut, channels_last=cl, return_u8=True)
            np.testing.assert_array_equal(u8[0].cpu().numpy(), g["out_" + k], err_msg=f"{k} cl={cl}")
            # fused ToTensor + inception.py:120-124 affine: bit-exact against the numpy restatement
            want = resize_oracle.normalize_input(resize_oracle.to_tensor(g["out_" + k]))
            got = out[0].cpu().numpy()
            assert got.shape == (3, 299, 299)
            np.testing.assert_array_equal(got, want, err_msg=f"{k} cl={cl} float")
            assert out.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)


@pytest.mark.parametrize("h,w", [(256, 256), (64, 48), (299, 299), (300, 299), (299, 301), (517, 31), (1024, 768), (7, 5)])
def test_resize_random_sizes_vs_oracle(dev, h, w):
    from tise_toolbox_amd import device
    rng = np.random.default_rng(h * 7 + w)
    n = 3
    imgs = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    out, u8 = device.resize_bilinear_u8(torch.as_tensor(imgs, device=dev), (299, 299), device.make_lut(False),
                                        channels_last=True, return_u8=True)
    only = device.resize_u8_only(torch.as_tensor(imgs, device=dev), (299, 299))     # the product path: uint8 out only (4 bytes per lane)
    for i in range(n):
        want = resize_oracle.resize_bilinear_u8(imgs[i], 299, 299)
        np.testing.assert_array_equal(u8[i].cpu().numpy(), want)
        np.testing.assert_array_equal(only[i].cpu().numpy(), want)
        np.testing.assert_array_equal(out[i].cpu().numpy(), resize_oracle.to_tensor(want))
    # a destination that is not a multiple of four bytes wide and not 299: the dword stores' row tails
    for (oh, ow) in ((61, 37), (300, 298)):
        got = device.resize_u8_only(torch.as_tensor(imgs[:1], device=dev), (oh, ow))
        np.testing.assert_array_equal(got[0].cpu().numpy(), resize_oracle.resize_bilinear_u8(imgs[0], oh, ow))


def test_resize_batch_and_empty(dev):
    from tise_toolbox_amd import device
    imgs = _cases.smooth_images(5, 256, 256, seed=1)
    out, u8 = device.resize_bilinear_u8(torch.as_tensor(imgs, device=dev), return_u8=True)
    for i in range(5):
        np.testing.assert_array_equal(u8[i].cpu().numpy(), resize_oracle.resize_bilinear_u8(imgs[i], 299, 299))
    empty = device.resize_bilinear_u8(torch.empty((0, 256, 256, 3), dtype=torch.uint8, device=dev))
    assert tuple(empty.shape) == (0, 3, 299, 299)


# ------------------------------------------------------------------------------------------------------------- helpers
class _Guarded:
    """A destination of ``nbytes`` inside a larger device buffer of canary bytes: at least one destination row (and at least
    256 bytes) before and after it.  ``odd`` puts a uint8 destination at an address that is 3 mod 4, as a slice of a batch
    buffer of 299 x 299 x 3 images is (the uint8-only path stores unaligned dwords)."""

    def __init__(self, dev, nbytes, row_bytes, odd=False):
        self.pad = (max(row_bytes, 256) + 255) // 256 * 256 + (3 if odd else 0)
        self.nbytes = nbytes
        total = 2 * self.pad + nbytes
        self.canary = ((np.arange(total, dtype=np.int64) * 131 + 89) & 255).astype(np.uint8)
        self.buf = torch.from_numpy(self.canary).to(dev)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + self.pad)

    def view(self, shape):
        return self.buf[self.pad:self.pad + self.nbytes].view(shape)

    def payload(self, dtype, shape):
        """The destination's content after the canary on both sides has been found intact."""
        host = self.buf.cpu().numpy()
        np.testing.assert_array_equal(host[:self.pad], self.canary[:self.pad], err_msg="bytes BEFORE the destination were written")
        np.testing.assert_array_equal(host[self.pad + self.nbytes:], self.canary[self.pad + self.nbytes:],
                                      err_msg="bytes AFTER the destination were written")
        return np.frombuffer(host[self.pad:self.pad + self.nbytes].tobytes(), dtype=dtype).reshape(shape)

    def assert_untouched(self):
        np.testing.assert_array_equal(self.buf.cpu().numpy(), self.canary)


def _launch(src, oh, ow, filt, lut, dst=None, nhwc=1, u8=None):
    """One call of the C entry point (bilinear through tise_resize_bilinear_u8, bicubic through tise_resize_u8)."""
    from tise_toolbox_amd import _lib
    n, h, w, _ = src.shape
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lutp = lut.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    sp = ctypes.c_void_p(src.data_ptr())
    if filt == "bilinear":
        _lib.call("tise_resize_bilinear_u8", sp, n, h, w, dst, oh, ow, nhwc, lutp, u8, stream)
    else:
        _lib.call("tise_resize_u8", sp, n, h, w, dst, oh, ow, nhwc, lutp, u8, 1, stream)


def _expected(imgs, oh, ow, filt):
    """Pillow's own resize of every image; the oracle must say the same."""
    want = np.stack([np.asarray(Image.fromarray(im).resize((ow, oh), PIL_FILTER[filt])) for im in imgs])
    for k, im in enumerate(imgs):
        np.testing.assert_array_equal(resize_oracle.resize_u8(im, oh, ow, filt), want[k], err_msg="oracle != Pillow")
    return want


def _float_of(want_u8, lut):
    """(N,oh,ow,3) uint8 -> (N,oh,ow,3) fp32: the table row of each channel applied to the byte, exactly."""
    return np.stack([lut[c][want_u8[..., c]] for c in range(3)], axis=-1)


def _products(dev, src, oh, ow, filt, lut):
    """The four products of one source batch, each written into a guarded destination: (float channels-last as (N,oh,ow,3),
    float planar (N,3,oh,ow), the uint8 next to the channels-last float, the uint8-only result)."""
    from tise_toolbox_amd import device
    n = src.shape[0]
    src = device._vertical_pass_first(src, oh, filt)         # the product's own step for Pillow's vertical-first region
    fb, ub = n * oh * ow * 3 * 4, n * oh * ow * 3
    g_cl, g_u8 = _Guarded(dev, fb, ow * 3 * 4), _Guarded(dev, ub, ow * 3, odd=True)
    _launch(src, oh, ow, filt, lut, dst=g_cl.ptr, nhwc=1, u8=g_u8.ptr)
    g_pl = _Guarded(dev, fb, ow * 4)
    _launch(src, oh, ow, filt, lut, dst=g_pl.ptr, nhwc=0)
    g_only = _Guarded(dev, ub, ow * 3, odd=True)
    if filt == "bilinear":                                  # the product's wrapper, writing into a slice of a byte buffer
        assert device.resize_u8_only(src, (oh, ow), out=g_only.view((n, oh, ow, 3))).data_ptr() == g_only.ptr.value
    else:
        _launch(src, oh, ow, filt, lut, u8=g_only.ptr)
    torch.cuda.current_stream().synchronize()
    return (g_cl.payload(np.float32, (n, oh, ow, 3)), g_pl.payload(np.float32, (n, 3, oh, ow)),
            g_u8.payload(np.uint8, (n, oh, ow, 3)), g_only.payload(np.uint8, (n, oh, ow, 3)))


def _check_all_products(dev, imgs, oh, ow, filt, lut=None):
    """``imgs``: (3,h,w,3) uint8, three DIFFERENT images (a wrong image index shows).  Image 1 is also run as a batch of one."""
    from tise_toolbox_amd import device
    lut = device.make_lut(True) if lut is None else lut
    assert imgs.shape[0] == 3
    want = _expected(imgs, oh, ow, filt)
    want_f = _float_of(want, lut)
    tag = f"{imgs.shape[1]}x{imgs.shape[2]} -> {oh}x{ow} {filt}"
    src = torch.from_numpy(np.ascontiguousarray(imgs)).to(dev)
    cl, pl, u8, only = _products(dev, src, oh, ow, filt, lut)
    np.testing.assert_array_equal(u8, want, err_msg=tag + ": uint8 next to the float output")
    np.testing.assert_array_equal(only, want, err_msg=tag + ": uint8 only")
    np.testing.assert_array_equal(cl, want_f, err_msg=tag + ": float channels-last")
    np.testing.assert_array_equal(pl, want_f.transpose(0, 3, 1, 2), err_msg=tag + ": float planar")
    one = _products(dev, src[1:2].contiguous(), oh, ow, filt, lut)
    for got, full, name in zip(one, (cl, pl, u8, only), ("channels-last", "planar", "uint8", "uint8 only")):
        np.testing.assert_array_equal(got[0], full[1], err_msg=tag + f": batch of one != image 1 of the batch ({name})")


def _three(h, w, seed, kind="random"):
    rng = np.random.default_rng(seed)
    if kind == "binary":                                    # 0 and 255 only: clip8 on both sides, bicubic overshoot
        return (rng.integers(0, 2, (3, h, w, 3), dtype=np.uint8) * 255).astype(np.uint8)
    return rng.integers(0, 256, (3, h, w, 3), dtype=np.uint8)


def _row_tile(h, w, oh, ow, filt):
    """The rule written in get_plan (resize.hip), applied to the oracle's bounds: the row-tile height a shape gets, None when
    even one output row per workgroup does not fit.  It selects cases only; it decides no expected value."""
    bounds, _ = resize_oracle.precompute_coeffs(h, oh, filt)
    lo, hi = bounds[:, 0], bounds[:, 0] + bounds[:, 1]
    rt = 16
    while True:
        span = max(int(hi[y0:y0 + rt].max() - lo[y0:y0 + rt].min()) for y0 in range(0, oh, rt))
        if span * (((3 * w + 15) & ~15) + ((3 * ow + 3) & ~3)) + 3072 <= 144 * 1024:
            return rt
        if rt == 1:
            return None
        rt >>= 1


def _assert_refused(dev, h, w, oh, ow, filt, n=3, src=None):
    """A refusal is TISE_ERR_UNSUPPORTED from the host, before any launch: the canary-filled destinations stay untouched."""
    from tise_toolbox_amd import _lib, device
    lut = device.make_lut(True)
    if src is None:
        src = torch.from_numpy(_three(h, w, seed=h + w)).to(dev)
    n = src.shape[0]                                         # full-size destinations, although nothing may be written
    g_f, g_u = _Guarded(dev, n * oh * ow * 3 * 4, ow * 3 * 4), _Guarded(dev, n * oh * ow * 3, ow * 3, odd=True)
    for kw in (dict(dst=g_f.ptr, nhwc=1, u8=g_u.ptr), dict(dst=g_f.ptr, nhwc=0), dict(u8=g_u.ptr)):
        with pytest.raises(_lib.TiseStatusError) as e:
            _launch(src, oh, ow, filt, lut, **kw)
        assert e.value.status == _lib.TISE_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    g_f.assert_untouched()
    g_u.assert_untouched()


# -------------------------------------------------------------------------------------------------------- case matrix
# wide sources with few rows: small in bytes, large in LDS per staged row
ROW_TILE_CASES = {
    "bilinear": [(256, 256, 299, 299), (64, 2000, 37, 100), (60, 4000, 30, 682), (20, 16000, 30, 33), (30, 16000, 20, 33),
                 (40, 12000, 20, 64)],
    "bicubic": [(256, 256, 299, 299), (64, 2000, 37, 100), (10, 7000, 20, 64), (60, 4000, 30, 682), (10, 11000, 20, 64),
                (20, 16000, 20, 33)],
}


@pytest.mark.parametrize("filt", FILTERS)
def test_every_row_tile_height_and_the_refusal(dev, filt):
    cases = ROW_TILE_CASES[filt]
    tiles = [_row_tile(*c, filt) for c in cases]
    assert set(tiles) == {16, 8, 4, 2, 1, None}, tiles
    for (h, w, oh, ow), rt in zip(cases, tiles):
        assert not resize_oracle.pillow_vertical_first(h, w, oh)
        if rt is None:
            _assert_refused(dev, h, w, oh, ow, filt)
        else:
            _check_all_products(dev, _three(h, w, seed=rt), oh, ow, filt)


@pytest.mark.parametrize("filt", FILTERS)
def test_register_limit_of_eight_elements_per_thread(dev, filt):
    """RS_MAXE = 8 elements per thread and row: ow * 3 <= 2048.  ow = 682 fills every slot, 683 is refused."""
    for w in (700, 100):
        for ow in (681, 682):
            _check_all_products(dev, _three(9, w, seed=w + ow), 5, ow, filt)
        _assert_refused(dev, 9, w, 5, 683, filt)


@pytest.mark.parametrize("filt", FILTERS)
def test_thin_and_tiny_sources_and_outputs(dev, filt):
    for (h, w) in ((1, 1), (1, 7), (7, 1), (2, 2), (1, 640), (640, 1), (2, 299), (299, 2)):
        _check_all_products(dev, _three(h, w, seed=h * 1000 + w), 299, 299, filt)
    for (oh, ow) in ((1, 1), (1, 299), (299, 1)):
        for (h, w) in ((1, 1), (7, 5), (64, 48), (100, 90)):
            assert _row_tile(h, w, oh, ow, filt) is not None
            _check_all_products(dev, _three(h, w, seed=oh * 7 + ow + h), oh, ow, filt)
    # one output row needs EVERY source row staged: 300 rows of 299 pixels beside a 299-pixel output row are beyond the LDS
    # budget of get_plan even at one output row per workgroup, and the call is refused, not approximated
    assert _row_tile(300, 299, 1, 299, filt) is None
    _assert_refused(dev, 300, 299, 1, 299, filt)


@pytest.mark.parametrize("filt", FILTERS)
def test_identity_sides(dev, filt):
    """h == oh and / or w == ow: Pillow skips that pass, the kernel copies.  Bicubic never takes the 3-tap paths (ksize 5 at
    every up-scale), so the identity inside the general kernel is a branch of its own."""
    for (h, w, oh, ow) in ((299, 120, 299, 299), (299, 640, 299, 299), (120, 299, 299, 299), (640, 299, 299, 299),
                           (299, 299, 299, 299), (224, 100, 224, 224), (224, 500, 224, 224), (100, 224, 224, 224),
                           (500, 224, 224, 224), (61, 37, 61, 37)):
        _check_all_products(dev, _three(h, w, seed=h + 3 * w, kind="binary" if h == 299 else "random"), oh, ow, filt)


def test_general_horizontal_and_vertical_loops(dev):
    """Bilinear, both sides shrinking by more than 2 : 1 and by a non-integer factor: the non-SMALLK kernel with cnt > 3
    vertical windows.  Bicubic beyond 1.4 : 1 to CLIP's geometry (clip_model.preprocess_geometry)."""
    from tise_toolbox_amd import clip_model
    for (h, w) in ((640, 427), (1000, 999), (427, 640)):
        for kind in ("random", "binary"):
            _check_all_products(dev, _three(h, w, seed=h, kind=kind), 299, 299, "bilinear")
    for (h, w) in ((512, 512), (640, 480), (480, 640)):
        nh, nw, _, _ = clip_model.preprocess_geometry(h, w)
        assert min(nh, nw) == 224
        for kind in ("random", "binary"):
            _check_all_products(dev, _three(h, w, seed=w, kind=kind), nh, nw, "bicubic", lut=clip_model.preprocess_lut())


def test_dword_row_tails_of_the_uint8_only_path(dev):
    """resize_u8_only stores four bytes per lane and finishes a row byte by byte: 3 * ow = 0, 1, 2, 3 mod 4, rows that start
    at every address modulo 4, three images, canary on both sides (in _check_all_products)."""
    seen = set()
    for ow in (36, 37, 38, 39, 299, 300, 1, 2, 3, 4, 5):
        seen.add(3 * ow % 4)
        for (h, w, oh) in ((64, 48, 61), (16, 20, 33)):            # h != oh, at most three vertical taps: the dword path
            _check_all_products(dev, _three(h, w, seed=ow), oh, ow, "bilinear")
    assert seen == {0, 1, 2, 3}


def test_staging_branch_follows_the_base_address(dev):
    """Rows of 48 pixels are 144 bytes, a multiple of 16: the 16-byte staging loads are taken when the base address allows
    it and the byte-wise loop when it does not (a view into a byte buffer)."""
    from tise_toolbox_amd import device
    imgs = _three(64, 48, seed=11)
    nbytes = imgs.size
    lut = device.make_lut(True)
    for filt in FILTERS:
        want = _expected(imgs, 299, 299, filt)
        for off in (0, 1, 8):
            big = torch.zeros(nbytes + 64, dtype=torch.uint8, device=dev)
            src = big[off:off + nbytes].view(3, 64, 48, 3)
            src.copy_(torch.from_numpy(imgs))
            assert src.is_contiguous() and src.data_ptr() % 16 == off
            cl, pl, u8, only = _products(dev, src, 299, 299, filt, lut)
            np.testing.assert_array_equal(u8, want, err_msg=f"offset {off}")
            np.testing.assert_array_equal(only, want, err_msg=f"offset {off}")
            np.testing.assert_array_equal(cl, _float_of(want, lut), err_msg=f"offset {off}")
            np.testing.assert_array_equal(pl, _float_of(want, lut).transpose(0, 3, 1, 2), err_msg=f"offset {off}")


def test_grid_limit_of_65535_images(dev):
    """The image index is blockIdx.y: 65 535 sources are accepted, 65 536 refused.  A 1 x 1 source has one tap of weight
    2**22 on each axis, so every output pixel is the source pixel (held to Pillow on a sample)."""
    from tise_toolbox_amd import device
    n = 65535
    rng = np.random.default_rng(65535)
    imgs = rng.integers(0, 256, (n + 1, 1, 1, 3), dtype=np.uint8)
    lut = device.make_lut(True)
    for k in (0, 1, 4097, n - 1):
        for filt in FILTERS:
            np.testing.assert_array_equal(_expected(imgs[k:k + 1], 2, 2, filt)[0], np.broadcast_to(imgs[k], (2, 2, 3)))
    want = np.broadcast_to(imgs[:n], (n, 2, 2, 3))
    src = torch.from_numpy(imgs).to(dev)
    for filt in FILTERS:
        cl, pl, u8, only = _products(dev, src[:n], 2, 2, filt, lut)
        np.testing.assert_array_equal(u8, want)
        np.testing.assert_array_equal(only, want)
        np.testing.assert_array_equal(cl, _float_of(want, lut))
        np.testing.assert_array_equal(pl, _float_of(want, lut).transpose(0, 3, 1, 2))
        _assert_refused(dev, 1, 1, 2, 2, filt, src=src)


def test_plan_cache_eviction_buffer_reuse_and_reallocation(dev):
    """More distinct source sizes than the plan cache holds (8192): every new plan past that evicts the least recently used
    one and is written into ITS device buffer; the first sizes are evicted by the end and are planned again, the last are
    still cached; a 256 x 256 -> 299 x 299 plan is larger than any of these buffers with their slack and is allocated anew.
    O-FID feeds thousands of distinct crop sizes, so this is a product path.  Every result is checked."""
    from tise_toolbox_amd import device
    oh, ow = 5, 7
    sizes = [(h, w) for h in range(1, 93) for w in range(1, 93)]
    assert len(sizes) > 8192
    rng = np.random.default_rng(8192)
    pool = rng.integers(0, 256, (92 * 92 * 3 + 8464,), dtype=np.uint8)

    def image(i):
        h, w = sizes[i]
        return pool[i:i + h * w * 3].reshape(h, w, 3)                  # a different window of the pool for every size

    def run(indices):
        for start in range(0, len(indices), 92):
            chunk = indices[start:start + 92]
            outs = [device.resize_u8_only(torch.from_numpy(np.ascontiguousarray(image(i))).to(dev).unsqueeze(0), (oh, ow)) for i in chunk]
            got = torch.cat(outs).cpu().numpy()
            for k, i in enumerate(chunk):
                h, w = sizes[i]
                want = np.asarray(Image.fromarray(image(i)).resize((ow, oh), Image.BILINEAR))
                np.testing.assert_array_equal(got[k], want, err_msg=f"{h}x{w}")
                np.testing.assert_array_equal(resize_oracle.resize_u8(image(i), oh, ow), want, err_msg=f"oracle {h}x{w}")

    run(list(range(len(sizes))))
    run(list(range(50)))                                              # evicted by now: planned again
    run(list(range(len(sizes) - 50, len(sizes))))                     # still cached
    _check_all_products(dev, _three(256, 256, seed=256), 299, 299, "bilinear")


def test_table_cache_alternation_and_a_side_stream(dev):
    """get_lut keys the device copies of the tables by CONTENT: three tables alternate over six calls, one of them a fresh
    array equal to an earlier one.  Then a size this process has not planned yet on a side stream (plan upload, table and
    launch with no help from the default stream)."""
    from tise_toolbox_amd import device
    imgs = _three(40, 56, seed=3)
    src = torch.from_numpy(imgs).to(dev)
    want = _expected(imgs, 50, 70, "bilinear")
    a, b, c = device.make_lut(True), device.make_lut(False), device.make_lut(False, scale_pm1=True)
    assert not np.array_equal(a, b) and not np.array_equal(b, c) and not np.array_equal(a, c)
    for lut in (a, b, c, b, np.array(a, copy=True), c):
        for cl in (True, False):
            out, u8 = device.resize_bilinear_u8(src, (50, 70), lut, channels_last=cl, return_u8=True)
            np.testing.assert_array_equal(u8.cpu().numpy(), want)
            np.testing.assert_array_equal(out.cpu().numpy(), _float_of(want, lut).transpose(0, 3, 1, 2))
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    fresh = np.ascontiguousarray(a[::-1])                             # a table no earlier call used
    for filt, (h, w, oh, ow) in (("bilinear", (41, 57, 53, 71)), ("bicubic", (43, 59, 29, 31))):
        imgs2 = _three(h, w, seed=h)
        want2 = _expected(imgs2, oh, ow, filt)
        with torch.cuda.stream(side):
            src2 = torch.from_numpy(imgs2).to(dev)
            out, u8 = device.resize_u8_lut(src2, (oh, ow), fresh, filter=filt, channels_last=True, return_u8=True)
            only = device.resize_u8_only(src2, (oh, ow)) if filt == "bilinear" else u8
        side.synchronize()
        np.testing.assert_array_equal(u8.cpu().numpy(), want2)
        np.testing.assert_array_equal(only.cpu().numpy(), want2)
        np.testing.assert_array_equal(out.cpu().numpy(), _float_of(want2, fresh).transpose(0, 3, 1, 2))


# Image.resize: ``if self.size[1] > self.size[0] * 100 and size[1] < self.size[1]`` -> the vertical pass runs first
RULE_CASES = [(480, 4, 299, 299, True), (480, 5, 299, 299, False), (1024, 8, 299, 299, True), (1000, 10, 299, 299, False),
              (5000, 48, 299, 299, True), (5000, 64, 299, 299, False), (5000, 16, 6000, 299, False)]


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("h,w,oh,ow,inside", RULE_CASES)
def test_pillows_vertical_first_region(dev, filt, h, w, oh, ow, inside):
    """A source more than 100 times taller than wide whose height shrinks: Pillow runs the vertical pass first.  The three
    wrappers of tise_toolbox_amd.device must equal the installed Pillow on both sides of the rule.  The kernel itself states
    one order (horizontal first): inside the rule ONE launch equals Pillow's (h, w) -> (h, ow) -> (oh, ow), which is why the
    wrappers issue two launches there."""
    from tise_toolbox_amd import device
    assert device.pillow_vertical_first(h, w, oh) is inside
    imgs = _three(h, w, seed=h + w)
    lut = device.make_lut(True)
    _check_all_products(dev, imgs, oh, ow, filt, lut)
    want = _expected(imgs, oh, ow, filt)
    src = torch.from_numpy(imgs).to(dev)
    for cl in (True, False):
        if filt == "bilinear":
            out, u8 = device.resize_bilinear_u8(src, (oh, ow), lut, channels_last=cl, return_u8=True)
        else:
            out, u8 = device.resize_u8_lut(src, (oh, ow), lut, filter="bicubic", channels_last=cl, return_u8=True)
        np.testing.assert_array_equal(u8.cpu().numpy(), want)
        np.testing.assert_array_equal(out.cpu().numpy(), _float_of(want, lut).transpose(0, 3, 1, 2))
        assert out.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
    np.testing.assert_array_equal(device.resize_u8_lut(src, (oh, ow), lut, filter=filt).cpu().numpy(),
                                  _float_of(want, lut).transpose(0, 3, 1, 2))
    if filt == "bilinear":
        np.testing.assert_array_equal(device.resize_u8_only(src, (oh, ow)).cpu().numpy(), want)
    if inside:
        g = _Guarded(dev, 3 * oh * ow * 3, ow * 3, odd=True)
        _launch(src, oh, ow, filt, lut, u8=g.ptr)
        torch.cuda.synchronize()
        hfirst = np.stack([np.asarray(Image.fromarray(im).resize((ow, h), PIL_FILTER[filt]).resize((ow, oh), PIL_FILTER[filt]))
                           for im in imgs])
        np.testing.assert_array_equal(g.payload(np.uint8, (3, oh, ow, 3)), hfirst)
