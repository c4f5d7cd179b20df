"""GPU: clean-fid's float32 bicubic resize (csrc/resize_f32.hip) and fid_score --mode clean on the MI355X.

Kernel: tise_resize_f32 and tise_resize_ragged_f32 against the numpy restatement of Pillow's algorithm (tests/_clean_resize_ref.py,
itself pinned to Pillow by tests/test_clean_resize_host.py) and against Pillow's own recorded outputs
(tests/golden/pil_resize_f32.npz), bit for bit, at the smallest shapes that reach each branch.  Engine: the float route feeds the
trunk the restatement's bits.  End to end: the CLI against the CPU route on the same files."""
import ctypes
import functools
import hashlib
import os
import time

import numpy as np
import pytest
import torch

from tests import _cases
from tests import _clean_resize_ref as ref

pytestmark = pytest.mark.gpu

NET = "inception-2015"
INF = float("inf")
STD = dict(clip=(0.0, 255.0), sub=128.0, div=128.0)           # clean-fid's clip and input map
RAW = dict(clip=(-INF, INF), sub=0.0, div=1.0)                # the identity: the resampled value itself


@functools.lru_cache(maxsize=None)
def _want(kind, seed, h, w, oh, ow, filt, order):
    """The restatement's unclipped (oh, ow, 3) float32 result, computed once per case and shared (read-only)."""
    y = ref.resize_f32(ref.content(kind, seed, h, w), (oh, ow), filt, order)
    y.setflags(write=False)
    return y


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _run(dev, x, out_hw, filt="bicubic", nhwc=True, order=0, clip=(0.0, 255.0), sub=128.0, div=128.0):
    """tise_resize_f32 on a (n, h, w, 3) uint8 array -> (n, oh, ow, 3) float32 array, whichever layout the kernel wrote."""
    from tise_toolbox_amd import _lib
    n, h, w, _ = x.shape
    oh, ow = out_hw
    src = torch.as_tensor(x, device=dev)
    dst = torch.full((n, oh, ow, 3) if nhwc else (n, 3, oh, ow), float("nan"), dtype=torch.float32, device=dev)
    _lib.call("tise_resize_f32", ctypes.c_void_p(src.data_ptr()), n, h, w, ctypes.c_void_p(dst.data_ptr()), oh, ow, 1 if nhwc else 0,
              {"bilinear": 0, "bicubic": 1}[filt], clip[0], clip[1], sub, div, order, _stream())
    out = dst if nhwc else dst.permute(0, 2, 3, 1)
    return out.cpu().numpy()


def _same_bits(got, want, what=""):
    g, w = ref.bits(got), ref.bits(want)
    assert g.shape == w.shape, (g.shape, w.shape)
    bad = np.argwhere(g != w)
    assert len(bad) == 0, f"{what}: {len(bad)} of {g.size} values differ in their bits, first at {tuple(bad[0])}: " \
                          f"{np.asarray(got)[tuple(bad[0])]!r} != {np.asarray(want)[tuple(bad[0])]!r}"


# (h, w, oh, ow): the smallest shapes that reach each branch of the kernel
SHAPES = [
    (37, 53, 41, 37),        # up on both axes (<= 5 taps: coefficients in registers); h*w*3 odd: images 2 and 3 of a batch start misaligned
    (64, 2000, 37, 100),     # down with 81 taps per horizontal window; LDS allows a row tile of 4 only
    (2000, 64, 37, 100),     # 219 vertical taps: no float32 row tile fits LDS, one streamed output row per workgroup
    (37, 53, 41, 53),        # identity on x: the horizontal pass is skipped
    (37, 53, 37, 41),        # identity on y
    (37, 53, 37, 53),        # identity on both: the clipped input
    (9, 1, 11, 13), (9, 5, 11, 13), (9, 6, 11, 13), (9, 17, 11, 13),      # w*3 = 3, 15, 18, 51 straddles the 16-byte load
    (8, 16, 11, 13),         # w*3 = 48: the 16-byte loads themselves (image 0; 384 bytes per image keep the others aligned too)
    (20, 24, 17, 19), (20, 24, 15, 19), (40, 24, 33, 7), (40, 24, 31, 7),  # oh one more / one less than a multiple of the row tile (16)
    (1, 1, 1, 1), (1, 1, 37, 41), (2, 3, 5, 4),
    (256, 256, 299, 299),    # the flagship shape (16-byte loads, 19 row tiles)
    (37, 53, 41, 52), (37, 53, 36, 52),   # w / ow just above 1: 7 taps on x, the first size past the register-coefficient border
                                          # (ksx <= 5) of hpass; the vertical pass has 5 taps (up) and 7 (just below 1) beside it
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_batch_kernel_equals_restatement(cuda_device, shape):
    """n = 3 (random, 0/255-only, random content), both output layouts, clean-fid's clip and affine; n = 1 and the identity
    affine on the first image."""
    h, w, oh, ow = shape
    cases = [("rand", 100), ("bw", 101), ("rand", 102)]
    x = np.stack([ref.content(k, s, h, w) for k, s in cases])
    raw = np.stack([_want(k, s, h, w, oh, ow, "bicubic", 0) for k, s in cases])
    want = ref.affine(raw, **STD)
    for nhwc in (True, False):
        _same_bits(_run(cuda_device, x, (oh, ow), nhwc=nhwc), want, f"n=3 nhwc={nhwc}")
    _same_bits(_run(cuda_device, x[:1], (oh, ow), **RAW), raw[:1], "n=1, identity affine")
    if (h, w) == (oh, ow):
        assert np.array_equal(_run(cuda_device, x, (oh, ow), **RAW), x.astype(np.float32))


@pytest.mark.parametrize("shape", [(37, 53, 41, 37), (64, 2000, 37, 100), (2000, 64, 37, 100), (9, 5, 11, 13), (40, 24, 33, 7),
                                   (18, 26, 9, 13)],         # bilinear at scale 2: support 2, 5 taps, the register path while shrinking
                         ids=lambda s: "%dx%d-%dx%d" % s)
def test_batch_kernel_bilinear(cuda_device, shape):
    h, w, oh, ow = shape
    cases = [("rand", 110), ("bw", 111), ("rand", 112)]
    x = np.stack([ref.content(k, s, h, w) for k, s in cases])
    want = ref.affine(np.stack([_want(k, s, h, w, oh, ow, "bilinear", 0) for k, s in cases]), **STD)
    for nhwc in (True, False):
        _same_bits(_run(cuda_device, x, (oh, ow), "bilinear", nhwc=nhwc), want, f"nhwc={nhwc}")


def test_clip_and_affine(cuda_device):
    """0/255 content overshoots to about -70 and 326: both clips act; other bounds and another affine follow the same two
    fp32 operations."""
    h, w, oh, ow = 37, 53, 41, 37
    x = ref.content("bw", 101, h, w)[None]
    raw = _want("bw", 101, h, w, oh, ow, "bicubic", 0)[None]
    assert raw.min() < -40 and raw.max() > 295
    got = _run(cuda_device, x, (oh, ow))
    assert got.min() == -1.0 and got.max() == np.float32(127.0 / 128.0)
    _same_bits(got, ref.affine(raw, **STD))
    for clip, sub, div in (((0.0, 255.0), 0.0, 1.0), ((10.5, 200.25), 3.0, 7.0), ((-INF, INF), 127.5, 127.5), ((0.0, 255.0), 0.0, 255.0)):
        _same_bits(_run(cuda_device, x, (oh, ow), clip=clip, sub=sub, div=div), ref.affine(raw, clip, sub, div), f"{clip} {sub} {div}")


@pytest.mark.parametrize("shape", [(64, 20, 17, 31), (9, 7, 20, 18), (300, 2, 37, 41), (37, 53, 37, 41), (37, 53, 41, 53),
                                   (37, 53, 41, 52), (37, 53, 36, 52)],
                         ids=lambda s: "%dx%d-%dx%d" % s)
def test_vertical_first_order(cuda_device, shape):
    """order = 1 at any shape is the restatement's vertical-first result (down, up, a skipped pass on either axis, and the
    7-tap horizontal pass, the first past the register-coefficient border, as the FINAL pass on float32 rows)."""
    h, w, oh, ow = shape
    cases = [("rand", 120), ("bw", 121), ("rand", 122)]
    x = np.stack([ref.content(k, s, h, w) for k, s in cases])
    want = ref.affine(np.stack([_want(k, s, h, w, oh, ow, "bicubic", 1) for k, s in cases]), **STD)
    for nhwc in (True, False):
        _same_bits(_run(cuda_device, x, (oh, ow), nhwc=nhwc, order=1), want, f"nhwc={nhwc}")


# ---- Pillow's recorded outputs -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "pil_resize_f32.npz"))
    out = []
    for i in range(int(g["n_cases"])):
        kind, seed, h, w, oh, ow, filt = [str(v) for v in g[f"case_{i}"]]
        out.append(dict(kind=kind, seed=int(seed), h=int(h), w=int(w), oh=int(oh), ow=int(ow), filt=filt,
                        out=g[f"out_{i}"] if f"out_{i}" in g.files else None,
                        sha=str(g[f"sha_{i}"]) if f"sha_{i}" in g.files else None,
                        rows=g[f"rows_{i}"] if f"rows_{i}" in g.files else None, step=int(g["row_step"])))
    return out


def _check_golden(got, c, what):
    if c["out"] is not None:
        _same_bits(got, c["out"], what)
    else:
        _same_bits(got[::c["step"]], c["rows"], what + " (every %d-th row)" % c["step"])
        assert hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest() == c["sha"], what + ": SHA-256 of the whole output"


def test_device_resize_f32_equals_pillow_golden(cuda_device, golden):
    """device.resize_f32 (which applies Pillow's tall-image rule itself) == Pillow's recorded bits on every case of the golden
    file: up, down, 0/255 content, bilinear, (1, 1), a skipped pass, (256, 256) -> (299, 299) and the tall (1000, 9) sources."""
    from tise_toolbox_amd import device
    assert any(c["h"] > 100 * c["w"] for c in golden) and any((c["h"], c["w"], c["oh"]) == (256, 256, 299) for c in golden)
    for c in golden:
        x = torch.as_tensor(ref.content(c["kind"], c["seed"], c["h"], c["w"])[None], device=cuda_device)
        for cl in (True, False):
            y = device.resize_f32(x, (c["oh"], c["ow"]), c["filt"], channels_last=cl, **RAW)
            assert tuple(y.shape) == (1, 3, c["oh"], c["ow"]) and y.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
            _check_golden(y.permute(0, 2, 3, 1).cpu().numpy()[0], c, "%(kind)s %(h)dx%(w)d -> %(oh)dx%(ow)d %(filt)s" % c)


def test_order_argument_on_the_tall_golden_case(cuda_device, golden):
    """(1000, 9) -> (299, 299) through the C entry point: order = 1 is Pillow's recorded output, order = 0 is not (about a quarter
    of the values differ by one ulp), so the rule cannot be dropped unnoticed."""
    c = next(c for c in golden if (c["h"], c["w"], c["oh"], c["ow"]) == (1000, 9, 299, 299))
    x = ref.content(c["kind"], c["seed"], c["h"], c["w"])[None]
    _check_golden(_run(cuda_device, x, (299, 299), order=1, **RAW)[0], c, "order=1")
    h0 = _run(cuda_device, x, (299, 299), order=0, **RAW)[0]
    _same_bits(h0, _want(c["kind"], c["seed"], 1000, 9, 299, 299, "bicubic", 0), "order=0")
    assert (ref.bits(h0[::c["step"]]) != ref.bits(c["rows"])).mean() > 0.05


# ---- ragged ----------------------------------------------------------------------------------------------------------------
RAGGED = [(37, 53), (64, 2000), (2000, 64), (4000, 9), (37, 71), (9, 100), (37, 100), (1, 1), (9, 5)]   # -> (37, 100): up, many taps,
#   streamed, TALL (vertical first), identity on y, identity on x, identity on both, one pixel, w*3 = 15


@pytest.mark.parametrize("count", [1, 9])
@pytest.mark.parametrize("misaligned", [False, True])
def test_ragged_equals_the_batch_entry_point(cuda_device, count, misaligned):
    from tise_toolbox_amd import device
    oh, ow = 37, 100
    shapes = RAGGED[3:4] if count == 1 else RAGGED
    assert any(device.pillow_vertical_first(h, w, oh) for h, w in shapes)
    imgs = [ref.content("bw" if i % 3 == 1 else "rand", 200 + i, h, w) for i, (h, w) in enumerate(shapes)]
    if misaligned:           # views at odd offsets of one buffer, as crops of a feed's output buffer are
        flat = torch.empty(sum(im.size + 1 for im in imgs), dtype=torch.uint8, device=cuda_device)
        crops, pos = [], 1
        for im in imgs:
            v = flat[pos:pos + im.size].view(im.shape)
            v.copy_(torch.as_tensor(im))
            crops.append(v)
            pos += im.size + 1
        assert any(c.data_ptr() % 16 for c in crops)
    else:
        crops = [torch.as_tensor(im, device=cuda_device) for im in imgs]
    for cl in (True, False):
        got = device.resize_ragged_f32(crops, (oh, ow), channels_last=cl)
        assert tuple(got.shape) == (len(imgs), 3, oh, ow)
        for i, c in enumerate(crops):
            one = device.resize_f32(c.contiguous().unsqueeze(0), (oh, ow), channels_last=cl)
            assert torch.equal(got[i].view(torch.int32), one[0].view(torch.int32)), (i, shapes[i], cl)
        want = np.stack([ref.clean_input(im, (oh, ow)) for im in imgs])           # order: Pillow's rule
        _same_bits(got.permute(0, 2, 3, 1).cpu().numpy(), want, f"channels_last={cl}")


def test_ragged_refuses_before_enqueueing(cuda_device):
    from tise_toolbox_amd import _lib, device
    good = torch.zeros((8, 8, 3), dtype=torch.uint8, device=cuda_device)
    wide = torch.zeros((2, 1 << 17, 3), dtype=torch.uint8, device=cuda_device)      # one source row is 384 KB: no row tile fits LDS
    with pytest.raises(_lib.TiseStatusError, match="image 1 of the batch"):
        device.resize_ragged_f32([good, wide], (4, 4))
    with pytest.raises(_lib.TiseStatusError):
        device.resize_f32(wide.unsqueeze(0), (4, 4))
    with pytest.raises(ValueError):
        device.resize_ragged_f32([], (4, 4))


# ---- launch edges and plan paths (the u8 kernel's are pinned in test_gpu_resize.py; this file's kernel has its own copy) ---------
def test_grid_limit_of_65535_images(cuda_device):
    """The image index of tise_resize_f32 is blockIdx.y: 65 535 sources are accepted, 65 536 refused with nothing written.
    A 1 x 1 source has one tap of weight 1.0 on each axis, so every output pixel is the source pixel after clip and affine:
    held to the restatement on a sample of images, and to that closed form (two fp32 operations, ref.affine) on every value
    of all 65 535, both layouts and both filters."""
    from tise_toolbox_amd import _lib
    n = 65535
    rng = np.random.default_rng(65535)
    imgs = rng.integers(0, 256, (n + 1, 1, 1, 3), dtype=np.uint8)
    clip = (10.0, 200.0)                                          # both clips act on some of the bytes
    want = ref.affine(np.broadcast_to(imgs[:n].astype(np.float32), (n, 2, 2, 3)), clip, 128.0, 128.0)
    for filt in ref.FILTERS:
        for k in (0, 1, 4097, n - 1):
            _same_bits(ref.clean_input(imgs[k], (2, 2), filt, clip=clip), want[k], f"restatement, image {k} {filt}")
        for nhwc in (True, False):
            _same_bits(_run(cuda_device, imgs[:n], (2, 2), filt, nhwc=nhwc, clip=clip), want, f"{filt} nhwc={nhwc}")
    src = torch.as_tensor(imgs, device=cuda_device)
    dst = torch.full((n + 1, 2, 2, 3), float("nan"), dtype=torch.float32, device=cuda_device)
    for filt in (0, 1):
        st = _lib.load().tise_resize_f32(ctypes.c_void_p(src.data_ptr()), n + 1, 1, 1, ctypes.c_void_p(dst.data_ptr()), 2, 2, 1, filt,
                                         0.0, 255.0, 128.0, 128.0, 0, _stream())
        assert st == _lib.TISE_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.isnan(dst).all()                                # nothing ran


RAGGED_CHUNK = 4096        # images per launch of tise_resize_ragged_f32 (csrc/resize_plan.h)

# Nine base images per output size, of RAGGED's kinds.  -> (5, 7): (2000, 64) and (64, 2000) are refused there (no tile fits
# LDS), so the streamed kind is (800, 64) (641 staged rows: 123 KB streamed, 177 KB with float32 rows) and the many-tap kind
# (16, 2000) (1145 taps per window, 97 KB).
BASES = {
    (37, 100): RAGGED,
    (5, 7): [(3, 4), (16, 2000), (800, 64), (4000, 9), (5, 11), (9, 7), (5, 7), (1, 1), (9, 5)],
}
OVER_48K = {(37, 100): 1, (5, 7): 2}       # a base whose workgroup needs more than 48 KB of LDS: (64, 2000) / (800, 64)


@functools.lru_cache(maxsize=None)
def _bases(out_hw):
    """The nine base images of an output size and the restatement's network input of each, computed once and shared."""
    imgs = [ref.content("bw" if i % 3 == 1 else "rand", 400 + i, h, w) for i, (h, w) in enumerate(BASES[out_hw])]
    want = np.stack([ref.clean_input(im, out_hw) for im in imgs])                  # order: Pillow's rule
    want.setflags(write=False)
    return imgs, want


def _base_views(dev, imgs):
    """The base images as views of ONE device buffer, each one byte after the other's end: some at odd addresses."""
    flat = torch.empty(sum(im.size + 1 for im in imgs), dtype=torch.uint8, device=dev)
    views, pos = [], 1
    for im in imgs:
        v = flat[pos:pos + im.size].view(im.shape)
        v.copy_(torch.as_tensor(im))
        views.append(v)
        pos += im.size + 1
    assert any(v.data_ptr() % 2 for v in views) and all(v.is_contiguous() for v in views)
    return views


def _ragged_nan(crops, out_hw, nhwc, pinned):
    """tise_resize_ragged_f32 as device.resize_ragged_f32 calls it (Pillow's rule per image, a page-locked table, the current
    stream), into a destination pre-filled with NaN.  -> (n, oh, ow, 3) view of what the kernel wrote."""
    from tise_toolbox_amd import _lib, device
    oh, ow = out_hw
    n = len(crops)
    dev = crops[0].device
    dst = torch.full((n, oh, ow, 3) if nhwc else (n, 3, oh, ow), float("nan"), dtype=torch.float32, device=dev)
    ptrs = np.fromiter((c.data_ptr() for c in crops), dtype=np.uint64, count=n)
    hs = np.fromiter((c.shape[0] for c in crops), dtype=np.int32, count=n)
    ws = np.fromiter((c.shape[1] for c in crops), dtype=np.int32, count=n)
    orders = np.fromiter((1 if device.pillow_vertical_first(c.shape[0], c.shape[1], oh) else 0 for c in crops), dtype=np.int32, count=n)
    need = n * (64 + 4 * oh) + 16 * (n // RAGGED_CHUNK + 1)
    assert pinned.numel() >= need and pinned.is_pinned()
    ws_dev = torch.empty(need, dtype=torch.uint8, device=dev)
    bad = ctypes.c_int64(-1)
    st = _lib.load().tise_resize_ragged_f32(ptrs.ctypes.data, hs.ctypes.data, ws.ctypes.data, orders.ctypes.data, n,
                                            ctypes.c_void_p(dst.data_ptr()), oh, ow, 1 if nhwc else 0, 1, 0.0, 255.0, 128.0, 128.0,
                                            ctypes.c_void_p(ws_dev.data_ptr()), need, ctypes.c_void_p(pinned.data_ptr()),
                                            ctypes.byref(bad), _stream())
    assert st == _lib.TISE_OK, (st, bad.value)
    torch.cuda.current_stream().synchronize()                    # the table and the workspace are read until here
    return dst if nhwc else dst.permute(0, 2, 3, 1)


def _assert_images_equal(got, nine, idx, what):
    """got[i] == nine[idx[i]] in every bit, on the device; the message names the first and last image that differ."""
    g, w = got.contiguous().view(torch.int32), nine.contiguous().view(torch.int32)
    assert not torch.isnan(got).any(), f"{what}: some of the destination was not written"
    same = torch.cat([(g[s:s + 1024] == w[idx[s:s + 1024]]).flatten(1).all(dim=1) for s in range(0, len(idx), 1024)])
    bad = torch.nonzero(~same).flatten().tolist()
    assert not bad, f"{what}: {len(bad)} of {len(idx)} images differ from their twin of the 9-image call: first {bad[0]}, last {bad[-1]}"


@pytest.fixture(scope="module")
def pinned_table():
    return torch.empty(8193 * (64 + 4 * 37) + 16 * 3, dtype=torch.uint8).pin_memory()


# n: one full launch, one image past it (a second launch of one image), two full launches and one image
@pytest.mark.parametrize("n", [RAGGED_CHUNK, RAGGED_CHUNK + 1, 2 * RAGGED_CHUNK + 1])
@pytest.mark.parametrize("out_hw", [(5, 7), (37, 100)], ids=lambda s: "%dx%d" % s)
def test_ragged_across_the_chunk_border(cuda_device, pinned_table, out_hw, n):
    """tise_resize_ragged_f32 launches 4096 images at a time, each launch with its own part of the table and its own
    destination offset.  The crops are views cycling through nine base images (some at odd addresses), both layouts.  The
    9-image call is held to the restatement; image i of the big call must equal image i mod 9 of it, bit for bit, compared on
    the device over every value.  At n = 4097 a second run keeps both bases that need more than 48 KB of LDS out of the first
    launch and puts one in the second launch alone, whose hipFuncSetAttribute then decides it."""
    imgs, want = _bases(out_hw)
    views = _base_views(cuda_device, imgs)
    big = [i for i, im in enumerate(imgs) if im.shape[:2] in ((64, 2000), (2000, 64), (16, 2000), (800, 64))]
    assert OVER_48K[out_hw] in big
    runs = [torch.arange(n) % 9]
    if n == RAGGED_CHUNK + 1:
        small = torch.tensor([i for i in range(9) if i not in big])
        runs.append(torch.cat([small[torch.arange(RAGGED_CHUNK) % len(small)], torch.tensor([OVER_48K[out_hw]])]))
    for nhwc in (True, False):
        nine = _ragged_nan(views, out_hw, nhwc, pinned_table)
        _same_bits(nine.cpu().numpy(), want, f"the 9-image call, nhwc={nhwc}")
        for r, idx in enumerate(runs):
            got = _ragged_nan([views[i] for i in idx.tolist()], out_hw, nhwc, pinned_table)
            _assert_images_equal(got, nine, idx.to(cuda_device), f"n={n} run {r} nhwc={nhwc}")


def test_ragged_two_launches_on_a_side_stream(cuda_device):
    """device.resize_ragged_f32 (its ring of page-locked tables in use) on a side stream, 4097 crops of three sizes and an
    output size this process has not planned: plan upload, table copy and both launches with no help from the default stream.
    The result of this shape is allocated here for the first time, so no earlier result can stand in for a missing write."""
    from tise_toolbox_amd import device
    oh, ow = 6, 9
    sizes = [(23, 29), (31, 17), (13, 41)]
    imgs = [ref.content("rand", 500 + i, h, w) for i, (h, w) in enumerate(sizes)]
    want = torch.from_numpy(np.stack([ref.clean_input(im, (oh, ow)) for im in imgs])).to(cuda_device)
    n = RAGGED_CHUNK + 1
    idx = torch.arange(n) % 3
    side = torch.cuda.Stream(device=cuda_device)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        views = _base_views(cuda_device, imgs)
        for cl in (True, False):
            got = device.resize_ragged_f32([views[i] for i in idx.tolist()], (oh, ow), channels_last=cl)
            assert tuple(got.shape) == (n, 3, oh, ow)
            side.synchronize()
            _assert_images_equal(got.permute(0, 2, 3, 1), want, idx.to(cuda_device), f"side stream, channels_last={cl}")
    side.synchronize()


def test_plan_cache_eviction_buffer_reuse_and_reallocation(cuda_device, pinned_table):
    """More distinct source sizes than the f32 plan cache holds (8192), as the u8 sibling in test_gpu_resize.py.  First all
    8464 sizes in ONE tise_resize_ragged_f32 call of three launches: planning the third launch's sizes evicts plans whose
    launch is still in flight (the synchronisation in get_plan_f orders the overwrite behind it); all 8464 results are held to
    the restatement.  Then device.resize_f32 one size at a time over every 7th size: the cache holds the last 8192, so the
    first 46 calls of that scan miss, each evicting the least recently used plan and writing its table into the victim's
    buffer, and the rest hit.  (Over ALL sizes, where every call misses, the test took 5.1 s on the MI355X machine -- 3.6 s of
    it the restatement on the host, 1.1 s that scan -- against 2.3 s for its u8 sibling in test_gpu_resize.py; every 7th
    keeps it within twice the sibling.)  Then the first 50 sizes again (42 of them evicted: planned again into reused
    buffers), the last 50 (still cached), and 256 x 256 -> 299 x 299, a plan larger than any of those buffers with their
    slack, allocated anew.  Every result is held to the restatement."""
    from tise_toolbox_amd import device
    oh, ow = 5, 7
    sizes = [(h, w) for h in range(1, 93) for w in range(1, 93)]
    assert len(sizes) > 8192 + 50 and len(sizes) <= 3 * RAGGED_CHUNK
    rng = np.random.default_rng(8192)
    pool = rng.integers(0, 256, (92 * 92 * 3 + 8464,), dtype=np.uint8)
    pool_dev = torch.as_tensor(pool, device=cuda_device)

    def image(i, p=pool):
        h, w = sizes[i]
        return p[i:i + h * w * 3].reshape(h, w, 3)                     # a different window of the pool for every size, any address

    t0 = time.time()
    want = np.stack([ref.clean_input(image(i), (oh, ow)) for i in range(len(sizes))])
    t1 = time.time()
    got = _ragged_nan([image(i, pool_dev) for i in range(len(sizes))], (oh, ow), True, pinned_table)
    _same_bits(got.cpu().numpy(), want, "one ragged call over 8464 sizes")
    t2 = time.time()

    def run(indices):
        for start in range(0, len(indices), 92):
            chunk = indices[start:start + 92]
            outs = [device.resize_f32(image(i, pool_dev).unsqueeze(0), (oh, ow)) for i in chunk]
            _same_bits(torch.cat(outs).permute(0, 2, 3, 1).cpu().numpy(), want[chunk], f"sizes {sizes[chunk[0]]} .. {sizes[chunk[-1]]}")

    run(list(range(0, len(sizes), 7)))
    run(list(range(50)))                                              # evicted by now: planned again
    run(list(range(len(sizes) - 50, len(sizes))))                     # still cached
    print(f"restatement of {len(sizes)} sizes on the host {t1 - t0:.2f} s; one ragged call {t2 - t1:.2f} s; one size at a time {time.time() - t2:.2f} s")
    cases = [("rand", 100), ("bw", 101), ("rand", 102)]
    x = np.stack([ref.content(k, s, 256, 256) for k, s in cases])
    big = ref.affine(np.stack([_want(k, s, 256, 256, 299, 299, "bicubic", 0) for k, s in cases]), **STD)
    for nhwc in (True, False):
        _same_bits(_run(cuda_device, x, (299, 299), nhwc=nhwc), big, f"256 x 256 -> 299 x 299 nhwc={nhwc}")


# ---- engine ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clean_engine(cuda_device):
    from tise_toolbox_amd.engine import RealismEngine
    torch.backends.cudnn.benchmark = False
    return RealismEngine(dims=2048, seed=0, network=NET, resize="clean")


def test_engine_clean_route_feeds_the_trunk_the_restatement(cuda_device, clean_engine):
    """features_from_u8 == the same trunk on the input the restatement builds on the host, to the last bit (the same launches
    on the same input bits); features_from_u8_list on equal-sized images == features_from_u8."""
    imgs = np.stack([ref.content("rand", 300 + i, 64, 80) for i in range(8)])
    x = torch.from_numpy(np.stack([ref.clean_input(im, (299, 299)) for im in imgs])).to(cuda_device).permute(0, 3, 1, 2)
    want, _ = clean_engine._trunk(x, prenormalized=True)
    want = want.clone()
    u8 = torch.as_tensor(imgs, device=cuda_device)
    got, _ = clean_engine.features_from_u8(u8)
    assert got.shape == (8, 2048) and torch.isfinite(got).all()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    lst, _ = clean_engine.features_from_u8_list([u8[i] for i in range(8)])
    assert torch.equal(lst.view(torch.int32), want.view(torch.int32))
    # the float route is not the uint8 route
    from tise_toolbox_amd.engine import RealismEngine
    ref_eng = RealismEngine(dims=2048, seed=0, network=NET, resize="reference")
    base, _ = ref_eng.features_from_u8(u8)
    assert (base - got).abs().max().item() > 1e-4 * base.abs().max().item()
    # ... and resize="reference" is the engine built without the argument, bit for bit
    plain, _ = RealismEngine(dims=2048, seed=0, network=NET).features_from_u8(u8)
    assert torch.equal(plain.view(torch.int32), base.view(torch.int32))
    assert clean_engine.resize == "clean" and ref_eng.resize == "reference"


def test_engine_refuses_clean_on_another_network(cuda_device):
    from tise_toolbox_amd.engine import RealismEngine
    with pytest.raises(ValueError, match="inception-2015"):
        RealismEngine(dims=2048, seed=0, resize="clean")
    with pytest.raises(ValueError, match="unknown resize"):
        RealismEngine(dims=2048, seed=0, network=NET, resize="bicubic")


# ---- end to end ------------------------------------------------------------------------------------------------------------
def _write(d, imgs):
    from PIL import Image
    d.mkdir(parents=True)
    for i, im in enumerate(imgs):
        Image.fromarray(im).save(d / f"{i:05d}.png")


def test_fid_cli_mode_clean_vs_cpu_route(cuda_device, tmp_path, monkeypatch, capsys):
    """fid_score --mode clean on two directories of 60 seeded 48 x 64 PNGs at batch 50 (drop-last would lose 10 images) against
    the CPU route on the same files: Pillow's float resize per channel, clip, (x - 128) / 128, the project's fp32
    InceptionV3(network="inception-2015") on the CPU with the same stand-in weights, np.cov over all 60 rows, the oracle's
    Frechet function.  |dFID| <= 1e-3 absolute (the project's standing budget).  On these images the CPU routes alone give
    30.85 for the clean route against 35.50 for the reference's route (uint8 bilinear resize, the first 50 images; 34.18 on all
    60, so the resize alone moves it too): the modes are told apart."""
    from PIL import Image
    from oracle import fid_oracle
    from tise_toolbox_amd import fid_score, img_data
    from tise_toolbox_amd.inception import InceptionV3
    from tise_toolbox_amd.weights import SYNTHETIC_TAG
    monkeypatch.setenv("TISE_CONV", "split")
    gdir, rdir = tmp_path / "gen", tmp_path / "ref"
    _write(gdir, _cases.smooth_images(60, 48, 64, seed=31))
    _write(rdir, _cases.smooth_images(60, 48, 64, seed=32, shift=0.15))
    stats, out = tmp_path / "gen_clean.npz", tmp_path / "fid.txt"
    argv = ["--batch-size", "50", "--path1", str(rdir), "--path2", str(gdir), "--num-workers", "0", "--synthetic-weights"]
    v = fid_score.main(argv + ["--mode", "clean", "--save-stats", str(stats), "--kid", "--saved_file", str(out)])
    assert out.read_text() == f"FID: {v}{fid_score.CLEAN_TAG}{SYNTHETIC_TAG}"           # result lines name the mode
    assert "KID: " in capsys.readouterr().out

    torch.set_num_threads(min(16, torch.get_num_threads()))
    model = InceptionV3([3], seed=0, network=NET).eval()

    def cpu_stats(root):
        files = img_data.get_filenames(str(root))
        assert len(files) == 60
        x = np.stack([ref.affine(ref.pil_resize_f32(np.asarray(Image.open(f).convert("RGB")), (299, 299))) for f in files])
        x = torch.from_numpy(x).permute(0, 3, 1, 2)
        with torch.no_grad():
            f = torch.cat([model(x[i:i + 20], prenormalized=True)[0].flatten(1) for i in range(0, 60, 20)]).numpy().astype(np.float64)
        return f.mean(axis=0), np.cov(f, rowvar=False), f
    mr, sr, _ = cpu_stats(rdir)
    mg, sg, fg = cpu_stats(gdir)
    want = fid_oracle.calculate_frechet_distance(mr, sr, mg, sg)
    print("FID --mode clean device", v, "cpu route", want, "difference", abs(v - want))
    assert abs(v - want) <= 1e-3
    with np.load(stats) as f:
        assert str(f["mode"]) == "clean" and str(f["network"]) == NET
        assert f["features"].shape == (60, 2048)                                       # every image: n is 60, not 50
        assert np.abs(f["mu"] - mg).max() <= 1e-4 * np.abs(mg).max()
    # the mode is visible: the reference's route on the same files (uint8 bilinear resize, the last 10 files dropped) is another number
    t = fid_score.main(argv + ["--network", NET])
    print("FID --mode tise --network inception-2015", t)
    assert abs(t - v) > 1e-3
    # the tagged statistics serve --mode clean and are refused by --mode tise; an explicit other network is refused
    v2 = fid_score.main(["--batch-size", "50", "--path1", str(stats), "--path2", str(rdir), "--num-workers", "0", "--synthetic-weights",
                         "--mode", "clean"])
    assert abs(v2 - v) <= 1e-6 * max(1.0, abs(v))
    with pytest.raises(RuntimeError, match="statistics of mode 'clean'"):
        fid_score.main(["--batch-size", "50", "--path1", str(stats), "--path2", str(rdir), "--num-workers", "0", "--synthetic-weights",
                        "--network", NET])
    with pytest.raises(SystemExit):
        fid_score.main(argv + ["--mode", "clean", "--network", "torchvision"])

