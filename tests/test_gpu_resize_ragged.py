"""resize_ragged_u8_kernel (csrc/resize.hip) against the batch entry point, byte for byte.

Both kernels run ONE tile function (resize_u8_tile), so a list of images of different sizes in one ragged launch must give,
crop by crop, what ``device.resize_u8_only`` (bilinear) / ``tise_resize_u8`` with a uint8 destination only (bicubic) give: the
branches that tests/test_gpu_resize.py pins on the batch kernel -- every row-tile height, the eight register slots, identity
sides, dword row tails, both staging branches -- are reached here through the ragged kernel, with neighbouring workgroups of
different sizes.  A fixed subset of every launch is also held to the installed Pillow, so the two entry points cannot be
wrong together.  Integer arithmetic: every comparison is exact.  Every destination lies inside canary bytes, at an address
that is 3 mod 4.

Every GPU step is an ordinary launch with valid arguments or a host-side refusal that returns before any launch.
"""
import ctypes

import numpy as np
import pytest
import torch
from PIL import Image

from tests.test_gpu_resize import FILTERS, PIL_FILTER, ROW_TILE_CASES, _Guarded, _launch, _row_tile

pytestmark = pytest.mark.gpu

RAGGED_CHUNK = 4096        # images per launch of tise_resize_ragged_u8 (csrc/resize_plan.h)
OFFSETS = (0, 1, 8)        # source addresses modulo 16, in turn


def _views(dev, shapes, seed):
    """Images of the given (h, w) as views into ONE byte buffer, at addresses 0, 1, 8 modulo 16 in turn.
    -> (host arrays, device views)"""
    rng = np.random.default_rng(seed)
    host = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    buf = torch.empty(sum(im.size + 32 for im in host) + 16, dtype=torch.uint8, device=dev)
    base = -buf.data_ptr() % 16
    views, pos = [], 0
    for k, im in enumerate(host):
        at = base + pos + OFFSETS[k % 3]
        v = buf[at:at + im.size].view(im.shape)
        v.copy_(torch.from_numpy(im))
        assert v.is_contiguous() and v.data_ptr() % 16 == OFFSETS[k % 3]
        views.append(v)
        pos += (im.size + 31) & ~15
    return host, views


def _ragged_status(views, oh, ow, filt, dst, pinned=None):
    """tise_resize_ragged_u8 on the current stream -> (status, bad_index)."""
    from tise_toolbox_amd import _lib
    n = len(views)
    dev = views[0].device
    ptrs = np.fromiter((v.data_ptr() for v in views), dtype=np.uint64, count=n)
    hs = np.fromiter((v.shape[0] for v in views), dtype=np.int32, count=n)
    ws = np.fromiter((v.shape[1] for v in views), dtype=np.int32, count=n)
    need = n * (64 + 4 * oh) + 16 * (n // RAGGED_CHUNK + 1)
    assert pinned is None or (pinned.numel() >= need and pinned.is_pinned())
    ws_dev = torch.empty(need, dtype=torch.uint8, device=dev)
    bad = ctypes.c_int64(-7)
    st = _lib.load().tise_resize_ragged_u8(ptrs.ctypes.data, hs.ctypes.data, ws.ctypes.data, n, dst, oh, ow, FILTERS.index(filt),
                                           ctypes.c_void_p(ws_dev.data_ptr()), need,
                                           ctypes.c_void_p(pinned.data_ptr()) if pinned is not None else None, ctypes.byref(bad),
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.current_stream().synchronize()                    # the table and the workspace are read until here
    return st, bad.value


def _ragged(views, oh, ow, filt, pinned=None):
    """One ragged call into a guarded destination -> (n, oh, ow, 3) uint8 on the host, the canaries found intact."""
    from tise_toolbox_amd import _lib
    n = len(views)
    g = _Guarded(views[0].device, n * oh * ow * 3, ow * 3, odd=True)
    assert g.ptr.value % 4 == 3
    assert _ragged_status(views, oh, ow, filt, g.ptr, pinned) == (_lib.TISE_OK, -1)
    return g.payload(np.uint8, (n, oh, ow, 3))


def _batch(view, oh, ow, filt):
    """The batch entry point on one crop, uint8 destination only -> (oh, ow, 3) on the host."""
    from tise_toolbox_amd import device
    src = view.contiguous().unsqueeze(0)
    if filt == "bilinear":
        return device.resize_u8_only(src, (oh, ow))[0].cpu().numpy()
    out = torch.empty((1, oh, ow, 3), dtype=torch.uint8, device=view.device)
    _launch(src, oh, ow, filt, device.make_lut(True), u8=ctypes.c_void_p(out.data_ptr()))
    return out[0].cpu().numpy()


def _pillow(im, oh, ow, filt):
    return np.asarray(Image.fromarray(im).resize((ow, oh), PIL_FILTER[filt]))


def _check_launch(dev, shapes, oh, ow, filt, seed, pillow_at):
    from tise_toolbox_amd import device
    assert not any(device.pillow_vertical_first(h, w, oh) for h, w in shapes)        # one launch states Pillow's order
    host, views = _views(dev, shapes, seed)
    got = _ragged(views, oh, ow, filt)
    for i, v in enumerate(views):
        np.testing.assert_array_equal(got[i], _batch(v, oh, ow, filt), err_msg=f"image {i} {shapes[i]} -> {oh}x{ow} {filt}: batch entry")
    for i in pillow_at:
        np.testing.assert_array_equal(got[i], _pillow(host[i], oh, ow, filt), err_msg=f"image {i} {shapes[i]} -> {oh}x{ow} {filt}: Pillow")


# -> (33, ow): up-scale on both sides (SMALLK, dword vertical path), a general horizontal window beside it, both sides
# shrinking, identity on y / on x / on both (for ow = 37), one pixel, one row, one column, and rows of 48 pixels (144 bytes, a
# multiple of 16) at all three addresses: the 16-byte staging loop at 0, the byte loop at 1 and 8
MIXED = [(16, 20), (64, 200), (100, 90), (33, 20), (16, 37), (33, 37), (1, 1), (1, 9), (9, 1), (20, 48), (20, 48), (20, 48), (64, 48)]


@pytest.mark.parametrize("filt", FILTERS)
def test_mixed_list_equals_the_batch_entry_point(cuda_device, filt):
    """Output widths 36..39: 3 * ow mod 4 covers {0, 1, 2, 3} (the dword stores' row tails); SMALLK and general tiles are
    neighbours in one grid."""
    assert {OFFSETS[k % 3] for k, s in enumerate(MIXED) if s == (20, 48)} == {0, 1, 8}
    tails = set()
    for ow in (36, 37, 38, 39):
        tails.add(3 * ow % 4)
        _check_launch(cuda_device, MIXED, 33, ow, filt, seed=ow, pillow_at=(0, 1, 5, 6, 10))
    assert tails == {0, 1, 2, 3}
    # vertical windows of more than three taps beside at most three: the loop over taps and the dword path in one grid
    _check_launch(cuda_device, [(100, 24), (10, 24), (100, 7), (13, 5)], 13, 7, filt, seed=13, pillow_at=(0, 2))


@pytest.mark.parametrize("filt", FILTERS)
def test_every_row_tile_height_through_the_ragged_kernel(cuda_device, filt):
    """The shapes of test_gpu_resize.ROW_TILE_CASES that get a plan, each between two small crops of other tile heights."""
    cases = [c for c in ROW_TILE_CASES[filt] if _row_tile(*c, filt) is not None]
    assert {_row_tile(*c, filt) for c in cases} == {16, 8, 4, 2, 1}
    for h, w, oh, ow in cases:
        _check_launch(cuda_device, [(16, 20), (h, w), (64, 200)], oh, ow, filt, seed=h + w, pillow_at=(1,))


@pytest.mark.parametrize("filt", FILTERS)
def test_eight_register_slots_and_the_refusal_past_them(cuda_device, filt):
    """ow = 682 fills all eight elements per thread (3 * 682 = 2046 <= 2048); ow = 683 is refused before anything runs."""
    from tise_toolbox_amd import _lib
    shapes = [(9, 700), (9, 100), (5, 682), (3, 3)]
    _check_launch(cuda_device, shapes, 5, 682, filt, seed=682, pillow_at=(0, 1))
    _, views = _views(cuda_device, shapes, 683)
    g = _Guarded(cuda_device, len(shapes) * 5 * 683 * 3, 683 * 3, odd=True)
    assert _ragged_status(views, 5, 683, filt, g.ptr) == (_lib.TISE_ERR_UNSUPPORTED, -1)
    g.assert_untouched()


def test_a_refused_size_leaves_the_destination_untouched(cuda_device):
    """(11960, 1000) -> 299 rows has 81 vertical taps over 3000-byte rows: no row tile fits LDS.  The list is refused as a
    whole, naming image 2, and the crops in front of it are not resized either."""
    from tise_toolbox_amd import _lib
    shapes = [(20, 17), (31, 640), (11960, 1000)]
    views = [torch.zeros((h, w, 3), dtype=torch.uint8, device=cuda_device) for h, w in shapes]
    g = _Guarded(cuda_device, 3 * 299 * 299 * 3, 299 * 3, odd=True)
    assert _ragged_status(views, 299, 299, "bilinear", g.ptr) == (_lib.TISE_ERR_UNSUPPORTED, 2)
    g.assert_untouched()


@pytest.mark.parametrize("with_pinned", [True, False])
def test_one_image_past_a_full_launch(cuda_device, with_pinned):
    """RAGGED_CHUNK + 1 sources of one to four pixels a side -> (5, 7): two launches, the second of one image, each with its own
    part of the table and its own destination offset.  The sources cycle through sixteen base crops; images 4095 and 4096 (the
    two sides of the border) and three others are held to Pillow, and every image to its twin of a sixteen-image call."""
    n = RAGGED_CHUNK + 1
    host, base = _views(cuda_device, [(1 + k % 4, 1 + k // 4) for k in range(16)], seed=4097)
    pinned = torch.empty(n * (64 + 4 * 5) + 32, dtype=torch.uint8).pin_memory() if with_pinned else None
    sixteen = _ragged(base, 5, 7, "bilinear", pinned)
    got = _ragged([base[i % 16] for i in range(n)], 5, 7, "bilinear", pinned)
    for i in (0, 1234, RAGGED_CHUNK - 2, RAGGED_CHUNK - 1, RAGGED_CHUNK):
        np.testing.assert_array_equal(got[i], _pillow(host[i % 16], 5, 7, "bilinear"), err_msg=f"image {i}")
    np.testing.assert_array_equal(got, sixteen[np.arange(n) % 16])
