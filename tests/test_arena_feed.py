"""The pipeline the JPEG feed and the crop feed share (tise_toolbox_amd/arena_feed.py: ArenaFeedLoader), every test written once
and run over both loaders: bookkeeping and ``close()`` on the host; on the device a second iteration of one object, a consumer
that walks away, a decode error, the fork hook with a loader of each kind alive, and how long an item stays valid.  Pixels are
compared with Pillow's ``Image.open(f).convert("RGB")`` byte for byte, counters exactly.  What is one feed's own (slots,
kernels, overflow, the CLIs) is in test_jpeg_host / test_gpu_jpeg and test_crop_feed_host / test_gpu_crop_feed."""
import os
import threading

import numpy as np
import pytest
import torch
from PIL import Image, UnidentifiedImageError

from tests import _jpeg_cases

KINDS = ["jpeg", "crop"]


def _feed(kind):
    """(module, loader class) of a feed, its decoder library built."""
    from tise_toolbox_amd import build, crop_feed, jpeg_feed
    if kind == "jpeg":
        build.build_jpeg(force=False, verbose=False)
        return jpeg_feed, jpeg_feed.JpegFeedLoader
    build.build_png(force=False, verbose=False)
    return crop_feed, crop_feed.CropFeedLoader


def _ragged_dir(kind, root, n, seed=0):
    """``n`` files of ``kind`` (JPEG 4:2:0 / RGB PNG), every one of its own size up to 96 x 96; (files, Pillow's pixels)."""
    rng = np.random.default_rng(seed)
    os.makedirs(root, exist_ok=True)
    files, want = [], []
    for i in range(n):
        h, w = int(rng.integers(8, 97)), int(rng.integers(8, 97))
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if kind == "jpeg":
            path = os.path.join(root, f"f_{i:03d}.jpg")
            _jpeg_cases.save_jpeg(img, path, quality=85, subsampling=2)
        else:
            path = os.path.join(root, f"f{i:03d}_cls{i % 3}_{i}.png")
            Image.fromarray(img).save(path)
        files.append(path)
        want.append(np.asarray(Image.open(path).convert("RGB")))
    return files, want


def _feed_threads(kind):
    return [t.name for t in threading.enumerate() if t.name.startswith(f"tise-{kind}-")]


def _closed(ld):
    from tise_toolbox_amd import arena_feed
    return ld._threads == [] and ld._pool is None and ld._arenas == [] and ld not in arena_feed._LIVE


def _as_they_arrive(ld):
    """Every image copied to the host before the next item is asked for; the items' lengths."""
    got, rows = [], []
    for item in ld:
        rows.append(len(item))
        got += [t.cpu().numpy() for t in item]
    return got, rows


def _same(got, want):
    return len(got) == len(want) and all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


# ---- host side ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_close_twice_is_harmless_and_drop_last_of_a_short_directory_is_empty(kind, tmp_path):
    _, loader = _feed(kind)
    files, want = _ragged_dir(kind, str(tmp_path / "d"), 7)
    ld = loader(files, 3, "cpu", workers=2)
    ld.close()                                                                  # never iterated
    got = [t.numpy() for item in ld for t in item]
    assert _same(got, want[:6]) and (ld.native, ld.pillow) == (6, 0)
    ld.close()
    ld.close()
    assert _closed(ld) and _feed_threads(kind) == []
    short = loader(files[:2], 3, "cpu", workers=2)                              # fewer files than a batch, drop-last
    assert len(short) == 0 and len(list(short)) == 0 and (short.native, short.pillow) == (0, 0)
    short.close()


@pytest.mark.parametrize("kind", KINDS)
def test_iter_host_honours_a_callers_item_rows(kind, tmp_path):
    _, loader = _feed(kind)
    files, want = _ragged_dir(kind, str(tmp_path / "d"), 11, seed=1)
    rows = [3, 1, 5, 2]
    ld = loader(files, 4, "cpu", workers=3, drop_last=False, item_rows=rows)
    assert ld.item_rows == rows and ld.starts == [0, 3, 4, 9, 11]
    items = list(ld.iter_host())
    assert [len(it) for it in items] == rows
    assert _same([t.numpy() for it in items for t in it], want) and (ld.native, ld.pillow) == (11, 0)
    with pytest.raises(AssertionError):
        loader(files, 4, "cpu", drop_last=False, item_rows=[3, 1, 5, 1])      # a schedule that does not cover the files


@pytest.mark.parametrize("kind", KINDS)
def test_two_threads_bind_the_decoder_once(kind, monkeypatch):
    mod, _ = _feed(kind)
    monkeypatch.setattr(mod, "_decoder", None)                                  # as in a process that has not bound it yet
    gate, got = threading.Barrier(2), [None, None]

    def bind(i):
        gate.wait()
        got[i] = mod.load_decoder()
    threads = [threading.Thread(target=bind, args=(i,)) for i in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert got[0] is not None and got[0] is got[1] is mod.load_decoder()


# ---- device side -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_second_iteration_and_how_long_an_item_stays_valid(kind, cuda_device, tmp_path):
    """2 * NBUF + 1 loader batches of 3 ragged images, so every arena is refilled twice; then the same object again: the same
    pixels, and its counters run on.

    The first pass copies every item out as it arrives, which both loaders must stand.  The second pass differs by loader,
    because their arena reuse rules do: a JPEG item VIEWS its arena's output buffer, which a later batch overwrites once the
    consumer's stream has passed the point at which it asked for the next item, so it is again compared as it arrives; a crop
    item OWNS its pixels (engine.coalesce_batches holds twenty loader batches of them), so all items are collected first and
    compared after the iteration has ended."""
    _, loader = _feed(kind)
    nb = 2 * loader.NBUF + 1
    files, want = _ragged_dir(kind, str(tmp_path / "d"), 3 * nb, seed=2)
    ld = loader(files, 3, cuda_device, workers=3)
    assert len(ld) == nb
    got, rows = _as_they_arrive(ld)
    assert rows == [3] * nb and _same(got, want) and (ld.native, ld.pillow) == (3 * nb, 0)
    assert _closed(ld)
    if kind == "jpeg":
        got, rows = _as_they_arrive(ld)
    else:
        held = [t for item in ld for t in item]
        torch.cuda.synchronize()
        got = [t.cpu().numpy() for t in held]
    assert _same(got, want) and (ld.native, ld.pillow) == (6 * nb, 0)
    assert _closed(ld) and _feed_threads(kind) == []


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_consumer_walks_away_after_the_first_item(kind, cuda_device, tmp_path):
    _, loader = _feed(kind)
    files, want = _ragged_dir(kind, str(tmp_path / "d"), 21, seed=3)
    ld = loader(files, 3, cuda_device, workers=3)
    it = iter(ld)
    first = [t.cpu().numpy() for t in next(it)]
    assert ld._threads and ld._arenas and not _closed(ld)
    ld.close()                                                                  # the iteration is still suspended at its first item
    assert _closed(ld) and _feed_threads(kind) == []
    it.close()
    assert _same(first, want[:3])
    for item in ld:                                                             # the plain ``break``
        break
    ld.close()
    assert _closed(ld) and _feed_threads(kind) == []
    got, rows = _as_they_arrive(loader(files, 3, cuda_device, workers=3))       # a fresh loader over the same files
    assert rows == [3] * 7 and _same(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_decode_error_surfaces_in_the_consumer_and_leaves_nothing_behind(kind, cuda_device, tmp_path):
    """A file Pillow cannot read in the SECOND batch (the host rejects it; nothing of its batch is launched).  The crop feed
    raises RuntimeError naming the file; the JPEG feed lets Pillow's own exception through."""
    _, loader = _feed(kind)
    files, want = _ragged_dir(kind, str(tmp_path / "d"), 12, seed=4)
    with open(files[4], "wb") as f:
        f.write(b"not an image at all")
    ld = loader(files, 3, cuda_device, workers=2)
    got = []
    if kind == "crop":
        with pytest.raises(RuntimeError, match=os.path.basename(files[4])):
            for item in ld:
                got += [t.cpu().numpy() for t in item]
    else:
        with pytest.raises(UnidentifiedImageError):
            for item in ld:
                got += [t.cpu().numpy() for t in item]
    assert _same(got, want[:3])                                                 # the batch before it arrived whole
    assert _closed(ld) and _feed_threads(kind) == []


@pytest.mark.gpu
def test_fork_hook_closes_live_loaders_of_both_kinds(cuda_device, tmp_path):
    """What os.register_at_fork(before=...) runs, called directly (a process with the GPU open is not forked here): a loader of
    each kind is in the middle of its iteration, both are closed and the page-locked arenas of both are released."""
    from tise_toolbox_amd import arena_feed
    live = []
    for kind in KINDS:
        _, loader = _feed(kind)
        files, want = _ragged_dir(kind, str(tmp_path / kind), 12, seed=5)
        ld = loader(files, 3, cuda_device, workers=2)
        it = iter(ld)
        assert _same([t.cpu().numpy() for t in next(it)], want[:3])
        live.append((ld, it))
    assert all(ld in arena_feed._LIVE and ld._arenas and ld._threads for ld, _ in live)
    arena_feed._close_all()
    assert all(_closed(ld) for ld, _ in live) and not any(_feed_threads(kind) for kind in KINDS)
    for _, it in live:
        it.close()
