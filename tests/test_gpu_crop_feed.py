"""The crop feed on the device (tise_toolbox_amd/crop_feed.py): PNGs of DIFFERENT sizes -> inflate-only slots packed into one
arena -> tise_png_unfilter_ragged_rgb8 (csrc/png_unfilter.hip), one launch for all of them == Pillow's
``Image.open(f).convert("RGB")`` byte for byte; lists of images of different sizes -> tise_resize_ragged_u8 (csrc/resize.hip),
one launch == Pillow's ``Image.resize`` and the per-image kernel byte for byte; the loader against Pillow; and the CLIs with
``--crop-feed native`` against the DataLoader route, value for value."""
import ctypes
import io
import os

import numpy as np
import pytest
import torch

from tests import _png_cases
from tests.test_crop_feed_host import GRAY_AT, INTERLACED_AT, PALETTE_AT, _crop_dir, _pillow

pytestmark = pytest.mark.gpu


def _pillow_rgb(blob):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"))


def _pack(blobs, force_pixels=()):
    """Host half of the feed on file images of any sizes: (arena, slot offsets, (h, w, mode) rows).  ``force_pixels``: indices
    that enter as Pillow-decoded pixels (mode 0), as files outside the native subset do."""
    from tise_toolbox_amd import crop_feed
    lib = crop_feed.load_decoder()
    offs, hwm, parts, pos = [], [], [], 0
    for i, blob in enumerate(blobs):
        rc, w, h, ch = crop_feed.probe(blob)
        assert rc == 0, (i, rc)
        if i in force_pixels:
            px = _pillow_rgb(blob)
            slot = np.zeros(64 + ((px.nbytes + 8 + 63) & ~63), dtype=np.uint8)
            slot[64:64 + px.nbytes] = px.reshape(-1)
            mode = 0
        else:
            sb = int(lib.tise_png_slot_bytes(h, w, ch if w * ch + 1 <= crop_feed.ROW_MAX else 0))
            slot = np.full(sb, 0xa5, dtype=np.uint8)
            sc = np.zeros(int(lib.tise_png_scratch_bytes(h, w, len(blob))) + 1024, dtype=np.uint8)
            m = ctypes.c_int(-1)
            rc = lib.tise_png_inflate_slot(blob, len(blob), slot.ctypes.data, sb, h, w, sc.ctypes.data, sc.size, None, None, ctypes.byref(m))
            assert rc == 0, (i, rc)
            mode = m.value
        offs.append(pos)
        hwm.append((h, w, mode))
        parts.append(slot)
        pos += slot.size
    return np.concatenate(parts), np.asarray(offs, dtype=np.int64), np.asarray(hwm, dtype=np.int32)


def _unfilter_ragged(arena, offs, hwm, out_align=1, pinned=False):
    """One launch; the outputs are packed ``out_align`` apart with 0x5a guard bytes around them.  Returns the images and checks
    the guards."""
    from tise_toolbox_amd import _lib
    dev = torch.device("cuda", 0)
    n = len(offs)
    oo, pos = [], 5 if out_align == 1 else 0
    for h, w, _ in hwm:
        oo.append(pos)
        pos += int(h) * int(w) * 3 + 3
        pos = (pos + out_align - 1) // out_align * out_align
    oo = np.asarray(oo, dtype=np.int64)
    a = torch.from_numpy(arena).to(dev)
    out = torch.full((pos + 64,), 0x5a, dtype=torch.uint8, device=dev)
    table = torch.empty(48 * n, dtype=torch.uint8, device=dev)
    pin = torch.empty(48 * n, dtype=torch.uint8).pin_memory() if pinned else None
    _lib.call("tise_png_unfilter_ragged_rgb8", a.data_ptr(), a.numel(), n, offs.ctypes.data, hwm.ctypes.data, oo.ctypes.data,
              out.data_ptr(), out.numel(), table.data_ptr(), table.numel(), pin.data_ptr() if pinned else None,
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    flat = out.cpu().numpy()
    imgs, covered = [], np.zeros(flat.size, dtype=bool)
    for (h, w, _), o in zip(hwm, oo):
        imgs.append(flat[o:o + h * w * 3].reshape(h, w, 3))
        covered[o:o + h * w * 3] = True
    assert (flat[~covered] == 0x5a).all(), "bytes outside the images were written"
    return imgs


def _unfilter_cases():
    rng = np.random.default_rng(2024)
    blobs, pixels = [], set()

    def add(h, w, bpp, filters, as_pixels=False, **kw):
        img = rng.integers(0, 256, (h, w, bpp), dtype=np.uint8)
        if as_pixels:
            pixels.add(len(blobs))
        blobs.append(_png_cases.write_png(img, filters, **kw))
    for bpp in (3, 4):
        add(1, 1, bpp, [4])
        add(1, 37, bpp, [1])                                                    # 1 x N
        add(41, 1, bpp, [y % 5 for y in range(41)])                             # N x 1
        for w in (1, 2, 3, 4, 5, 6, 7):                                         # w * 3 mod 4 in all residues (and w * 4)
            add(9, w, bpp, list(rng.integers(0, 5, 9)))
        for h in (63, 64, 65, 129):                                             # around the 64-row block, two blocks and a row
            add(h, 50 + h % 7, bpp, [(y * 3 + h) % 5 for y in range(h)])
        for ft in range(5):                                                     # every filter type on every row
            add(70, 33, bpp, [ft] * 70)
        add(130, 67, bpp, list(rng.integers(0, 5, 130)), idat_sizes=[1, 2, 3, 50, 7])
        add(24, 19, bpp, None, as_pixels=True)                                  # a mode-0 slot between filtered ones
    add(3, 2730, 3, [4, 3, 1])                                                  # a row of 3 * 2730 + 1 = 8191 bytes
    add(5, 2047, 4, [2, 4, 3, 1, 0])                                            # 8189
    add(4, 2048, 4, [4, 3, 2, 1])                                               # 8193: over the limit, arrives as mode 0
    add(2, 2731, 3, [4, 1])                                                     # 8194: over the limit, arrives as mode 0
    add(200, 256, 3, list(rng.integers(0, 5, 200)))
    add(256, 256, 4, list(rng.integers(0, 5, 256)))
    return blobs, pixels


@pytest.mark.parametrize("out_align,pinned", [(1, False), (16, True)])
def test_ragged_unfilter_equals_pillow_in_one_mixed_launch(cuda_device, out_align, pinned):
    blobs, pixels = _unfilter_cases()
    want = [_pillow_rgb(b) for b in blobs]
    arena, offs, hwm = _pack(blobs, force_pixels=pixels)
    modes = hwm[:, 2].tolist()
    assert set(modes) == {0, 3, 4}
    assert modes[-4] == 0 and modes[-3] == 0 and modes[-6] == 3 and modes[-5] == 4          # the rows over the limit came as pixels
    assert all(modes[i] == 0 for i in pixels)
    got = _unfilter_ragged(arena, offs, hwm, out_align, pinned)
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g.shape != w.shape or not np.array_equal(g, w)]
    assert not bad, [(i, hwm[i].tolist()) for i in bad]


def _resize_sources(sizes, seed, dev, misalign=True):
    """Device images of the given (h, w) as views at ODD byte offsets of one buffer (what a feed's packed output gives)."""
    rng = np.random.default_rng(seed)
    host = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    total = sum(im.size + 17 for im in host) + 64
    buf = torch.empty(total, dtype=torch.uint8, device=dev)
    views, pos = [], 1 if misalign else 0
    for k, im in enumerate(host):
        v = buf[pos:pos + im.size].view(im.shape)
        v.copy_(torch.from_numpy(im))
        views.append(v)
        pos += im.size + (1 + 2 * (k % 8) if misalign else 0)
        if not misalign:
            pos = (pos + 15) & ~15
    return host, views


RESIZE_SIZES = [(427, 640), (640, 427), (20, 17), (400, 100), (100, 400), (299, 50), (50, 299), (299, 299), (299, 640), (700, 299),
                (1, 1), (3, 500), (500, 3), (1, 300), (298, 300), (64, 64), (256, 256), (33, 71), (1200, 900), (480, 4), (480, 5)]


@pytest.mark.parametrize("misalign", [True, False])
def test_ragged_resize_equals_pillow_and_the_per_image_kernel(cuda_device, misalign):
    from PIL import Image
    from tise_toolbox_amd import device
    host, views = _resize_sources(RESIZE_SIZES, 7, cuda_device, misalign)
    assert any(v.data_ptr() % 16 for v in views) == misalign
    got = device.resize_ragged_u8(views, (299, 299))
    assert tuple(got.shape) == (len(host), 299, 299, 3)
    g = got.cpu().numpy()
    for i, im in enumerate(host):
        want = np.asarray(Image.fromarray(im).resize((299, 299), Image.BILINEAR))
        assert np.array_equal(g[i], want), ("pillow", i, im.shape[:2])
        one = device.resize_u8_only(views[i].contiguous().unsqueeze(0), (299, 299))[0]
        assert torch.equal(got[i], one), ("per-image", i, im.shape[:2])
    # BICUBIC to 224 (the CLIP preprocess' filter), the same list
    gb = device.resize_ragged_u8(views, (224, 224), filter="bicubic").cpu().numpy()
    for i, im in enumerate(host):
        want = np.asarray(Image.fromarray(im).resize((224, 224), Image.BICUBIC))
        assert np.array_equal(gb[i], want), ("bicubic", i, im.shape[:2])
    # into a caller's buffer, and a list of one
    out = torch.zeros((2, 299, 299, 3), dtype=torch.uint8, device=cuda_device)
    assert device.resize_ragged_u8(views[:2], (299, 299), out=out) is out and torch.equal(out, got[:2])
    assert torch.equal(device.resize_ragged_u8(views[5:6], (299, 299))[0], got[5])


def test_ragged_resize_refuses_a_size_before_anything_is_enqueued(cuda_device):
    from tise_toolbox_amd import _lib, device
    ok = torch.zeros((30, 40, 3), dtype=torch.uint8, device=cuda_device)
    huge = torch.zeros((11960, 1000, 3), dtype=torch.uint8, device=cuda_device)          # 81 vertical taps over 3000-byte rows: no row tile fits LDS
    out = torch.full((3, 299, 299, 3), 0x5a, dtype=torch.uint8, device=cuda_device)
    with pytest.raises(_lib.TiseStatusError, match="image 2 of the batch") as e:
        device.resize_ragged_u8([ok, ok, huge], (299, 299), out=out)
    assert e.value.status == _lib.TISE_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == 0x5a).all())                                                       # nothing ran
    with pytest.raises(_lib.TiseStatusError):                                              # the per-image kernel refuses the same size
        device.resize_u8_only(huge.unsqueeze(0), (299, 299))
    with pytest.raises(ValueError):
        device.resize_ragged_u8([], (299, 299))


def test_more_sizes_in_one_call_than_the_plan_cache_holds(cuda_device):
    """9 000 images of 9 000 different sizes in ONE call (the plan cache holds 8 192): the call is cut into launches whose plans
    cannot evict each other, and every image still equals Pillow's resize."""
    from PIL import Image
    from tise_toolbox_amd import device
    sizes = [(h, w) for h in range(1, 101) for w in range(1, 91)]
    assert len(set(sizes)) == 9000
    rng = np.random.default_rng(9)
    order = rng.permutation(len(sizes))
    sizes = [sizes[i] for i in order]
    host, views = _resize_sources(sizes, 10, cuda_device)
    got = device.resize_ragged_u8(views, (16, 12)).cpu().numpy()
    for i in list(range(0, 9000, 7)) + list(range(8990, 9000)):
        want = np.asarray(Image.fromarray(host[i]).resize((12, 16), Image.BILINEAR))
        assert np.array_equal(got[i], want), (i, sizes[i])


def test_features_from_u8_list_takes_device_views_and_equals_per_image_resizes(cuda_device):
    """The network input of a ragged list is the per-image resize's, whatever the crops' alignment: pool3 rows bit for bit."""
    from tise_toolbox_amd import device
    from tise_toolbox_amd.engine import RealismEngine
    eng = RealismEngine(dims=2048, seed=0)
    sizes = [(64, 48), (120, 90), (33, 71), (200, 17), (17, 200), (299, 299), (5, 5)]
    _, views = _resize_sources(sizes, 3, cuda_device)
    fa, _ = eng.features_from_u8_list(views)
    u8 = torch.cat([device.resize_u8_only(v.contiguous().unsqueeze(0), (299, 299)) for v in views])
    fb, _ = eng._trunk_u8(u8) if eng._u8_stem else (None, None)
    if fb is not None:
        assert torch.equal(fa, fb)


@pytest.mark.timeout(600)
def test_loader_on_the_device_equals_pillow(cuda_device, tmp_path):
    from PIL import Image
    from tise_toolbox_amd import crop_feed
    files = _crop_dir(str(tmp_path / "d"))
    want = [_pillow(f) for f in files]
    planted = (PALETTE_AT, GRAY_AT, INTERLACED_AT)
    for bs, drop_last, arena in ((6, False, None), (7, True, None), (40, False, None), (5, False, 16384), (64, False, None)):
        ld = crop_feed.CropFeedLoader(files, bs, cuda_device, workers=4, chunk=3, drop_last=drop_last, arena_bytes=arena)
        got = []
        for item in ld:
            assert isinstance(item, list) and all(t.is_cuda and t.dtype == torch.uint8 for t in item)
            got.extend(t.cpu().numpy() for t in item)
        n_used = (40 // bs) * bs if drop_last else 40
        assert len(got) == n_used, (bs, len(got))
        for i in range(n_used):
            assert got[i].shape == want[i].shape and np.array_equal(got[i], want[i]), (bs, i, files[i])
        n_pl = sum(1 for p in planted if p < n_used)
        assert (ld.native, ld.pillow) == (n_used - n_pl, n_pl), (bs, ld.native, ld.pillow)
        assert (ld.alone > 0) == (arena is not None), (bs, ld.alone)                      # the small arena overflows, the default never
        assert "crop feed" in ld.feed_line(1.0) and not ld._threads and not ld._arenas
    # items stay valid while later batches are produced (engine.coalesce_batches holds many of them): collect first, compare after
    ld = crop_feed.CropFeedLoader(files, 3, cuda_device, workers=4, drop_last=False)
    held = [t for item in ld for t in item]
    torch.cuda.synchronize()
    assert all(np.array_equal(t.cpu().numpy(), w) for t, w in zip(held, want))
    # images of one size: dense items
    rng = np.random.default_rng(1)
    same = []
    for i in range(10):
        f = str(tmp_path / f"s{i}_a_{i}.png")
        Image.fromarray(rng.integers(0, 256, (19, 23, 3), dtype=np.uint8)).save(f)
        same.append(f)
    ld = crop_feed.CropFeedLoader(same, 4, cuda_device, workers=2)
    items = list(ld)
    assert [tuple(it.shape) for it in items] == [(4, 19, 23, 3)] * 2 and ld.pillow == 0
    assert np.array_equal(torch.cat(items).cpu().numpy(), np.stack([_pillow(f) for f in same[:8]]))
    # an unreadable file raises in the consumer, naming the file, and leaves no thread behind
    open(files[9], "wb").write(b"\x89PNG\r\n\x1a\n garbage")
    ld = crop_feed.CropFeedLoader(files, 6, cuda_device, workers=3, drop_last=False)
    with pytest.raises(RuntimeError, match=os.path.basename(files[9])):
        list(ld)
    assert not ld._threads and ld._pool is None


def _crop_dirs(tmp_path, n_gen=46, n_ref=53):
    """Two crop directories ({stem}_{class}_{k}.png, every crop its own size, RGB and RGBA, only native-subset files)."""
    from PIL import Image
    from tests import _cases
    classes = ["dog", "traffic light", "cup"]
    pool = _cases.smooth_images(16, 200, 200, seed=17)
    out = []
    for side, n, seed in (("ref", n_ref, 1), ("gen", n_gen, 2)):
        d = tmp_path / side
        d.mkdir()
        rng = np.random.default_rng(seed)
        for k in range(n):
            h, w = int(rng.integers(16, 200)), int(rng.integers(16, 200))
            im = np.roll(pool[k % 16], 3 * k + seed, axis=1)[:h, :w]
            f = d / f"im{seed}_{k}_{classes[k % 3]}_{k}.png"
            if k % 5 == 0:
                rgba = np.concatenate([im, np.full((h, w, 1), 200, np.uint8)], axis=2)
                f.write_bytes(_png_cases.write_png(rgba, [(k + y) % 5 for y in range(h)]))
            else:
                Image.fromarray(im).save(f)
        out.append(str(d))
    return out


@pytest.mark.timeout(1500)
def test_clis_give_the_dataloader_routes_values(cuda_device, tmp_path, capfd):
    """Synthetic weights, ragged crop directories: plain FID with --crop-feed native == --png-feed dataloader exactly;
    --per-class with the flag unset (native) == --crop-feed dataloader for every class; O-IS identical on both routes; two
    ranks on this GPU reproduce the one-process per-class values (as test_ragged_crops_one_trunk_pass_and_per_class_fid)."""
    from tests.test_gpu_pipeline import _run_ranks
    from tise_toolbox_amd import feeds, fid_score, object_centric_inception_score as ois
    ref, gen = _crop_dirs(tmp_path)
    base = ["--batch-size", "8", "--path1", ref, "--path2", gen, "--label", "O-FID", "--num-classes", "80", "--num-workers", "0",
            "--synthetic-weights"]
    capfd.readouterr()
    a = fid_score.main(base + ["--crop-feed", "native"])
    err = capfd.readouterr().err
    assert err.count("[tise] crop feed:") == 2 and "falling back" not in err, err
    assert feeds.last.kind == "crop"
    ld = feeds.last.loader
    assert (ld.native, ld.pillow, ld.alone) == (40, 0, 0)                                   # 46 files, batch 8, drop-last
    b = fid_score.main(base + ["--png-feed", "dataloader"])
    assert "crop feed" not in capfd.readouterr().err
    print("O-FID native", a, "dataloader", b)
    assert a == b
    # --per-class: flag unset -> the native feed (the first file probes as a native-subset PNG)
    pa = fid_score.main(base + ["--per-class"])
    err = capfd.readouterr().err
    assert err.count("[tise] crop feed:") == 2, err
    assert feeds.last.kind == "crop"
    ld = feeds.last.loader
    assert (ld.native, ld.pillow) == (46, 0)                                                # every crop is used
    pb = fid_score.main(base + ["--per-class", "--crop-feed", "dataloader"])
    assert "crop feed" not in capfd.readouterr().err
    pc = fid_score.main(base + ["--per-class", "--crop-feed", "native"])
    print("per-class native", dict(pa), "dataloader", dict(pb))
    assert list(pa) == list(pb) == ["cup", "dog", "traffic light"] and dict(pa) == dict(pb) == dict(pc)
    # O-IS
    ia = ois.main(["--image_dir", gen, "--gpu_id", "0", "--synthetic-weights"])
    assert "[tise] crop feed:" in capfd.readouterr().err
    assert feeds.last.kind == "crop" and (feeds.last.loader.native, feeds.last.loader.pillow) == (46, 0)
    ib = ois.main(["--image_dir", gen, "--gpu_id", "0", "--synthetic-weights", "--crop-feed", "dataloader"])
    assert "crop feed" not in capfd.readouterr().err
    ic = ois.main(["--image_dir", gen, "--gpu_id", "0", "--synthetic-weights", "--crop-feed", "native"])
    print("O-IS native", ia, "dataloader", ib)
    assert ia == ib == ic
    # two ranks, one GPU
    outw = tmp_path / "pc_2.txt"
    res = _run_ranks(2, base + ["--per-class", "--saved_file", str(outw)], tmp_path, timeout=500)
    assert all(rc == 0 for rc, _ in res), res
    assert "[tise] crop feed: 23 images" in res[0][1] and "0 by Pillow" in res[0][1], res[0][1]
    lines = outw.read_text().splitlines()
    got = {ln[len("O-FID["):ln.index("]")]: float(ln.split("]: ")[1].split()[0]) for ln in lines if ln.startswith("O-FID[")}
    assert list(got) == list(pa)
    for c in pa:
        # N << d: the shards change the fp64 summation order of S (tests/test_gpu_pipeline.py, the same bound)
        assert abs(got[c] - pa[c]) <= 1e-9 * max(1.0, abs(pa[c])) + 1e-5, (c, got[c], pa[c])
    outp = tmp_path / "fid_2.txt"
    res = _run_ranks(2, base + ["--crop-feed", "native", "--saved_file", str(outp)], tmp_path, timeout=500)
    assert all(rc == 0 for rc, _ in res), res
    assert abs(float(outp.read_text().split()[1]) - a) <= 1e-9 * max(1.0, abs(a)) + 1e-5
