"""CPU: the crop feed's host half (tise_toolbox_amd/crop_feed.py, CropFeedLoader.iter_host) over directories of PNGs whose
sizes all differ -- order, drop-last, a short last batch, pixels equal to Pillow's ``Image.open(f).convert("RGB")``
(image_realism/FID/img_data.py:19-25), and the counts of files decoded natively / by Pillow equal to what was planted, so that
no set passes by falling back; an unreadable file raises naming it; no thread survives ``close()``; the CLIs know the flag."""
import os
import threading

import numpy as np
import pytest
import torch

from tests import _png_cases

PALETTE_AT, GRAY_AT, INTERLACED_AT = 7, 19, 31


def _write_interlaced_rgb(path, img):
    """An Adam7-interlaced 8-bit RGB PNG (IHDR interlace = 1) written by hand: Pillow's writer has no such option."""
    import struct
    import zlib
    h, w, _ = img.shape
    raw = b""
    for ys, xs, dy, dx in ((0, 0, 8, 8), (0, 4, 8, 8), (4, 0, 8, 4), (0, 2, 4, 4), (2, 0, 4, 2), (0, 1, 2, 2), (1, 0, 2, 1)):
        sub = img[ys::dy, xs::dx]
        if sub.shape[0] == 0 or sub.shape[1] == 0:
            continue
        for row in sub:
            raw += b"\0" + row.tobytes()
    blob = b"\x89PNG\r\n\x1a\n" + _png_cases._chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 1))
    blob += _png_cases._chunk(b"IDAT", zlib.compress(raw)) + _png_cases._chunk(b"IEND", b"")
    with open(path, "wb") as f:
        f.write(blob)


def _crop_dir(root, n=40, seed=3, planted=True):
    """n PNGs, every one of its own size, RGB and RGBA mixed, written by Pillow (adaptive filters) or by the test writer (chosen
    filters, split IDATs); ``planted``: a palette, a gray and an interlaced file at known positions."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    os.makedirs(root, exist_ok=True)
    files = []
    for i in range(n):
        h, w = int(rng.integers(1, 90)), int(rng.integers(1, 90))
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        f = os.path.join(root, f"img{i:03d}_cls{i % 3}_{i}.png")
        if planted and i == PALETTE_AT:
            Image.fromarray(img).convert("P").save(f)
        elif planted and i == GRAY_AT:
            Image.fromarray(img[..., 0]).save(f)
        elif planted and i == INTERLACED_AT:
            _write_interlaced_rgb(f, img)
        elif i % 4 == 1:
            rgba = np.concatenate([img, rng.integers(0, 256, (h, w, 1), dtype=np.uint8)], axis=2)
            with open(f, "wb") as fh:
                fh.write(_png_cases.write_png(rgba, list(rng.integers(0, 5, h)), idat_sizes=[5, 40]))
        elif i % 4 == 2:
            with open(f, "wb") as fh:
                fh.write(_png_cases.write_png(img, [(i + y) % 5 for y in range(h)]))
        else:
            Image.fromarray(img).save(f)
        files.append(f)
    return files


def _pillow(f):
    from PIL import Image
    return np.asarray(Image.open(f).convert("RGB"))


def _flat(items):
    out = []
    for it in items:
        out.extend([t.numpy() for t in it] if isinstance(it, list) else [t.numpy() for t in it])
    return out


@pytest.mark.parametrize("bs,drop_last", [(6, True), (6, False), (40, True), (1, True), (64, False)])
def test_iter_host_order_pixels_and_counts(tmp_path, bs, drop_last):
    from tise_toolbox_amd import crop_feed
    files = _crop_dir(str(tmp_path / "d"))
    want = [_pillow(f) for f in files]
    ld = crop_feed.CropFeedLoader(files, bs, "cpu", workers=3, drop_last=drop_last)
    items = list(ld.iter_host())
    n_used = (40 // bs) * bs if drop_last else 40
    assert len(ld) == len(items) == (n_used // bs if drop_last else -(-40 // bs))
    assert [len(it) for it in items] == ld.item_rows and sum(ld.item_rows) == n_used
    if not drop_last and 40 % bs:
        assert len(items[-1]) == 40 % bs                                       # the short last batch
    got = _flat(items)
    assert len(got) == n_used
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.uint8 and g.shape == w.shape and np.array_equal(g, w), (i, files[i])
    planted = sum(1 for p in (PALETTE_AT, GRAY_AT, INTERLACED_AT) if p < n_used)
    assert ld.pillow == planted and ld.native == n_used - planted, (ld.native, ld.pillow)
    assert list(iter(ld)) is not None                                           # a CPU device iterates the host road
    ld.close()


def test_subset_only_directory_never_touches_pillow_and_dense_batches_stack(tmp_path):
    from PIL import Image
    from tise_toolbox_amd import crop_feed
    files = _crop_dir(str(tmp_path / "d"), n=23, seed=11, planted=False)
    ld = crop_feed.CropFeedLoader(files, 5, "cpu", workers=2, drop_last=False)
    items = list(ld.iter_host())
    assert ld.pillow == 0 and ld.native == 23 and ld.first_pillow_reason is None
    assert all(isinstance(it, list) for it in items) and [len(it) for it in items] == [5, 5, 5, 5, 3]
    # images of one size: the item is the dense tensor collate_u8 makes
    rng = np.random.default_rng(1)
    same = []
    for i in range(6):
        f = str(tmp_path / f"s{i}_a_{i}.png")
        Image.fromarray(rng.integers(0, 256, (9, 13, 3), dtype=np.uint8)).save(f)
        same.append(f)
    ld = crop_feed.CropFeedLoader(same, 3, "cpu", workers=2)
    items = list(ld.iter_host())
    assert ld.pillow == 0 and ld.native == 6
    assert all(isinstance(it, torch.Tensor) and tuple(it.shape) == (3, 9, 13, 3) for it in items)
    assert np.array_equal(torch.cat(items).numpy(), np.stack([_pillow(f) for f in same]))


def test_many_decode_threads_share_no_inflate_state(tmp_path):
    """16 decode threads at once, on both entries the feed calls (the complete decode and inflate-into-a-slot), over 300
    subset files of compressible content, several rounds: every file is decoded natively and equals Pillow.  libdeflate's
    decompressor holds the tables of the stream it is decoding, so the host library keeps one per THREAD; one shared by the
    threads made a few files of every hundred fail their zlib check and go to Pillow (or worse)."""
    import ctypes
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    from tise_toolbox_amd import crop_feed
    rng = np.random.default_rng(23)
    files = []
    for i in range(300):
        h, w = int(rng.integers(16, 200)), int(rng.integers(16, 200))
        img = (np.add.outer(np.arange(h) * (i % 7 + 1), np.arange(w) * 3)[..., None] + rng.integers(0, 24, (h, w, 3))).astype(np.uint8)
        f = str(tmp_path / f"t{i:03d}_c_{i}.png")
        Image.fromarray(img).save(f)
        files.append(f)
    want = [_pillow(f) for f in files]
    for _ in range(3):
        ld = crop_feed.CropFeedLoader(files, 50, "cpu", workers=16, drop_last=False)
        got = _flat(list(ld.iter_host()))
        assert (ld.native, ld.pillow) == (300, 0), (ld.native, ld.pillow, ld.first_pillow_reason)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
    lib = crop_feed.load_decoder()

    def slot(i):
        blob = open(files[i], "rb").read()
        h, w = want[i].shape[:2]
        sb = int(lib.tise_png_slot_bytes(h, w, 3))
        buf, sc = np.zeros(sb, dtype=np.uint8), np.empty(int(lib.tise_png_scratch_bytes(h, w, len(blob))), dtype=np.uint8)
        mode = ctypes.c_int(-1)
        rc = lib.tise_png_inflate_slot(blob, len(blob), buf.ctypes.data, sb, h, w, sc.ctypes.data, sc.size, None, None, ctypes.byref(mode))
        return rc, mode.value
    with ThreadPoolExecutor(16) as pool:
        for _ in range(3):
            assert set(pool.map(slot, range(300))) == {(crop_feed.PNG_OK, 3)}


def test_crc_doubt_goes_to_pillow_and_unreadable_file_raises_naming_it(tmp_path):
    from tise_toolbox_amd import crop_feed
    files = _crop_dir(str(tmp_path / "d"), n=8, seed=5, planted=False)
    blob = bytearray(open(files[3], "rb").read())
    pos = blob.index(b"IEND") + 4                                               # IEND's CRC: Pillow never reads it, the native parser refuses
    blob[pos] ^= 0xff
    open(files[3], "wb").write(bytes(blob))
    want = _pillow(files[3])
    ld = crop_feed.CropFeedLoader(files, 4, "cpu", workers=2)
    got = _flat(list(ld.iter_host()))
    assert np.array_equal(got[3], want) and (ld.native, ld.pillow) == (7, 1)
    assert os.path.basename(files[3]) in ld.first_pillow_reason
    open(files[5], "wb").write(b"not an image at all")
    ld = crop_feed.CropFeedLoader(files, 4, "cpu", workers=2)
    with pytest.raises(RuntimeError, match=os.path.basename(files[5])):
        list(ld.iter_host())
    os.remove(files[6])
    ld = crop_feed.CropFeedLoader(files[6:], 2, "cpu", workers=2)
    with pytest.raises(RuntimeError, match=os.path.basename(files[6])):
        list(ld.iter_host())


def test_no_thread_survives_close(tmp_path):
    from tise_toolbox_amd import crop_feed
    files = _crop_dir(str(tmp_path / "d"), n=30, seed=2, planted=False)
    before = {t.ident for t in threading.enumerate()}
    ld = crop_feed.CropFeedLoader(files, 4, "cpu", workers=4)
    it = ld.iter_host()
    next(it)
    next(it)
    it.close()                                                                  # the consumer walks away in the middle
    ld.close()
    left = [t.name for t in threading.enumerate() if t.ident not in before]
    assert left == [], left


def test_probe_use_native_and_arena_size(tmp_path):
    from tise_toolbox_amd import crop_feed
    files = _crop_dir(str(tmp_path / "d"), n=40, seed=3)
    assert crop_feed.probe_file(files[0]) and not crop_feed.probe_file(files[PALETTE_AT])
    assert not crop_feed.probe_file(files[GRAY_AT]) and not crop_feed.probe_file(files[INTERLACED_AT])
    assert not crop_feed.probe_file(str(tmp_path / "missing.png"))
    assert crop_feed.use_native(files, None) and crop_feed.use_native(files, "native")
    assert not crop_feed.use_native(files, "dataloader") and not crop_feed.use_native([], "native")
    assert not crop_feed.use_native(files[PALETTE_AT:], None) and crop_feed.use_native(files[PALETTE_AT:], "native")
    a = crop_feed.pick_arena_bytes(files, 8)
    assert a % 4096 == 0 and (1 << 20) <= a <= (1 << 30)


def test_clis_know_the_flag():
    from tise_toolbox_amd import fid_score, object_centric_inception_score as ois
    p = fid_score._build_parser()
    assert p.parse_args(["--path2", "x"]).crop_feed is None
    assert p.parse_args(["--path2", "x", "--crop-feed", "native"]).crop_feed == "native"
    assert p.parse_args(["--path2", "x", "--crop-feed", "dataloader"]).crop_feed == "dataloader"
    with pytest.raises(SystemExit):
        p.parse_args(["--path2", "x", "--crop-feed", "ring"])
    assert ois.parse_args([]).crop_feed is None and ois.parse_args(["--crop-feed", "native"]).crop_feed == "native"


def test_ragged_entries_reject_bad_arguments_without_a_gpu():
    """Both ragged entries check every size they index with on the host, before any HIP call: fake device addresses, each call
    has exactly one defect (a launch would need a device this test does not have)."""
    import ctypes
    from tise_toolbox_amd import _lib
    lib = _lib.load()
    bad, uns = _lib.TISE_ERR_INVALID_ARG, _lib.TISE_ERR_UNSUPPORTED
    A, D, T = 0x7f0000000000, 0x7f0000100000, 0x7f0000200000

    def unf(arena=A, arena_bytes=1 << 16, offs=(0, 4096), hwm=((4, 5, 3), (3, 2, 4)), outs=(0, 64), dst=D, dst_bytes=1 << 12,
            table=T, table_bytes=1 << 10, pinned=None, n=None):
        n = len(offs) if n is None else n
        so = np.asarray(offs, dtype=np.int64)
        hm = np.asarray(hwm, dtype=np.int32).reshape(-1, 3)
        oo = np.asarray(outs, dtype=np.int64)
        return lib.tise_png_unfilter_ragged_rgb8(arena, arena_bytes, n, so.ctypes.data, hm.ctypes.data, oo.ctypes.data, dst, dst_bytes,
                                                 table, table_bytes, pinned, None)
    assert unf(n=0) == _lib.TISE_OK
    cases = dict(
        null_arena=dict(arena=None), null_dst=dict(dst=None), null_table=dict(table=None), negative_n=dict(n=-1),
        misaligned_arena=dict(arena=A + 2), misaligned_table=dict(table=T + 4), misaligned_pinned=dict(pinned=A + 4),
        misaligned_offset=dict(offs=(0, 4098)), negative_offset=dict(offs=(-64, 4096)),
        zero_h=dict(hwm=((0, 5, 3), (3, 2, 4))), zero_w=dict(hwm=((4, 0, 3), (3, 2, 4))), huge_h=dict(hwm=((65536, 5, 3), (3, 2, 4))),
        mode_1=dict(hwm=((4, 5, 1), (3, 2, 4))), mode_5=dict(hwm=((4, 5, 3), (3, 2, 5))),
        row_over_limit_rgb=dict(hwm=((1, 2731, 3), (3, 2, 4)), arena_bytes=1 << 20, dst_bytes=1 << 20),      # 3 * 2731 + 1 = 8194
        row_over_limit_rgba=dict(hwm=((1, 2048, 4), (3, 2, 4)), arena_bytes=1 << 20, dst_bytes=1 << 20),     # 4 * 2048 + 1 = 8193
        slot_beyond_arena=dict(offs=(0, (1 << 16) - 64)),                          # header fits, payload does not
        slack_beyond_arena=dict(offs=(0, 4096), arena_bytes=4096 + 64 + 3 * 9 + 7),  # payload fits, the 8 bytes of staging slack do not
        mode0_beyond_arena=dict(hwm=((4, 5, 3), (3, 2, 0)), arena_bytes=4096 + 64 + 17),
        out_beyond_dst=dict(outs=(0, (1 << 12) - 17)), negative_out=dict(outs=(-1, 64)),
        table_too_small=dict(table_bytes=95), negative_arena=dict(arena_bytes=-1),
    )
    for name, kw in cases.items():
        assert unf(**kw) == bad, name
    assert unf(offs=(0,) * ((1 << 20) + 1), hwm=((1, 1, 3),) * ((1 << 20) + 1), outs=(0,) * ((1 << 20) + 1), table_bytes=1 << 30) == uns

    S = 0x7f0000400000

    def rs(ptrs=(S, S + 999), hs=(20, 31), ws=(17, 640), dst=D, oh=299, ow=299, filt=0, wsd=T, ws_bytes=1 << 20, pinned=None, n=None):
        n = len(ptrs) if n is None else n
        pp = np.asarray([p or 0 for p in ptrs], dtype=np.uint64)
        hh, ww = np.asarray(hs, dtype=np.int32), np.asarray(ws, dtype=np.int32)
        badi = ctypes.c_int64(-7)
        st = lib.tise_resize_ragged_u8(pp.ctypes.data, hh.ctypes.data, ww.ctypes.data, n, dst, oh, ow, filt, wsd, ws_bytes, pinned,
                                       ctypes.byref(badi), None)
        return st, badi.value
    assert rs(n=0) == (_lib.TISE_OK, -1)
    for name, kw in dict(null_dst=dict(dst=None), null_ws=dict(wsd=None), negative_n=dict(n=-1), zero_oh=dict(oh=0), zero_ow=dict(ow=0),
                         filter_2=dict(filt=2), misaligned_ws=dict(wsd=T + 8), misaligned_pinned=dict(pinned=A + 8),
                         ws_too_small=dict(ws_bytes=2 * (64 + 4 * 299) + 15)).items():
        assert rs(**kw) == (bad, -1), name
    assert rs(ptrs=(S, None)) == (bad, 1)
    assert rs(hs=(20, 0)) == (bad, 1) and rs(ws=(-3, 640)) == (bad, 0)
    assert rs(ow=700)[0] == uns                                                 # ow * 3 > 2048: no kernel instance
    # a size the plan builder refuses (no row tile fits LDS: 81 vertical taps over rows of 3000 bytes), named by index
    assert rs(hs=(20, 31, 11960), ws=(17, 640, 1000), ptrs=(S, S, S)) == (uns, 2)
    assert rs(hs=(11960, 31), ws=(1000, 640), filt=1) == (uns, 0)
