"""GPU: tise_jpeg_reconstruct_rgb8 (csrc/jpeg_idct.hip) and the JPEG feed against Pillow and the host decoder, byte for byte;
the CLIs' statistics with --jpeg-feed native against the path it replaces, bit for bit."""
import ctypes
import os

import numpy as np
import pytest
import torch
from PIL import Image

from . import _cases, _jpeg_cases as jc

SLOT_HDR = 256


def _slots(jf, blobs, slot_bytes=None):
    """Host arena of one slot per file (entropy-decoded natively; asserts that), its stride."""
    lib = jf.load_decoder()
    need = []
    for b in blobs:
        rc, w, h, lay = jf.probe(b)
        assert rc == 0
        need.append(int(lib.tise_jpeg_slot_bytes(w, h, lay)))
    sb = slot_bytes or (max(need) + 15) & ~15
    arena = np.zeros((len(blobs), sb), dtype=np.uint8)
    for i, b in enumerate(blobs):
        assert lib.tise_jpeg_entropy_decode(b, len(b), arena[i].ctypes.data, sb, None, None) == 0
    return arena, sb


PAD = 256                                  # canary bytes on either side of every device buffer (a multiple of 16)
CANARY_DST, CANARY_WS, CANARY_SLOTS = 0xAB, 0xE7, 0x5A


class _Guarded:
    """The slots of one arena in HBM, inside a larger allocation of canary bytes, for any number of guarded launches."""

    def __init__(self, arena, sb, device_arena=None):
        """``device_arena``: what the DEVICE holds when it is to differ from the host copy the entry point validates."""
        self.arena, self.sb, self.n = arena, sb, arena.shape[0]
        self.dev = torch.device("cuda", 0)
        nbytes = self.n * sb
        self.raw_big = torch.full((PAD + nbytes + PAD,), CANARY_SLOTS, dtype=torch.uint8, device=self.dev)
        self.raw = self.raw_big[PAD:PAD + nbytes]
        self.raw.copy_(torch.from_numpy((arena if device_arena is None else device_arena).reshape(-1)))
        self.before = self.raw_big.clone()                                     # the slots are inputs: they must come back unchanged
        assert self.raw.data_ptr() % 16 == 0

    def run(self, sizes, align=16, residue=0, ws_poison=0xCD, pinned=False, stream=None, packed_headers=False):
        """One tise_jpeg_reconstruct_rgb8 over the arena -> [(h, w, 3) arrays].  ``dst`` and the workspace are sub-views of larger
        allocations: ``dst`` at an address ``residue`` mod 4, exactly the extent of the images ``align`` apart; the workspace 16-byte
        aligned, exactly what tise_jpeg_workspace_bytes answers, pre-filled with ``ws_poison``.  Afterwards every byte around them,
        the gaps between the images and the slots must be what they were.  ``pinned``: the launch's table goes through page-locked
        memory of the caller (the product's path); ``stream``: a side stream, the read-back waits for its event;
        ``packed_headers``: the host headers come from a copy of their own, 256 bytes apart."""
        from tise_toolbox_amd import _lib
        n, sb, dev = self.n, self.sb, self.dev
        offs, pos = jc.plan_offsets(sizes, align)
        out_big = torch.full((PAD + residue + pos + PAD,), CANARY_DST, dtype=torch.uint8, device=dev)
        dst = out_big[PAD + residue:PAD + residue + pos]
        wsb = ctypes.c_size_t()
        _lib.call("tise_jpeg_workspace_bytes", n, sb, ctypes.byref(wsb))
        ws_big = torch.full((PAD + wsb.value + PAD,), CANARY_WS, dtype=torch.uint8, device=dev)
        ws = ws_big[PAD:PAD + wsb.value]
        ws.fill_(ws_poison)
        assert ws.data_ptr() % 16 == 0 and dst.data_ptr() % 4 == residue and ws.numel() == wsb.value
        hdrs, hstride = (np.ascontiguousarray(self.arena[:, :SLOT_HDR]), SLOT_HDR) if packed_headers else (self.arena, sb)
        table = torch.empty(n * 64, dtype=torch.uint8).pin_memory() if pinned else None
        cur = torch.cuda.current_stream(dev)
        if stream is not None:
            stream.wait_stream(cur)                                            # the fills above ran on the current stream
        _lib.call("tise_jpeg_reconstruct_rgb8", self.raw.data_ptr(), n, sb, hdrs.ctypes.data, hstride, offs.ctypes.data, dst.data_ptr(), pos,
                  ws.data_ptr(), wsb.value, table.data_ptr() if pinned else None, (stream or cur).cuda_stream)
        if stream is not None:
            done = torch.cuda.Event()
            done.record(stream)
            cur.wait_event(done)
        host = out_big.cpu().numpy()                                           # on the current stream, behind the event
        ws_host = ws_big.cpu().numpy()
        slots_same = torch.equal(self.raw_big, self.before)
        torch.cuda.synchronize()
        lo = PAD + residue
        outside = np.ones(host.size, dtype=bool)
        for i, (h, w) in enumerate(sizes):
            outside[lo + int(offs[i]):lo + int(offs[i]) + h * w * 3] = False
        assert (host[outside] == CANARY_DST).all(), "written before dst, after it or between two images"
        assert (ws_host[:PAD] == CANARY_WS).all() and (ws_host[PAD + wsb.value:] == CANARY_WS).all(), "written outside the workspace"
        assert slots_same, "the slots or the bytes around them changed"
        return [host[lo + int(offs[i]):lo + int(offs[i]) + h * w * 3].reshape(h, w, 3) for i, (h, w) in enumerate(sizes)]


def _reconstruct(arena, sb, sizes, align=16, **kw):
    return _Guarded(arena, sb).run(sizes, align=align, **kw)


def _pixel_slot(sb, pix):
    """A mode-0 slot: pixels decoded on the host."""
    slot = np.zeros((1, sb), dtype=np.uint8)
    hdr = slot[0, :64].view(np.int32)
    hdr[0], hdr[1], hdr[2], hdr[12] = 0, pix.shape[1], pix.shape[0], pix.size
    slot[0, SLOT_HDR:SLOT_HDR + pix.size] = pix.reshape(-1)
    return slot


def _bad(names, got, want):
    bad = [names[i] for i in range(len(want)) if not np.array_equal(got[i], want[i])]
    return len(bad), bad[:10]


@pytest.fixture(scope="module")
def jf():
    from tise_toolbox_amd import jpeg_feed
    jpeg_feed.load_decoder()
    return jpeg_feed


class _Matrix:
    pass


@pytest.fixture(scope="module")
def matrix(jf, tmp_path_factory):
    """jc.matrix_cases and one mode-0 slot: files, Pillow's pixels and the slots in HBM, built once for the module."""
    m = _Matrix()
    cases = jc.matrix_cases(tmp_path_factory.mktemp("matrix"))
    m.names = [name for name, _ in cases] + ["mode-0"]
    m.blobs = [b for _, b in cases]
    pix = np.random.default_rng(0).integers(0, 256, jc.PIXEL_SLOT[::-1] + (3,), dtype=np.uint8)
    m.want = [jc.pillow_rgb(b) for b in m.blobs] + [pix]
    m.sizes = [w.shape[:2] for w in m.want]
    arena, m.sb = _slots(jf, m.blobs)
    m.arena = np.concatenate([arena, _pixel_slot(m.sb, pix)])
    m.layouts = [jc.LAYOUT_NAMES[jf.probe(b)[3]] for b in m.blobs] + ["pix"]
    m.guarded = _Guarded(m.arena, m.sb)
    yield m
    m.guarded = None


@pytest.mark.gpu
def test_kernel_equals_pillow_and_host_decoder_on_the_whole_matrix(jf, matrix):
    """ONE ragged launch over the Pillow matrix, the extremes, tiny chroma, a table per component, dense blocks near the guard
    and a mode-0 slot; again with the page-locked table, on a side stream, and with a packed copy of the headers."""
    m = matrix
    assert len(m.blobs) >= 1024 + 20 + 10 + 6 + 88
    for kw in (dict(), dict(pinned=True), dict(stream=torch.cuda.Stream()), dict(packed_headers=True)):
        got = m.guarded.run(m.sizes, **kw)
        assert _bad(m.names, got, m.want) == (0, []), sorted(kw)
    for i in range(0, len(m.blobs), 7):                                        # image by image (dense offsets, no alignment)
        one = _reconstruct(m.arena[i:i + 1], m.sb, m.sizes[i:i + 1], align=1)[0]
        assert np.array_equal(one, m.want[i]), m.names[i]
        rc, host = jf.decode_rgb8(m.blobs[i])
        assert rc == 0 and np.array_equal(host, m.want[i]), m.names[i]


def _writer_cases(tmp_path):
    return jc.writer_extremes() + jc.tiny_chroma(tmp_path) + jc.distinct_tables() + jc.dense_out_of_range()


@pytest.mark.gpu
def test_stale_workspace_and_garbage_in_the_device_copy_of_the_headers(jf, tmp_path):
    """The planes are written before they are read, whatever the workspace held; and the kernels take the geometry from the
    launch's table alone: bytes 0..63 of every slot header in HBM are garbage here while the host copy the entry point validates is
    intact.  (The quantisation tables at 64..255 are read from the device by design and stay.)"""
    cases = _writer_cases(tmp_path)
    names, blobs = [n for n, _ in cases], [b for _, b in cases]
    want = [jc.pillow_rgb(b) for b in blobs]
    sizes = [w.shape[:2] for w in want]
    arena, sb = _slots(jf, blobs)
    g = _Guarded(arena, sb)
    for poison in (0x00, 0xFF):
        assert _bad(names, g.run(sizes, ws_poison=poison), want) == (0, []), poison
    hostile = arena.copy()
    rng = np.random.default_rng(17)
    hostile[:, :64] = rng.integers(0, 256, (len(blobs), 64), dtype=np.uint8)
    hostile[::3, :64] = 0xFF                                                   # sizes of -1
    hostile[1::3, :64].view(np.int32)[:] = 0x7fffffff
    assert _bad(names, _Guarded(arena, sb, device_arena=hostile).run(sizes), want) == (0, [])


@pytest.mark.gpu
def test_every_residue_of_the_output_address_and_dense_offsets(jf, matrix, tmp_path):
    """The dword store is taken per thread by the address: one odd-width 4:2:0 image at each residue of dst mod 4, then the
    whole matrix at dense offsets (every image starts where the last one ended) from an odd address."""
    img = _cases.smooth_images(1, 30, 45, seed=6)[0]
    blob = jc.save_jpeg(img, str(tmp_path / "r.jpg"), quality=85, subsampling=2)
    want = jc.pillow_rgb(blob)
    arena, sb = _slots(jf, [blob])
    g = _Guarded(arena, sb)
    stores = set()
    for residue in range(4):
        census = jc.branch_census([(45, 30, "420", residue)])
        stores.add((census["store-npx4-dword"] > 0, census["store-npx4-bytes"] > 0))
        assert census["store-npx1"] == 30
        assert np.array_equal(g.run([(30, 45)], align=1, residue=residue)[0], want), residue
    assert (True, True) in stores                                              # 135 bytes a row: both stores within one image
    m = matrix
    for residue in (0, 3):
        offs, _ = jc.plan_offsets(m.sizes, align=1)
        census = jc.branch_census([(w, h, lay, residue + int(o)) for (h, w), lay, o in zip(m.sizes, m.layouts, offs)])
        assert all(v > 0 for v in census.values()), census
        assert _bad(m.names, m.guarded.run(m.sizes, align=1, residue=residue), m.want) == (0, []), residue


@pytest.mark.gpu
def test_one_large_image_sets_the_grid_for_many_tiny_ones(jf, tmp_path):
    """grid.x follows the largest image: 640 x 480 first, in the middle and last among 48 images of 1 x 1 and 3 x 2 and a mode-0
    slot, whose workgroups beyond their own work must leave without touching anything."""
    p = str(tmp_path / "i.jpg")
    big = jc.save_jpeg(_cases.smooth_images(1, 480, 640, seed=8)[0], p, quality=75, subsampling=2)
    rng = np.random.default_rng(8)
    small = []
    for i in range(48):
        w, h = ((1, 1), (3, 2))[i % 2]
        kw = dict(mode="L") if i % 3 == 0 else dict(subsampling=(i // 2) % 3)
        small.append(jc.save_jpeg(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), p, quality=90, **kw))
    pix = rng.integers(0, 256, (2, 5, 3), dtype=np.uint8)
    for at in (0, 24, 48):
        blobs = small[:at] + [big] + small[at:]
        arena, sb = _slots(jf, blobs)
        k = 11 if at else 30                                                    # the pixel slot: after and before the large image
        arena = np.ascontiguousarray(np.concatenate([arena[:k], _pixel_slot(sb, pix), arena[k:]]))
        want = [jc.pillow_rgb(b) for b in blobs]
        want.insert(k, pix)
        sizes = [w.shape[:2] for w in want]
        lay = [jc.LAYOUT_NAMES[jf.probe(b)[3]] for b in blobs]
        lay.insert(k, "pix")
        offs, _ = jc.plan_offsets(sizes, align=1)
        census = jc.branch_census([(w, h, l, int(o)) for (h, w), l, o in zip(sizes, lay, offs)])
        assert census["idct-workgroups-idle"] >= 48 * 224 and census["mode0-copy"] == 10
        got = _reconstruct(arena, sb, sizes, align=1, pinned=True)
        assert _bad([str(i) for i in range(len(want))], got, want) == (0, []), at


@pytest.mark.gpu
def test_images_of_libjpegs_largest_dimension(jf):
    """65500 pixels on either axis: the longest rows of quads, the longest unit / quads split and the largest pitch products."""
    cases = jc.long_edges()
    want = [jc.pillow_rgb(b) for _, b in cases]
    assert [w.shape[:2] for w in want] == [(h, w) for w, h, _ in jc.LONG_EDGES]
    for (name, blob), px in zip(cases, want):
        arena, sb = _slots(jf, [blob])
        assert np.array_equal(_reconstruct(arena, sb, [px.shape[:2]], align=1, residue=1)[0], px), name
    b = jc._blank(1, 1, jc.LAYOUTS["gray"])
    b[0][..., 0] = 40
    dot = jc.jw.write_jpeg(1, 1, b, [np.full(64, 2, dtype=np.int32)])
    blobs = [blob for _, blob in cases[:2]] + [dot] + [blob for _, blob in cases[2:]]
    want = want[:2] + [jc.pillow_rgb(dot)] + want[2:]
    arena, sb = _slots(jf, blobs)
    got = _reconstruct(arena, sb, [w.shape[:2] for w in want])
    assert _bad([str(i) for i in range(len(want))], got, want) == (0, [])


@pytest.mark.gpu
def test_a_launch_of_65535_images(jf):
    """grid.y at its limit: 65535 gray images of 1 x 1, slots 384 bytes apart, tiled from one decoded file; the DC of some is
    written into the slot.  Every pixel against the host restatement, the altered ones against Pillow's decode of a file that
    holds that DC (whose slot is the altered slot, byte for byte)."""
    lib = jf.load_decoder()
    n, q = 65535, 8

    def dot(dc):
        b = jc._blank(1, 1, jc.LAYOUTS["gray"])
        b[0][..., 0] = dc
        return jc.jw.write_jpeg(1, 1, b, [np.full(64, q, dtype=np.int32)])
    one, sb = _slots(jf, [dot(5)])
    assert sb == 384 == lib.tise_jpeg_slot_bytes(1, 1, 0)
    arena = np.ascontiguousarray(np.tile(one, (n, 1)))
    altered = {0: -100, 1: 50, 255: 127, 256: -128, 257: 300, 32767: -300, 32768: 3, 40000: 0, 65533: -7, 65534: 77}
    for i, dc in altered.items():
        arena[i, SLOT_HDR:SLOT_HDR + 2].view(np.int16)[0] = dc
    sizes = [(1, 1)] * n
    got = np.stack(_reconstruct(arena, sb, sizes, align=1, residue=1, pinned=True)).reshape(n, 3)
    host = np.zeros((n, 3), dtype=np.uint8)
    for i in range(n):
        assert lib.tise_jpeg_reconstruct_slot_rgb8(arena.ctypes.data + i * sb, sb, host.ctypes.data + 3 * i, 3) == 0
    assert np.array_equal(got, host)
    assert len(np.unique(got[:, 0])) == len({min(max(128 + dc, 0), 255) for dc in list(altered.values()) + [5]}) == 9   # the images do differ
    for i, dc in list(altered.items()) + [(2, 5), (65000, 5)]:
        blob = dot(dc)
        slot, _ = _slots(jf, [blob])
        assert np.array_equal(slot[0], arena[i]), i
        assert np.array_equal(got[i], jc.pillow_rgb(blob).reshape(3)), (i, dc)


@pytest.mark.gpu
def test_one_launch_mixes_samplings_grayscale_and_a_pixel_slot(jf, tmp_path):
    img = _cases.smooth_images(1, 45, 70, seed=4)[0]
    p = str(tmp_path / "m.jpg")
    blobs = [jc.save_jpeg(img, p, quality=80, subsampling=0), jc.save_jpeg(img[:33, :21], p, quality=80, subsampling=1),
             jc.save_jpeg(img[:17], p, quality=80, subsampling=2), jc.save_jpeg(img, p, quality=80, mode="L")]
    arena, sb = _slots(jf, blobs, slot_bytes=(SLOT_HDR + 45 * 70 * 6 + 4096 + 15) & ~15)
    pix = np.random.default_rng(0).integers(0, 256, (31, 23, 3), dtype=np.uint8)   # mode 0: pixels decoded on the host
    extra = np.zeros((1, sb), dtype=np.uint8)
    hdr = extra[0, :64].view(np.int32)
    hdr[0], hdr[1], hdr[2], hdr[12] = 0, 23, 31, pix.size
    extra[0, SLOT_HDR:SLOT_HDR + pix.size] = pix.reshape(-1)
    arena = np.ascontiguousarray(np.concatenate([arena[:2], extra, arena[2:]]))
    want = [jc.pillow_rgb(blobs[0]), jc.pillow_rgb(blobs[1]), pix, jc.pillow_rgb(blobs[2]), jc.pillow_rgb(blobs[3])]
    got = _reconstruct(arena, sb, [w.shape[:2] for w in want], align=1)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


@pytest.mark.gpu
def test_loader_takes_the_largest_slot_image_and_one_beyond_it(jf, tmp_path):
    """A slot sized exactly for 64 x 64 4:2:0: such a file is decoded natively, a 96 x 96 one in the same batch fits neither as
    coefficients nor as pixels and arrives through Pillow on its own."""
    rng = np.random.default_rng(1)
    files, want = [], []
    for i, (w, h) in enumerate([(64, 64), (96, 96), (40, 30), (64, 64)]):
        path = str(tmp_path / f"{i}.jpg")
        jc.save_jpeg(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), path, quality=90, subsampling=2)
        files.append(path)
        want.append(np.asarray(Image.open(path).convert("RGB")))
    sb = int(jf.load_decoder().tise_jpeg_slot_bytes(64, 64, 3))
    loader = jf.JpegFeedLoader(files, 4, "cuda:0", workers=2, slot_bytes=sb)
    items = list(loader)
    torch.cuda.synchronize()
    assert len(items) == 1 and isinstance(items[0], list)
    for t, w in zip(items[0], want):
        assert np.array_equal(t.cpu().numpy(), w)
    assert (loader.native, loader.pillow, loader.oversize) == (3, 1, 1)


@pytest.mark.gpu
def test_loader_cycles_its_arenas_over_a_ragged_directory(jf, tmp_path):
    """More than 2 x NBUF loader batches, so every arena is reused twice: sizes change from batch to batch, one batch is of one
    size (a dense tensor), a progressive file (Pillow's pixels in a mode-0 slot) and a file beyond the slots (travels on its
    own) stand first and last in a batch.  Every delivered tensor is Pillow's, the counters are exact; with drop-last, without
    it (a short last batch), with a schedule of the caller's, and on a second iteration of the same object."""
    bs, nfiles = 6, 52
    assert nfiles // bs >= 2 * jf.JpegFeedLoader.NBUF + 1
    rng = np.random.default_rng(21)
    progressive, beyond = {2 * bs, 4 * bs + bs - 1}, {1 * bs + bs - 1, 5 * bs}
    files, want = [], []
    for i in range(nfiles):
        w, h = int(rng.integers(9, 41)), int(rng.integers(9, 41))
        kw = dict(quality=int(rng.choice([60, 85, 95])), subsampling=int(rng.choice([0, 1, 2])))
        if i // bs == 3:
            w, h, kw = 24, 16, dict(quality=80, subsampling=2)                 # a batch of one size
        if i in beyond:
            w, h = 96, 96
        if i in progressive:
            kw["progressive"] = True
        path = str(tmp_path / f"f_{i:03d}.jpg")
        jc.save_jpeg(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), path, **kw)
        files.append(path)
        want.append(np.asarray(Image.open(path).convert("RGB")))
    sb = int(jf.load_decoder().tise_jpeg_slot_bytes(64, 64, 3))

    def deliver(loader):
        got, shapes = [], []
        for item in loader:                                                    # copied out before the loader may reuse the arena
            shapes.append(len(item))
            got += [t.cpu().numpy() for t in item]
        return got, shapes

    def same(got, n):
        return len(got) == n and all(np.array_equal(g, w) for g, w in zip(got, want))

    full = jf.JpegFeedLoader(files, bs, "cuda:0", workers=3, slot_bytes=sb, drop_last=False)
    assert len(full) == 9
    got, shapes = deliver(full)
    assert shapes == [6] * 8 + [4] and same(got, 52)
    assert (full.native, full.pillow, full.oversize) == (48, 4, 2)
    got, shapes = deliver(full)                                                # the same object again; its counters run on
    assert shapes == [6] * 8 + [4] and same(got, 52)
    assert (full.native, full.pillow, full.oversize) == (96, 8, 4)
    whole = jf.JpegFeedLoader(files, bs, "cuda:0", workers=3, slot_bytes=sb)
    items = list(whole)
    assert len(items) == len(whole) == 8 and isinstance(items[0], list) and tuple(items[3].shape) == (6, 16, 24, 3)
    got, shapes = deliver(whole)
    assert shapes == [6] * 8 and same(got, 48)
    assert (whole.native, whole.pillow, whole.oversize) == (2 * 44, 2 * 4, 2 * 2)
    rows = [5, 6, 3, 6, 6, 1, 6, 6, 6, 5, 2]
    sched = jf.JpegFeedLoader(files, bs, "cuda:0", workers=3, slot_bytes=sb, drop_last=False, item_rows=rows)
    got, shapes = deliver(sched)
    assert shapes == rows and same(got, 52)
    assert (sched.native, sched.pillow, sched.oversize) == (48, 4, 2)
    torch.cuda.synchronize()


def test_argument_validation_without_a_launch(jf, tmp_path):
    """NULL, misalignment and headers that disagree with themselves come back TISE_ERR_INVALID_ARG before any HIP call (fake
    device addresses: a launch would need a device this test does not have)."""
    from tise_toolbox_amd import _lib
    lib = _lib.load()
    bad = _lib.TISE_ERR_INVALID_ARG
    blob = jc.save_jpeg(_cases.smooth_images(1, 40, 56, seed=1)[0], str(tmp_path / "a.jpg"), quality=80, subsampling=2)
    arena, sb = _slots(jf, [blob, blob])
    S, D, W = 0x7f0000000000, 0x7f0000100000, 0x7f0000200000
    offs = np.array([0, 40 * 56 * 3], dtype=np.int64)
    wsb = ctypes.c_size_t()
    assert lib.tise_jpeg_workspace_bytes(2, sb, ctypes.byref(wsb)) == 0
    assert lib.tise_jpeg_workspace_bytes(2, sb + 8, ctypes.byref(wsb)) == bad and lib.tise_jpeg_workspace_bytes(-1, sb, ctypes.byref(wsb)) == bad

    def call(slots=S, n=2, stride=sb, hdrs=None, hstride=sb, o=offs, dst=D, dbytes=2 * 40 * 56 * 3, ws=W, wbytes=None, table=None):
        hdrs = arena if hdrs is None else hdrs
        return lib.tise_jpeg_reconstruct_rgb8(slots, n, stride, hdrs.ctypes.data if hdrs is not False else None, hstride,
                                              o.ctypes.data if o is not None else None, dst, dbytes, ws, wsb.value if wbytes is None else wbytes, table, None)
    assert call(n=0) == _lib.TISE_OK                                           # nothing to do, no launch
    # grid y: 65535 images is the most one launch takes (test_a_launch_of_65535_images runs it); one more is refused before any HIP call
    assert call(n=65536) == _lib.TISE_ERR_UNSUPPORTED and call(n=1 << 40) == _lib.TISE_ERR_UNSUPPORTED
    assert lib.tise_jpeg_workspace_bytes(65535, sb, ctypes.byref(wsb)) == 0 and lib.tise_jpeg_workspace_bytes(65536, sb, ctypes.byref(wsb)) == bad
    assert lib.tise_jpeg_workspace_bytes(2, sb, ctypes.byref(wsb)) == 0
    for kw in (dict(slots=None), dict(dst=None), dict(ws=None), dict(hdrs=False), dict(o=None), dict(n=-1), dict(slots=S + 8),
               dict(ws=W + 4), dict(stride=sb + 8), dict(stride=128), dict(dbytes=2 * 40 * 56 * 3 - 1), dict(wbytes=wsb.value - 1),
               dict(wbytes=64), dict(stride=sb - 16, hstride=sb), dict(o=np.array([0, -4], dtype=np.int64)), dict(table=0x7f0000300004)):
        assert call(**kw) == bad, kw
    for field, delta in ((6, 1), (9, 1), (7, -1), (12, 128), (12, -128), (1, 9), (2, 17), (3, 1), (4, -1), (5, 1), (0, 1), (0, -1)):
        h2 = arena.copy()
        h2[1, :64].view(np.int32)[field] += delta                             # block counts / payload / size / sampling / mode disagree
        assert call(hdrs=h2) == bad, (field, delta)


def _write_set(root, sizes, n, seed=0):
    os.makedirs(root, exist_ok=True)
    imgs = {s: _cases.smooth_images(8, s[1], s[0], seed=seed + s[0]) for s in set(sizes)}
    rng = np.random.default_rng(seed)
    for i in range(n):
        w, h = sizes[i % len(sizes)]
        img = imgs[(w, h)][i % 8].astype(np.int16) + rng.integers(-12, 13, (h, w, 3))
        jc.save_jpeg(np.clip(img, 0, 255).astype(np.uint8), os.path.join(root, f"im_{i:05d}.jpg"), quality=75, subsampling=2)


def _fid_stats(path, batch_size, jpeg_feed, png_feed="ring"):
    from tise_toolbox_amd import feeds, fid_score
    fid_score._FEED = feeds.Options(png_feed=png_feed, jpeg_feed=jpeg_feed)
    try:
        with fid_score._own_model(2048, None, None, 0) as model:
            mu, sigma = fid_score._compute_statistics_of_path(path, model, batch_size, 2048, True, num_workers=4)
        return np.asarray(mu), np.asarray(sigma), feeds.last.loader if feeds.last.kind == "jpeg" else None
    finally:
        fid_score._FEED = feeds.Options()


@pytest.mark.gpu
def test_fid_statistics_and_is_of_one_size_set_equal_the_pillow_path_bit_for_bit(jf, tmp_path):
    root = str(tmp_path / "one")
    _write_set(root, [(256, 256)], 500)
    mu_n, sig_n, loader = _fid_stats(root, 50, "native")
    assert loader is not None and (loader.native, loader.pillow) == (500, 0)
    mu_p, sig_p, none = _fid_stats(root, 50, "pillow")
    assert none is None
    print("one size: max |dmu|", np.abs(mu_n - mu_p).max(), "max |dsigma|", np.abs(sig_n - sig_p).max())
    assert np.array_equal(mu_n, mu_p) and np.array_equal(sig_n, sig_p)
    from tise_toolbox_amd import feeds, inception_score as isc
    from tise_toolbox_amd import img_data
    files = img_data.get_filenames(root)
    res = {}
    for mode in ("native", "pillow"):
        isc.configure(jpeg_feed=mode, batch_size=50)
        res[mode] = isc.get_inception_score(files, splits=10)
        assert (feeds.last.kind == "jpeg") == (mode == "native")
    isc.configure(jpeg_feed=None)
    print("IS*", res)
    assert res["native"] == res["pillow"]


@pytest.mark.gpu
def test_fid_statistics_of_a_ragged_set_equal_the_dataloader_path_bit_for_bit(jf, tmp_path):
    root = str(tmp_path / "ragged")
    sizes = [(640, 480), (500, 375), (480, 640), (375, 500), (333, 500), (500, 333), (640, 427), (427, 640), (256, 256), (300, 200),
             (121, 97), (64, 48)]
    _write_set(root, sizes, 300, seed=3)
    mu_n, sig_n, loader = _fid_stats(root, 50, "native")
    assert loader is not None and (loader.native, loader.pillow) == (300, 0)
    mu_d, sig_d, _ = _fid_stats(root, 50, "native", png_feed="dataloader")     # --png-feed dataloader: the torch DataLoader path
    print("ragged: max |dmu|", np.abs(mu_n - mu_d).max(), "max |dsigma|", np.abs(sig_n - sig_d).max())
    assert np.array_equal(mu_n, mu_d) and np.array_equal(sig_n, sig_d)
