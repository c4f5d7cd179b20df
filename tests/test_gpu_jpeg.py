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


def _reconstruct(arena, sb, sizes, align=16):
    from tise_toolbox_amd import _lib
    n = arena.shape[0]
    offs, pos = np.zeros(n, dtype=np.int64), 0
    for i, (h, w) in enumerate(sizes):
        offs[i] = pos
        pos += (h * w * 3 + align - 1) // align * align
    dev = torch.device("cuda", 0)
    raw = torch.from_numpy(arena.reshape(-1)).to(dev)
    out = torch.full((pos + 64,), 0xAB, dtype=torch.uint8, device=dev)
    wsb = ctypes.c_size_t()
    _lib.call("tise_jpeg_workspace_bytes", n, sb, ctypes.byref(wsb))
    ws = torch.empty(wsb.value, dtype=torch.uint8, device=dev)
    _lib.call("tise_jpeg_reconstruct_rgb8", raw.data_ptr(), n, sb, arena.ctypes.data, sb, offs.ctypes.data, out.data_ptr(), pos,
              ws.data_ptr(), wsb.value, None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[pos:] == 0xAB).all()                                          # nothing written past the checked extent
    return [host[int(offs[i]):int(offs[i]) + h * w * 3].reshape(h, w, 3) for i, (h, w) in enumerate(sizes)]


@pytest.fixture(scope="module")
def jf():
    from tise_toolbox_amd import jpeg_feed
    jpeg_feed.load_decoder()
    return jpeg_feed


@pytest.mark.gpu
def test_kernel_equals_pillow_and_host_decoder_on_the_whole_matrix(jf, tmp_path):
    cases = jc.pillow_matrix(tmp_path) + jc.writer_extremes() + jc.tiny_chroma(tmp_path)
    blobs = [b for _, b in cases]
    want = [jc.pillow_rgb(b) for b in blobs]
    sizes = [w.shape[:2] for w in want]
    arena, sb = _slots(jf, blobs)
    got = _reconstruct(arena, sb, sizes)                                       # ONE ragged launch over everything
    bad = [cases[i][0] for i in range(len(cases)) if not np.array_equal(got[i], want[i])]
    assert not bad, (len(bad), bad[:10])
    for i in range(0, len(cases), 7):                                          # image by image (dense offsets, no alignment)
        one = _reconstruct(arena[i:i + 1], sb, sizes[i:i + 1], align=1)[0]
        assert np.array_equal(one, want[i]), cases[i][0]
        rc, host = jf.decode_rgb8(blobs[i])
        assert rc == 0 and np.array_equal(host, want[i]), cases[i][0]


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
    from tise_toolbox_amd import fid_score
    fid_score._JPEG_FEED["mode"], fid_score._PNG_FEED["mode"] = jpeg_feed, png_feed
    fid_score._compute_statistics_of_path.last_jpeg_loader = None
    try:
        with fid_score._own_model(2048, None, None, 0) as model:
            mu, sigma = fid_score._compute_statistics_of_path(path, model, batch_size, 2048, True, num_workers=4)
        return np.asarray(mu), np.asarray(sigma), fid_score._compute_statistics_of_path.last_jpeg_loader
    finally:
        fid_score._JPEG_FEED["mode"], fid_score._PNG_FEED["mode"] = None, "ring"


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
    from tise_toolbox_amd import inception_score as isc
    from tise_toolbox_amd import img_data
    files = img_data.get_filenames(root)
    res = {}
    for mode in ("native", "pillow"):
        isc.configure(jpeg_feed=mode, batch_size=50)
        isc.feed_images.last_jpeg_loader = None
        res[mode] = isc.get_inception_score(files, splits=10)
        assert (isc.feed_images.last_jpeg_loader is not None) == (mode == "native")
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
