"""JPEG feed of the drop-in CLIs: decode THREADS -> page-locked arenas of coefficient slots -> side-stream H2D ->
IDCT / upsampling / colour conversion in HBM -> device batches of images of any size.

Replaces, for JPEG directories (the real-image side of every comparison: COCO val2014, the CUB photographs), the
hand-over of image_realism/FID/fid_score.py:215-217 -- ``DataLoader(dataset, batch_size, drop_last=True, num_workers=8)``
whose workers run ``Image.open(f).convert("RGB")`` (img_data.py:19-25).  The recipe is the PNG feed's (png_ring.py): the
strictly serial part of a file -- here marker parsing and Huffman decoding -- stays on the host in a small plain-C decoder
(csrc/jpeg_decode.c -> libtise_jpeg.so), everything data-parallel runs on the GPU (csrc/jpeg_idct.hip:
tise_jpeg_reconstruct_rgb8), the result is byte-identical to Pillow, and anything doubtful is handed to Pillow.

The pipeline (threads, arenas, side stream, items) is arena_feed.ArenaFeedLoader's; what is this feed's own:
  * a decode thread writes one SLOT per file -- [256-byte header | int16 quantised coefficients], include/tise_jpeg.h -- all
    slots of an arena the same size; a file the decoder refuses is decoded by Pillow in the same thread and enters the arena
    as pixels (slot mode 0); a file whose pixels do not fit a slot either travels on its own;
  * ONE host->device copy of the slots and ONE tise_jpeg_reconstruct_rgb8 launch per loader batch, into the arena's own output
    buffer, which the item's tensors view.
``len()`` counts whole ``batch_size`` batches (drop-last, fid_score.py:90-96).
"""
import ctypes
import os
import threading
import time

import numpy as np
import torch

from . import _lib
from .arena_feed import ArenaFeedLoader, _pillow_rgb

_HERE = os.path.dirname(os.path.abspath(__file__))
JPEG_LIB_PATH = os.path.join(_HERE, "libtise_jpeg.so")
TISE_JPEG_OK, TISE_JPEG_UNSUPPORTED, TISE_JPEG_CORRUPT, TISE_JPEG_SIZE = 0, 1, 2, 3
SLOT_HDR = 256
_REASONS = {TISE_JPEG_UNSUPPORTED: "outside the native subset", TISE_JPEG_CORRUPT: "malformed or doubtful",
            TISE_JPEG_SIZE: "larger than an arena slot"}

_c_u8p = ctypes.c_void_p
_c_intp = ctypes.POINTER(ctypes.c_int)
DECODER_SIGNATURES = {
    "tise_jpeg_slot_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "tise_jpeg_probe": (ctypes.c_int, [_c_u8p, ctypes.c_size_t, _c_intp, _c_intp, _c_intp]),
    "tise_jpeg_entropy_decode": (ctypes.c_int, [_c_u8p, ctypes.c_size_t, _c_u8p, ctypes.c_size_t, _c_intp, _c_intp]),
    "tise_jpeg_reconstruct_slot_rgb8": (ctypes.c_int, [_c_u8p, ctypes.c_size_t, _c_u8p, ctypes.c_size_t]),
    "tise_jpeg_decode_rgb8": (ctypes.c_int, [_c_u8p, ctypes.c_size_t, _c_u8p, ctypes.c_size_t, _c_intp, _c_intp]),
}
_decoder = None
_decoder_lock = threading.Lock()


def load_decoder():
    """libtise_jpeg.so bound with ctypes (once).  A missing library is an error: build it with tise_toolbox_amd.build."""
    global _decoder
    with _decoder_lock:
        if _decoder is None:
            if not os.path.exists(JPEG_LIB_PATH):
                raise _lib.TiseLibraryError(f"{JPEG_LIB_PATH} not found: build it with `python -m tise_toolbox_amd.build`")
            lib = ctypes.CDLL(JPEG_LIB_PATH)
            for name, (res, args) in DECODER_SIGNATURES.items():
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = res, args
            _decoder = lib
    return _decoder


def probe(blob):
    """(status, w, h, layout) of a JPEG file image (marker parse only)."""
    w, h, lay = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rc = load_decoder().tise_jpeg_probe(blob, len(blob), ctypes.byref(w), ctypes.byref(h), ctypes.byref(lay))
    return rc, w.value, h.value, lay.value


def probe_file(path):
    """True when ``path`` is a JPEG of the native subset (what --jpeg-feed native looks at: the shard's first file)."""
    try:
        with open(path, "rb") as f:
            blob = f.read()
    except OSError:
        return False
    return probe(blob)[0] == TISE_JPEG_OK


def use_native(files, mode):
    """Does ``files`` (a directory's shard, walk order) take the native feed?  ``mode`` "native": when its first file is a JPEG of
    the native subset; "pillow": never; None (the CLIs' default): when, besides, its first 64 files differ in size -- measured
    (profiles/r07a_jpeg_feed.txt): ragged JPEG sets run 6.5 x faster on the native feed than on the DataLoader path they took
    before, 256 x 256 sets of one size 1.7 x SLOWER than through Pillow in the PNG ring's 14 decode processes."""
    if mode == "pillow" or not files:
        return False
    if not os.path.exists(JPEG_LIB_PATH):
        if mode == "native":
            load_decoder()                                                      # asked for by name: a missing library is an error
        return False                                                            # a tree built before the JPEG feed existed: every other path works as it did
    if not probe_file(files[0]):
        return False
    if mode == "native":
        return True
    sizes = set()
    for path in files[:64]:
        try:
            with open(path, "rb") as f:
                rc, w, h, _ = probe(f.read(1 << 16))
        except OSError:
            continue
        sizes.add((rc, w, h) if rc == TISE_JPEG_OK else (rc, path))
    return len(sizes) > 1


def decode_rgb8(blob):
    """(status, (h, w, 3) uint8 array | None): the complete native decode on the host (tise_jpeg_decode_rgb8)."""
    rc, w, h, _ = probe(blob)
    if rc != TISE_JPEG_OK:
        return rc, None
    out = np.empty((h, w, 3), dtype=np.uint8)
    rc = load_decoder().tise_jpeg_decode_rgb8(blob, len(blob), out.ctypes.data, out.nbytes, None, None)
    return rc, (out if rc == TISE_JPEG_OK else None)


def decode_file_host(path):
    """(pixels (h, w, 3) uint8, status of the native decoder): native when it takes the file, Pillow otherwise."""
    with open(path, "rb") as f:
        blob = f.read()
    rc, px = decode_rgb8(blob)
    if rc == TISE_JPEG_OK:
        return px, rc
    return _pillow_rgb(path), rc


def _put_header_pixels(hdr_i32, w, h):
    hdr_i32[:] = 0
    hdr_i32[0], hdr_i32[1], hdr_i32[2], hdr_i32[12] = 0, w, h, h * w * 3


def pick_slot_bytes(files, rows=1):
    """Slot size for arenas of ``rows`` slots: the largest coefficient slot among the first 64 files (marker parse only) with a
    quarter of headroom while an arena stays below 1 GiB, a multiple of 4096.  Larger files arrive through Pillow."""
    lib, need = load_decoder(), 0
    for path in files[:64]:
        try:
            with open(path, "rb") as f:
                blob = f.read(1 << 16)
        except OSError:
            continue
        rc, w, h, lay = probe(blob)
        if rc == TISE_JPEG_OK:
            need = max(need, int(lib.tise_jpeg_slot_bytes(w, h, lay)), SLOT_HDR + h * w * 3)
    if need == 0:
        need = SLOT_HDR + 640 * 640 * 3
    roomy = min(need + need // 4, max(need, (1 << 30) // max(1, int(rows))))
    return (roomy + 4095) & ~4095


class JpegFeedLoader(ArenaFeedLoader):
    FEED, OK, REASONS = "jpeg", TISE_JPEG_OK, _REASONS
    _decode_file_host = staticmethod(decode_file_host)

    def __init__(self, files, batch_size, device, workers=None, chunk=4, slot_bytes=None, drop_last=True, item_rows=None):
        super().__init__(files, batch_size, device, workers, chunk, drop_last, item_rows)
        self.slot_bytes = int(slot_bytes) if slot_bytes else 0
        self.oversize = 0

    def __len__(self):
        return -(-self.n_rows // self.bs) if self.bs > 0 else 0

    def _make_arenas(self, nbuf, rows, dev):
        """Arenas of ``rows`` slots.  Slot size: the caller's, or the largest coefficient slot among the first files (marker parse
        only) with a quarter of headroom; larger files arrive through Pillow."""
        self._dec = load_decoder()
        self.slot_bytes = sb = (self.slot_bytes + 15) & ~15 if self.slot_bytes else pick_slot_bytes(self.files, rows)
        ws_bytes = ctypes.c_size_t()
        _lib.call("tise_jpeg_workspace_bytes", rows, sb, ctypes.byref(ws_bytes))
        arenas = []
        for _ in range(nbuf):
            pinned = torch.empty(rows * sb + rows * 64, dtype=torch.uint8).pin_memory()   # the slots + scratch for the launch's device table
            arenas.append({"pinned": pinned, "np": pinned.numpy(), "addr": pinned.data_ptr(), "rows": rows,
                           "raw": torch.empty(rows * sb, dtype=torch.uint8, device=dev),
                           "ws": torch.empty(ws_bytes.value, dtype=torch.uint8, device=dev),
                           "out": torch.empty(rows * (sb * 3 // 2 + 16), dtype=torch.uint8, device=dev),
                           "consumed": torch.cuda.Event()})
        return arenas

    # The reuse rule: items VIEW the arena's ``out``, so an arena is refilled (and its ``out`` overwritten by the next launch)
    # only after the consumer's stream has passed the point at which the item was handed back.
    def _handed_back(self, arena, stream):
        arena["consumed"].record(stream)

    def _await_reusable(self, arena):
        arena["consumed"].synchronize()                                         # returns at once while nothing was recorded

    def _decode_into(self, arena, idx, path, extra):
        """One file -> slot ``idx`` of ``arena`` (coefficients, or Pillow's pixels), or -> ``extra[idx]`` when it fits no slot."""
        t0 = time.perf_counter()
        sb = self.slot_bytes
        base = arena["addr"] + idx * sb
        with open(path, "rb") as f:
            blob = f.read()
        w, h = ctypes.c_int(), ctypes.c_int()
        rc = self._dec.tise_jpeg_entropy_decode(blob, len(blob), base, sb, ctypes.byref(w), ctypes.byref(h))
        if rc != TISE_JPEG_OK:
            px = _pillow_rgb(path)
            hh, ww = px.shape[:2]
            hdr = arena["np"][idx * sb:idx * sb + 64].view(np.int32)
            if SLOT_HDR + px.nbytes <= sb and ww <= 65535 and hh <= 65535:
                _put_header_pixels(hdr, ww, hh)
                arena["np"][idx * sb + SLOT_HDR:idx * sb + SLOT_HDR + px.nbytes] = px.reshape(-1)
            else:                                                               # travels on its own: the slot holds a 1 x 1 placeholder
                _put_header_pixels(hdr, 1, 1)
                extra[idx] = np.ascontiguousarray(px)
                with self._lock:
                    self.oversize += 1
        self._count(rc, path)
        with self._lock:
            self.decode_seconds += time.perf_counter() - t0

    def _launch(self, arena, nrow, extra, side):
        a, rows, sb = arena, arena["rows"], self.slot_bytes
        hdrs = a["np"][:rows * sb].reshape(rows, sb)[:, :12].view(np.int32)    # mode, width, height of every slot
        sizes = [(int(hdrs[i, 2]), int(hdrs[i, 1])) for i in range(nrow)]
        offs, total = self._pack(sizes, extra, range(nrow))
        if total > a["out"].numel():
            raise RuntimeError("jpeg feed: a batch's pixels exceed the output buffer")
        _lib.call("tise_memcpy_h2d_async", a["raw"].data_ptr(), a["addr"], nrow * sb, side.cuda_stream)
        _lib.call("tise_jpeg_reconstruct_rgb8", a["raw"].data_ptr(), nrow, sb, a["addr"], sb, offs.ctypes.data, a["out"].data_ptr(),
                  a["out"].numel(), a["ws"].data_ptr(), a["ws"].numel(), a["addr"] + rows * sb, side.cuda_stream)
        return sizes, offs, a["out"]

    def feed_line(self, wall):
        """The ``[tise] jpeg feed: ...`` line of the CLIs."""
        return self._feed_line(wall, f"{self.native} decoded natively, {self.pillow} by Pillow{self._why()}", "entropy decoding",
                               f"slot {self.slot_bytes} bytes, items of {min(self.item_rows)}..{max(self.item_rows)} images")
