"""PNG feed for directories whose images differ in size -- the cropped-object directories behind O-FID, ``--per-class`` O-FID
and O-IS (``{stem}_{class}_{k}.png``, object_fidelity/crop_object.py:45: one size per crop): decode THREADS -> page-locked
arenas of packed inflate-only slots -> side-stream H2D -> the row filters of ALL images of a loader batch reversed by one
launch in HBM -> device batches of images of any size.

Replaces, for such directories, the hand-over of object_fidelity/O-FID/fid_score.py:215-217 and
object_fidelity/O-IS/object_centric_inception_score.py:31-33 -- a ``DataLoader`` whose workers run
``Image.open(f).convert("RGB")`` and pickle every crop to the main process, which then copied each crop to the device on its
own.  The division of labour is the PNG ring's (png_ring.py): the strictly serial part of a file -- chunk parsing, CRC-32,
zlib inflate -- stays on the host (csrc/png_decode.c -> libtise_png.so, bound with ctypes, which releases the GIL in the call),
the row filters run on the GPU (csrc/png_unfilter.hip: tise_png_unfilter_ragged_rgb8), the result is byte-identical to Pillow,
and anything doubtful is handed to Pillow.

The pipeline (threads, arenas, side stream, items) is arena_feed.ArenaFeedLoader's; what is this feed's own:
  * a decode thread probes a file, reserves a slot of ITS size -- [64-byte header | filtered rows], include/tise_png.h -- at the
    next 64-byte aligned offset of the arena and inflates into it; a file outside the native subset (palette, gray, 16-bit,
    interlaced, any CRC doubt) is decoded by Pillow in the same thread and enters the arena as pixels (slot mode 0), as does a
    file whose rows exceed the kernel's 8192 bytes (decoded natively); a file the arena has no room left for travels on its own;
  * ONE host->device copy of the arena's used part and ONE tise_png_unfilter_ragged_rgb8 launch per loader batch, into a device
    buffer of the batch's own that the item's tensors keep alive -- engine.coalesce_batches gathers the ragged items of many
    loader batches into one trunk pass.
``len()`` counts loader batches (``drop_last``: whole ones only, fid_score.py:90-96).
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
PNG_LIB_PATH = os.path.join(_HERE, "libtise_png.so")
PNG_OK, PNG_UNSUPPORTED, PNG_CORRUPT, PNG_SIZE, PNG_SCRATCH = range(5)
SLOT_HDR = 64                  # csrc/png_decode.c: TISE_PNG_SLOT_HDR
ROW_MAX = 8192                 # csrc/png_decode.c: TISE_PNG_DEVICE_ROW_MAX (bytes of a filtered row the kernel stages)
TABLE_ENTRY = 48               # csrc/png_unfilter.hip: sizeof(RaggedImg)
_REASONS = {PNG_UNSUPPORTED: "outside the native subset", PNG_CORRUPT: "malformed or doubtful", PNG_SCRATCH: "scratch"}

_decoder = None
_decoder_lock = threading.Lock()


def load_decoder():
    """libtise_png.so bound with ctypes (once).  A missing library is an error: build it with tise_toolbox_amd.build."""
    global _decoder
    with _decoder_lock:
        if _decoder is None:
            if not os.path.exists(PNG_LIB_PATH):
                raise _lib.TiseLibraryError(f"{PNG_LIB_PATH} not found: build it with `python -m tise_toolbox_amd.build`")
            lib = ctypes.CDLL(PNG_LIB_PATH)
            ip = ctypes.POINTER(ctypes.c_int)
            lib.tise_png_probe.restype = ctypes.c_int
            lib.tise_png_probe.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ip, ip, ip]
            lib.tise_png_scratch_bytes.restype = ctypes.c_size_t
            lib.tise_png_scratch_bytes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_size_t]
            lib.tise_png_slot_bytes.restype = ctypes.c_size_t
            lib.tise_png_slot_bytes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
            lib.tise_png_decode_rgb8.restype = ctypes.c_int
            lib.tise_png_decode_rgb8.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                 ctypes.c_void_p, ctypes.c_size_t, ip, ip]
            lib.tise_png_inflate_slot.restype = ctypes.c_int
            lib.tise_png_inflate_slot.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int,
                                                  ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ip, ip, ip]
            _decoder = lib
    return _decoder


def probe(blob):
    """(status, w, h, channels) of a PNG file image (chunk parse + CRC only)."""
    w, h, ch = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rc = load_decoder().tise_png_probe(blob, len(blob), ctypes.byref(w), ctypes.byref(h), ctypes.byref(ch))
    return rc, w.value, h.value, ch.value


def probe_file(path):
    """True when ``path`` is a PNG of the native subset (8-bit RGB / RGBA, not interlaced, every CRC right)."""
    try:
        with open(path, "rb") as f:
            blob = f.read()
    except OSError:
        return False
    return probe(blob)[0] == PNG_OK


def use_native(files, mode):
    """Does ``files`` (a directory's shard, walk order) take this feed?  ``mode`` "native": yes; "dataloader": no; None (the
    default of --per-class and O-IS): when its first file probes as a PNG of the native subset."""
    if mode == "dataloader" or not files:
        return False
    if mode == "native":
        load_decoder()                                                          # asked for by name: a missing library is an error
        return True
    return os.path.exists(PNG_LIB_PATH) and probe_file(files[0])


_tls = threading.local()


def _scratch(nbytes):
    buf = getattr(_tls, "scratch", None)
    if buf is None or buf.size < nbytes:
        buf = _tls.scratch = np.empty(nbytes + (nbytes >> 2) + 4096, dtype=np.uint8)
    return buf


def _native_rgb(lib, blob, h, w):
    """(status, pixels | None): the complete native decode on the host (tise_png_decode_rgb8)."""
    out = np.empty((h, w, 3), dtype=np.uint8)
    sc = _scratch(lib.tise_png_scratch_bytes(h, w, len(blob)))
    rc = lib.tise_png_decode_rgb8(blob, len(blob), out.ctypes.data, h, w, sc.ctypes.data, sc.size, None, None)
    return rc, (out if rc == PNG_OK else None)


def decode_file_host(path):
    """(pixels (h, w, 3) uint8, status of the native decoder): native when it takes the file, Pillow otherwise.  A file neither
    can read raises RuntimeError naming it."""
    lib = load_decoder()
    try:
        with open(path, "rb") as f:
            blob = f.read()
        rc, w, h, _ = probe(blob)
        if rc == PNG_OK:
            rc, px = _native_rgb(lib, blob, h, w)
            if rc == PNG_OK:
                return px, rc
        return _pillow_rgb(path), rc
    except Exception as e:                                                      # noqa: BLE001
        raise RuntimeError(f"crop feed: cannot read {path}: {type(e).__name__}: {e}") from e


def pick_arena_bytes(files, rows):
    """Bytes of an arena for loader batches of ``rows`` files: ``rows`` slots of the largest size among the first 64 files
    (chunk parse only) -- crops average far below their largest, so a batch rarely fills it -- at least 1 MiB, at most 1 GiB, a
    multiple of 4096.  Files a batch has no room left for travel on their own."""
    lib, need = load_decoder(), 0
    for path in files[:64]:
        try:
            with open(path, "rb") as f:
                rc, w, h, ch = probe(f.read())
        except OSError:
            continue
        if rc == PNG_OK:
            need = max(need, int(lib.tise_png_slot_bytes(h, w, ch if w * ch + 1 <= ROW_MAX else 0)))
    if need == 0:
        need = SLOT_HDR + 256 * 257 * 4
    total = min(max(need * max(1, int(rows)), 1 << 20), 1 << 30)
    return (total + 4095) & ~4095


class CropFeedLoader(ArenaFeedLoader):
    FEED, OK, REASONS = "crop", PNG_OK, _REASONS
    _decode_file_host = staticmethod(decode_file_host)

    def __init__(self, files, batch_size, device, workers=None, chunk=8, arena_bytes=None, drop_last=True, item_rows=None):
        super().__init__(files, batch_size, device, workers, chunk, drop_last, item_rows)
        self.arena_bytes = int(arena_bytes) if arena_bytes else 0
        self.alone = self.host_unfiltered = 0

    def __len__(self):
        return len(self.item_rows)

    def _make_arenas(self, nbuf, rows, dev):
        self._dec = load_decoder()
        _lib.load()
        cap = self.arena_bytes = ((self.arena_bytes + 63) & ~63) if self.arena_bytes else pick_arena_bytes(self.files, rows)
        arenas = []
        for _ in range(nbuf):
            pinned = torch.empty(cap + rows * TABLE_ENTRY, dtype=torch.uint8).pin_memory()   # the slots + scratch for the launch's device table
            arenas.append({"pinned": pinned, "np": pinned.numpy(), "addr": pinned.data_ptr(), "cap": cap, "used": 0,
                           "offs": np.zeros(rows, dtype=np.int64), "hwm": np.zeros((rows, 3), dtype=np.int32),
                           "raw": torch.empty(cap, dtype=torch.uint8, device=dev),
                           "table": torch.empty(rows * TABLE_ENTRY, dtype=torch.uint8, device=dev)})
        return arenas

    # The reuse rule: items OWN their pixels (a buffer per batch), so engine.coalesce_batches may hold many of them and the
    # consumer's progress says nothing about the arena.  It (page-locked slots + their device copy) is refilled once the side
    # stream has read it: the copy and the unfilter launch of the batch that came out of it are done.
    def _await_reusable(self, arena):
        arena["ready"].synchronize()                                            # returns at once while nothing was recorded
        arena["used"] = 0

    def _reserve(self, arena, nbytes):
        """Offset of ``nbytes`` (a multiple of 64) in ``arena``, or None when the batch has filled it."""
        with self._lock:
            off = arena["used"]
            if off + nbytes > arena["cap"]:
                return None
            arena["used"] = off + nbytes
            return off

    def _decode_into(self, arena, idx, path, extra):
        """One file -> a slot of its own size in ``arena`` (filtered rows, or pixels), or -> ``extra[idx]`` when the arena is full."""
        t0 = time.perf_counter()
        lib = self._dec
        try:
            with open(path, "rb") as f:
                blob = f.read()
            w, h, ch = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
            rc = lib.tise_png_probe(blob, len(blob), ctypes.byref(w), ctypes.byref(h), ctypes.byref(ch))
            done = False
            if rc == PNG_OK:
                hh, ww = h.value, w.value
                bpp = ch.value if ww * ch.value + 1 <= ROW_MAX else 0           # a row beyond the kernel's limit: unfiltered here (mode 0)
                sb = int(lib.tise_png_slot_bytes(hh, ww, bpp))
                off = self._reserve(arena, sb)
                if off is not None:
                    sc = _scratch(lib.tise_png_scratch_bytes(hh, ww, len(blob)))
                    mode = ctypes.c_int(-1)
                    rc = lib.tise_png_inflate_slot(blob, len(blob), arena["addr"] + off, sb, hh, ww, sc.ctypes.data, sc.size,
                                                   None, None, ctypes.byref(mode))
                    if rc == PNG_OK:
                        arena["offs"][idx] = off
                        arena["hwm"][idx] = (hh, ww, mode.value)
                        if mode.value == 0:
                            with self._lock:
                                self.host_unfiltered += 1
                        done = True
                else:
                    rc, px = _native_rgb(lib, blob, hh, ww)
                    if rc == PNG_OK:
                        extra[idx] = px
                        arena["hwm"][idx] = (hh, ww, -1)
                        with self._lock:
                            self.alone += 1
                        done = True
            if not done:                                                        # outside the subset, or any doubt: Pillow decides or raises
                px = _pillow_rgb(path)
                hh, ww = px.shape[:2]
                sb = SLOT_HDR + ((px.nbytes + 8 + 63) & ~63)
                off = self._reserve(arena, sb) if hh <= 65535 and ww <= 65535 else None
                if off is not None:
                    arena["np"][off:off + SLOT_HDR] = 0
                    arena["np"][off + SLOT_HDR:off + SLOT_HDR + px.nbytes] = px.reshape(-1)
                    arena["offs"][idx] = off
                    arena["hwm"][idx] = (hh, ww, 0)
                else:
                    extra[idx] = np.ascontiguousarray(px)
                    arena["hwm"][idx] = (hh, ww, -1)
                    with self._lock:
                        self.alone += 1
        except Exception as e:                                                  # noqa: BLE001 -- re-raised in the consumer
            raise RuntimeError(f"crop feed: cannot read {path}: {type(e).__name__}: {e}") from e
        self._count(rc, path)
        with self._lock:
            self.decode_seconds += time.perf_counter() - t0

    def _launch(self, arena, nrow, extra, side):
        a = arena
        hwm = a["hwm"][:nrow]
        sizes = [(int(hwm[i, 0]), int(hwm[i, 1])) for i in range(nrow)]
        inside = np.flatnonzero(hwm[:, 2] >= 0)                                 # the images whose slots are in the arena
        offs, total = self._pack(sizes, extra, inside)
        with torch.cuda.stream(side):
            pix = torch.empty(max(total, 16), dtype=torch.uint8, device=self.device)    # this batch's pixels: kept alive by the item
        if len(inside):
            _lib.call("tise_memcpy_h2d_async", a["raw"].data_ptr(), a["addr"], a["used"], side.cuda_stream)
            so = np.ascontiguousarray(a["offs"][:nrow][inside])
            hm = np.ascontiguousarray(hwm[inside])
            oo = np.ascontiguousarray(offs[inside])
            _lib.call("tise_png_unfilter_ragged_rgb8", a["raw"].data_ptr(), a["cap"], len(inside), so.ctypes.data, hm.ctypes.data,
                      oo.ctypes.data, pix.data_ptr(), pix.numel(), a["table"].data_ptr(), a["table"].numel(),
                      a["addr"] + a["cap"], side.cuda_stream)
        return sizes, offs, pix

    def feed_line(self, wall):
        """The ``[tise] crop feed: ...`` line of the CLIs."""
        rows = f"{min(self.item_rows)}..{max(self.item_rows)}" if self.item_rows else "0"
        return self._feed_line(wall, f"{self.native} decoded natively ({self.host_unfiltered} of them unfiltered on the host), {self.pillow} "
                               f"by Pillow{self._why()}, {self.alone} copied on their own", "inflating",
                               f"arena {self.arena_bytes} bytes, items of {rows} images")
