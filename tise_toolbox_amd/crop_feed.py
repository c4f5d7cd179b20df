"""PNG feed for directories whose images differ in size -- the cropped-object directories behind O-FID, ``--per-class`` O-FID
and O-IS (``{stem}_{class}_{k}.png``, object_fidelity/crop_object.py:45: one size per crop): decode THREADS -> page-locked
arenas of packed inflate-only slots -> side-stream H2D -> the row filters of ALL images of a loader batch reversed by one
launch in HBM -> device batches of images of any size.

Replaces, for such directories, the hand-over of object_fidelity/O-FID/fid_score.py:215-217 and
object_fidelity/O-IS/object_centric_inception_score.py:31-33 -- a ``DataLoader`` whose workers run
``Image.open(f).convert("RGB")`` and pickle every crop to the main process, which then copied each crop to the device on its
own.  The recipe is jpeg_feed.JpegFeedLoader's, with the PNG ring's division of labour (png_ring.py): the strictly serial part
of a file -- chunk parsing, CRC-32, zlib inflate -- stays on the host (csrc/png_decode.c -> libtise_png.so, bound with ctypes,
which releases the GIL in the call), the row filters run on the GPU (csrc/png_unfilter.hip: tise_png_unfilter_ragged_rgb8), the
result is byte-identical to Pillow, and anything doubtful is handed to Pillow.

  * decode threads (png_ring.auto_workers() of them) probe a file, reserve a slot of ITS size -- [64-byte header | filtered
    rows], include/tise_png.h -- at the next 64-byte aligned offset of one of three page-locked arenas, one arena per loader
    batch, and inflate into it; a file outside the native subset (palette, gray, 16-bit, interlaced, any CRC doubt) is decoded
    by Pillow in the same thread and enters the arena as pixels (slot mode 0), as does a file whose rows exceed the kernel's
    8192 bytes (decoded natively); a file the arena has no room left for travels on its own;
  * a feeder thread enqueues ONE host->device copy of the arena's used part and ONE tise_png_unfilter_ragged_rgb8 launch per
    loader batch on device.feed_stream and hands the batch over with an event (the contract of img_data.U8CacheLoader).  The
    pixels of a batch live in a device buffer of their own that the item's tensors keep alive -- engine.coalesce_batches gathers
    the ragged items of many loader batches into one trunk pass -- so an arena (page-locked slots + their device copy) is
    reused once the consumer has moved past the batch that came out of it AND the side stream has finished reading it;
  * an item is what img_data.collate_u8 makes of the same files: a (B, H, W, 3) device tensor when the batch's images agree
    in size, else a list of (H_i, W_i, 3) device tensors -- engine.coalesce_batches and RealismEngine.features_from_u8_list
    treat it as they treat the DataLoader's output, so the fp64 sums are the same to the last bit.
``len()`` counts loader batches (``drop_last``: whole ones only, fid_score.py:90-96); order is the order of ``files``.
"""
import ctypes
import os
import queue
import threading
import time
import weakref
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib

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


def _pillow_rgb(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert("RGB"))                                     # img_data.py:21 (a writable copy)


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


class CropFeedLoader:
    NBUF = 3
    pregrouped = False                     # items are LOADER batches: the consumer coalesces them as it does a DataLoader's

    def __init__(self, files, batch_size, device, workers=None, chunk=8, arena_bytes=None, drop_last=True, item_rows=None):
        self.files = list(files)
        self.bs = int(batch_size)
        self.device = torch.device(device)
        self.drop_last = bool(drop_last)                                       # False (--per-class, O-IS: every crop is used): a short last batch
        if self.bs <= 0:
            self.n_rows = 0
        else:
            self.n_rows = (len(self.files) // self.bs) * self.bs if self.drop_last else len(self.files)   # fid_score.py:90-96
        self.files = self.files[:self.n_rows]
        self.item_rows = [min(self.bs, self.n_rows - r) for r in range(0, self.n_rows, self.bs)] if self.bs > 0 else []
        if item_rows is not None:
            assert sum(item_rows) == self.n_rows and all(r > 0 for r in item_rows)
            self.item_rows = list(item_rows)
        self.starts = [0]
        for r in self.item_rows:
            self.starts.append(self.starts[-1] + r)
        from .png_ring import auto_workers
        self.workers = int(workers) if workers else auto_workers()
        self.chunk = max(1, int(chunk))
        self.arena_bytes = int(arena_bytes) if arena_bytes else 0
        self.native = self.pillow = self.alone = self.host_unfiltered = 0
        self.first_pillow_reason = None
        self.decode_seconds = self.wait_seconds = self.copy_seconds = 0.0      # summed over the decode threads / feeder waiting for them / feeder enqueueing
        self.first_item_event = self.last_item_event = None
        self.first_item_rows = 0
        self._lock = threading.Lock()
        self._pid = os.getpid()
        self._arenas, self._threads, self._stop, self._pool = [], [], None, None

    def __len__(self):
        return len(self.item_rows)

    def _count(self, rc, path):
        with self._lock:
            if rc == PNG_OK:
                self.native += 1
            else:
                self.pillow += 1
                if self.first_pillow_reason is None:
                    self.first_pillow_reason = f"{os.path.basename(path)}: {_REASONS.get(rc, rc)}"

    # ---- host consumers (no GPU): CPU tests ---------------------------------------------------------------------------------
    def iter_host(self):
        """Loader batches as img_data.collate_u8 makes them, from host decodes (tise_png_decode_rgb8; Pillow for the rest)."""
        from .img_data import collate_u8

        def one(path):
            t0 = time.perf_counter()
            px, rc = decode_file_host(path)
            self._count(rc, path)
            with self._lock:
                self.decode_seconds += time.perf_counter() - t0
            return torch.from_numpy(px)
        pool = ThreadPoolExecutor(self.workers, thread_name_prefix="tise-crop-decode")
        try:
            st, nb = self.starts, len(self.item_rows)
            pending = [pool.map(one, self.files[st[b]:st[b + 1]]) for b in range(min(2, nb))]
            for b in range(nb):
                if b + 2 < nb:
                    pending.append(pool.map(one, self.files[st[b + 2]:st[b + 3]]))
                yield collate_u8(list(pending.pop(0)))
        finally:
            pool.shutdown(wait=True, cancel_futures=True)

    # ---- device batches -----------------------------------------------------------------------------------------------------
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

    def __iter__(self):
        if not self.n_rows:
            return
        if self.device.type != "cuda":
            yield from self.iter_host()
            return
        dev, bs, nb, starts = self.device, max(self.item_rows), len(self.item_rows), self.starts
        self._dec = load_decoder()
        _lib.load()
        cap = self.arena_bytes = ((self.arena_bytes + 63) & ~63) if self.arena_bytes else pick_arena_bytes(self.files, bs)
        nbuf = min(self.NBUF, nb)
        from .device import feed_stream
        side = feed_stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        arenas = []
        for _ in range(nbuf):
            pinned = torch.empty(cap + bs * TABLE_ENTRY, dtype=torch.uint8).pin_memory()   # the slots + scratch for the launch's device table
            a = {"pinned": pinned, "np": pinned.numpy(), "addr": pinned.data_ptr(), "cap": cap, "used": 0,
                 "offs": np.zeros(bs, dtype=np.int64), "hwm": np.zeros((bs, 3), dtype=np.int32),
                 "raw": torch.empty(cap, dtype=torch.uint8, device=dev), "table": torch.empty(bs * TABLE_ENTRY, dtype=torch.uint8, device=dev)}
            for t in (a["raw"], a["table"]):
                t.record_stream(side)
            arenas.append(a)
        self._arenas = arenas
        _LIVE.add(self)
        ready = [torch.cuda.Event() for _ in range(nbuf)]
        handed = [threading.Semaphore(1) for _ in range(nbuf)]
        used_once = [False] * nbuf
        submitted, out = queue.Queue(), queue.Queue()
        stop = threading.Event()
        self._stop = (stop, handed)
        pool = self._pool = ThreadPoolExecutor(self.workers, thread_name_prefix="tise-crop-decode")
        side_h = side.cuda_stream

        def submitter():
            try:
                for b in range(nb):
                    k = b % nbuf
                    handed[k].acquire()                                         # the consumer has moved past the batch out of arena k ...
                    if stop.is_set():
                        submitted.put(RuntimeError("crop feed stopped"))
                        return
                    if used_once[k]:
                        ready[k].synchronize()                                  # ... and the side stream has read the arena (copy + unfilter launch)
                    arenas[k]["used"] = 0
                    extra = {}
                    files = self.files[starts[b]:starts[b + 1]]
                    futs = [pool.submit(lambda lo=lo, k=k, files=files, extra=extra: [self._decode_into(arenas[k], i, files[i], extra)
                                                                                      for i in range(lo, min(lo + self.chunk, len(files)))])
                            for lo in range(0, len(files), self.chunk)]
                    submitted.put((k, futs, extra))
            except BaseException as e:                                          # noqa: BLE001 -- re-raised in the consumer
                submitted.put(e)

        def feeder():
            try:
                torch.cuda.set_device(dev)
                for b in range(nb):
                    item = submitted.get()
                    if isinstance(item, BaseException):
                        raise item
                    k, futs, extra = item
                    tw = time.perf_counter()
                    for f in futs:
                        f.result()
                    self.wait_seconds += time.perf_counter() - tw
                    if stop.is_set():
                        return
                    a = arenas[k]
                    nrow = self.item_rows[b]
                    hwm = a["hwm"][:nrow]
                    sizes = [(int(hwm[i, 0]), int(hwm[i, 1])) for i in range(nrow)]
                    dense = not extra and all(s == sizes[0] for s in sizes)
                    inside = np.flatnonzero(hwm[:, 2] >= 0)                     # the images whose slots are in the arena
                    offs = np.zeros(nrow, dtype=np.int64)
                    pos = 0
                    for i in inside:
                        offs[i] = pos
                        h, w = sizes[i]
                        pos += h * w * 3 if dense else (h * w * 3 + 15) & ~15
                    tw = time.perf_counter()
                    with torch.cuda.stream(side):
                        pix = torch.empty(max(pos, 16), dtype=torch.uint8, device=dev)      # this batch's pixels: kept alive by the item
                    if len(inside):
                        _lib.call("tise_memcpy_h2d_async", a["raw"].data_ptr(), a["addr"], a["used"], side_h)
                        so = np.ascontiguousarray(a["offs"][:nrow][inside])
                        hm = np.ascontiguousarray(hwm[inside])
                        oo = np.ascontiguousarray(offs[inside])
                        _lib.call("tise_png_unfilter_ragged_rgb8", a["raw"].data_ptr(), cap, len(inside), so.ctypes.data, hm.ctypes.data,
                                  oo.ctypes.data, pix.data_ptr(), pix.numel(), a["table"].data_ptr(), a["table"].numel(),
                                  a["addr"] + cap, side_h)
                    if dense:
                        h, w = sizes[0]
                        batch = pix[:nrow * h * w * 3].view(nrow, h, w, 3)
                    else:
                        batch = []
                        with torch.cuda.stream(side):
                            for i, (h, w) in enumerate(sizes):
                                if i in extra:                                   # a file beyond the arena: its pixels, copied on their own
                                    batch.append(torch.from_numpy(extra[i]).to(dev))
                                else:
                                    batch.append(pix[int(offs[i]):int(offs[i]) + h * w * 3].view(h, w, 3))
                    ready[k].record(side)
                    used_once[k] = True
                    self.copy_seconds += time.perf_counter() - tw
                    out.put((k, batch, pix))
            except BaseException as e:                                          # noqa: BLE001 -- re-raised in the consumer
                out.put(e)

        self._threads = [threading.Thread(target=submitter, name="tise-crop-submit", daemon=True),
                         threading.Thread(target=feeder, name="tise-crop-feeder", daemon=True)]
        for th in self._threads:
            th.start()
        try:
            for b in range(nb):
                item = out.get()
                if isinstance(item, BaseException):
                    try:
                        raise item
                    finally:
                        item = None                                             # no cycle through this frame (png_ring.PngRingLoader.__iter__)
                k, batch, pix = item
                cur = torch.cuda.current_stream(dev)
                if b == 1:
                    self.first_item_rows = self.item_rows[0]
                    self.first_item_event = torch.cuda.Event(enable_timing=True)
                    self.first_item_event.record(cur)
                cur.wait_event(ready[k])
                pix.record_stream(cur)                                          # allocated on the side stream, used on the consumer's
                if isinstance(batch, list):
                    for t in batch:
                        if t.untyped_storage().data_ptr() != pix.untyped_storage().data_ptr():
                            t.record_stream(cur)
                yield batch
                item = batch = pix = None
                handed[k].release()
            if self.first_item_event is not None:
                self.last_item_event = torch.cuda.Event(enable_timing=True)
                self.last_item_event.record(torch.cuda.current_stream(dev))
        finally:
            self.close()

    def steady_seconds(self):
        """Device time between the end of the first and of the last loader batch's work (None with fewer than two)."""
        if self.first_item_event is None or self.last_item_event is None:
            return None
        self.last_item_event.synchronize()
        return self.first_item_event.elapsed_time(self.last_item_event) * 1e-3

    def close(self):
        """Stop the threads, drain the side stream and release the page-locked arenas (also before any fork: a child of a
        process that holds page-locked memory crashes inside the HIP runtime, see png_ring.py)."""
        if os.getpid() != getattr(self, "_pid", os.getpid()):
            return
        if self._stop is not None:
            stop, handed = self._stop
            self._stop = None
            stop.set()
            for h in handed:
                h.release()
            for th in self._threads:
                th.join()
            self._threads = []
        if self._pool is not None:
            self._pool.shutdown(wait=True, cancel_futures=True)
            self._pool = None
        if self._arenas:
            if self.device.type == "cuda":
                from .device import feed_stream
                feed_stream(self.device).synchronize()
            self._arenas = []                                                   # drops the pinned tensors: torch unpins on release
            _LIVE.discard(self)

    def __del__(self):
        try:
            self.close()
        except Exception:                                                       # noqa: BLE001
            pass

    def feed_line(self, wall):
        """The ``[tise] crop feed: ...`` line of the CLIs."""
        n = self.native + self.pillow
        steady = ""
        sec = self.steady_seconds() if self.device.type == "cuda" else None
        if sec and n > self.first_item_rows:
            steady = f"; after the first batch {(n - self.first_item_rows) / sec:.0f} images/s"
        why = f" (first: {self.first_pillow_reason})" if self.first_pillow_reason else ""
        rows = f"{min(self.item_rows)}..{max(self.item_rows)}" if self.item_rows else "0"
        return (f"[tise] crop feed: {n} images in {wall:.2f} s ({n / max(wall, 1e-9):.0f} images/s on this rank{steady}); {self.native} decoded "
                f"natively ({self.host_unfiltered} of them unfiltered on the host), {self.pillow} by Pillow{why}, {self.alone} copied on their "
                f"own; {self.workers} decode threads: {self.decode_seconds:.2f} s of inflating summed over the threads, feeder waited "
                f"{self.wait_seconds:.2f} s for them and spent {self.copy_seconds:.2f} s on copies and launches; arena {self.arena_bytes} "
                f"bytes, items of {rows} images")


_LIVE = weakref.WeakSet()                  # loaders that hold page-locked arenas


def _close_all():
    for ld in list(_LIVE):
        try:
            ld.close()
        except Exception:                                                       # noqa: BLE001
            pass


if hasattr(os, "register_at_fork"):
    os.register_at_fork(before=_close_all)
