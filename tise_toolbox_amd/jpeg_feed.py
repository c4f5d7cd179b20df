"""JPEG feed of the drop-in CLIs: decode THREADS -> page-locked arenas of coefficient slots -> side-stream H2D ->
IDCT / upsampling / colour conversion in HBM -> device batches of images of any size.

Replaces, for JPEG directories (the real-image side of every comparison: COCO val2014, the CUB photographs), the
hand-over of image_realism/FID/fid_score.py:215-217 -- ``DataLoader(dataset, batch_size, drop_last=True, num_workers=8)``
whose workers run ``Image.open(f).convert("RGB")`` (img_data.py:19-25).  The recipe is the PNG feed's (png_ring.py): the
strictly serial part of a file -- here marker parsing and Huffman decoding -- stays on the host in a small plain-C decoder
(csrc/jpeg_decode.c -> libtise_jpeg.so), everything data-parallel runs on the GPU (csrc/jpeg_idct.hip:
tise_jpeg_reconstruct_rgb8), the result is byte-identical to Pillow, and anything doubtful is handed to Pillow.

  * decode threads (png_ring.auto_workers() of them; ctypes releases the GIL in the call) write one SLOT per file --
    [256-byte header | int16 quantised coefficients], include/tise_jpeg.h -- into one of three page-locked arenas, one arena
    per loader batch; a file the decoder refuses is decoded by Pillow in the same thread and enters the arena as pixels (slot
    mode 0); a file whose pixels do not fit a slot either travels on its own;
  * a feeder thread enqueues ONE host->device copy of the arena and ONE tise_jpeg_reconstruct_rgb8 launch per loader batch on
    device.feed_stream and hands the batch over with an event (the contract of img_data.U8CacheLoader); an arena is reused
    only after the consumer's stream has passed the batch that came out of it;
  * an item is what img_data.collate_u8 makes of the same files: a (B, H, W, 3) device tensor when the batch's images agree
    in size, else a list of (H_i, W_i, 3) device tensors -- engine.coalesce_u8 and RealismEngine.features_from_u8_list treat
    it as they treat the DataLoader's output, so the fp64 sums are the same to the last bit.
``len()`` counts whole ``batch_size`` batches (drop-last, fid_score.py:90-96); order is the order of ``files``.
"""
import ctypes
import os
import queue
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib

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


def load_decoder():
    """libtise_jpeg.so bound with ctypes (once).  A missing library is an error: build it with tise_toolbox_amd.build."""
    global _decoder
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


def _pillow_rgb(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert("RGB"))                                     # img_data.py:21 (a writable copy)


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


class JpegFeedLoader:
    NBUF = 3
    pregrouped = False                     # items are LOADER batches: the consumer coalesces them as it does a DataLoader's

    def __init__(self, files, batch_size, device, workers=None, chunk=4, slot_bytes=None, drop_last=True, item_rows=None):
        self.files = list(files)
        self.bs = int(batch_size)
        self.device = torch.device(device)
        self.drop_last = bool(drop_last)                                       # False (IS*: every image is used): a short last batch
        if self.bs <= 0:
            self.n_rows = 0
        else:
            self.n_rows = (len(self.files) // self.bs) * self.bs if self.drop_last else len(self.files)   # fid_score.py:90-96
        self.files = self.files[:self.n_rows]
        # rows of the consecutive items: loader batches, or -- ``item_rows`` -- a schedule of the caller's (IS*: the device
        # batches of engine.item_schedule, as the PNG ring delivers them, so that both feeds reduce in the same order)
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
        self.slot_bytes = int(slot_bytes) if slot_bytes else 0
        self.native = self.pillow = self.oversize = 0
        self.first_pillow_reason = None
        self.decode_seconds = self.wait_seconds = self.copy_seconds = 0.0      # summed over the decode threads / feeder waiting for them / feeder enqueueing
        self.first_item_event = self.last_item_event = None
        self.first_item_rows = 0
        self._lock = threading.Lock()
        self._pid = os.getpid()
        self._arenas, self._threads, self._stop, self._pool = [], [], None, None

    def __len__(self):
        return -(-self.n_rows // self.bs) if self.bs > 0 else 0

    def _count(self, rc, path):
        with self._lock:
            if rc == TISE_JPEG_OK:
                self.native += 1
            else:
                self.pillow += 1
                if self.first_pillow_reason is None:
                    self.first_pillow_reason = f"{os.path.basename(path)}: {_REASONS.get(rc, rc)}"

    # ---- host consumers (no GPU): the --u8-cache build, CPU tests -----------------------------------------------------------
    def iter_host(self):
        """Loader batches as img_data.collate_u8 makes them, from host decodes (tise_jpeg_decode_rgb8; Pillow for the rest)."""
        from .img_data import collate_u8

        def one(path):
            t0 = time.perf_counter()
            px, rc = decode_file_host(path)
            self._count(rc, path)
            with self._lock:
                self.decode_seconds += time.perf_counter() - t0
            return torch.from_numpy(px)
        with ThreadPoolExecutor(self.workers) as pool:
            st, nb = self.starts, len(self.item_rows)
            pending = [pool.map(one, self.files[st[b]:st[b + 1]]) for b in range(min(2, nb))]
            for b in range(nb):
                if b + 2 < nb:
                    pending.append(pool.map(one, self.files[st[b + 2]:st[b + 3]]))
                yield collate_u8(list(pending.pop(0)))

    # ---- device batches -----------------------------------------------------------------------------------------------------
    def _pick_slot_bytes(self):
        """Slot size of the arenas: the largest coefficient slot among the first files (marker parse only), with a quarter of
        headroom, a multiple of 4096.  Larger files arrive through Pillow."""
        if self.slot_bytes:
            return (self.slot_bytes + 15) & ~15
        return pick_slot_bytes(self.files, max(self.item_rows))

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

    def __iter__(self):
        if not self.n_rows:
            return
        if self.device.type != "cuda":
            yield from self.iter_host()
            return
        dev, bs, nb, starts = self.device, max(self.item_rows), len(self.item_rows), self.starts
        self._dec = load_decoder()
        self.slot_bytes = sb = self._pick_slot_bytes()
        nbuf = min(self.NBUF, nb)
        out_cap = bs * (sb * 3 // 2 + 16)
        ws_bytes = ctypes.c_size_t()
        _lib.call("tise_jpeg_workspace_bytes", bs, sb, ctypes.byref(ws_bytes))
        from .device import feed_stream
        side = feed_stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        arenas = []
        for _ in range(nbuf):
            pinned = torch.empty(bs * sb + bs * 64, dtype=torch.uint8).pin_memory()   # the slots + scratch for the launch's device table
            a = {"pinned": pinned, "np": pinned.numpy(), "addr": pinned.data_ptr(),
                 "raw": torch.empty(bs * sb, dtype=torch.uint8, device=dev), "ws": torch.empty(ws_bytes.value, dtype=torch.uint8, device=dev),
                 "out": torch.empty(out_cap, dtype=torch.uint8, device=dev)}
            for t in (a["raw"], a["ws"], a["out"]):
                t.record_stream(side)
            arenas.append(a)
        self._arenas = arenas
        _LIVE.add(self)
        ready = [torch.cuda.Event() for _ in range(nbuf)]
        consumed = [torch.cuda.Event() for _ in range(nbuf)]
        handed = [threading.Semaphore(1) for _ in range(nbuf)]
        submitted, out = queue.Queue(), queue.Queue()
        stop = threading.Event()
        self._stop = (stop, handed)
        pool = self._pool = ThreadPoolExecutor(self.workers, thread_name_prefix="tise-jpeg-decode")
        side_h = side.cuda_stream

        def submitter():
            try:
                for b in range(nb):
                    k = b % nbuf
                    handed[k].acquire()                                         # the consumer returned arena k ...
                    if stop.is_set():
                        submitted.put(RuntimeError("jpeg feed stopped"))
                        return
                    consumed[k].synchronize()                                   # ... and its stream is past the batch that came out of it
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
                    hdrs = a["np"][:bs * sb].reshape(bs, sb)[:, :12].view(np.int32)        # mode, width, height of every slot
                    sizes = [(int(hdrs[i, 2]), int(hdrs[i, 1])) for i in range(nrow)]
                    dense = not extra and all(s == sizes[0] for s in sizes)
                    offs = np.zeros(nrow, dtype=np.int64)
                    pos = 0
                    for i, (h, w) in enumerate(sizes):
                        offs[i] = pos
                        pos += h * w * 3 if dense else (h * w * 3 + 15) & ~15
                    if pos > out_cap:
                        raise RuntimeError("jpeg feed: a batch's pixels exceed the output buffer")
                    tw = time.perf_counter()
                    _lib.call("tise_memcpy_h2d_async", a["raw"].data_ptr(), a["addr"], nrow * sb, side_h)
                    _lib.call("tise_jpeg_reconstruct_rgb8", a["raw"].data_ptr(), nrow, sb, a["addr"], sb, offs.ctypes.data,
                              a["out"].data_ptr(), out_cap, a["ws"].data_ptr(), ws_bytes.value, a["addr"] + bs * sb, side_h)
                    if dense:
                        h, w = sizes[0]
                        batch = a["out"][:nrow * h * w * 3].view(nrow, h, w, 3)
                    else:
                        batch = []
                        with torch.cuda.stream(side):
                            for i, (h, w) in enumerate(sizes):
                                if i in extra:                                   # a file beyond the slots: Pillow's pixels, copied on their own
                                    batch.append(torch.from_numpy(extra[i]).to(dev))
                                else:
                                    batch.append(a["out"][int(offs[i]):int(offs[i]) + h * w * 3].view(h, w, 3))
                    ready[k].record(side)
                    self.copy_seconds += time.perf_counter() - tw
                    out.put((k, batch))
            except BaseException as e:                                          # noqa: BLE001 -- re-raised in the consumer
                out.put(e)

        self._threads = [threading.Thread(target=submitter, name="tise-jpeg-submit", daemon=True),
                         threading.Thread(target=feeder, name="tise-jpeg-feeder", daemon=True)]
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
                k, batch = item
                cur = torch.cuda.current_stream(dev)
                if b == 1:
                    self.first_item_rows = self.item_rows[0]
                    self.first_item_event = torch.cuda.Event(enable_timing=True)
                    self.first_item_event.record(cur)
                cur.wait_event(ready[k])
                if isinstance(batch, list):
                    for t in batch:
                        if t.untyped_storage().data_ptr() != arenas[k]["out"].untyped_storage().data_ptr():
                            t.record_stream(cur)                                # allocated on the side stream, used on the consumer's
                yield batch
                item = batch = None
                consumed[k].record(torch.cuda.current_stream(dev))
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
        """The ``[tise] jpeg feed: ...`` line of the CLIs."""
        n = self.native + self.pillow
        steady = ""
        sec = self.steady_seconds() if self.device.type == "cuda" else None
        if sec and n > self.first_item_rows:
            steady = f"; after the first batch {(n - self.first_item_rows) / sec:.0f} images/s"
        why = f" (first: {self.first_pillow_reason})" if self.first_pillow_reason else ""
        return (f"[tise] jpeg feed: {n} images in {wall:.2f} s ({n / max(wall, 1e-9):.0f} images/s on this rank{steady}); {self.native} decoded "
                f"natively, {self.pillow} by Pillow{why}; {self.workers} decode threads: {self.decode_seconds:.2f} s of entropy decoding "
                f"summed over the threads, feeder waited {self.wait_seconds:.2f} s for them and spent {self.copy_seconds:.2f} s on copies "
                f"and launches; slot {self.slot_bytes} bytes, items of {min(self.item_rows)}..{max(self.item_rows)} images")


import weakref  # noqa: E402
_LIVE = weakref.WeakSet()                  # loaders that hold page-locked arenas


def _close_all():
    for ld in list(_LIVE):
        try:
            ld.close()
        except Exception:                                                       # noqa: BLE001
            pass


if hasattr(os, "register_at_fork"):
    os.register_at_fork(before=_close_all)
