"""The pipeline the JPEG feed (jpeg_feed.py) and the crop feed (crop_feed.py) share: decode THREADS -> page-locked arenas ->
side-stream H2D -> one launch per loader batch in HBM -> device batches of images of any size.

  * decode threads (png_ring.auto_workers() of them; ctypes releases the GIL in the call) fill one of NBUF page-locked arenas,
    one arena per loader batch (``_decode_into``); an image the arena cannot take travels on its own (``extra``);
  * a feeder thread enqueues the host->device copy of the arena and ONE launch per loader batch on device.feed_stream
    (``_launch``) and hands the batch over with an event (the contract of img_data.U8CacheLoader);
  * an item is what img_data.collate_u8 makes of the same files: a (B, H, W, 3) device tensor when the batch's images agree in
    size, else a list of (H_i, W_i, 3) device tensors -- engine.coalesce_batches and RealismEngine.features_from_u8_list treat
    it as they treat the DataLoader's output, so the fp64 sums are the same to the last bit;
  * WHEN an arena may be refilled depends on what the items view, so each feed states its own rule (``_await_reusable``,
    ``_handed_back``); the two rules are not interchangeable.
A feed supplies ``FEED``, ``OK``, ``REASONS``, ``_decode_file_host``, ``_make_arenas``, ``_decode_into``, ``_launch``, the
reuse rule, ``__len__`` and ``feed_line``.  Order is the order of ``files``.
"""
import os
import queue
import threading
import time
import weakref
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch


def _pillow_rgb(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert("RGB"))                                     # img_data.py:21 (a writable copy)


def _is_dense(sizes, extra):
    return not extra and all(s == sizes[0] for s in sizes)


class ArenaFeedLoader:
    NBUF = 3
    pregrouped = False                     # items are LOADER batches: the consumer coalesces them as it does a DataLoader's
    FEED = None                            # "jpeg" / "crop": thread names, the "stopped" message, the feed line
    OK = 0                                 # the native decoder's status for a file it took
    REASONS = {}                           # its other statuses, in words

    def __init__(self, files, batch_size, device, workers, chunk, drop_last, item_rows):
        self.files = list(files)
        self.bs = int(batch_size)
        self.device = torch.device(device)
        self.drop_last = bool(drop_last)                                       # False (IS*, --per-class, O-IS: every image is used): a short last batch
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
        self.native = self.pillow = 0
        self.first_pillow_reason = None
        self.decode_seconds = self.wait_seconds = self.copy_seconds = 0.0      # summed over the decode threads / feeder waiting for them / feeder enqueueing
        self.first_item_event = self.last_item_event = None
        self.first_item_rows = 0
        self._lock = threading.Lock()
        self._pid = os.getpid()
        self._arenas, self._threads, self._stop, self._pool = [], [], None, None

    def _count(self, rc, path):
        with self._lock:
            if rc == self.OK:
                self.native += 1
            else:
                self.pillow += 1
                if self.first_pillow_reason is None:
                    self.first_pillow_reason = f"{os.path.basename(path)}: {self.REASONS.get(rc, rc)}"

    # ---- host consumers (no GPU): the --u8-cache build, CPU tests -----------------------------------------------------------
    def iter_host(self):
        """Loader batches as img_data.collate_u8 makes them, from host decodes (the native decoder; Pillow for the rest)."""
        from .img_data import collate_u8

        def one(path):
            t0 = time.perf_counter()
            px, rc = self._decode_file_host(path)
            self._count(rc, path)
            with self._lock:
                self.decode_seconds += time.perf_counter() - t0
            return torch.from_numpy(px)
        pool = ThreadPoolExecutor(self.workers, thread_name_prefix=f"tise-{self.FEED}-decode")
        try:
            st, nb = self.starts, len(self.item_rows)
            pending = [pool.map(one, self.files[st[b]:st[b + 1]]) for b in range(min(2, nb))]
            for b in range(nb):
                if b + 2 < nb:
                    pending.append(pool.map(one, self.files[st[b + 2]:st[b + 3]]))
                yield collate_u8(list(pending.pop(0)))
        finally:
            pool.shutdown(wait=True, cancel_futures=True)                       # an error or a consumer that walks away: queued decodes are dropped

    # ---- device batches -----------------------------------------------------------------------------------------------------
    def _make_arenas(self, nbuf, rows, dev):
        """``nbuf`` arenas for loader batches of up to ``rows`` files: dicts with "pinned" (page-locked tensor), "np" (its numpy
        view), "addr", the arena's device tensors and whatever the feed's own methods keep there."""
        raise NotImplementedError

    def _decode_into(self, arena, idx, path, extra):
        """One file -> ``arena`` as image ``idx`` of its batch, or -> ``extra[idx]`` (pixels) when the arena cannot take it."""
        raise NotImplementedError

    def _launch(self, arena, nrow, extra, side):
        """Enqueue the copy and the launch of a filled arena on ``side``.  Returns the (h, w) of the ``nrow`` images, the byte
        offsets of their pixels (``_pack``) and the device buffer those offsets refer to."""
        raise NotImplementedError

    def _await_reusable(self, arena):
        """Block the submitter until ``arena`` may be refilled (the consumer has already handed its last batch back)."""
        raise NotImplementedError

    def _handed_back(self, arena, stream):
        """The consumer, on ``stream``, has given back the item that came out of ``arena``."""

    @staticmethod
    def _pack(sizes, extra, rows):
        """(offsets, total bytes) of the pixels of images ``rows`` in one buffer: end to end when the item is dense, else 16
        bytes aligned."""
        dense = _is_dense(sizes, extra)
        offs = np.zeros(len(sizes), dtype=np.int64)
        pos = 0
        for i in rows:
            offs[i] = pos
            h, w = sizes[i]
            pos += h * w * 3 if dense else (h * w * 3 + 15) & ~15
        return offs, pos

    def __iter__(self):
        if not self.n_rows:
            return
        if self.device.type != "cuda":
            yield from self.iter_host()
            return
        dev, nb, starts = self.device, len(self.item_rows), self.starts
        nbuf = min(self.NBUF, nb)
        from .device import feed_stream
        side = feed_stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        arenas = self._make_arenas(nbuf, max(self.item_rows), dev)
        for a in arenas:
            a["ready"] = torch.cuda.Event()                                     # the side stream has done the batch out of this arena
            a["device"] = [t for t in a.values() if torch.is_tensor(t) and t.is_cuda]
            for t in a["device"]:
                t.record_stream(side)
        self._arenas = arenas
        _LIVE.add(self)
        handed = [threading.Semaphore(1) for _ in range(nbuf)]
        submitted, out = queue.Queue(), queue.Queue()
        stop = threading.Event()
        self._stop = (stop, handed)
        pool = self._pool = ThreadPoolExecutor(self.workers, thread_name_prefix=f"tise-{self.FEED}-decode")

        def submitter():
            try:
                for b in range(nb):
                    k = b % nbuf
                    handed[k].acquire()                                         # the consumer returned arena k ...
                    if stop.is_set():
                        submitted.put(RuntimeError(f"{self.FEED} feed stopped"))
                        return
                    self._await_reusable(arenas[k])                             # ... and the feed's reuse rule holds
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
                    tw = time.perf_counter()
                    sizes, offs, buf = self._launch(a, nrow, extra, side)
                    fresh = [buf] if all(buf is not t for t in a["device"]) else []     # tensors allocated on the side stream
                    if _is_dense(sizes, extra):
                        h, w = sizes[0]
                        batch = buf[:nrow * h * w * 3].view(nrow, h, w, 3)
                    else:
                        batch = []
                        with torch.cuda.stream(side):
                            for i, (h, w) in enumerate(sizes):
                                if i in extra:                                   # an image beyond the arena: its pixels, copied on their own
                                    batch.append(torch.from_numpy(extra[i]).to(dev))
                                    fresh.append(batch[-1])
                                else:
                                    batch.append(buf[int(offs[i]):int(offs[i]) + h * w * 3].view(h, w, 3))
                    a["ready"].record(side)
                    self.copy_seconds += time.perf_counter() - tw
                    out.put((k, batch, fresh))
            except BaseException as e:                                          # noqa: BLE001 -- re-raised in the consumer
                out.put(e)

        self._threads = [threading.Thread(target=submitter, name=f"tise-{self.FEED}-submit", daemon=True),
                         threading.Thread(target=feeder, name=f"tise-{self.FEED}-feeder", daemon=True)]
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
                k, batch, fresh = item
                cur = torch.cuda.current_stream(dev)
                if b == 1:
                    self.first_item_rows = self.item_rows[0]
                    self.first_item_event = torch.cuda.Event(enable_timing=True)
                    self.first_item_event.record(cur)
                cur.wait_event(arenas[k]["ready"])
                for t in fresh:
                    t.record_stream(cur)                                        # allocated on the side stream, used on the consumer's
                yield batch
                item = batch = fresh = None
                self._handed_back(arenas[k], torch.cuda.current_stream(dev))
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

    def _feed_line(self, wall, decoded, work, tail):
        """``[tise] <feed> feed: <count, rates>; <decoded>; <threads and their seconds of <work>>; <tail>``."""
        n = self.native + self.pillow
        steady = ""
        sec = self.steady_seconds() if self.device.type == "cuda" else None
        if sec and n > self.first_item_rows:
            steady = f"; after the first batch {(n - self.first_item_rows) / sec:.0f} images/s"
        return (f"[tise] {self.FEED} feed: {n} images in {wall:.2f} s ({n / max(wall, 1e-9):.0f} images/s on this rank{steady}); {decoded}; "
                f"{self.workers} decode threads: {self.decode_seconds:.2f} s of {work} summed over the threads, feeder waited "
                f"{self.wait_seconds:.2f} s for them and spent {self.copy_seconds:.2f} s on copies and launches; {tail}")

    def _why(self):
        return f" (first: {self.first_pillow_reason})" if self.first_pillow_reason else ""


_LIVE = weakref.WeakSet()                  # loaders of either feed that hold page-locked arenas


def _close_all():
    for ld in list(_LIVE):
        try:
            ld.close()
        except Exception:                                                       # noqa: BLE001
            pass


if hasattr(os, "register_at_fork"):
    os.register_at_fork(before=_close_all)
