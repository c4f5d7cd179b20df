"""Which feed serves an image set, and the life cycle around it: the one place every CLI goes through.  A consumer
names its ``Site`` and hands ``run`` this rank's files and a ``consume(loader)`` (how a batch is used, what is accumulated: its own);
``run`` picks the loader (``choose``), builds it, times ``consume``, closes the loader whatever happens, prints the feed line on the
main rank, remembers the loader in ``last`` and applies the one ragged-directory rule (the PNG ring has one slot shape)."""
import os
import sys
import threading
import time
from collections import namedtuple
from dataclasses import dataclass

import torch
import torch.utils.data

from . import dist as tdist, img_data, png_ring
from .engine import device_batch_images
from .hostinfo import cfs_throttle


@dataclass(frozen=True)
class Options:
    """The feed flags of the CLIs: --png-feed ring | dataloader (the IS CLIs spell it "loader"), --jpeg-feed None | native | pillow
    (jpeg_feed.use_native), --crop-feed None | native | dataloader (crop_feed.use_native), --num-workers (0 / None: auto)."""
    png_feed: str = "ring"
    jpeg_feed: str = None
    crop_feed: str = None
    num_workers: int = 0

    def __post_init__(self):
        object.__setattr__(self, "png_feed", "dataloader" if self.png_feed == "loader" else self.png_feed)


# A consumer's fixed policy.  kinds: the loaders it allows, in priority order; drop_last: whole loader batches only (the reference's
# FID) or every image; crop_on_request: the crop feed only for --crop-feed native (a plain directory: otherwise --png-feed decides),
# not on crop_feed.use_native's probe; ring_when_empty: a rank without files still takes the ring's road (nothing is started, no
# DataLoader workers are forked); png_line: the ring and the DataLoader print "[tise] png feed" (bench.py reads it); ragged_raises:
# under torchrun a rank that meets a ragged directory raises -- its consume holds collectives (False: RP / PA embed per rank).
Site = namedtuple("Site", "kinds drop_last crop_on_request ring_when_empty png_line ragged_raises", defaults=(False, False, False, True))
FID = Site(("jpeg", "crop", "ring", "dataloader"), True, crop_on_request=True, ring_when_empty=True, png_line=True)
FID_ALL = FID._replace(drop_last=False)                           # fid_score --mode clean: the FID site, every image used
CROPS = Site(("crop", "dataloader"), False)                       # fid_score --per-class, O-IS
IS = Site(("jpeg", "ring", "dataloader"), False)
PAIRED = Site(("jpeg", "ring", "dataloader"), False)              # paired.py, side one of the pairs: every image used, the kinds of IS
CLIP = Site(("ring", "dataloader"), False, ragged_raises=False)   # RP_coco, PA

Last = namedtuple("Last", "kind loader")
last = Last(None, None)              # the most recent session, finished or failed (tests and tools/*_feed_probe.py read it)
_RING_PREFETCH = {}                  # directory -> PngRingLoader whose workers are already decoding (started before the model was built)
_RING_LOCK = threading.Lock()        # the second directory's prefetch is started from the first loader's feeder thread


def resolve_workers(num_workers, world=1):
    return int(num_workers) if num_workers and int(num_workers) > 0 else png_ring.auto_workers(world)


def u8_dataloader(files_or_dataset, batch_size, workers, drop_last, pin_memory=True, collate=img_data.collate_u8, max_workers=32):
    """The DataLoader road: decoded uint8 HWC images of a file list, stacked or -- ragged -- listed by img_data.collate_u8.  A caller's
    own dataset is taken as it is (O-IS: a Subset, maybe of float tensors, exactly ``workers`` processes; RP / PA: clip's preprocess)."""
    dataset = files_or_dataset if isinstance(files_or_dataset, torch.utils.data.Dataset) else img_data.Dataset(None, None, files_or_dataset)
    n = workers if max_workers is None else min(max_workers, workers)
    return torch.utils.data.DataLoader(dataset, batch_size=batch_size, shuffle=False, drop_last=drop_last, num_workers=n, collate_fn=collate,
                                       pin_memory=pin_memory, worker_init_fn=img_data.worker_init)


def choose(files, options, allow):
    """-> "jpeg" | "crop" | "ring" | "dataloader": the first kind of the Site ``allow`` that the flags and the first files of this
    rank's ``files`` admit.  Probes files (jpeg_feed.use_native, crop_feed.use_native); builds nothing, calls no GPU."""
    from . import crop_feed, jpeg_feed
    ring = options.png_feed == "ring"
    for kind in allow.kinds:
        if kind == "jpeg" and ring and files and jpeg_feed.use_native(files, options.jpeg_feed):
            return kind
        if kind == "crop" and ((options.crop_feed == "native" and files) if allow.crop_on_request else crop_feed.use_native(files, options.crop_feed)):
            return kind
        if kind == "ring" and ring and (files or allow.ring_when_empty) or kind == "dataloader":
            return kind
    raise ValueError(f"no feed among {allow.kinds} for {options}")


def build_loader(kind, files, device, batch_size, workers, drop_last, **kw):
    """The loader of ``kind`` over ``files``; ``kw``: what a site passes beyond the common arguments."""
    if kind in ("jpeg", "crop"):
        from . import crop_feed, jpeg_feed
        cls = jpeg_feed.JpegFeedLoader if kind == "jpeg" else crop_feed.CropFeedLoader
        return cls(files, batch_size, device, workers=workers, drop_last=drop_last, **kw)
    if kind == "ring":                   # whole batches of ITS batch size; items are device batches (engine.device_batch_images)
        kw.setdefault("group", device_batch_images(batch_size) // batch_size)
        return png_ring.PngRingLoader(files, batch_size, device, workers=workers, start=True, **kw)
    return u8_dataloader(kw.pop("dataset", files), batch_size, workers, drop_last, **kw)


def prefetch_png_ring(path, batch_size, options):
    """Start the decode workers of an image directory NOW (before the model is built / while the other side is still in the
    network): the FID site's ``run(..., prefetch_key=path)`` picks the running loader up.  No GPU call is made here."""
    if options.png_feed != "ring" or path.endswith(".npz") or not os.path.isdir(path):
        return None
    with _RING_LOCK:
        if path not in _RING_PREFETCH:
            rank, world, local_rank = tdist.env_world()
            shard, _ = tdist.shard_files(img_data.get_filenames(path), batch_size, rank, world)
            if not shard or choose(shard, options, FID) != "ring":
                return None
            dev = torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_initialized() else local_rank)
            _RING_PREFETCH[path] = build_loader("ring", shard, dev, batch_size, resolve_workers(options.num_workers, world), True)
        return _RING_PREFETCH[path]


def session(kind, loader, consume, line=None):
    """``consume(loader)`` once, timed.  The loader is closed on every road out (the ring: its feeder thread is stopped and joined
    before the ring is unregistered); after a success ``line(seconds)`` is printed on the main rank."""
    global last
    last = Last(kind, loader)
    t0 = time.perf_counter()
    try:
        out = consume(loader)
    finally:
        if hasattr(loader, "close"):
            loader.close()
    if line is not None and tdist.is_main():
        print(line(time.perf_counter() - t0), file=sys.stderr)
    return out


def _alloc_trace():
    """TISE_ALLOC_TRACE=1 (probe): how much of the loop went into hipMalloc (caching allocator misses)."""
    st = torch.cuda.memory_stats() if os.environ.get("TISE_ALLOC_TRACE") == "1" else None
    return "" if st is None else (f"; allocator: {st.get('num_device_alloc', 0)} device allocations, "
                                  f"{st.get('reserved_bytes.all.peak', 0) / 2**30:.1f} GiB reserved, {st.get('num_alloc_retries', 0)} retries")


def _png_line(kind, loader, n, batch_size):
    """The "[tise] png feed" line of the ring / of the DataLoader, as a function of the seconds the loop took."""
    tail = f"loader batch {batch_size}, device batch {device_batch_images(batch_size)})"
    if kind == "dataloader":
        return lambda wall: (f"[tise] png feed: {n} images in {wall:.2f} s ({n / wall:.0f} images/s on this rank, {loader.num_workers} "
                             f"DataLoader decode workers, {tail}")
    thr0 = cfs_throttle()

    def line(wall):
        sec = loader.steady_seconds()
        steady = f"; after the first device batch {(n - loader.first_item_rows) / sec:.0f} images/s" if sec else ""
        dec = f", all decoded {loader.decode_seconds:.2f} s after the workers started" if loader.decode_seconds else ""
        thr1 = cfs_throttle()
        dec += _alloc_trace()
        dec += (f"; feeder waited {loader.wait_decode_seconds:.2f} s for decode, {loader.wait_buffer_seconds:.2f} s for a device buffer, "
                f"{loader.wait_copy_seconds + loader.enqueue_seconds:.2f} s on copies; cgroup CPU throttling during the loop: "
                f"{thr1[0] - thr0[0]} periods, {(thr1[1] - thr0[1]) / 1e3:.0f} ms")
        return (f"[tise] png feed: {n} images in {wall:.2f} s ({n / wall:.0f} images/s on this rank{steady}; "
                f"{loader.workers} decode processes -> shared pinned ring{dec}; {tail}")
    return line


def run(site, files, options, consume, device, batch_size, world=None, loader_args=None, prefetch_key=None):
    """One pass of this rank's ``files`` through ``consume(loader)`` -> what consume returns.  ``loader_args``: kind -> the keyword
    arguments (or a function making them, called only when the kind is chosen) of the site's loader of that kind beyond (files,
    device, batch_size, the resolved worker count, the site's drop-last rule).  ``prefetch_key``: the directory prefetch_png_ring
    may have started the ring under.  On RaggedImages one process runs ``consume`` AGAIN, on the DataLoader; a torchrun rank raises."""
    world = tdist.env_world()[1] if world is None else world
    common = dict(batch_size=batch_size, workers=resolve_workers(options.num_workers, world), drop_last=site.drop_last)

    def attempt(kind):
        extra = (loader_args or {}).get(kind, {})
        kw = {**common, **(extra() if callable(extra) else extra)}
        if kind == "ring":
            with _RING_LOCK:             # a prefetch of this directory from the other loader's feeder thread waits until this one stands
                loader = _RING_PREFETCH.pop(prefetch_key, None)
                if loader is None:
                    loader = build_loader(kind, files, device, **kw)
            loader.device = torch.device(device)
        else:
            loader = build_loader(kind, files, device, **kw)
        png_line = site.png_line and len(files) and kind in ("ring", "dataloader")
        line = loader.feed_line if kind in ("jpeg", "crop") else _png_line(kind, loader, len(files), batch_size) if png_line else None
        return session(kind, loader, consume, line)

    kind = choose(files, options, site)
    try:
        return attempt(kind)
    except png_ring.RaggedImages as e:
        if kind != "ring":
            raise
        if world > 1 and site.ragged_raises:     # calculate_activation_statistics has agreed on the failure collectively by now
            raise RuntimeError(f"--png-feed ring under torchrun needs images of one size ({e}); use --png-feed dataloader") from e
        print(f"[tise] png feed: images of different sizes ({e}); falling back to the DataLoader path", file=sys.stderr)
    return attempt("dataloader")


def encode_files(per_batch, files, device, batch_size, workers, feed, dataset, rgb_only, width, dtype):
    """The image loop of the towers (site CLIP): ``per_batch(x)`` -> device rows of every loader batch of ``files``, in order, every
    file used -> one (len(files), width) tensor of ``dtype``.  The ring delivers uint8 batches of the files' own size (``rgb_only``:
    it takes plain RGB files only), the DataLoader what ``dataset`` -- the tower's preprocess in the workers -- returns."""
    out = []

    def consume(loader):
        out.clear()                                           # the DataLoader pass after a ring that met an odd file starts afresh
        for x in loader:
            out.append(per_batch(x))
    run(CLIP, files, Options(png_feed=feed, num_workers=workers), consume, device, batch_size, tdist.world_size(),
        loader_args={"ring": {"batch_size": 1, "group": batch_size, "rgb_only": rgb_only},
                     "dataloader": {"dataset": dataset, "pin_memory": False, "collate": None}})
    return torch.cat(out).contiguous() if out else torch.empty((0, width), dtype=dtype, device=device)
