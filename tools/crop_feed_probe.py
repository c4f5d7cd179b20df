"""Rates of the crop feed (DESIGN.md "The crop feed"; result: profiles/*_crop_feed.txt).

  host   ms per file on ONE thread: inflate only (tise_png_inflate_slot), the complete native decode, Pillow (no GPU needed)
  gpu    images/s of the --per-class image loop (fid_score._class_statistics, one model for all runs: feed -> ragged device
         batches of up to 1000 crops -> resize -> trunk -> pool3 rows grouped by class) on the same files, ALTERNATING runs,
         page cache warm; prints every run, then median and spread (max - min) per mode:
           native       crop_feed.CropFeedLoader, one resize launch per device batch
           parent       the route before the crop feed existed: DataLoader workers + collate_u8 + one host->device copy and
                        one resize launch per crop (restated below: RealismEngine.features_from_u8_list as it was)
           dataloader   today's --crop-feed dataloader: the DataLoader, but one resize launch per device batch
  kernels  one pass of the native feed and nothing else, for a ``rocprofv3 --kernel-trace --stats`` run (--kernels-only)
  launch   the two ragged resize launches alone (--launch-only; no files): tise_resize_ragged_u8 and tise_resize_ragged_f32 on
           the first ``--crops`` (1 000) sizes of the directory below as resident device crops -> 299 x 299, table in page-locked
           memory; per round the calls are enqueued back to back between two device events until they fill a tenth of a second;
           median and spread (max - min) of the rounds, ms per launch, and the host's time to enqueue one call (the device
           figure is the kernel's as long as that is the smaller one)

The synthetic crop directory (seeded, documented here because the result depends on it): ``--files`` (6 000) PNGs named
``im_{i}_{class}_{i}.png`` over 80 class tokens; height and width drawn independently and uniformly from 16..256 with
numpy.random.default_rng(1); pixels are a window of one of 16 smooth low-frequency colour fields with mild noise (what bench.py
feeds: compresses like a photograph, not like noise), rolled by a random offset; every fifth file carries an alpha channel
(RGBA); written by Pillow's PNG writer at its default compression (adaptive row filters).

    python tools/crop_feed_probe.py --root /tmp/crop_probe [--files 6000] [--pairs 3] [--host-only | --kernels-only]
    python tools/crop_feed_probe.py --launch-only [--crops 1000] [--rounds 7]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synthetic(n, h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    out = []
    for _ in range(n):
        img = np.zeros((h, w, 3), np.float32)
        for c in range(3):
            fx, fy, ph = rng.uniform(0.5, 6) / w, rng.uniform(0.5, 6) / h, rng.uniform(0, 6.28)
            img[..., c] = 128 + 100 * np.sin(6.28 * (fx * xx + fy * yy) + ph)
        out.append(np.clip(img + rng.normal(0, 6, img.shape), 0, 255).astype(np.uint8))
    return out


def crop_draws(n):
    """(h, w, roll) of the directory's first n files."""
    rng = np.random.default_rng(1)
    return [(int(rng.integers(16, 257)), int(rng.integers(16, 257)), int(rng.integers(0, 256))) for _ in range(n)]


def make_set(root, n):
    from PIL import Image
    d = os.path.join(root, "crops")
    if os.path.isdir(d) and len(os.listdir(d)) == n:
        return d
    os.makedirs(d, exist_ok=True)
    pool = synthetic(16, 256, 256, seed=5)
    for i, (h, w, roll) in enumerate(crop_draws(n)):
        img = np.roll(pool[i % 16], roll, axis=1)[:h, :w]
        if i % 5 == 0:
            img = np.concatenate([img, np.full((h, w, 1), 255, np.uint8)], axis=2)
        Image.fromarray(img).save(os.path.join(d, f"im_{i:06d}_class{i % 80:02d}_{i}.png"))
    return d


def host_probe(d, n=300):
    from PIL import Image
    from tise_toolbox_amd import build, crop_feed
    build.build_png(verbose=False)
    lib = crop_feed.load_decoder()
    files = sorted(os.path.join(d, f) for f in os.listdir(d))[:n]
    blobs = [open(f, "rb").read() for f in files]
    meta = [crop_feed.probe(b) for b in blobs]
    slot = np.empty(1 << 20, np.uint8)
    out = np.empty(1 << 20, np.uint8)
    sc = np.empty(1 << 21, np.uint8)
    res = {}
    for rep in range(3):
        t0 = time.perf_counter()
        for b, (_, w, h, ch) in zip(blobs, meta):
            assert lib.tise_png_inflate_slot(b, len(b), slot.ctypes.data, int(lib.tise_png_slot_bytes(h, w, ch)), h, w, sc.ctypes.data, sc.size,
                                             None, None, None) == 0
        t1 = time.perf_counter()
        for b, (_, w, h, ch) in zip(blobs, meta):
            assert lib.tise_png_decode_rgb8(b, len(b), out.ctypes.data, h, w, sc.ctypes.data, sc.size, None, None) == 0
        t2 = time.perf_counter()
        for f in files:
            np.asarray(Image.open(f).convert("RGB"))
        t3 = time.perf_counter()
        for k, v in (("inflate only", t1 - t0), ("native full", t2 - t1), ("pillow", t3 - t2)):
            res.setdefault(k, []).append(v / len(files) * 1e3)
    kb = sum(len(b) for b in blobs) / len(blobs) / 1e3
    print(f"host, one thread, {len(files)} crops ({kb:.1f} kB each), ms per file (best of 3): " +
          ", ".join(f"{k} {min(v):.3f}" for k, v in res.items()), flush=True)


def _features_from_u8_list_per_crop(self, crops):
    """RealismEngine.features_from_u8_list before the ragged resize kernel: one copy and one resize launch per crop."""
    import torch
    from tise_toolbox_amd import device
    u8 = torch.empty((len(crops), 299, 299, 3), dtype=torch.uint8, device=self.device)
    for i, c in enumerate(crops):
        if c.dim() == 4:
            c = c[0]
        device.resize_u8_only(c.to(self.device, non_blocking=True).unsqueeze(0), (299, 299), out=u8[i:i + 1])
    return self._trunk_u8(u8)


def gpu_probe(d, modes, pairs, batch_size):
    import torch
    from tise_toolbox_amd import feeds, fid_score, img_data
    from tise_toolbox_amd.engine import RealismEngine
    n = len(img_data.get_filenames(d))
    rates = {m: [] for m in modes}
    one_launch = RealismEngine.features_from_u8_list
    with fid_score._own_model(2048, None, 80, 0) as model:
        for rep in range(pairs + 1):                                       # the first round warms page cache, code objects, allocator, plans
            for m in modes:
                fid_score._FEED = feeds.Options(crop_feed="native" if m == "native" else "dataloader")
                RealismEngine.features_from_u8_list = _features_from_u8_list_per_crop if m == "parent" else one_launch
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fid_score._class_statistics(d, model, batch_size, 2048, 0)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if rep:
                    rates[m].append(n / dt)
                print(f"  crops run {rep} {m}: {n} images in {dt:.2f} s = {n / dt:.0f} images/s" + ("" if rep else " (warm-up, not counted)"), flush=True)
    fid_score._FEED = feeds.Options()
    RealismEngine.features_from_u8_list = one_launch
    for m in modes:
        r = rates[m]
        print(f"crops {m}: median {statistics.median(r):.0f} images/s, spread {max(r) - min(r):.0f} (runs {' '.join(f'{x:.0f}' for x in r)})", flush=True)


def kernels_only(d, batch_size):
    import torch
    from tise_toolbox_amd import feeds, fid_score
    fid_score._FEED = feeds.Options(crop_feed="native")
    with fid_score._own_model(2048, None, 80, 0) as model:
        fid_score._class_statistics(d, model, batch_size, 2048, 0)
        torch.cuda.synchronize()


def launch_probe(n, rounds, out_hw=(299, 299)):
    import torch
    from tise_toolbox_amd import _lib
    dev = torch.device("cuda", 0)
    oh, ow = out_hw
    pool = synthetic(16, 256, 256, seed=5)
    crops = [torch.from_numpy(np.ascontiguousarray(np.roll(pool[i % 16], roll, axis=1)[:h, :w])).to(dev)
             for i, (h, w, roll) in enumerate(crop_draws(n))]
    ptrs = np.fromiter((c.data_ptr() for c in crops), dtype=np.uint64, count=n)
    hs = np.fromiter((c.shape[0] for c in crops), dtype=np.int32, count=n)
    ws = np.fromiter((c.shape[1] for c in crops), dtype=np.int32, count=n)
    orders = np.zeros(n, dtype=np.int32)
    need = n * (64 + 4 * oh) + 16 * (n // 4096 + 1)
    ws_dev = torch.empty(need, dtype=torch.uint8, device=dev)
    pinned = torch.empty(need, dtype=torch.uint8).pin_memory()
    u8 = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device=dev)
    f32 = torch.empty((n, oh, ow, 3), dtype=torch.float32, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib, bad = _lib.load(), ctypes.c_int64(-1)
    args = (ctypes.c_void_p(ws_dev.data_ptr()), need, ctypes.c_void_p(pinned.data_ptr()), ctypes.byref(bad), stream)
    calls = {
        "ragged u8": lambda: lib.tise_resize_ragged_u8(ptrs.ctypes.data, hs.ctypes.data, ws.ctypes.data, n, ctypes.c_void_p(u8.data_ptr()),
                                                        oh, ow, 0, *args),
        "ragged f32": lambda: lib.tise_resize_ragged_f32(ptrs.ctypes.data, hs.ctypes.data, ws.ctypes.data, orders.ctypes.data, n,
                                                          ctypes.c_void_p(f32.data_ptr()), oh, ow, 1, 1, 0.0, 255.0, 128.0, 128.0, *args),
    }
    print(f"{n} resident crops, sides 16..256 ({int(hs.astype(np.int64) @ ws) * 3 / 1e6:.1f} MB) -> {oh} x {ow}, {rounds} rounds, alternating", flush=True)
    reps, dev_ms, host_ms = {}, {k: [] for k in calls}, {k: [] for k in calls}
    for k, f in calls.items():                                                 # warm-up: plans, code objects; then size a round
        for _ in range(3):
            assert f() == _lib.TISE_OK, (k, bad.value)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(5):
            f()
        b.record()
        b.synchronize()
        reps[k] = max(5, int(100.0 / (a.elapsed_time(b) / 5)) + 1)
    for _ in range(rounds):
        for k, f in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            t0 = time.perf_counter()
            for _ in range(reps[k]):
                f()
            t1 = time.perf_counter()
            b.record()
            b.synchronize()
            dev_ms[k].append(a.elapsed_time(b) / reps[k])
            host_ms[k].append((t1 - t0) / reps[k] * 1e3)
    for k in calls:
        d = dev_ms[k]
        print(f"  {k:10s} median {statistics.median(d):7.4f} ms per launch  spread {max(d) - min(d):6.4f}  min {min(d):7.4f}  max {max(d):7.4f}"
              f"  ({reps[k]} launches per round; host enqueue {statistics.median(host_ms[k]):.4f} ms per call)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root")
    ap.add_argument("--launch-only", action="store_true")
    ap.add_argument("--crops", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--files", type=int, default=6000)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--batch-size", type=int, default=50)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    if args.launch_only:
        launch_probe(args.crops, args.rounds)
        return
    if not args.root:
        ap.error("--root is required without --launch-only")
    d = make_set(args.root, args.files)
    if args.kernels_only:
        kernels_only(d, args.batch_size)
        return
    host_probe(d)
    if args.host_only:
        return
    gpu_probe(d, ["native", "parent", "dataloader"], args.pairs, args.batch_size)


if __name__ == "__main__":
    main()
