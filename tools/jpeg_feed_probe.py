"""Rates of the JPEG feed (DESIGN.md "The JPEG feed"; result: profiles/*_jpeg_feed.txt).

  host   seconds per file on ONE thread: tise_jpeg_entropy_decode, tise_jpeg_decode_rgb8, Pillow's full decode (no GPU needed)
  gpu    images/s of the FID image loop (fid_score._compute_statistics_of_path, one model for all runs) with --jpeg-feed native
         against --jpeg-feed pillow (the previous path) on the same files, ALTERNATING runs, page cache warm; for the ragged
         set also --png-feed dataloader.  Prints every run, then median and spread (max - min) per mode.

    python tools/jpeg_feed_probe.py --root /tmp/jpeg_probe [--one-size 12000] [--ragged 6000] [--pairs 3] [--host-only]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RAGGED = [(640, 480), (500, 375), (480, 640), (375, 500), (640, 427), (500, 333), (427, 640), (333, 500), (640, 426), (500, 374)]


def synthetic(n, h, w, seed):
    """Smooth low-frequency colour fields plus mild noise (what bench.py feeds): compresses like a photograph, not like noise."""
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


def make_sets(root, n_one, n_ragged):
    from PIL import Image
    for name, n, sizes in (("one", n_one, [(256, 256)]), ("ragged", n_ragged, RAGGED)):
        d = os.path.join(root, name)
        if os.path.isdir(d) and len(os.listdir(d)) == n:
            continue
        os.makedirs(d, exist_ok=True)
        pools = {s: synthetic(16, s[1], s[0], seed=s[0] * 7 + s[1]) for s in sizes}
        rng = np.random.default_rng(1)
        for i in range(n):
            s = sizes[int(rng.integers(0, len(sizes)))]
            img = np.roll(pools[s][i % 16], int(rng.integers(0, s[0])), axis=1)
            Image.fromarray(img).save(os.path.join(d, f"im_{i:06d}.jpg"), "JPEG", quality=75, subsampling=2)
    return os.path.join(root, "one"), os.path.join(root, "ragged")


def host_probe(d, n=300):
    from PIL import Image
    from tise_toolbox_amd import build, jpeg_feed
    build.build_jpeg(verbose=False)
    lib = jpeg_feed.load_decoder()
    files = sorted(os.path.join(d, f) for f in os.listdir(d))[:n]
    blobs = [open(f, "rb").read() for f in files]
    slot = np.empty(1 << 22, np.uint8)
    out = np.empty(1 << 22, np.uint8)
    res = {}
    for rep in range(3):
        t0 = time.perf_counter()
        for b in blobs:
            assert lib.tise_jpeg_entropy_decode(b, len(b), slot.ctypes.data, slot.size, None, None) == 0
        t1 = time.perf_counter()
        for b in blobs:
            assert lib.tise_jpeg_decode_rgb8(b, len(b), out.ctypes.data, out.size, None, None) == 0
        t2 = time.perf_counter()
        for f in files:
            np.asarray(Image.open(f).convert("RGB"))
        t3 = time.perf_counter()
        for k, v in (("entropy", t1 - t0), ("native full", t2 - t1), ("pillow", t3 - t2)):
            res.setdefault(k, []).append(v / len(files) * 1e3)
    mb = sum(len(b) for b in blobs) / len(blobs) / 1e3
    print(f"host, one thread, {len(files)} files of {os.path.basename(d)} ({mb:.1f} kB each), ms per file (best of 3): " +
          ", ".join(f"{k} {min(v):.3f}" for k, v in res.items()), flush=True)


def gpu_probe(d, modes, pairs, batch_size):
    import torch
    from tise_toolbox_amd import feeds, fid_score, img_data
    n = len(img_data.get_filenames(d)) // batch_size * batch_size
    rates = {m: [] for m in modes}
    with fid_score._own_model(2048, None, None, 0) as model:
        for rep in range(pairs + 1):                                       # the first round warms page cache, code objects, allocator
            for m in modes:
                fid_score._FEED = feeds.Options(png_feed="dataloader" if m == "dataloader" else "ring",
                                                jpeg_feed="pillow" if m == "pillow" else "native")
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fid_score._compute_statistics_of_path(d, model, batch_size, 2048, True, num_workers=0)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if rep:
                    rates[m].append(n / dt)
                print(f"  {os.path.basename(d)} run {rep} {m}: {n} images in {dt:.2f} s = {n / dt:.0f} images/s" + ("" if rep else " (warm-up, not counted)"), flush=True)
    fid_score._FEED = feeds.Options()
    for m in modes:
        r = rates[m]
        print(f"{os.path.basename(d)} {m}: median {statistics.median(r):.0f} images/s, spread {max(r) - min(r):.0f} (runs {' '.join(f'{x:.0f}' for x in r)})", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", required=True)
    ap.add_argument("--one-size", type=int, default=12000)
    ap.add_argument("--ragged", type=int, default=6000)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--batch-size", type=int, default=50)
    ap.add_argument("--host-only", action="store_true")
    args = ap.parse_args()
    one, ragged = make_sets(args.root, args.one_size, args.ragged)
    host_probe(one)
    host_probe(ragged)
    if args.host_only:
        return
    gpu_probe(one, ["native", "pillow"], args.pairs, args.batch_size)
    gpu_probe(ragged, ["native", "pillow", "dataloader"], args.pairs, args.batch_size)


if __name__ == "__main__":
    main()
