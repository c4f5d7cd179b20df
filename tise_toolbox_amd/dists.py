#!/usr/bin/env python3
"""DISTS of image PAIRS on MI355X: the texture-tolerant full-reference column, beside PSNR, SSIM, LPIPS and rFID, of autoencoder,
tokenizer, super-resolution and codec tables (Ding, Ma, Wang & Simoncelli 2020; the definition is restated in dists_model.py).

    python -m tise_toolbox_amd.dists --path1 ORIG --path2 RECON [--self-pairs N --seed S] [--per-pair OUT.csv]
        [--saved_file OUT.txt] [--batch-size 50] [--weights VGG.pth] [--dists-weights W.pt] [--synthetic-weights]
        [--png-feed ring|dataloader] [--jpeg-feed native|pillow] [--num-workers 0] [--gpu_id 0]

Pairing, the self-pair draw and the two-sided feed loop are ``paired``'s (pair_files, list_files, draw_self_pairs,
paired_from_files with its per-batch hook); per batch the pairs go through ``dists_hip.HipDists``.  The result line is
``DISTS: mean +- std``, the population standard deviation, formed on the host in fp64 from {n, sum, sum of squares}; under
torchrun the pairs are sharded and one all-reduce of those three sums is the only exchange (--per-pair gathers its rows besides),
rank 0 writes.  Two parameter files are needed -- torchvision's VGG-16 (--weights, default $TORCH_HOME/hub/checkpoints/
vgg16-397923af.pth, the file LPIPS takes) and the DISTS_pytorch package's alpha / beta (--dists-weights, no default); neither
comes with the project.  --synthetic-weights runs seeded stand-ins and tags every result line (weights.py).
"""
import argparse
import os

import numpy as np
import torch

from . import _lib, dist as tdist, dists_model, feeds, paired, weights as tweights
from .lpips import sums


def dists_from_images(xs, ys, model=None):
    """Two (N,H,W,3) uint8 device tensors or two lists of (H_i,W_i,3) uint8 device tensors (pair by pair one size, every side
    >= 16) -> (N,) float64 numpy array.  ``model``: a ``dists_hip.HipDists`` or a ``dists_model.DistsVGG16`` (packed for the
    device on every call); None: seeded stand-in parameters (seed 0) -- a plumbing run, as --synthetic-weights."""
    from .dists_hip import HipDists
    if model is None:
        model = dists_model.DistsVGG16().init_synthetic(0)
    if not isinstance(model, HipDists):
        model = HipDists(model)
    return model(xs, ys)


def result_from_sums(s):
    """{n, sum, sum of squares} (lpips.sums: additive over shards) -> mean and population standard deviation."""
    s = np.asarray(s, dtype=np.float64)
    if int(s[0]) < 1:
        raise RuntimeError("DISTS needs at least one pair")
    mean = s[1] / s[0]
    var = max(s[2] / s[0] - mean * mean, 0.0) if np.isfinite(mean) else float("nan")
    return {"n": int(s[0]), "dists": float(mean), "dists_std": float(np.sqrt(var))}


def result_lines(res, tag=""):
    return [f"DISTS: {res['dists']} +- {res['dists_std']}{tag}"]


def per_pair_csv(files1, files2, per):
    rows = ["pair,file1,file2,h,w,dists"]
    for i, (f1, f2) in enumerate(zip(files1, files2)):
        rows.append(f"{i},{f1},{f2},{int(per['h'][i])},{int(per['w'][i])},{float(per['dists'][i])!r}")
    return "\n".join(rows) + "\n"


def _evaluate(files1, files2, hip, batch_size, options, device):
    rank, world, _ = tdist.env_world()
    lo, hi = tdist.shard_range(len(files1), rank, world)

    def per_batch(xs, ys):
        return {"dists": hip(xs, ys) if len(xs) else np.zeros(0), "h": np.array([a.shape[0] for a in xs], dtype=np.int64),
                "w": np.array([a.shape[1] for a in xs], dtype=np.int64)}
    per = paired.paired_from_files(files1[lo:hi], files2[lo:hi], False, batch_size, options, device, per_batch=per_batch)
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    acc = torch.from_numpy(sums(per["dists"])).to(dev)
    tdist.all_reduce_sum_(acc)                               # {n, sum, sum of squares}: the only exchange
    res = result_from_sums(acc.cpu().numpy())
    res["per_pair"], res["files1"], res["files2"], res["range"] = per, list(files1), list(files2), (lo, hi)
    return res


def _hip(model, device):
    from .engine import require_gpu
    from .dists_hip import HipDists
    require_gpu()
    return model if isinstance(model, HipDists) else HipDists(model, device)


def calculate_dists_given_paths(path1, path2, model, batch_size=50, options=None, device=None):
    """DISTS of every pair of two directories (paired.pair_files) -> dict: dists, dists_std, n; per_pair (this rank's arrays
    dists, h, w), files1, files2, range.  ``model``: DistsVGG16 or HipDists.  Under torchrun every rank returns the totals."""
    files1, files2 = paired.pair_files(path1, path2)
    return _evaluate(files1, files2, _hip(model, device), batch_size, options, device)


def calculate_dists_self_pairs(path, n_pairs, model, seed=0, batch_size=50, options=None, device=None):
    """``n_pairs`` random pairs (paired.draw_self_pairs) of ONE directory's sorted file list -> calculate_dists_given_paths' dict."""
    files = paired.list_files(path)
    idx = paired.draw_self_pairs(len(files), n_pairs, seed)
    return _evaluate([files[i] for i in idx[:, 0]], [files[j] for j in idx[:, 1]], _hip(model, device), batch_size, options, device)


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="DISTS of image pairs")
    parser.add_argument("--path1", required=True, type=str, help="folder of originals (with --self-pairs: the one folder)")
    parser.add_argument("--path2", default=None, type=str, help="folder of reconstructions, paired by relative path without extension")
    parser.add_argument("--self-pairs", default=0, type=int, help="N random pairs (i != j) of --path1 instead of two folders")
    parser.add_argument("--seed", default=0, type=int, help="seed of the --self-pairs draw and of the --synthetic-weights parameters")
    parser.add_argument("--per-pair", default="", type=str, help="write one CSV line per pair here")
    parser.add_argument("--saved_file", default="", type=str, help="write the result line here as well")
    parser.add_argument("--batch-size", default=50, type=int)
    parser.add_argument("--weights", default="", type=str, help="torchvision VGG-16 state_dict (vgg16-397923af.pth)")
    parser.add_argument("--dists-weights", default="", type=str, help="the DISTS_pytorch package's alpha / beta (weights.pt)")
    parser.add_argument("--synthetic-weights", action="store_true",
                        help="seeded stand-in parameters: plumbing / throughput runs only (result lines are tagged)")
    parser.add_argument("--png-feed", default="ring", choices=["ring", "dataloader"])
    parser.add_argument("--jpeg-feed", default=None, choices=["native", "pillow"])
    parser.add_argument("--num-workers", default=0, type=int, help="image decode processes per side (0 = auto)")
    parser.add_argument("--gpu_id", default="0", type=str)
    args = parser.parse_args(argv)
    if args.self_pairs:
        if args.path2:
            parser.error("--self-pairs takes --path1 only")
    elif not args.path2:
        parser.error("give --path2, or --self-pairs N")
    if args.synthetic_weights and (args.weights or args.dists_weights):
        parser.error("--synthetic-weights and --weights / --dists-weights are mutually exclusive")
    return args


def resolve_model(args):
    """-> (DistsVGG16, tag).  The trunk file: --weights, else the default cache path (LPIPS's) if it exists; alpha / beta have no
    default path.  Anything missing without --synthetic-weights is an error, never a silent stand-in."""
    if args.synthetic_weights:
        tweights.warn_synthetic("DISTS VGG-16")
        return dists_model.build_model(synthetic=True, seed=args.seed), tweights.SYNTHETIC_TAG
    trunk = args.weights or (dists_model.default_weights_path() if os.path.exists(dists_model.default_weights_path()) else "")
    for path in (trunk, args.dists_weights):
        if path and not os.path.exists(path):
            raise RuntimeError("Invalid path: %s" % path)
    if not trunk or not args.dists_weights:
        raise RuntimeError(
            "no parameters for DISTS VGG-16: it needs torchvision's VGG-16 (--weights PATH, or the file at "
            f"{dists_model.default_weights_path()!r}) and the DISTS_pytorch package's alpha / beta (--dists-weights PATH, weights.pt); "
            "neither can be downloaded here.  Pass both, or --synthetic-weights for a plumbing/throughput run with seeded stand-ins")
    return dists_model.build_model(trunk, args.dists_weights), ""


def main(argv=None):
    args = parse_args(argv)
    if not torch.cuda.is_available():
        raise _lib.TiseLibraryError("dists needs an MI355X: there is no CPU path")
    rank, world, local_rank = tdist.init_from_env()
    dev = torch.device(f"cuda:{local_rank}" if world > 1 else f"cuda:{args.gpu_id}")
    torch.cuda.set_device(dev)
    model, tag = resolve_model(args)
    options = feeds.Options(png_feed=args.png_feed, jpeg_feed=args.jpeg_feed, num_workers=args.num_workers)
    if args.self_pairs:
        res = calculate_dists_self_pairs(args.path1, args.self_pairs, model, args.seed, args.batch_size, options, dev)
    else:
        res = calculate_dists_given_paths(args.path1, args.path2, model, args.batch_size, options, dev)
    lines = result_lines(res, tag)
    if args.per_pair:
        per, (lo, hi) = res["per_pair"], res["range"]
        cols = [np.arange(lo, hi, dtype=np.float64), per["h"], per["w"], per["dists"]]
        rows = tdist.all_gather_rows(torch.from_numpy(np.stack([np.asarray(c, dtype=np.float64) for c in cols], axis=1)).to(dev)).cpu().numpy()
        if tdist.is_main():
            with open(args.per_pair, "w") as f:
                f.write(per_pair_csv(res["files1"], res["files2"], {"h": rows[:, 1], "w": rows[:, 2], "dists": rows[:, 3]}))
    if tdist.is_main():
        if args.saved_file:
            with open(args.saved_file, "w") as f:
                f.write("\n".join(lines))                                  # no trailing newline, like paired --saved_file
        print("\n".join(lines))
    return res


if __name__ == "__main__":
    tdist.run_cli(main)
