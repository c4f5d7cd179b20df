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
from . import dist as tdist, dists_model, paired


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
    """{n, sum, sum of squares} (paired.value_sums: additive over shards) -> mean and population standard deviation."""
    return paired.value_result(s, "dists", "DISTS")


def result_lines(res, tag=""):
    return [f"DISTS: {res['dists']} +- {res['dists_std']}{tag}"]


def per_pair_csv(files1, files2, per):
    return paired.value_csv("dists", files1, files2, per)


def _evaluate(files1, files2, model, batch_size, options, device):
    from .engine import require_gpu
    from .dists_hip import HipDists
    require_gpu()
    hip = model if isinstance(model, HipDists) else HipDists(model, device)
    return paired.evaluate_pairs(files1, files2, paired.value_per_batch("dists", hip), lambda per: paired.value_sums(per["dists"]),
                                 result_from_sums, batch_size, options, device)


def calculate_dists_given_paths(path1, path2, model, batch_size=50, options=None, device=None):
    """DISTS of every pair of two directories (paired.pair_files) -> dict: dists, dists_std, n; per_pair (this rank's arrays
    dists, h, w), files1, files2, range.  ``model``: DistsVGG16 or HipDists.  Under torchrun every rank returns the totals."""
    return _evaluate(*paired.pair_files(path1, path2), model, batch_size, options, device)


def calculate_dists_self_pairs(path, n_pairs, model, seed=0, batch_size=50, options=None, device=None):
    """``n_pairs`` random pairs (paired.draw_self_pairs) of ONE directory's sorted file list -> calculate_dists_given_paths' dict."""
    return _evaluate(*paired.self_pair_files(path, n_pairs, seed), model, batch_size, options, device)


def parse_args(argv=None):
    return paired.parse_model_pair_args(argv, "DISTS of image pairs", "--dists-weights",
                                        "the DISTS_pytorch package's alpha / beta (weights.pt)")


def resolve_model(args):
    """-> (DistsVGG16, tag).  The trunk file: --weights, else the default cache path (LPIPS's) if it exists; alpha / beta have no
    default path.  Anything missing without --synthetic-weights is an error, never a silent stand-in."""
    default = dists_model.default_weights_path()
    missing = ("no parameters for DISTS VGG-16: it needs torchvision's VGG-16 (--weights PATH, or the file at "
               f"{default!r}) and the DISTS_pytorch package's alpha / beta (--dists-weights PATH, weights.pt); "
               "neither can be downloaded here.  Pass both, or --synthetic-weights for a plumbing/throughput run with seeded stand-ins")
    return paired.resolve_model_files(args, "DISTS VGG-16", args.dists_weights, default, dists_model.build_model, missing)


def main(argv=None):
    args = parse_args(argv)
    dev = paired.cli_device(args, "dists")
    model, tag = resolve_model(args)
    if args.self_pairs:
        res = calculate_dists_self_pairs(args.path1, args.self_pairs, model, args.seed, args.batch_size, paired.feed_options(args), dev)
    else:
        res = calculate_dists_given_paths(args.path1, args.path2, model, args.batch_size, paired.feed_options(args), dev)
    return paired.finish_cli(args, res, result_lines(res, tag), ["dists"], per_pair_csv, dev)


if __name__ == "__main__":
    tdist.run_cli(main)
