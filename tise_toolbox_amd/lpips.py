#!/usr/bin/env python3
"""LPIPS (VGG-16) of image PAIRS on MI355X: the fourth column, beside PSNR, SSIM and rFID, of autoencoder, tokenizer,
super-resolution and editing tables (Zhang et al. 2018; the definition is restated in lpips_model.py).

    python -m tise_toolbox_amd.lpips --path1 ORIG --path2 RECON [--self-pairs N --seed S] [--per-pair OUT.csv]
        [--saved_file OUT.txt] [--batch-size 50] [--weights VGG.pth] [--lpips-weights LIN.pth] [--synthetic-weights]
        [--png-feed ring|dataloader] [--jpeg-feed native|pillow] [--num-workers 0] [--gpu_id 0]

Pairing, the self-pair draw and the two-sided feed loop are ``paired``'s (pair_files, list_files, draw_self_pairs,
paired_from_files with its per-batch hook); per batch the pairs go through ``lpips_hip.HipLpips``.  The result line is
``LPIPS (vgg): mean +- std``, the population standard deviation, formed on the host in fp64 from {n, sum, sum of squares}; under
torchrun the pairs are sharded and one all-reduce of those three sums is the only exchange (--per-pair gathers its rows besides),
rank 0 writes.  Two parameter files are needed -- torchvision's VGG-16 (--weights, default $TORCH_HOME/hub/checkpoints/
vgg16-397923af.pth) and the lpips package's linear layers (--lpips-weights); neither comes with the project.
--synthetic-weights runs seeded stand-ins and tags every result line (weights.py).
"""
from . import dist as tdist, lpips_model, paired

NET = "vgg"


def lpips_from_images(xs, ys, model=None):
    """Two (N,H,W,3) uint8 device tensors or two lists of (H_i,W_i,3) uint8 device tensors (pair by pair one size, every side
    >= 16) -> (N,) float64 numpy array.  ``model``: a ``lpips_hip.HipLpips`` or an ``lpips_model.LpipsVGG16`` (packed for the
    device on every call); None: seeded stand-in parameters (seed 0) -- a plumbing run, as --synthetic-weights."""
    from .lpips_hip import HipLpips
    if model is None:
        model = lpips_model.LpipsVGG16().init_synthetic(0)
    if not isinstance(model, HipLpips):
        model = HipLpips(model)
    return model(xs, ys)


def result_from_sums(s):
    """{n, sum, sum of squares} (paired.value_sums: additive over shards) -> mean and population standard deviation."""
    return paired.value_result(s, "lpips", "LPIPS")


def result_lines(res, tag=""):
    return [f"LPIPS ({NET}): {res['lpips']} +- {res['lpips_std']}{tag}"]


def per_pair_csv(files1, files2, per):
    return paired.value_csv("lpips", files1, files2, per)


def _evaluate(files1, files2, model, batch_size, options, device):
    from .engine import require_gpu
    from .lpips_hip import HipLpips
    require_gpu()
    hip = model if isinstance(model, HipLpips) else HipLpips(model, device)
    return paired.evaluate_pairs(files1, files2, paired.value_per_batch("lpips", hip), lambda per: paired.value_sums(per["lpips"]),
                                 result_from_sums, batch_size, options, device)


def calculate_lpips_given_paths(path1, path2, model, batch_size=50, options=None, device=None):
    """LPIPS of every pair of two directories (paired.pair_files) -> dict: lpips, lpips_std, n; per_pair (this rank's arrays
    lpips, h, w), files1, files2, range.  ``model``: LpipsVGG16 or HipLpips.  Under torchrun every rank returns the totals."""
    return _evaluate(*paired.pair_files(path1, path2), model, batch_size, options, device)


def calculate_lpips_self_pairs(path, n_pairs, model, seed=0, batch_size=50, options=None, device=None):
    """``n_pairs`` random pairs (paired.draw_self_pairs) of ONE directory's sorted file list -> calculate_lpips_given_paths' dict."""
    return _evaluate(*paired.self_pair_files(path, n_pairs, seed), model, batch_size, options, device)


def parse_args(argv=None):
    return paired.parse_model_pair_args(argv, "LPIPS (VGG-16) of image pairs", "--lpips-weights",
                                        "the lpips package's linear layers for VGG-16 (vgg.pth)")


def resolve_model(args):
    """-> (LpipsVGG16, tag).  The trunk file: --weights, else the default cache path if it exists; the linear layers have no
    default path.  Anything missing without --synthetic-weights is an error, never a silent stand-in."""
    default = lpips_model.default_weights_path()
    missing = ("no parameters for LPIPS VGG-16: it needs torchvision's VGG-16 (--weights PATH, or the file at "
               f"{default!r}) and the lpips package's linear layers (--lpips-weights PATH); neither can be "
               "downloaded here.  Pass both, or --synthetic-weights for a plumbing/throughput run with seeded stand-ins")
    return paired.resolve_model_files(args, "LPIPS VGG-16", args.lpips_weights, default, lpips_model.build_model, missing)


def main(argv=None):
    args = parse_args(argv)
    dev = paired.cli_device(args, "lpips")
    model, tag = resolve_model(args)
    if args.self_pairs:
        res = calculate_lpips_self_pairs(args.path1, args.self_pairs, model, args.seed, args.batch_size, paired.feed_options(args), dev)
    else:
        res = calculate_lpips_given_paths(args.path1, args.path2, model, args.batch_size, paired.feed_options(args), dev)
    return paired.finish_cli(args, res, result_lines(res, tag), ["lpips"], per_pair_csv, dev)


if __name__ == "__main__":
    tdist.run_cli(main)
