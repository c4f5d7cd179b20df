#!/usr/bin/env python3
"""FD-DINOv2 on MI355X: the Frechet distance -- and KD, precision / recall / density / coverage -- in DINOv2 ViT space.

Stein et al. 2023 ("Exposing flaws of generative model evaluation metrics and their fair treatment of diffusion models", the
`dgm-eval` package) find that Inception pool3 space misranks modern generators against human judgement and recommend the same
Frechet distance on the class token of DINOv2 ViT-L/14 (1024-d), reported together with a kernel distance and the k-nearest-
neighbour metrics in that space:

    FD-DINOv2   |mu1 - mu2|^2 + tr(S1 + S2 - 2 (S1 S2)^(1/2)) of np.mean / np.cov of the feature rows: device.StatsAccumulator(d)
                and engine.frechet_solver(d), the FID machinery at width d (384 / 768 / 1024)
    KD-DINOv2   (--kd)   kid.kid_from_features: 100 subsets of at most 1000 rows, the polynomial kernel (k(x, y) = (x.y / d + 1)^3)
                -- dgm-eval's KD; printed as mean +- std over the subsets
    --prdc      the four numbers of prdc.prdc_from_features(ref, gen, nearest_k = 5)
    --authpct   (needs --train) authenticity.authpct_from_features(train, gen): the share of generated samples that are not copies
                of a training image; --nearest-train OUT.csv lists every sample's nearest training row
    --vendi     vendi.vendi_from_features of the generated and of the reference rows (linear kernel, q = 1)
    --fd-infinity   fd_infinity.fd_infinity_from_features(ref, gen): FD extrapolated to infinitely many samples (seeded subsets)

THE TOWER is dinov2_hip.HipDino (csrc/clip_ops.hip): fp16 matrix-core operands, fp32 accumulation, an fp32 residual stream and
fp32 features -- the arithmetic of torch.autocast(fp16); dgm-eval runs the tower in fp32.  ``--arch`` chooses vits14 / vitb14 /
vitl14 (default); the result lines, the feature files' network tag (``dinov2-vitl14`` ...) and the default parameter file
(``$TORCH_HOME/hub/checkpoints/dinov2_vitl14_pretrain.pth``) follow.  ``TISE_DINO=torch`` runs the module under autocast on
library kernels instead (the A/B route).

PREPROCESSING (dinov2_model.preprocess): RGB, Pillow 8-bit bicubic resize straight to 224 x 224, ImageNet mean / std.  It and
the position-table rule are restated from memory; with the parity of the tower itself they are UNPINNED (README).

The run, the feature files, the shared options and the result lines are feature_space.py's; this module describes the space
(``space``) and adds its own options.  KD's subsets are drawn over the walk order the rows are gathered in.
"""
import argparse

from . import dist as tdist, feature_space as fs, weights as tweights
from .feature_space import NEAREST_TRAIN_COLUMNS, write_nearest_train_csv  # noqa: F401

ARCH = "vitl14"


def arch_info(arch=ARCH):
    """-> (feature width, network tag, weights kind | None) of a tower of dinov2_model.CONFIGS.  A configuration registered at run
    time gets a tag spelt from its name and no default parameter file."""
    from . import dinov2_model
    dims = dinov2_model.get_config(arch)["width"]
    tag = "dinov2-" + "".join(c if c.isalnum() else "-" for c in str(arch).lower()).strip("-")
    kind = f"dinov2-{arch}"
    return dims, tag, kind if kind in tweights._KINDS else None


def space(arch=ARCH, weights=None, seed=0):
    """The space of one DINOv2 tower (an unknown ``arch`` is refused here).  ``weights=None``: seeded stand-in parameters of ``seed``."""
    from . import cmmd
    dims, network, _ = arch_info(arch)

    def build_tower(dev):
        from . import dinov2_hip
        return dinov2_hip.build_tower(weights, dev, arch, seed)
    return fs.Space("fd_dinov2", network, dims, build_tower, cmmd.embed_image_dir)      # HipDino brings its preprocess to that loop


def check_feature_file(path, arch=ARCH):
    return fs.check_feature_file(path, arch_info(arch)[1], "fd_dinov2")


def load_features_npz(path, arch=ARCH):
    dims, network, _ = arch_info(arch)
    return fs.load_features_npz(path, network, dims, "fd_dinov2")


fd_dinov2_from_features = fs.frechet_from_features


def calculate_fd_dinov2_given_paths(paths, batch_size=50, weights=None, seed=0, num_workers=0, feed="ring", arch=ARCH, kd=False,
                                    prdc_k=None, save_features="", train=None, authpct=False, nearest_train="", vendi=False,
                                    fd_infinity=False, fd_infinity_seed=0):
    """-> dict(fd=float, kd=(mean, std) | None, prdc=OrderedDict | None) of two paths, each a directory or a feature file.
    ``weights=None``: seeded stand-in parameters (the CLI only allows that behind --synthetic-weights).  ``save_features``: the
    FIRST path's rows (the reference set) are written there with their mu, sigma and the network tag.
    The memorization and diversity numbers add keys only when asked for: ``authpct`` (float; needs ``train``, the training set's
    directory or feature file) and, with ``nearest_train`` (a CSV path, written by rank 0), the per-sample table; ``vendi`` and
    ``vendi_reference`` (floats: the second and the first path's); ``fd_infinity`` (the dict of fd_infinity_from_features)."""
    asked = dict(kd=kd, prdc=prdc_k is not None, authpct=authpct, vendi=vendi, fd_infinity=fd_infinity)
    return fs.fd_result(fs.given_paths(space(arch, weights, seed), paths, batch_size, num_workers, feed, save_features, train,
                                       ["fd"] + [k for k, v in asked.items() if v], prdc_k, nearest_train, fd_infinity_seed))


def result_lines(res, arch, tag=""):
    return fs.result_lines(res, f"DINOv2 ({arch})", tag)


def parse_args(argv=None):
    from . import dinov2_model
    parser = argparse.ArgumentParser(description="FD-DINOv2 (and KD, precision / recall / density / coverage) on a DINOv2 ViT tower")
    fs.add_arguments(parser, "paths")
    parser.add_argument("--arch", default=ARCH, choices=list(dinov2_model.CONFIGS), help="the tower (default vitl14, the published metric's)")
    fs.add_arguments(parser, "kd", space="DINOv2")
    parser.add_argument("--train", default="", type=str, help="the generator's training images: a directory, or a feature file of --save-features (same --arch)")
    parser.add_argument("--authpct", action="store_true", help="also report AuthPct: the share of --path2 samples that are not nearer to a --train row than that row's own nearest training neighbour")
    parser.add_argument("--nearest-train", default="", type=str, metavar="OUT.csv",
                        help="write every --path2 row's nearest --train row, its squared distance and the authentic flag to this CSV")
    parser.add_argument("--vendi", action="store_true", help="also report the Vendi score (linear kernel, q = 1) of --path2, and of --path1 for comparison")
    parser.add_argument("--fd-infinity", action="store_true", help="also report FD-infinity: FD extrapolated to infinitely many --path2 samples")
    parser.add_argument("--fd-infinity-seed", type=int, default=0, help="seed of the --fd-infinity subsets (default 0)")
    fs.add_arguments(parser, "weights batch output", weights_help="DINOv2 state_dict (.pth) of the chosen tower; default: "
                     "$TORCH_HOME/hub/checkpoints/dinov2_<arch>_pretrain.pth")
    args = fs.parse_fd_args(parser, argv)
    if (args.authpct or args.nearest_train) and not args.train:
        parser.error("--authpct and --nearest-train need the training set: --train PATH")
    return args


def main(argv=None):
    args = parse_args(argv)
    _, network, kind = arch_info(args.arch)
    wpath, tag = fs.start_cli(args, "fd_dinov2", network, kind, f"DINOv2 {args.arch}")
    res = calculate_fd_dinov2_given_paths([args.path1, args.path2], args.batch_size, wpath, args.seed, args.num_workers, args.png_feed,
                                          args.arch, args.kd, args.prdc_k if args.prdc else None, args.save_features, args.train or None,
                                          args.authpct, args.nearest_train, args.vendi, args.fd_infinity, args.fd_infinity_seed)
    tdist.write_lines(result_lines(res, args.arch, tag), args.saved_file)
    return res


if __name__ == "__main__":
    tdist.run_cli(main)
