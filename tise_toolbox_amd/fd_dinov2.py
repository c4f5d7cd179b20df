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

Every image of a directory is used.  Under torchrun the files are sharded as contiguous index ranges and the rows gathered in
walk order on every rank (cmmd.embed_image_dir); rank 0 prints and writes.  KD's subsets are drawn over that walk order.
"""
import argparse
import os

import numpy as np
import torch

from . import _lib, dist as tdist, weights as tweights

ARCH = "vitl14"
NEAREST_TRAIN_COLUMNS = ("gen_row", "train_row", "d2", "authentic", "gen_file", "train_file")


def arch_info(arch=ARCH):
    """-> (feature width, network tag, weights kind | None) of a tower of dinov2_model.CONFIGS.  A configuration registered at run
    time gets a tag spelt from its name and no default parameter file."""
    from . import dinov2_model
    dims = dinov2_model.get_config(arch)["width"]
    tag = "dinov2-" + "".join(c if c.isalnum() else "-" for c in str(arch).lower()).strip("-")
    kind = f"dinov2-{arch}"
    return dims, tag, kind if kind in tweights._KINDS else None


def statistics(feats):
    """(mu, sigma) of fp32 device rows -> fp64 numpy arrays: np.mean / np.cov (ddof 1) on the device."""
    from . import cmmd
    return cmmd.clip_statistics(feats)


def fd_dinov2_from_features(f1, f2):
    """The Frechet distance of two feature sets (device tensors or numpy arrays, (n, dims)) -> Python float."""
    from . import cmmd, fid_score
    from .engine import require_gpu
    if cmmd._width(f1) != cmmd._width(f2):
        raise ValueError(f"feature widths differ: {cmmd._width(f1)} and {cmmd._width(f2)}")
    require_gpu()
    dev = f1.device if isinstance(f1, torch.Tensor) and f1.is_cuda else torch.device("cuda", torch.cuda.current_device())
    (m1, s1), (m2, s2) = statistics(cmmd._to_device_f32(f1, dev)), statistics(cmmd._to_device_f32(f2, dev))
    return float(fid_score.calculate_frechet_distance(m1, s1, m2, s2))


def check_feature_file(path, arch=ARCH):
    """The refusal of load_features_npz on the file's network tag alone (no rows are read, no GPU is needed)."""
    from . import fid_score
    network = arch_info(arch)[1]
    with np.load(path, allow_pickle=True) as f:
        if "network" not in f.files:
            raise RuntimeError(f"{path}: no network tag: not a feature file of {network} (make one with fd_dinov2 --save-features)")
        fid_score.check_stats_network(path, str(f["network"]), network)


def load_features_npz(path, arch=ARCH):
    """-> (features fp32 (n, dims), mu, sigma) of a file --save-features wrote under the SAME ``arch``; a file of another
    network or architecture, or one without the rows, is refused."""
    from . import fid_score
    dims, network, _ = arch_info(arch)
    with np.load(path, allow_pickle=True) as f:
        tag = str(f["network"]) if "network" in f.files else None
        if tag is None:
            raise RuntimeError(f"{path}: no network tag: not a feature file of {network} (make one with fd_dinov2 --save-features)")
        fid_score.check_stats_network(path, tag, network)
        if "features" not in f.files:
            raise RuntimeError(f"{path}: no 'features' array in this file; make it with fd_dinov2 --save-features")
        feats = np.ascontiguousarray(f["features"], dtype=np.float32)
        if feats.ndim != 2 or feats.shape[1] != dims:
            raise RuntimeError(f"{path}: features of shape {feats.shape}, expected (n, {dims})")
        return feats, f["mu"][:], f["sigma"][:]


def _side(path, tower, dev, batch_size, num_workers, feed, arch):
    """-> (fp32 device rows, mu, sigma) of a directory or a feature file."""
    from . import cmmd
    if path.endswith(".npz"):
        feats, mu, sigma = load_features_npz(path, arch)
        return torch.as_tensor(feats, device=dev), mu, sigma
    feats = cmmd.embed_image_dir(tower(), path, dev, batch_size, num_workers, feed)
    if feats.shape[0] == 0:
        raise RuntimeError(f"no images under {path}")
    return (feats,) + statistics(feats)


def write_nearest_train_csv(path, near, gen_path, train_path):
    """One line per generated row under a header line: gen_row,train_row,d2,authentic,gen_file,train_file.  A file column is
    filled from img_data.get_filenames (the walk order the rows were embedded in) when that side is a directory, else empty."""
    import csv
    from . import img_data
    gen_files = img_data.get_filenames(gen_path) if os.path.isdir(gen_path) else None
    train_files = img_data.get_filenames(train_path) if os.path.isdir(train_path) else None
    if gen_files is not None and len(gen_files) != len(near["idx"]):
        raise RuntimeError(f"{gen_path}: {len(gen_files)} files now, {len(near['idx'])} rows were embedded")
    with open(path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(NEAREST_TRAIN_COLUMNS)
        for g, (t, d2, a) in enumerate(zip(near["idx"].tolist(), near["d2_gen"].tolist(), near["authentic"].tolist())):
            w.writerow([g, t, repr(d2), int(a), gen_files[g] if gen_files is not None else "",
                        train_files[t] if train_files is not None else ""])


def calculate_fd_dinov2_given_paths(paths, batch_size=50, weights=None, seed=0, num_workers=0, feed="ring", arch=ARCH, kd=False,
                                    prdc_k=None, save_features="", train=None, authpct=False, nearest_train="", vendi=False,
                                    fd_infinity=False, fd_infinity_seed=0):
    """-> dict(fd=float, kd=(mean, std) | None, prdc=OrderedDict | None) of two paths, each a directory or a feature file.
    ``weights=None``: seeded stand-in parameters (the CLI only allows that behind --synthetic-weights).  ``save_features``: the
    FIRST path's rows (the reference set) are written there with their mu, sigma and the network tag.
    The memorization and diversity numbers add keys only when asked for: ``authpct`` (float; needs ``train``, the training set's
    directory or feature file) and, with ``nearest_train`` (a CSV path, written by rank 0), the per-sample table; ``vendi`` and
    ``vendi_reference`` (floats: the second and the first path's); ``fd_infinity`` (the dict of fd_infinity_from_features)."""
    from . import dinov2_hip, fid_score
    arch_info(arch)                                                        # an unknown arch: say so before anything is read
    if (authpct or nearest_train) and not train:
        raise ValueError("authpct / nearest_train need the training set: train=PATH (a directory or a feature file)")
    every = list(paths) + ([train] if train else [])
    for p in every:
        if not os.path.exists(p):
            raise RuntimeError("Invalid path: %s" % p)
    for p in every:                                                        # refusals that need no GPU come first
        if p.endswith(".npz"):
            check_feature_file(p, arch)
    if not torch.cuda.is_available():
        raise _lib.TiseLibraryError("fd_dinov2 needs an MI355X: there is no CPU path")
    _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    built = []

    def tower():                                                           # two feature files need no tower at all
        if not built:
            built.append(dinov2_hip.build_tower(weights, dev, arch, seed))
        return built[0]
    f1, m1, s1 = _side(paths[0], tower, dev, batch_size, num_workers, feed, arch)
    if save_features and tdist.is_main():
        fid_score.save_stats_npz(save_features, m1, s1, arch_info(arch)[1], f1)
    f2, m2, s2 = _side(paths[1], tower, dev, batch_size, num_workers, feed, arch)
    out = dict(fd=float(fid_score.calculate_frechet_distance(m1, s1, m2, s2)), kd=None, prdc=None)
    if kd:
        from . import kid
        out["kd"] = kid.kid_from_features(f1, f2, subsets=100, subset_size=1000)
    if prdc_k is not None:
        from . import prdc
        out["prdc"] = prdc.prdc_from_features(f1, f2, nearest_k=int(prdc_k))
    # every rank holds the same rows in the same order and evaluates these itself, as the k-NN metrics above
    if authpct or nearest_train:
        from . import authenticity
        ft = _side(train, tower, dev, batch_size, num_workers, feed, arch)[0]
        near = authenticity.nearest_train(ft, f2)
        if authpct:
            out["authpct"] = authenticity.authpct_from_counts(near["authentic"].sum(), len(near["authentic"]))
        if nearest_train and tdist.is_main():
            write_nearest_train_csv(nearest_train, near, paths[1], train)
    if vendi:
        from . import vendi as tvendi
        out["vendi"], out["vendi_reference"] = tvendi.vendi_from_features(f2), tvendi.vendi_from_features(f1)
    if fd_infinity:
        from . import fd_infinity as tfdinf
        out["fd_infinity"] = tfdinf.fd_infinity_from_features(f1, f2, seed=int(fd_infinity_seed))
    return out


def result_lines(res, arch, tag=""):
    lines = [f"FD-DINOv2 ({arch}): {res['fd']}{tag}"]
    if res["kd"] is not None:
        lines.append(f"KD-DINOv2 ({arch}): {res['kd'][0]} +- {res['kd'][1]}{tag}")
    if res["prdc"] is not None:
        lines += [f"{name.capitalize()}-DINOv2 ({arch}): {res['prdc'][name]}{tag}" for name in ("precision", "recall", "density", "coverage")]
    if "authpct" in res:
        lines.append(f"AuthPct-DINOv2 ({arch}): {res['authpct']}{tag}")
    if "vendi" in res:
        lines += [f"Vendi-DINOv2 ({arch}): {res['vendi']}{tag}", f"Vendi-DINOv2 reference ({arch}): {res['vendi_reference']}{tag}"]
    if "fd_infinity" in res:
        lines.append(f"FD-infinity-DINOv2 ({arch}): {res['fd_infinity']['fd_infinity']}{tag}")
    return lines


def parse_args(argv=None):
    from . import dinov2_model
    parser = argparse.ArgumentParser(description="FD-DINOv2 (and KD, precision / recall / density / coverage) on a DINOv2 ViT tower")
    parser.add_argument("--path1", type=str, required=True, help="reference images: a directory, or a feature file of --save-features")
    parser.add_argument("--path2", type=str, required=True, help="generated images: a directory, or a feature file of --save-features")
    parser.add_argument("--arch", default=ARCH, choices=list(dinov2_model.CONFIGS), help="the tower (default vitl14, the published metric's)")
    parser.add_argument("--kd", action="store_true", help="also report the kernel distance (KID's estimator in DINOv2 space)")
    parser.add_argument("--prdc", action="store_true", help="also report precision, recall, density and coverage in DINOv2 space")
    parser.add_argument("--prdc-k", type=int, default=5, help="nearest neighbours of --prdc (default 5)")
    parser.add_argument("--train", default="", type=str, help="the generator's training images: a directory, or a feature file of --save-features (same --arch)")
    parser.add_argument("--authpct", action="store_true", help="also report AuthPct: the share of --path2 samples that are not nearer to a --train row than that row's own nearest training neighbour")
    parser.add_argument("--nearest-train", default="", type=str, metavar="OUT.csv",
                        help="write every --path2 row's nearest --train row, its squared distance and the authentic flag to this CSV")
    parser.add_argument("--vendi", action="store_true", help="also report the Vendi score (linear kernel, q = 1) of --path2, and of --path1 for comparison")
    parser.add_argument("--fd-infinity", action="store_true", help="also report FD-infinity: FD extrapolated to infinitely many --path2 samples")
    parser.add_argument("--fd-infinity-seed", type=int, default=0, help="seed of the --fd-infinity subsets (default 0)")
    parser.add_argument("--weights", default=None, type=str, help="DINOv2 state_dict (.pth) of the chosen tower; default: $TORCH_HOME/hub/checkpoints/dinov2_<arch>_pretrain.pth")
    parser.add_argument("--synthetic-weights", action="store_true",
                        help="seeded stand-in tower (plumbing / throughput only; results are tagged)")
    parser.add_argument("--seed", default=0, type=int, help="seed of the stand-in parameters")
    parser.add_argument("--batch-size", type=int, default=50)
    parser.add_argument("--save-features", default="", type=str,
                        help="write --path1's feature rows (fp32), mu, sigma and the network tag to this .npz")
    parser.add_argument("--saved_file", default="", type=str, help="write the result lines here as well")
    parser.add_argument("--png-feed", default="ring", choices=["ring", "dataloader"])
    parser.add_argument("--num-workers", default=0, type=int, help="image decode processes (0 = auto)")
    parser.add_argument("--gpu", default="0", type=str, help="GPU to use")
    args = parser.parse_args(argv)
    if args.weights and args.synthetic_weights:
        parser.error("--synthetic-weights and --weights are mutually exclusive")
    if args.prdc and not 1 <= args.prdc_k <= 16:
        parser.error("--prdc-k must lie in 1 .. 16")
    if (args.authpct or args.nearest_train) and not args.train:
        parser.error("--authpct and --nearest-train need the training set: --train PATH")
    return args


def main(argv=None):
    args = parse_args(argv)
    for p in (args.path1, args.path2, args.train):                         # a file of another network: refused before the GPU is asked for
        if p.endswith(".npz") and os.path.exists(p):
            check_feature_file(p, args.arch)
    if not torch.cuda.is_available():
        raise _lib.TiseLibraryError("fd_dinov2 needs an MI355X: there is no CPU path")
    rank, world, local_rank = tdist.init_from_env()
    dev = torch.device(f"cuda:{local_rank}" if world > 1 else f"cuda:{args.gpu}")
    torch.cuda.set_device(dev)
    wpath, tag = tweights.resolve(args.weights, args.synthetic_weights, arch_info(args.arch)[2], f"DINOv2 {args.arch}")
    res = calculate_fd_dinov2_given_paths([args.path1, args.path2], args.batch_size, wpath, args.seed, args.num_workers, args.png_feed,
                                          args.arch, args.kd, args.prdc_k if args.prdc else None, args.save_features, args.train or None,
                                          args.authpct, args.nearest_train, args.vendi, args.fd_infinity, args.fd_infinity_seed)
    lines = result_lines(res, args.arch, tag)
    if tdist.is_main():
        if args.saved_file:
            with open(args.saved_file, "w") as f:
                f.write("\n".join(lines))                                  # no trailing newline, like fid_score --saved_file
        print("\n".join(lines))
    return res


if __name__ == "__main__":
    tdist.run_cli(main)
