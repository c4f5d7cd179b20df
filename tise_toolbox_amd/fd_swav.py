#!/usr/bin/env python3
"""FD-SwAV on MI355X: the Frechet distance -- and KD, precision / recall / density / coverage -- on the 2048-d pooled features of the
SwAV ResNet-50.

Morozov et al. 2021 ("On Self-Supervised Image Representations for GAN Evaluation") and Kynkaanniemi et al. 2023 ("The Role of
ImageNet Classes in Frechet Inception Distance") find that the features of a self-supervised network rank generators closer to
human judgement than Inception pool3, whose space is aligned with the ImageNet classes; the `swav` encoder of the `dgm-eval`
package (Stein et al. 2023, which fd_dinov2.py follows for DINOv2) is this metric:

    FD-SwAV     |mu1 - mu2|^2 + tr(S1 + S2 - 2 (S1 S2)^(1/2)) of np.mean / np.cov of the feature rows: device.StatsAccumulator(2048)
                and the Frechet solver, the FID machinery
    KD-SwAV     (--kd)   kid.kid_from_features: 100 subsets of at most 1000 rows, the polynomial kernel; printed as mean +- std
    --prdc      the four numbers of prdc.prdc_from_features(ref, gen, nearest_k = 5)

THE TOWER is resnet_hip.HipResNet50 on the split-precision convolutions (csrc/conv_split.hip, csrc/conv_pipe.hip, csrc/resnet.hip):
fp32-accurate features, no library convolution.  ``TISE_RESNET=torch`` runs the fp32 module on library kernels instead (the A/B
route).  The default parameter file is ``$TORCH_HOME/hub/checkpoints/swav_800ep_pretrain.pth.tar``.

PREPROCESSING (resnet_model.preprocess_u8): RGB, Pillow's 8-bit bicubic resize straight to 224 x 224, the BYTES kept; the tower
applies the ImageNet mean / std table itself.  The resize runs on the device for ring batches (csrc/resize.hip, Pillow-exact) and
in the DataLoader's workers with Pillow itself for a ragged directory: both hand the tower the same bytes.  The transform and the
file name are restated from memory; with the parity of the tower itself they are UNPINNED (README).

Every image of a directory is used.  Under torchrun the files are sharded as contiguous index ranges and the rows gathered in
walk order on every rank (as cmmd.embed_image_dir does); rank 0 prints and writes.
"""
import argparse
import os

import numpy as np
import torch

from . import _lib, dist as tdist, weights as tweights
from .resnet_model import NETWORK, OUT_DIM

RESOLUTION = 224
KIND = "swav-resnet50"


def statistics(feats):
    """(mu, sigma) of fp32 device rows -> fp64 numpy arrays: np.mean / np.cov (ddof 1) on the device."""
    from . import cmmd
    return cmmd.clip_statistics(feats)


def fd_swav_from_features(f1, f2):
    """The Frechet distance of two feature sets (device tensors or numpy arrays, (n, 2048)) -> Python float."""
    from . import cmmd, fid_score
    from .engine import require_gpu
    if cmmd._width(f1) != cmmd._width(f2):
        raise ValueError(f"feature widths differ: {cmmd._width(f1)} and {cmmd._width(f2)}")
    require_gpu()
    dev = f1.device if isinstance(f1, torch.Tensor) and f1.is_cuda else torch.device("cuda", torch.cuda.current_device())
    (m1, s1), (m2, s2) = statistics(cmmd._to_device_f32(f1, dev)), statistics(cmmd._to_device_f32(f2, dev))
    return float(fid_score.calculate_frechet_distance(m1, s1, m2, s2))


def check_feature_file(path):
    """The refusal of load_features_npz on the file's network tag alone (no rows are read, no GPU is needed)."""
    from . import fid_score
    with np.load(path, allow_pickle=True) as f:
        if "network" not in f.files:
            raise RuntimeError(f"{path}: no network tag: not a feature file of {NETWORK} (make one with fd_swav --save-features)")
        fid_score.check_stats_network(path, str(f["network"]), NETWORK)


def load_features_npz(path):
    """-> (features fp32 (n, 2048), mu, sigma) of a file --save-features wrote; a file of another network, or one without the
    rows, is refused."""
    check_feature_file(path)
    with np.load(path, allow_pickle=True) as f:
        if "features" not in f.files:
            raise RuntimeError(f"{path}: no 'features' array in this file; make it with fd_swav --save-features")
        feats = np.ascontiguousarray(f["features"], dtype=np.float32)
        if feats.ndim != 2 or feats.shape[1] != OUT_DIM:
            raise RuntimeError(f"{path}: features of shape {feats.shape}, expected (n, {OUT_DIM})")
        return feats, f["mu"][:], f["sigma"][:]


class _Paths(torch.utils.data.Dataset):
    """The DataLoader road: Pillow's own resize in the workers, the (224, 224, 3) bytes."""

    def __init__(self, paths, size=RESOLUTION):
        self.paths, self.size = paths, size

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, i):
        from PIL import Image
        from .resnet_model import preprocess_u8
        return preprocess_u8(Image.open(self.paths[i]), self.size)


@torch.no_grad()
def encode_paths(tower, paths, dev, batch, workers=0, feed="ring"):
    """``tower.features_from_u8`` of the files ``paths``, in order, every file used -> (len(paths), 2048) fp32 device rows.  The ring
    delivers uint8 batches of the files' own size, resized on the device; the DataLoader's workers resized with Pillow: the tower
    gets (n, 224, 224, 3) uint8 on both roads."""
    from . import device, feeds
    out = []

    def consume(loader):
        out.clear()                                           # the DataLoader pass after a ring that met an odd file starts afresh
        for x in loader:
            x = x.to(dev)
            if tuple(x.shape[1:3]) != (RESOLUTION, RESOLUTION):
                x = device.resize_u8_filter_only(x, (RESOLUTION, RESOLUTION), "bicubic")
            out.append(tower.features_from_u8(x))
    feeds.run(feeds.CLIP, paths, feeds.Options(png_feed=feed, num_workers=workers), consume, dev, batch, tdist.world_size(),
              loader_args={"ring": {"batch_size": 1, "group": batch, "rgb_only": False},
                           "dataloader": {"dataset": _Paths(paths), "pin_memory": False, "collate": None}})
    return torch.cat(out).contiguous() if out else torch.empty((0, OUT_DIM), dtype=torch.float32, device=dev)


def embed_image_dir(tower, path, dev, batch, workers=0, feed="ring"):
    """fp32 (n, 2048) features of EVERY image under ``path``, in img_data.get_filenames' walk order, on every rank."""
    from . import img_data
    files = img_data.get_filenames(path)
    rank, world, _ = tdist.env_world()
    lo, hi = tdist.shard_range(len(files), rank, world)
    return tdist.all_gather_rows(encode_paths(tower, files[lo:hi], dev, batch, workers, feed))


def _side(path, tower, dev, batch_size, num_workers, feed):
    """-> (fp32 device rows, mu, sigma) of a directory or a feature file."""
    if path.endswith(".npz"):
        feats, mu, sigma = load_features_npz(path)
        return torch.as_tensor(feats, device=dev), mu, sigma
    feats = embed_image_dir(tower(), path, dev, batch_size, num_workers, feed)
    if feats.shape[0] == 0:
        raise RuntimeError(f"no images under {path}")
    return (feats,) + statistics(feats)


def calculate_fd_swav_given_paths(paths, batch_size=50, weights=None, seed=0, num_workers=0, feed="ring", kd=False, prdc_k=None,
                                  save_features=""):
    """-> dict(fd=float, kd=(mean, std) | None, prdc=OrderedDict | None) of two paths, each a directory or a feature file.
    ``weights=None``: seeded stand-in parameters (the CLI only allows that behind --synthetic-weights).  ``save_features``: the
    FIRST path's rows (the reference set) are written there with their mu, sigma and the network tag."""
    from . import fid_score, resnet_hip
    for p in paths:
        if not os.path.exists(p):
            raise RuntimeError("Invalid path: %s" % p)
    for p in paths:                                                        # refusals that need no GPU come first
        if p.endswith(".npz"):
            check_feature_file(p)
    if not torch.cuda.is_available():
        raise _lib.TiseLibraryError("fd_swav needs an MI355X: there is no CPU path")
    _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    built = []

    def tower():                                                           # two feature files need no tower at all
        if not built:
            built.append(resnet_hip.build_tower(weights, dev, seed))
        return built[0]
    f1, m1, s1 = _side(paths[0], tower, dev, batch_size, num_workers, feed)
    if save_features and tdist.is_main():
        fid_score.save_stats_npz(save_features, m1, s1, NETWORK, f1)
    f2, m2, s2 = _side(paths[1], tower, dev, batch_size, num_workers, feed)
    out = dict(fd=float(fid_score.calculate_frechet_distance(m1, s1, m2, s2)), kd=None, prdc=None)
    if kd:
        from . import kid
        out["kd"] = kid.kid_from_features(f1, f2, subsets=100, subset_size=1000)
    if prdc_k is not None:
        from . import prdc
        out["prdc"] = prdc.prdc_from_features(f1, f2, nearest_k=int(prdc_k))
    return out


def result_lines(res, tag=""):
    lines = [f"FD-SwAV: {res['fd']}{tag}"]
    if res["kd"] is not None:
        lines.append(f"KD-SwAV: {res['kd'][0]} +- {res['kd'][1]}{tag}")
    if res["prdc"] is not None:
        lines += [f"{name.capitalize()}-SwAV: {res['prdc'][name]}{tag}" for name in ("precision", "recall", "density", "coverage")]
    return lines


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="FD-SwAV (and KD, precision / recall / density / coverage) on the SwAV ResNet-50")
    parser.add_argument("--path1", type=str, required=True, help="reference images: a directory, or a feature file of --save-features")
    parser.add_argument("--path2", type=str, required=True, help="generated images: a directory, or a feature file of --save-features")
    parser.add_argument("--kd", action="store_true", help="also report the kernel distance (KID's estimator in SwAV space)")
    parser.add_argument("--prdc", action="store_true", help="also report precision, recall, density and coverage in SwAV space")
    parser.add_argument("--prdc-k", type=int, default=5, help="nearest neighbours of --prdc (default 5)")
    parser.add_argument("--weights", default=None, type=str,
                        help="SwAV checkpoint or torchvision-style ResNet-50 state dict; default: $TORCH_HOME/hub/checkpoints/swav_800ep_pretrain.pth.tar")
    parser.add_argument("--synthetic-weights", action="store_true",
                        help="seeded stand-in tower (plumbing / throughput only; results are tagged)")
    parser.add_argument("--seed", default=0, type=int, help="seed of the stand-in parameters")
    parser.add_argument("--batch-size", type=int, default=50)
    parser.add_argument("--save-features", default="", type=str,
                        help="write --path1's feature rows (fp32), mu, sigma and the network tag to this .npz")
    parser.add_argument("--saved_file", default="", type=str, help="write the result lines here as well")
    parser.add_argument("--png-feed", default="ring", choices=["ring", "dataloader"])
    parser.add_argument("--num-workers", default=0, type=int, help="image decode processes (0 = auto)")
    parser.add_argument("--gpu_id", default="0", type=str, help="GPU to use")
    args = parser.parse_args(argv)
    if args.weights and args.synthetic_weights:
        parser.error("--synthetic-weights and --weights are mutually exclusive")
    if args.prdc and not 1 <= args.prdc_k <= 16:
        parser.error("--prdc-k must lie in 1 .. 16")
    return args


def main(argv=None):
    args = parse_args(argv)
    for p in (args.path1, args.path2):                                     # a file of another network: refused before the GPU is asked for
        if p.endswith(".npz") and os.path.exists(p):
            check_feature_file(p)
    if not torch.cuda.is_available():
        raise _lib.TiseLibraryError("fd_swav needs an MI355X: there is no CPU path")
    rank, world, local_rank = tdist.init_from_env()
    dev = torch.device(f"cuda:{local_rank}" if world > 1 else f"cuda:{args.gpu_id}")
    torch.cuda.set_device(dev)
    wpath, tag = tweights.resolve(args.weights, args.synthetic_weights, KIND)
    res = calculate_fd_swav_given_paths([args.path1, args.path2], args.batch_size, wpath, args.seed, args.num_workers, args.png_feed,
                                        args.kd, args.prdc_k if args.prdc else None, args.save_features)
    lines = result_lines(res, tag)
    if tdist.is_main():
        if args.saved_file:
            with open(args.saved_file, "w") as f:
                f.write("\n".join(lines))                                  # no trailing newline, like fid_score --saved_file
        print("\n".join(lines))
    return res


if __name__ == "__main__":
    tdist.run_cli(main)
