#!/usr/bin/env python3
"""FD-SwAV on MI355X: the Frechet distance -- and KD, precision / recall / density / coverage -- on the 2048-d pooled features of the
SwAV ResNet-50.

Morozov et al. 2021 ("On Self-Supervised Image Representations for GAN Evaluation") and Kynkaanniemi et al. 2023 ("The Role of
ImageNet Classes in Frechet Inception Distance") find that the features of a self-supervised network rank generators closer to
human judgement than Inception pool3, whose space is aligned with the ImageNet classes; the `swav` encoder of the `dgm-eval`
package (Stein et al. 2023) is this metric:

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

The run, the feature files, the shared options and the result lines are feature_space.py's; this module describes the space (``space``)
and holds the tower's image loop.
"""
import argparse

import torch

from . import dist as tdist, feature_space as fs
from .resnet_model import NETWORK, OUT_DIM

RESOLUTION = 224
KIND = "swav-resnet50"


def space(weights=None, seed=0):
    """The SwAV ResNet-50 space.  ``weights=None``: seeded stand-in parameters of ``seed``."""
    def build_tower(dev):
        from . import resnet_hip
        return resnet_hip.build_tower(weights, dev, seed)
    return fs.Space("fd_swav", NETWORK, OUT_DIM, build_tower, embed_image_dir)


def check_feature_file(path):
    return fs.check_feature_file(path, NETWORK, "fd_swav")


def load_features_npz(path):
    return fs.load_features_npz(path, NETWORK, OUT_DIM, "fd_swav")


fd_swav_from_features = fs.frechet_from_features


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

    def per_batch(x):
        x = x.to(dev)
        if tuple(x.shape[1:3]) != (RESOLUTION, RESOLUTION):
            x = device.resize_u8_filter_only(x, (RESOLUTION, RESOLUTION), "bicubic")
        return tower.features_from_u8(x)
    return feeds.encode_files(per_batch, paths, dev, batch, workers, feed, _Paths(paths), False, OUT_DIM, torch.float32)


def embed_image_dir(tower, path, dev, batch, workers=0, feed="ring"):
    """fp32 (n, 2048) features of EVERY image under ``path``, in img_data.get_filenames' walk order, on every rank."""
    return fs.embed_image_dir(lambda files: encode_paths(tower, files, dev, batch, workers, feed), path)


def calculate_fd_swav_given_paths(paths, batch_size=50, weights=None, seed=0, num_workers=0, feed="ring", kd=False, prdc_k=None,
                                  save_features=""):
    """-> dict(fd=float, kd=(mean, std) | None, prdc=OrderedDict | None) of two paths, each a directory or a feature file.
    ``weights=None``: seeded stand-in parameters (the CLI only allows that behind --synthetic-weights).  ``save_features``: the
    FIRST path's rows (the reference set) are written there with their mu, sigma and the network tag."""
    want = ["fd"] + ["kd"] * bool(kd) + ["prdc"] * (prdc_k is not None)
    return fs.fd_result(fs.given_paths(space(weights, seed), paths, batch_size, num_workers, feed, save_features, want=want, prdc_k=prdc_k))


def result_lines(res, tag=""):
    return fs.result_lines(res, "SwAV", tag)


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="FD-SwAV (and KD, precision / recall / density / coverage) on the SwAV ResNet-50")
    fs.add_arguments(parser, "paths kd weights batch output", space="SwAV", gpu="--gpu_id", weights_help="SwAV checkpoint or "
                     "torchvision-style ResNet-50 state dict; default: $TORCH_HOME/hub/checkpoints/swav_800ep_pretrain.pth.tar")
    return fs.parse_fd_args(parser, argv)


def main(argv=None):
    args = parse_args(argv)
    wpath, tag = fs.start_cli(args, "fd_swav", NETWORK, KIND, gpu="gpu_id")
    res = calculate_fd_swav_given_paths([args.path1, args.path2], args.batch_size, wpath, args.seed, args.num_workers, args.png_feed,
                                        args.kd, args.prdc_k if args.prdc else None, args.save_features)
    tdist.write_lines(result_lines(res, tag), args.saved_file)
    return res


if __name__ == "__main__":
    tdist.run_cli(main)
