#!/usr/bin/env python3
"""IS* for CUB birds on MI355X: drop-in for the reference ``image_realism/IS/bird/inception_score_star_bird.py``.

    python -m tise_toolbox_amd.inception_score_bird --image_folder DIR --saved_file OUT.txt \\
        [--checkpoint_dir IS/bird/inception_finetuned_models/birds_valid299/model.ckpt]

What the reference does, and what runs here:

* network: the 2016 TF-slim InceptionV3 fine-tuned to 50 bird classes + background (``--num_classes 50`` -> 51 logits),
  restored from the TensorFlow checkpoint ``--checkpoint_dir`` with the exponential-moving-average shadows (:196-201).
  Here ``--network slim`` of the toolbox (inception.py), its weights read by tf_checkpoint.py; the trunk and the
  classifier run in HIP as for every other network.
* input: ``scipy.misc.imresize(img, (299, 299, 3), interp="bilinear")`` then ``/ 127.5 - 1.0`` (:64-71): the Pillow-exact
  device resize and the ``slim`` input table (device.make_lut).
* sampling (:80-101): the files in ``os.walk`` order (``img_data.get_filenames``), ``np.random.shuffle`` of their indices,
  and only the first ``floor(N / batch_size) * batch_size`` of that order are scored; the splits follow that order.  The
  reference's shuffle is unseeded, and so is ours unless ``--shuffle-seed S`` is given: under ``np.random.seed(S)`` the
  reference draws exactly the order ``bird_order`` draws.  ``--batch_size`` decides only this selection; the device batch
  is the toolbox's own.  Under torchrun one order is drawn on rank 0 and broadcast to every rank.
* reduction (:189-194, :98-108): logits[:, 1:] / T_BIRD, softmax, 10 splits, KL, exp, mean / std -- csrc/is_score.hip.
* output: ``mean: %.2f std: %.2f`` on stdout and ``IS = {mean}  +-  {std}`` in ``--saved_file`` (:110, :208-209).

Deviation (INTEGRATION deviation 5): every image is decoded with ``convert("RGB")``.  The reference tiles a gray image's
bytes over three channels with ``np.resize`` (:65-66: not a channel copy) and fails on RGBA files.
"""
import os
import sys
from argparse import ArgumentDefaultsHelpFormatter, ArgumentParser

import numpy as np

from . import dist as tdist, inception_score as isc, weights as tweights
from .engine import T_BIRD

DEFAULT_CHECKPOINT = os.path.join("IS", "bird", "inception_finetuned_models", "birds_valid299", "model.ckpt")


def bird_order(n, seed=None):
    """The reference's ``indices = list(np.arange(n)); np.random.shuffle(indices)`` (:84-85): with ``seed`` the stream of
    ``np.random.seed(seed)``, without it NumPy's global generator as the reference leaves it (unseeded)."""
    indices = list(np.arange(n))
    if seed is None:
        np.random.shuffle(indices)
    else:
        np.random.RandomState(seed).shuffle(indices)
    return np.asarray(indices, dtype=np.int64)


def bird_selection(files, batch_size, seed=None, order=None):
    """Files the reference scores, in the order it scores them: the first floor(N / batch_size) * batch_size of the
    shuffled order (:83-94)."""
    if order is None:
        order = bird_order(len(files), seed)
    keep = (len(files) // batch_size) * batch_size
    return [files[int(i)] for i in order[:keep]]


def _shared_order(n, seed):
    """One order for every rank of a torchrun job (RP_coco.py's rule): drawn on rank 0, broadcast."""
    rank, world, _ = tdist.env_world()
    if world == 1:
        return bird_order(n, seed)
    import torch
    import torch.distributed as dist
    dev = torch.device("cuda", torch.cuda.current_device())
    t = torch.from_numpy(bird_order(n, seed)).to(dev) if rank == 0 else torch.empty(n, dtype=torch.int64, device=dev)
    dist.broadcast(t, src=0)
    return t.cpu().numpy()


def check_first_image(path):
    """The reference's asserts on its first image (:76-79), on the image as the toolbox decodes it (RGB, uint8)."""
    from PIL import Image
    with Image.open(path) as im:
        img = np.asarray(im.convert("RGB"))
    assert img.ndim == 3
    assert np.max(img) > 10, f"{path}: the first image's maximum is {np.max(img)} (the reference asserts > 10)"
    assert np.min(img) >= 0.0


def _build_parser():
    parser = ArgumentParser(formatter_class=ArgumentDefaultsHelpFormatter)
    # tf.app.flags of the reference (:35-49)
    parser.add_argument("--checkpoint_dir", type=str, default=DEFAULT_CHECKPOINT,
                        help="TensorFlow checkpoint of the fine-tuned network (V1 file or V2 prefix)")
    parser.add_argument("--image_folder", type=str, default="")
    parser.add_argument("--num_classes", type=int, default=50, help="bird classes; the network has one more (background 0)")
    parser.add_argument("--splits", type=int, default=10)
    parser.add_argument("--batch_size", type=int, default=64, help="decides which images are scored (floor(N / batch_size) * batch_size)")
    parser.add_argument("--gpu", type=int, default=0)
    parser.add_argument("--saved_file", type=str, default="")
    # the toolbox's own
    parser.add_argument("--synthetic-weights", action="store_true",
                        help="seeded stand-in parameters (plumbing / throughput only; results are tagged)")
    parser.add_argument("--seed", type=int, default=0, help="seed of the --synthetic-weights parameters")
    parser.add_argument("--shuffle-seed", type=int, default=None,
                        help="seed of the image order (default: unseeded, like the reference); S draws what the reference "
                             "draws under np.random.seed(S)")
    parser.add_argument("--temperature", type=float, default=T_BIRD, help="IS* temperature (the reference's T_BIRD)")
    parser.add_argument("--num-workers", type=int, default=0, help="decode processes (0: automatic)")
    parser.add_argument("--png-feed", type=str, default="ring", choices=["ring", "loader"],
                        help="ring: native decode processes + shared pinned ring; loader: the DataLoader path")
    parser.add_argument("--jpeg-feed", type=str, default=None, choices=["native", "pillow"],
                        help="native: JPEG files of the native subset (the CUB photographs) are Huffman-decoded by threads of this "
                             "process and reconstructed on the GPU (jpeg_feed.py); pillow: every file through Pillow.  Default: native "
                             "for image sets whose files differ in size, pillow for sets of one size")
    return parser


def main(argv=None):
    args = _build_parser().parse_args(argv)
    rank, world, _ = tdist.init_from_env()
    if world == 1:
        os.environ.setdefault("HIP_VISIBLE_DEVICES", str(args.gpu))
    # --synthetic-weights with an explicit --checkpoint_dir is refused (weights.resolve); the default path is not a request
    explicit = args.checkpoint_dir != DEFAULT_CHECKPOINT
    wpath, tag = tweights.resolve(args.checkpoint_dir if explicit or not args.synthetic_weights else None,
                                  args.synthetic_weights, "slim")
    isc.configure(weights=wpath, num_classes=args.num_classes + 1, seed=args.seed, temperature=args.temperature,
                  rule="bird", drop_first_class=True, fc_bias="auto", network="slim", num_workers=args.num_workers,
                  png_feed=args.png_feed, jpeg_feed=args.jpeg_feed)
    print(args.image_folder)
    files = isc.img_data.get_filenames(args.image_folder)
    if not files:
        raise SystemExit(f"no .jpg / .png files under {args.image_folder!r}")
    check_first_image(files[0])
    print("images", len(files))
    images = bird_selection(files, args.batch_size, order=_shared_order(len(files), args.shuffle_seed))
    if not images:
        raise SystemExit(f"{len(files)} images and --batch_size {args.batch_size}: floor(N / batch_size) = 0 batches "
                         f"(the reference scores no image and fails)")
    from .engine import run_with_exact_fallback
    mean, std = run_with_exact_fallback(lambda: isc.get_inception_score(images, splits=args.splits), "the Inception Score")
    if tdist.is_main():
        print("mean:", "%.2f" % mean, "std:", "%.2f" % std + tag)
        if args.saved_file:
            with open(args.saved_file, "w") as f:
                f.write(f"IS = {mean}  +-  {std}" + tag)
    sys.stdout.flush()
    return mean, std


if __name__ == "__main__":
    tdist.run_cli(main)
