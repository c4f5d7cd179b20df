#!/usr/bin/env python3
"""Counting alignment: drop-in for counting_alignment/CA.py.

Same CLI (CA.py:105-112: --image_dir --ct_input_file --result_file --gpu_id), same input pickle (a list of items {caption_id,
counting_info: {class name: count}, ..}), images at ``image_dir/<caption_id>.png`` (:173), same preprocessing (:120-128: RGB,
Pillow's 8-bit bilinear resize straight to 448 x 448, the ImageNet mean / std), same prediction (:150-166: a class is present when
its confidence is > 0, its count is np.round(present * mean of the density map), half to even; a class is predicted when the count
is not 0 -- it may be negative), same per-item error (:176-185: over the keys of counting_info, sqrt(mean((gt - pred)^2)) with pred =
0.0 for a key that is not predicted or not one of the 80 names) and the same result text ``CA = {mean over the items}`` (:187-194).

THE COUNTER is countseg_hip.HipCountSeg: the ResNet-50 trunk of FD-SwAV used fully convolutionally, one split-precision 1 x 1
convolution and csrc/countseg.hip; confidence and density mean leave the device as fp64.  ``TISE_COUNTSEG=torch`` runs the fp32
module on library kernels instead (the A/B route).  The network itself is restated, not ported: parity with the ``nest`` package
is UNPINNED (README), and the loader takes the head under this project's names only.

As in RP_coco.py / PA.py the order of work changes: an image that occurs in several items is encoded once, the images in batches
(the resize on the device for ring batches -- csrc/resize.hip, Pillow-exact -- and in the DataLoader's workers with Pillow itself
for a ragged directory).  Under torchrun the items are sharded and {sum of rmse, n} all-reduced once.  Nothing runs at import.
"""
import argparse
import os
import pickle

import numpy as np
import torch

from . import _lib, dist as tdist, weights as tweights

RESOLUTION = 448                                                             # CA.py:121
KIND = "countseg"
# the 80 MS-COCO category names in category-id order (CA.py's ``nms``): facts of the dataset
CLASS_NAMES = (
    "person", "bicycle", "car", "motorcycle", "airplane", "bus", "train", "truck", "boat", "traffic light",
    "fire hydrant", "stop sign", "parking meter", "bench", "bird", "cat", "dog", "horse", "sheep", "cow",
    "elephant", "bear", "zebra", "giraffe", "backpack", "umbrella", "handbag", "tie", "suitcase", "frisbee",
    "skis", "snowboard", "sports ball", "kite", "baseball bat", "baseball glove", "skateboard", "surfboard", "tennis racket", "bottle",
    "wine glass", "cup", "fork", "knife", "spoon", "bowl", "banana", "apple", "sandwich", "orange",
    "broccoli", "carrot", "hot dog", "pizza", "donut", "cake", "chair", "couch", "potted plant", "bed",
    "dining table", "toilet", "tv", "laptop", "mouse", "remote", "keyboard", "cell phone", "microwave", "oven",
    "toaster", "sink", "refrigerator", "book", "clock", "vase", "scissors", "teddy bear", "hair drier", "toothbrush",
)
_INDEX = {name: i for i, name in enumerate(CLASS_NAMES)}


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="Counting alignment (CA) on CountSeg over the split-precision ResNet-50")
    parser.add_argument("--image_dir", default="", type=str, help="Path to the folder containing generated images.")
    parser.add_argument("--ct_input_file", default="captions/CA_input_captions.pkl", type=str)
    parser.add_argument("--result_file", default="", type=str, help="Path to file saving result")
    parser.add_argument("--gpu_id", default=0, type=int)
    parser.add_argument("--weights", default=None, type=str,
                        help="CountSeg checkpoint ({'model': state_dict} or a state dict; trunk as features.*, head as mix / cls / den); "
                             "default: weights/coco14.pt")
    parser.add_argument("--synthetic-weights", action="store_true",
                        help="seeded stand-in parameters (plumbing / throughput only; results are tagged)")
    parser.add_argument("--seed", default=0, type=int, help="seed of the stand-in parameters")
    parser.add_argument("--batch-size", default=50, type=int)
    parser.add_argument("--num-workers", default=0, type=int, help="image decode processes (0 = auto)")
    parser.add_argument("--png-feed", default="ring", choices=["ring", "dataloader"])
    parser.add_argument("--per-image", default="", metavar="OUT.csv", help="item,caption_id,rmse,predicted (name:count;..) per item")
    return parser.parse_args(argv)


# ---- the host arithmetic (CA.py:150-187) ------------------------------------------------------------------------------------------
def predicted_counts(rows):
    """(n, 2 C) fp64 rows [conf | den] -> (n, C) fp64 counts: np.round((conf > 0) * den), numpy's half-to-even; class c is
    predicted where the count is not 0 (it may be negative)."""
    rows = np.asarray(rows, dtype=np.float64)
    c = rows.shape[1] // 2
    return np.round((rows[:, :c] > 0).astype(np.float64) * rows[:, c:])


def item_rmse(counting_info, counts):
    """One item: over the keys of ``counting_info`` in their order, pred = the count when the key is one of the 80 names and
    predicted, else 0.0; sqrt(mean((gt - pred)^2)) in fp64."""
    gt = np.asarray([float(v) for v in counting_info.values()], dtype=np.float64)
    pred = np.asarray([float(counts[_INDEX[k]]) if k in _INDEX and counts[_INDEX[k]] != 0 else 0.0 for k in counting_info],
                      dtype=np.float64)
    return float(np.sqrt(np.mean((gt - pred) ** 2)))


def predicted_text(counts):
    """``name:count;..`` of the predicted classes in class order (the CSV's last column)."""
    return ";".join(f"{CLASS_NAMES[i]}:{int(counts[i])}" for i in range(len(CLASS_NAMES)) if counts[i] != 0)


def load_items(path):
    with open(path, "rb") as f:
        items = pickle.load(f)
    if not isinstance(items, (list, tuple)):
        raise ValueError(f"{path}: a list of items {{caption_id, counting_info, ..}} is expected (got {type(items).__name__})")
    for k, it in enumerate(items):
        if not isinstance(it, dict) or "caption_id" not in it or not isinstance(it.get("counting_info"), dict):
            raise ValueError(f"{path}: item {k} has no caption_id / counting_info")
        if not it["counting_info"]:
            raise ValueError(f"{path}: item {k} (caption_id {it['caption_id']}) has an empty counting_info: its error is undefined")
    return list(items)


class _Paths(torch.utils.data.Dataset):
    """The DataLoader road: Pillow's own resize in the workers, the (448, 448, 3) bytes."""

    def __init__(self, paths):
        self.paths = paths

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, i):
        from PIL import Image
        from .countseg_model import preprocess_u8
        return preprocess_u8(Image.open(self.paths[i]), RESOLUTION)


@torch.no_grad()
def encode_paths(counter, paths, dev, batch, workers=0, feed="ring"):
    """``counter.rows_from_u8`` of the files ``paths``, in order, every file used -> (len(paths), 2 C) fp64 device rows.  The ring
    delivers uint8 batches of the files' own size, resized on the device; the DataLoader's workers resized with Pillow: the counter
    gets (n, 448, 448, 3) uint8 on both roads."""
    from . import device, feeds

    def per_batch(x):
        x = x.to(dev)
        if tuple(x.shape[1:3]) != (RESOLUTION, RESOLUTION):
            x = device.resize_u8_filter_only(x, (RESOLUTION, RESOLUTION), "bilinear")
        return counter.rows_from_u8(x)
    return feeds.encode_files(per_batch, paths, dev, batch, workers, feed, _Paths(paths), False, 2 * counter.n_classes, torch.float64)


def ca_of_items(counter, items, image_dir, dev, batch, workers=0, feed="ring"):
    """-> (rmse per item (n,) fp64, counts per item (n, C) fp64).  An image that occurs in several items is encoded once; a missing
    file is refused by name before anything is encoded."""
    table, order = {}, []
    for it in items:
        p = os.path.join(image_dir, str(it["caption_id"]) + ".png")
        if p not in table:
            if not os.path.isfile(p):
                raise FileNotFoundError(f"CA: {p} (caption_id {it['caption_id']}) does not exist")
            table[p] = len(table)
        order.append(table[p])
    if not items:
        return np.zeros(0), np.zeros((0, len(CLASS_NAMES)))
    rows = encode_paths(counter, list(table), dev, batch, workers, feed).cpu().numpy()
    counts = predicted_counts(rows)[np.asarray(order)]
    return np.asarray([item_rmse(it["counting_info"], counts[k]) for k, it in enumerate(items)], dtype=np.float64), counts


def main(argv=None):
    args = parse_args(argv)
    if not torch.cuda.is_available():
        raise _lib.TiseLibraryError("CA needs an MI355X: there is no CPU path")
    rank, world, local_rank = tdist.init_from_env()
    if world > 1 and args.per_image:
        raise RuntimeError("--per-image under torchrun: the items are sharded and only {sum, n} is exchanged; run one process")
    dev = torch.device(f"cuda:{local_rank}" if world > 1 else f"cuda:{args.gpu_id}")
    torch.cuda.set_device(dev)
    wpath, tag = tweights.resolve(args.weights, args.synthetic_weights, KIND)
    items = load_items(args.ct_input_file)
    print("Load data from: ", args.ct_input_file)
    from . import countseg_hip
    counter = countseg_hip.build_counter(wpath, dev, args.seed)
    lo, hi = tdist.shard_range(len(items), rank, world)
    rmse, counts = ca_of_items(counter, items[lo:hi], args.image_dir, dev, args.batch_size, args.num_workers, args.png_feed)
    sums = torch.tensor([float(np.sum(rmse)), float(len(rmse))], dtype=torch.float64, device=dev)
    tdist.all_reduce_sum_(sums)
    total, n = (float(v) for v in sums.cpu())
    # one process: np.mean's own (pairwise) sum, the reference's figure to the bit; sharded: the sum of the ranks' sums
    ca = float(np.mean(rmse)) if world == 1 and len(rmse) else (total / n if n else float("nan"))
    if tdist.is_main():
        if args.per_image:
            with open(args.per_image, "w") as f:
                f.write("item,caption_id,rmse,predicted\n")
                for k, it in enumerate(items):
                    f.write(f"{k},{it['caption_id']},{float(rmse[k])!r},{predicted_text(counts[k])}\n")
        if args.result_file:
            with open(args.result_file, "w") as f:
                f.write(f"CA = {ca}{tag}")                                    # CA.py:190-191
        print(f"CA = {ca}{tag}")                                              # :194
    return {"ca": ca, "n": int(n), "rmse": rmse, "counts": counts}


if __name__ == "__main__":
    tdist.run_cli(main)
