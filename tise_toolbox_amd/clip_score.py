#!/usr/bin/env python3
"""CLIPScore on MI355X: the paired image-caption cosine that text-to-image work reports beside FID.

    python -m tise_toolbox_amd.clip_score --image_dir D (--captions FILE.json | --rp_input_file FILE.pkl)
        [--tower ViT-B/32|ViT-L/14@336|ViT-H-14] [--weights PATH] [--vocab PATH] [--prefix "A photo depicts "] [--w 2.5]
        [--save-features OUT.npz] [--saved_file OUT.txt] [--batch-size 256] [--synthetic-weights] [--gpu_id 0]

CLIPScore (Hessel et al., EMNLP 2021, "CLIPScore: A Reference-free Evaluation Metric for Image Captioning"): with c the caption
embedding and v the image embedding of a pair,

    CLIPScore = w * max(cos(c, v), 0),   w = 2.5,   reported as the mean over the pairs (+- the population std here).

The second result line, ``Cosine x100``, is the plain mean cosine times 100.  On ``--tower ViT-H-14`` with HPS v2's fine-tuned
parameters (Wu et al. 2023; an open_clip ViT-H/14 state_dict) and ``--prefix ""`` that is the HPS v2 number.  PickScore's
published file is a Hugging Face ``CLIPModel`` and is refused (openclip_model.py); RefCLIPScore is out of scope.

INPUTS.  ``--captions``: a JSON object {file name, with or without its extension: caption}, the layout of Hessel's
``clipscore.py``; every image file of the directory must have a caption and every caption an image.  ``--rp_input_file``: the
reference toolbox's R-precision pickle (text_relevance/RP_coco.py: a list of {caption_id, caption, mismatched_captions}); the
pair is the TRUE caption and ``<caption_id>.png``.  Every pair is used.

WHAT RUNS WHERE.  The images go through RP_coco.encode_paths (the PNG ring, clip's preprocess on the device at the tower's
resolution), the DISTINCT captions -- each with ``--prefix`` in front, CLIPScore's "A photo depicts " by default -- through
RP_coco.embed_texts; the towers are clip_hip.HipTowers (TISE_CLIP=torch, and ViT-H-14 by itself -- it is wider than the 1024
columns HipTowers holds --: the fp16 module on library kernels).  The cosines come from
``device.paired_cosine`` (csrc/clip_ops.hip, tise_paired_cosine: fp64 in a fixed order, one wave per pair, no n x n product), the
mean and the population std are formed in fp64 on the host from ``{n, sum, sum of squares}``.  Under torchrun the PAIRS are
sharded and the only exchange is one all-reduce of those three numbers for each of the two result lines.

UNPINNED, restated from memory: the prefix string and w = 2.5 (Hessel's clipscore.py), open_clip's ViT-H-14 configuration and
preprocessing (openclip_model.py).  Parity of any tower with the `clip` / `open_clip` packages is unpinned: there are no
parameter files here.  What is pinned: the cosine kernel against extended precision, the result lines against numpy fp64 on the
saved rows, and the towers against this project's own fp32 module on seeded parameters.
"""
import argparse
import json
import os
import pickle

import numpy as np
import torch

from . import _lib, clip_model, device, dist as tdist, openclip_model, weights as tweights

PREFIX = "A photo depicts "          # Hessel's clipscore.py, from memory
W = 2.5
TOWER = "ViT-B/32"
IMAGE_EXTENSIONS = (".png", ".jpg", ".jpeg")
# weights._KINDS entry of a tower's default parameter file; ViT-H-14 has none (--weights or --synthetic-weights)
_KINDS = {"ViT-B/32": "clip", "ViT-L/14@336": "clip-l14-336", "ViT-H-14": None}


def towers():
    return list(clip_model.CONFIGS) + list(openclip_model.CONFIGS)


# ---- host logic ------------------------------------------------------------------------------------------------------
def pairs_from_captions(image_dir, captions):
    """{file name with or without extension: caption} -> ([image path], [caption]) sorted by path.  Refused, with the reason: a
    caption whose image is not in the directory, an image file of the directory without a caption, a name given twice (with and
    without its extension), a caption that is not a string."""
    if not isinstance(captions, dict):
        raise RuntimeError("the captions file must hold one JSON object {file name: caption}")
    files = sorted(f for f in os.listdir(image_dir) if f.lower().endswith(IMAGE_EXTENSIONS))
    by_stem = {}
    for f in files:
        by_stem.setdefault(os.path.splitext(f)[0], []).append(f)
    chosen = {}
    for key, cap in captions.items():
        if not isinstance(cap, str):
            raise RuntimeError(f"the caption of {key!r} is not a string")
        if key in files:
            f = key
        elif len(by_stem.get(key, [])) == 1:
            f = by_stem[key][0]
        elif key in by_stem:
            raise RuntimeError(f"caption {key!r} names more than one image of {image_dir}: {by_stem[key]}")
        else:
            raise RuntimeError(f"missing image: caption {key!r} has no image file in {image_dir}")
        if f in chosen:
            raise RuntimeError(f"image {f!r} has two captions (given with and without its extension)")
        chosen[f] = cap
    for f in files:
        if f not in chosen:
            raise RuntimeError(f"missing caption: image {f!r} of {image_dir} has no entry in the captions file")
    return [os.path.join(image_dir, f) for f in files], [chosen[f] for f in files]


def pairs_from_rp(image_dir, rp_input):
    """The reference's RP pickle -> ([<image_dir>/<caption_id>.png], [true caption]) in item order."""
    paths, caps = [], []
    for n, item in enumerate(rp_input):
        if not isinstance(item, dict) or "caption_id" not in item:
            raise RuntimeError(f"item {n} of the RP input has no 'caption_id'")
        if not isinstance(item.get("caption"), str):
            raise RuntimeError(f"missing caption: item {n} (caption_id {item['caption_id']}) of the RP input has no 'caption'")
        p = os.path.join(image_dir, str(item["caption_id"]) + ".png")
        if not os.path.exists(p):
            raise RuntimeError(f"missing image: {p} (caption_id {item['caption_id']} of the RP input)")
        paths.append(p)
        caps.append(item["caption"])
    return paths, caps


def load_pairs(image_dir, captions_file=None, rp_input_file=None):
    if bool(captions_file) == bool(rp_input_file):
        raise RuntimeError("give exactly one of --captions FILE.json and --rp_input_file FILE.pkl")
    if not os.path.isdir(image_dir):
        raise RuntimeError("Invalid path: %s" % image_dir)
    if captions_file:
        with open(captions_file) as f:
            return pairs_from_captions(image_dir, json.load(f))
    with open(rp_input_file, "rb") as f:
        return pairs_from_rp(image_dir, pickle.load(f))


def score_sums(cos, w=W):
    """fp64 cosines of a shard -> (2, 3) float64 [[n, sum, sum of squares] of w max(cos, 0), the same of cos]: additive over
    shards, an empty one included."""
    cos = np.asarray(cos, dtype=np.float64).reshape(-1)
    s = float(w) * np.maximum(cos, 0.0)                                     # np.maximum keeps a NaN: a zero row shows in the result
    return np.array([[cos.size, s.sum(), (s * s).sum()], [cos.size, cos.sum(), (cos * cos).sum()]], dtype=np.float64)


def result_from_sums(sums):
    """(2, 3) sums -> dict: clip_score (mean), clip_score_std (population std), cosine_x100 (100 mean cos), n."""
    sums = np.asarray(sums, dtype=np.float64)
    n = int(sums[0, 0])
    if n < 1:
        raise RuntimeError("CLIPScore needs at least one image-caption pair")
    mean = sums[0, 1] / n
    var = max(sums[0, 2] / n - mean * mean, 0.0) if np.isfinite(mean) else float("nan")
    return {"clip_score": float(mean), "clip_score_std": float(np.sqrt(var)), "cosine_x100": float(100.0 * sums[1, 1] / n), "n": n}


def result_lines(res, tower, tag=""):
    return [f"CLIPScore ({tower}): {res['clip_score']} +- {res['clip_score_std']}{tag}",
            f"Cosine x100 ({tower}): {res['cosine_x100']}{tag}"]


# ---- device ----------------------------------------------------------------------------------------------------------
def _to_device(f, dev):
    if isinstance(f, torch.Tensor):
        return f.to(dev) if f.dtype in (torch.float16, torch.float32) else f.to(dev, torch.float32)
    f = np.ascontiguousarray(f)
    return torch.as_tensor(f if f.dtype == np.float16 else f.astype(np.float32), device=dev)


def paired_cosines(img, txt):
    """cos of row i of ``img`` with row i of ``txt`` ((n, d) device tensors or numpy arrays, fp16 or fp32, normalised or not) ->
    (n,) float64 numpy array from device.paired_cosine."""
    from .engine import require_gpu
    require_gpu()
    dev = img.device if isinstance(img, torch.Tensor) and img.is_cuda else torch.device("cuda", torch.cuda.current_device())
    a, b = _to_device(img, dev), _to_device(txt, dev)
    if a.dtype != b.dtype:
        a, b = a.float(), b.float()
    return device.paired_cosine(a, b).cpu().numpy()


def clip_score_from_features(img, txt, w=W):
    """Paired embeddings -> dict(clip_score, clip_score_std, cosine_x100, n, cos): the two result lines' numbers and the fp64
    cosines they are the statistics of."""
    cos = paired_cosines(img, txt)
    res = result_from_sums(score_sums(cos, w))
    res["cos"] = cos
    return res


def tower_kind(tower):
    if tower not in towers():
        raise ValueError(f"unknown tower {tower!r}: one of {towers()}")
    return _KINDS.get(tower)


def _tokenizer(vocab):
    return clip_model.BPETokenizer(vocab) if vocab else clip_model.HashTokenizer()


@torch.no_grad()
def embed_pairs(model, tokenizer, paths, captions, dev, batch_size=256, prefix=PREFIX, num_workers=0, feed="ring"):
    """-> (image rows (n, d) fp16 as the tower gives them, caption rows (n, d) fp16: RP_coco.embed_texts' normalised rows of the
    distinct prefixed captions, gathered per pair)."""
    from . import RP_coco
    table, index = {}, []
    for c in captions:
        index.append(table.setdefault(prefix + c, len(table)))
    img = RP_coco.encode_paths(model, paths, dev, batch_size, num_workers, feed, True, lambda f: f, torch.float16)
    if not paths:
        return img, img.clone()
    txt = RP_coco.embed_texts(model, tokenizer, list(table), dev, batch_size)
    return img, txt[torch.as_tensor(index, dtype=torch.int64, device=dev)].contiguous()


def calculate_clip_score_given_paths(image_dir, captions_file=None, rp_input_file=None, tower=TOWER, weights=None, vocab=None,
                                     prefix=PREFIX, w=W, batch_size=256, seed=0, num_workers=0, feed="ring", save_features=""):
    """The CLI as a function -> dict (clip_score_from_features' keys, ``cos`` being this rank's).  ``weights=None``: seeded
    stand-in parameters (the CLI only allows that behind --synthetic-weights).  Under torchrun every rank returns the totals."""
    tower_kind(tower)
    paths, captions = load_pairs(image_dir, captions_file, rp_input_file)
    if not torch.cuda.is_available():
        raise _lib.TiseLibraryError("clip_score needs an MI355X: there is no CPU path")
    _lib.load()
    from . import RP_coco
    dev = torch.device("cuda", torch.cuda.current_device())
    model, _ = RP_coco.build_towers(weights, dev, tower, seed)
    rank, world, _ = tdist.env_world()
    lo, hi = tdist.shard_range(len(paths), rank, world)
    img, txt = embed_pairs(model, _tokenizer(vocab), paths[lo:hi], captions[lo:hi], dev, batch_size, prefix, num_workers, feed)
    cos = device.paired_cosine(img, txt).cpu().numpy()
    if save_features:
        rows = tdist.all_gather_rows(torch.cat([img.float(), txt.float()], 1))
        if tdist.is_main():
            d = img.shape[1]
            np.savez(save_features, image_features=rows[:, :d].cpu().numpy(), text_features=rows[:, d:].cpu().numpy(),
                     tower=np.array(tower), prefix=np.array(prefix), w=np.float64(w))
    acc = torch.from_numpy(score_sums(cos, w)).to(dev)
    tdist.all_reduce_sum_(acc)                                              # {n, sum, sum of squares} x 2: the only exchange
    res = result_from_sums(acc.cpu().numpy())
    res["cos"] = cos
    return res


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="CLIPScore: w * max(cos(image, caption), 0) over image-caption pairs")
    parser.add_argument("--image_dir", required=True, type=str, help="folder of generated images")
    parser.add_argument("--captions", default=None, type=str, help="JSON object {file name, with or without extension: caption}")
    parser.add_argument("--rp_input_file", default=None, type=str, help="the R-precision pickle: true caption and <caption_id>.png")
    parser.add_argument("--tower", default=TOWER, choices=towers())
    parser.add_argument("--weights", default=None, type=str, help="state_dict of the chosen tower (OpenAI / open_clip native layout)")
    parser.add_argument("--vocab", default=None, type=str, help="bpe_simple_vocab_16e6.txt.gz (required with real weights)")
    parser.add_argument("--prefix", default=PREFIX, type=str, help='in front of every caption (CLIPScore: "A photo depicts "; HPS v2: "")')
    parser.add_argument("--w", default=W, type=float, help="CLIPScore's rescaling (2.5)")
    parser.add_argument("--save-features", default="", type=str, help="write the paired rows (image_features, text_features) to this .npz")
    parser.add_argument("--saved_file", default="", type=str, help="write the result lines here as well")
    parser.add_argument("--batch-size", default=256, type=int)
    parser.add_argument("--synthetic-weights", action="store_true",
                        help="seeded stand-in towers + word-hash tokenizer (plumbing / throughput only; results are tagged)")
    parser.add_argument("--seed", default=0, type=int, help="seed of the stand-in parameters")
    parser.add_argument("--num-workers", default=0, type=int, help="image decode processes (0 = auto)")
    parser.add_argument("--png-feed", default="ring", choices=["ring", "dataloader"])
    parser.add_argument("--gpu_id", default="0", type=str)
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    if not torch.cuda.is_available():
        raise _lib.TiseLibraryError("clip_score needs an MI355X: there is no CPU path")
    rank, world, local_rank = tdist.init_from_env()
    dev = torch.device(f"cuda:{local_rank}" if world > 1 else f"cuda:{args.gpu_id}")
    torch.cuda.set_device(dev)
    wpath, tag = tweights.resolve(args.weights, args.synthetic_weights, tower_kind(args.tower), f"CLIP {args.tower}")
    if wpath is not None and not args.vocab:
        raise RuntimeError("real CLIP weights need the BPE vocabulary: pass --vocab bpe_simple_vocab_16e6.txt.gz")
    res = calculate_clip_score_given_paths(args.image_dir, args.captions, args.rp_input_file, args.tower, wpath, args.vocab, args.prefix,
                                           args.w, args.batch_size, args.seed, args.num_workers, args.png_feed, args.save_features)
    tdist.write_lines(result_lines(res, args.tower, tag), args.saved_file)
    return res


if __name__ == "__main__":
    tdist.run_cli(main)
