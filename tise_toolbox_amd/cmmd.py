#!/usr/bin/env python3
"""CLIP-space realism metrics on MI355X: CMMD and CLIP-FID on the ViT-B/32 or the ViT-L/14@336 image tower.

The reference toolbox measures realism in Inception pool3 space only.  The two metrics current text-to-image work reports beside
FID live on CLIP image embeddings:

CMMD (Jayasumana et al., CVPR 2024, "Rethinking FID: Towards a Better Evaluation Metric for Image Generation"): the squared
maximum mean discrepancy of the two sets of L2-NORMALISED embeddings under the Gaussian kernel

    k(a, b) = exp(-|a - b|^2 / (2 sigma^2)),   sigma = 10   (GAMMA = 1 / 200),   reported x 1000 (SCALE).

With Sxx, Syy the kernel sums over i != j and Sxy the sum over all pairs (``device.GaussianMMD``, csrc/mmd.hip: fp64 matrix
cores, fp64 exp, fixed summation order, no n x n matrix),

    V-statistic (default):   SCALE ((Sxx + n) / n^2 + (Syy + m) / m^2 - 2 Sxy / (n m))
    unbiased (--unbiased):   SCALE (Sxx / (n (n - 1)) + Syy / (m (m - 1)) - 2 Sxy / (n m))

The default is what the PUBLISHED IMPLEMENTATION computes -- the mean of each full kernel matrix, diagonal included, every
diagonal entry taken as exactly 1 (k(a, a)) -- so that figures compare with it; the paper's formula is the unbiased one.  Every
term lies between 0.98 and 1 and the result is of order 1e-5 .. 1e-2: the published code evaluates it in fp32, here the sums
are fp64 and two runs give the same bits.

CLIP-FID (Kynkaanniemi et al. 2022, "The Role of ImageNet Classes in Frechet Inception Distance"; clean-fid's
``clip_vit_b_32`` mode): the Frechet distance of the UN-normalised embeddings -- ``device.StatsAccumulator(dims)`` and
``engine.frechet_solver(dims)``, the FID machinery at another width (512 or 768).  ``--clip-fid`` works at either tower and its
result line names the tower; ONLY the ViT-B/32 one is clean-fid's definition.

THE TOWER.  ``--tower`` chooses it and the result lines, the feature files' network tag and the default parameter file follow:

    ViT-B/32 (default)   224 px, 50 tokens, 512-d   tag clip-vit-b32       ~/.cache/clip/ViT-B-32.pt
    ViT-L/14@336         336 px, 577 tokens, 768-d  tag clip-vit-l14-336   ~/.cache/clip/ViT-L-14-336px.pt

Both run on clip_hip.HipTowers.encode_image (csrc/clip_ops.hip).  ViT-L/14@336 is the tower of the published CMMD figures
(Jayasumana et al. 2024): its 577-token sequences run on tise_attention_long_f16 (streamed keys, online softmax) and its patch
size 14 on tise_patchify_pad_f16 (588 columns padded to 640).  With the real ViT-L/14@336 parameters a CMMD from here is the
metric the paper defines -- same tower, same kernel, same bandwidth, same V-statistic -- and so COMPARABLE with published
figures up to what still differs: the preprocessing below (clip._transform at 336, not the CMMD loader's crop-then-resize),
the fp16 tower (the published code runs its tower in fp32), and that PARITY of these towers with the real `clip` package is
UNPINNED: there are no parameter files here, so the towers are tested against this project's own fp32 module on seeded
parameters only.  A ViT-B/32 CMMD compares with other ViT-B/32 figures only.  A feature file of one tower is refused under
the other.

PREPROCESSING is clip._transform as clip_model restates it: convert to RGB, bicubic resize of the short side to the tower's
resolution (224 or 336), centre crop.  CMMD's own loader crops the centre square BEFORE the resize; the two are identical for
square images and differ by a rounding of the crop window otherwise.

Every image of a directory is used (no drop-last).  The run, the feature files and the shared options are feature_space.py's;
this module holds the CMMD arithmetic, the towers' table and the description of their space (``space``).
"""
import argparse

import torch

from . import device, dist as tdist, feature_space as fs

SIGMA = 10.0
GAMMA = 1 / (2 * SIGMA ** 2)
SCALE = 1000.0
DIMS = 512
NETWORK = "clip-vit-b32"             # the tag of a feature file (fid_score.check_stats_network)
TOWER = "ViT-B/32"                   # the default tower; DIMS and NETWORK above are its width and tag

# per tower of clip_model.CONFIGS: (network tag of its feature files, weights._KINDS entry of its default parameter file)
_TOWERS = {"ViT-B/32": (NETWORK, "clip"), "ViT-L/14@336": ("clip-vit-l14-336", "clip-l14-336")}


def tower_info(tower=TOWER):
    """-> (feature width, network tag, weights kind | None) of a tower of clip_model.CONFIGS.  A configuration registered at
    run time gets a tag spelt from its name and no default parameter file."""
    from . import clip_model
    dims = clip_model.get_config(tower)["embed_dim"]
    if tower in _TOWERS:
        return (dims,) + _TOWERS[tower]
    return dims, "clip-" + "".join(c if c.isalnum() else "-" for c in tower.lower()).strip("-"), None


def cmmd_from_sums(sums, n, m, unbiased=False):
    """(Sxx, Syy, Sxy) of n and m rows -> CMMD x 1000 as a Python float (the module docstring's two estimators).  Host only."""
    n, m = int(n), int(m)
    need = 2 if unbiased else 1
    if n < need or m < need:
        raise ValueError(f"CMMD needs at least {need} row{'s' if need > 1 else ''} per side (got {n} and {m})")
    sxx, syy, sxy = (float(v) for v in sums)
    if unbiased:
        return SCALE * (sxx / (n * (n - 1)) + syy / (m * (m - 1)) - 2 * sxy / (n * m))
    return SCALE * ((sxx + n) / (n * n) + (syy + m) / (m * m) - 2 * sxy / (n * m))


def normalize_rows(t):
    """Rows of an fp32 tensor divided by their fp32 L2 norms (the published implementation's rule; NOT the fp16 normalisation of
    RP_coco.embed_paths, whose rounding of 1e-3 per element would be of the order of the metric)."""
    if t.dtype != torch.float32:
        raise ValueError("rows are normalised in float32")
    return t / t.norm(dim=-1, keepdim=True)


def cmmd_from_features(f1, f2, unbiased=False, sigma=SIGMA):
    """CMMD x 1000 of two embedding sets (device tensors or numpy arrays, (n, dims), un-normalised) -> Python float.  The rows are
    widened to fp32 and normalised in fp32 on the device; ONE grouped launch of one group."""
    if fs.width(f1) != fs.width(f2):
        raise ValueError(f"feature widths differ: {fs.width(f1)} and {fs.width(f2)}")
    if not sigma > 0:
        raise ValueError(f"sigma must be positive (got {sigma})")
    from .engine import require_gpu
    require_gpu()
    dev = f1.device if isinstance(f1, torch.Tensor) and f1.is_cuda else torch.device("cuda", torch.cuda.current_device())
    x, y = normalize_rows(fs.rows_f32(f1, dev)), normalize_rows(fs.rows_f32(f2, dev))
    n, m = x.shape[0], y.shape[0]
    cmmd_from_sums((0.0, 0.0, 0.0), n, m, unbiased)                        # too few rows: say so before the launch
    s = device.GaussianMMD(dev, 1 / (2 * float(sigma) ** 2)).sums(x, y, [0, n], [0, m]).cpu().numpy()
    return cmmd_from_sums(s[0], n, m, unbiased)


@torch.no_grad()
def embed_image_dir(towers, path, dev, batch, workers=0, feed="ring"):
    """Un-normalised fp32 (n, towers.out_dim) embeddings of EVERY image under ``path``, in img_data.get_filenames' walk order, on every
    rank.  The loop is RP_coco.embed_paths' (feeds.CLIP: the PNG ring + clip_model.preprocess_device, the DataLoader for a
    ragged directory); the fp16 rows of the tower are widened, not normalised."""
    from . import RP_coco
    return fs.embed_image_dir(lambda files: RP_coco.encode_paths(towers, files, dev, batch, workers, feed, True, lambda f: f.float(),
                                                                 torch.float32), path)


def space(tower=TOWER, weights=None, seed=0):
    """The space of one CLIP image tower (an unknown ``tower`` is refused here).  ``weights=None``: seeded stand-in parameters of
    ``seed`` (RP_coco.build_towers)."""
    dims, network, _ = tower_info(tower)

    def build_tower(dev):
        from . import RP_coco
        return RP_coco.build_towers(weights, dev, tower, seed)[0]
    return fs.Space("cmmd", network, dims, build_tower, embed_image_dir)


clip_statistics = fs.statistics


def save_features_npz(path, feats, mu, sigma, tower=TOWER):
    """The feature file of --save-features: ``features`` (fp32, un-normalised, walk order), ``mu``, ``sigma`` and the network tag
    of ``tower``."""
    fs.save_features_npz(path, feats, mu, sigma, tower_info(tower)[1])


def load_features_npz(path, tower=TOWER):
    dims, network, _ = tower_info(tower)
    return fs.load_features_npz(path, network, dims, "cmmd")


def _given_paths(paths, batch_size, weights, seed, num_workers, feed, unbiased, clip_fid, save_features, want_cmmd=True,
                 tower=TOWER):
    """-> (CMMD | None, CLIP-FID | None).  Without ``clip_fid`` and ``save_features`` no statistics kernel runs."""
    res = fs.given_paths(space(tower, weights, seed), paths, batch_size, num_workers, feed, save_features,
                         want=["cmmd"] * bool(want_cmmd) + ["fd"] * bool(clip_fid), unbiased=unbiased)
    return res.get("cmmd"), res.get("fd")


def calculate_cmmd_given_paths(paths, batch_size=50, weights=None, seed=0, num_workers=0, feed="ring", unbiased=False,
                               save_features="", tower=TOWER):
    """CMMD x 1000 (on ``tower``: ViT-B/32 or ViT-L/14@336) of two paths -- directories or feature files -> Python float.  ``weights=None``: seeded stand-in
    parameters (the CLI only allows that behind --synthetic-weights).  ``save_features``: the FIRST path's rows (the reference
    set: embedded once, compared with many generated sets) are written there with their mu and sigma."""
    return _given_paths(paths, batch_size, weights, seed, num_workers, feed, unbiased, False, save_features, tower=tower)[0]


def calculate_clip_fid_given_paths(paths, batch_size=50, weights=None, seed=0, num_workers=0, feed="ring", save_features="",
                                   tower=TOWER):
    """CLIP-FID (on ``tower``; only the ViT-B/32 one is clean-fid's clip_vit_b_32 definition) of two paths -> Python float: the
    Frechet distance of the un-normalised embeddings' (mu, sigma) from device.StatsAccumulator(dims) and
    engine.frechet_solver(dims)."""
    return _given_paths(paths, batch_size, weights, seed, num_workers, feed, False, True, save_features, want_cmmd=False,
                        tower=tower)[1]


def parse_args(argv=None):
    from . import clip_model
    parser = argparse.ArgumentParser(description="CMMD and CLIP-FID on a CLIP image tower (ViT-B/32, or the paper's ViT-L/14@336)")
    parser.add_argument("--tower", default=TOWER, choices=list(clip_model.CONFIGS),
                        help="ViT-B/32 (default; clean-fid's CLIP-FID tower) or ViT-L/14@336 (the tower of the published CMMD figures)")
    fs.add_arguments(parser, "paths batch weights", weights_help="OpenAI CLIP state_dict (.pt) of the chosen tower; default: "
                     "~/.cache/clip/ViT-B-32.pt or ViT-L-14-336px.pt")
    parser.add_argument("--clip-fid", action="store_true", help="also report the Frechet distance of the un-normalised embeddings")
    parser.add_argument("--unbiased", action="store_true",
                        help="the paper's unbiased estimator instead of the published implementation's V-statistic")
    fs.add_arguments(parser, "output", rows="embeddings (fp32, un-normalised)")
    return parser.parse_args(argv)                             # --weights with --synthetic-weights: weights.resolve refuses it


def main(argv=None):
    args = parse_args(argv)
    _, network, kind = tower_info(args.tower)
    wpath, tag = fs.start_cli(args, "cmmd", network, kind, f"CLIP {args.tower}")
    value, fid = _given_paths([args.path1, args.path2], args.batch_size, wpath, args.seed, args.num_workers, args.png_feed,
                              args.unbiased, args.clip_fid, args.save_features, tower=args.tower)
    lines = [f"CMMD ({args.tower}): {value}{tag}"]
    if args.clip_fid:
        lines.append(f"CLIP-FID ({args.tower}): {fid}{tag}")
    tdist.write_lines(lines, args.saved_file)
    return value, fid


if __name__ == "__main__":
    tdist.run_cli(main)

