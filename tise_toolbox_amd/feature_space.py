"""The runner of the feature-space metrics: embed two image sets with a tower, then compare the rows.

cmmd.py (CLIP), fd_dinov2.py (DINOv2) and fd_swav.py (SwAV ResNet-50) each describe their ``Space`` and keep what is theirs -- the
tower's table, the metric's arithmetic, their own options -- and everything else is here, once: the (rows, dims) check and the
widening of rows, np.mean / np.cov on the device, the feature files with their network tag, the two sides of a run (a directory or
a file of --save-features), the run itself, the shared options and the result lines.

A run (``given_paths``) goes: existence checks; the refusals that need no GPU (a feature file of another network); the GPU and the
library; side one; --save-features (rank 0); side two; then only the numbers that were asked for, each a call into its own module
(cmmd, fid_score, kid, prdc, authenticity, vendi, fd_infinity).  A tower is built when the first directory needs it: two feature
files need none.

Every image of a directory is used.  Under torchrun the files are sharded as contiguous index ranges and the rows gathered in walk
order on every rank (``embed_image_dir``: dist.all_gather_rows, as the --kid path); every rank evaluates the numbers itself on the
same rows and rank 0 prints and writes.
"""
import os
from collections import namedtuple

import numpy as np
import torch

from . import _lib, device, dist as tdist

# tool: the CLI's name in messages; network: the tag of its feature files; dims: the feature width; build_tower(dev) -> tower;
# embed_dir(tower, path, dev, batch, workers, feed) -> fp32 device rows of every image under ``path``, the same on every rank
Space = namedtuple("Space", "tool network dims build_tower embed_dir")

NEAREST_TRAIN_COLUMNS = ("gen_row", "train_row", "d2", "authentic", "gen_file", "train_file")


# ---- rows and feature files ----------------------------------------------------------------------------------------------------
def width(f):
    """The width of (rows, dims) features, from the shape alone: what a caller checks before it asks for a GPU."""
    shape = tuple(np.shape(f))
    if len(shape) != 2:
        raise ValueError("features must be (rows, dims)")
    return shape[1]


def rows_f32(f, dev):
    """(rows, dims) features, a tensor or a numpy array -> an fp32 tensor on ``dev``."""
    width(f)
    if isinstance(f, torch.Tensor):
        return f.to(dev, torch.float32)
    return torch.as_tensor(np.ascontiguousarray(f, dtype=np.float32), device=dev)


def statistics(feats):
    """(mu, sigma) of fp32 device rows -> fp64 numpy arrays: np.mean / np.cov (ddof 1) on the device."""
    stats = device.StatsAccumulator(feats.shape[1], feats.device)
    stats.update(feats)
    mu, sigma = stats.finalize()
    out = mu.cpu().numpy(), sigma.cpu().numpy()
    stats.close()
    return out


def frechet_from_features(f1, f2):
    """The Frechet distance of two feature sets (device tensors or numpy arrays, (n, dims)) -> Python float."""
    from . import fid_score
    from .engine import require_gpu
    if width(f1) != width(f2):
        raise ValueError(f"feature widths differ: {width(f1)} and {width(f2)}")
    require_gpu()
    dev = f1.device if isinstance(f1, torch.Tensor) and f1.is_cuda else torch.device("cuda", torch.cuda.current_device())
    (m1, s1), (m2, s2) = statistics(rows_f32(f1, dev)), statistics(rows_f32(f2, dev))
    return float(fid_score.calculate_frechet_distance(m1, s1, m2, s2))


def check_feature_file(path, network, tool):
    """The refusal of load_features_npz on the file's network tag alone (no rows are read, no GPU is needed)."""
    from . import fid_score
    with np.load(path, allow_pickle=True) as f:
        if "network" not in f.files:
            raise RuntimeError(f"{path}: no network tag: not a feature file of {network} (make one with {tool} --save-features)")
        fid_score.check_stats_network(path, str(f["network"]), network)


def load_features_npz(path, network, dims, tool):
    """-> (features fp32 (n, dims), mu, sigma) of a file ``tool`` --save-features wrote on the SAME network.  A file of another
    network (or of none: an Inception {mu, sigma} file), one without the rows and one of another width are refused."""
    check_feature_file(path, network, tool)
    with np.load(path, allow_pickle=True) as f:
        if "features" not in f.files:
            raise RuntimeError(f"{path}: no 'features' array in this file; make it with {tool} --save-features")
        feats = np.ascontiguousarray(f["features"], dtype=np.float32)
        if feats.ndim != 2 or feats.shape[1] != dims:
            raise RuntimeError(f"{path}: features of shape {feats.shape}, expected (n, {dims})")
        return feats, f["mu"][:], f["sigma"][:]


def save_features_npz(path, feats, mu, sigma, network):
    """The feature file of --save-features: ``features`` (fp32, walk order), ``mu``, ``sigma`` and the network tag."""
    from . import fid_score
    fid_score.save_stats_npz(path, mu, sigma, network, feats)


# ---- the image loop ------------------------------------------------------------------------------------------------------------
def embed_image_dir(encode, path):
    """``encode(files)`` -> device rows, on this rank's contiguous share of the files under ``path`` (img_data.get_filenames' walk
    order) -> the rows of EVERY image, in that order, on every rank."""
    from . import img_data
    files = img_data.get_filenames(path)
    rank, world, _ = tdist.env_world()
    lo, hi = tdist.shard_range(len(files), rank, world)
    return tdist.all_gather_rows(encode(files[lo:hi]))


# ---- the two sides and the run -------------------------------------------------------------------------------------------------
def side(space, path, tower, dev, batch_size, num_workers, feed, want_stats=True):
    """-> (fp32 device rows, mu, sigma) of a directory or a feature file.  ``tower()`` is called for a directory only; without
    ``want_stats`` a directory's mu and sigma are None and no statistics kernel runs."""
    if path.endswith(".npz"):
        feats, mu, sigma = load_features_npz(path, space.network, space.dims, space.tool)
        return torch.as_tensor(feats, device=dev), mu, sigma
    feats = space.embed_dir(tower(), path, dev, batch_size, num_workers, feed)
    if feats.shape[0] == 0:
        raise RuntimeError(f"no images under {path}")
    mu, sigma = statistics(feats) if want_stats else (None, None)
    return feats, mu, sigma


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


def given_paths(space, paths, batch_size=50, num_workers=0, feed="ring", save_features="", train=None, want=("fd",), prdc_k=5,
                nearest_train="", fd_infinity_seed=0, unbiased=False):
    """The numbers ``want`` names, of two paths (each a directory or a feature file of ``space``) -> dict with those keys only:
    ``cmmd`` (float; ``unbiased``), ``fd`` (float), ``kd`` ((mean, std)), ``prdc`` (OrderedDict; ``prdc_k``), ``authpct`` (float; needs
    ``train``, the training set's directory or feature file), ``vendi`` (with ``vendi_reference``: the second and the first path's),
    ``fd_infinity`` (the dict of fd_infinity_from_features; ``fd_infinity_seed``).  ``save_features``: the FIRST path's rows (the
    reference set: embedded once, compared with many generated sets) are written there with their mu, sigma and the network tag.
    ``nearest_train``: a CSV path, every generated row's nearest training row (needs ``train`` too).  Rank 0 writes both."""
    from . import fid_score
    want = set(want)
    if ("authpct" in want or nearest_train) and not train:
        raise ValueError("authpct / nearest_train need the training set: train=PATH (a directory or a feature file)")
    every = list(paths) + ([train] if train else [])
    for p in every:
        if not os.path.exists(p):
            raise RuntimeError("Invalid path: %s" % p)
    for p in every:                                                        # refusals that need no GPU come first
        if p.endswith(".npz"):
            check_feature_file(p, space.network, space.tool)
    if not torch.cuda.is_available():
        raise _lib.TiseLibraryError(f"{space.tool} needs an MI355X: there is no CPU path")
    _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    built = []

    def tower():                                                           # two feature files need no tower at all
        if not built:
            built.append(space.build_tower(dev))
        return built[0]
    feed_args = (dev, batch_size, num_workers, feed)
    f1, m1, s1 = side(space, paths[0], tower, *feed_args, "fd" in want or bool(save_features))
    if save_features and tdist.is_main():
        save_features_npz(save_features, f1, m1, s1, space.network)
    f2, m2, s2 = side(space, paths[1], tower, *feed_args, "fd" in want)
    out = {}
    if "cmmd" in want:
        from . import cmmd
        out["cmmd"] = cmmd.cmmd_from_features(f1, f2, unbiased)
    if "fd" in want:
        out["fd"] = float(fid_score.calculate_frechet_distance(m1, s1, m2, s2))
    if "kd" in want:
        from . import kid
        out["kd"] = kid.kid_from_features(f1, f2, subsets=100, subset_size=1000)
    if "prdc" in want:
        from . import prdc
        out["prdc"] = prdc.prdc_from_features(f1, f2, nearest_k=int(prdc_k))
    # every rank holds the same rows in the same order and evaluates these itself, as the k-NN metrics above
    if "authpct" in want or nearest_train:
        from . import authenticity
        near = authenticity.nearest_train(side(space, train, tower, *feed_args, False)[0], f2)
        if "authpct" in want:
            out["authpct"] = authenticity.authpct_from_counts(near["authentic"].sum(), len(near["authentic"]))
        if nearest_train and tdist.is_main():
            write_nearest_train_csv(nearest_train, near, paths[1], train)
    if "vendi" in want:
        from . import vendi
        out["vendi"], out["vendi_reference"] = vendi.vendi_from_features(f2), vendi.vendi_from_features(f1)
    if "fd_infinity" in want:
        from . import fd_infinity
        out["fd_infinity"] = fd_infinity.fd_infinity_from_features(f1, f2, seed=int(fd_infinity_seed))
    return out


def fd_result(res):
    """given_paths' dict in the shape the FD CLIs return: ``fd``, ``kd`` and ``prdc`` always (None when not asked for), then the rest."""
    return {"fd": res["fd"], "kd": res.get("kd"), "prdc": res.get("prdc"), **{k: v for k, v in res.items() if k not in ("fd", "kd", "prdc")}}


def result_lines(res, label, tag=""):
    """The FD / KD / PRDC / AuthPct / Vendi / FD-infinity lines of the numbers ``res`` holds.  ``label``: "SwAV", "DINOv2 (vitl14)"."""
    name, _, arch = label.partition(" ")                                   # the reference's Vendi line puts its word between the two
    lines = [f"FD-{label}: {res['fd']}{tag}"]
    if res.get("kd") is not None:
        lines.append(f"KD-{label}: {res['kd'][0]} +- {res['kd'][1]}{tag}")
    if res.get("prdc") is not None:
        lines += [f"{n.capitalize()}-{label}: {res['prdc'][n]}{tag}" for n in ("precision", "recall", "density", "coverage")]
    if "authpct" in res:
        lines.append(f"AuthPct-{label}: {res['authpct']}{tag}")
    if "vendi" in res:
        lines += [f"Vendi-{label}: {res['vendi']}{tag}", f"Vendi-{name} reference{' ' + arch if arch else ''}: {res['vendi_reference']}{tag}"]
    if "fd_infinity" in res:
        lines.append(f"FD-infinity-{label}: {res['fd_infinity']['fd_infinity']}{tag}")
    return lines


# ---- the CLI scaffold ----------------------------------------------------------------------------------------------------------
def add_arguments(parser, groups, weights_help=None, rows="feature rows (fp32)", space="", gpu="--gpu"):
    """The options the three CLIs share, group by group in the order of ``groups`` (a CLI adds its own between two calls):
    ``paths``, ``kd`` (with --prdc and --prdc-k; ``space`` names it in the help), ``weights`` (with --synthetic-weights and
    --seed), ``batch``, ``output`` (--save-features, --saved_file, the feed's two and ``gpu``)."""
    add = parser.add_argument
    for group in groups.split():
        if group == "paths":
            add("--path1", type=str, required=True, help="reference images: a directory, or a feature file of --save-features")
            add("--path2", type=str, required=True, help="generated images: a directory, or a feature file of --save-features")
        elif group == "kd":
            add("--kd", action="store_true", help=f"also report the kernel distance (KID's estimator in {space} space)")
            add("--prdc", action="store_true", help=f"also report precision, recall, density and coverage in {space} space")
            add("--prdc-k", type=int, default=5, help="nearest neighbours of --prdc (default 5)")
        elif group == "weights":
            add("--weights", default=None, type=str, help=weights_help)
            add("--synthetic-weights", action="store_true", help="seeded stand-in tower (plumbing / throughput only; results are tagged)")
            add("--seed", default=0, type=int, help="seed of the stand-in parameters")
        elif group == "batch":
            add("--batch-size", type=int, default=50)
        elif group == "output":
            add("--save-features", default="", type=str, help=f"write --path1's {rows}, mu, sigma and the network tag to this .npz")
            add("--saved_file", default="", type=str, help="write the result lines here as well")
            add("--png-feed", default="ring", choices=["ring", "dataloader"])
            add("--num-workers", default=0, type=int, help="image decode processes (0 = auto)")
            add(gpu, default="0", type=str, help="GPU to use")
        else:
            raise ValueError(f"unknown option group {group!r}")


def parse_fd_args(parser, argv):
    """parse_args of an FD CLI, with the refusals of the ``weights`` and ``kd`` groups."""
    args = parser.parse_args(argv)
    if args.weights and args.synthetic_weights:
        parser.error("--synthetic-weights and --weights are mutually exclusive")
    if args.prdc and not 1 <= args.prdc_k <= 16:
        parser.error("--prdc-k must lie in 1 .. 16")
    return args


def start_cli(args, tool, network, kind, what=None, gpu="gpu"):
    """What a CLI does between its parser and its run -> (parameter file | None, result tag): a feature file of another network is
    refused before the GPU is asked for, then the device (paired.cli_device), then weights.resolve."""
    from . import paired, weights
    for p in (args.path1, args.path2, getattr(args, "train", "")):
        if p.endswith(".npz") and os.path.exists(p):
            check_feature_file(p, network, tool)
    paired.cli_device(args, tool, gpu)
    return weights.resolve(args.weights, args.synthetic_weights, kind, what)
