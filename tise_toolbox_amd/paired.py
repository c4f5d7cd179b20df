#!/usr/bin/env python3
"""PSNR, SSIM and MS-SSIM of image PAIRS on MI355X: image i of one directory against image i of another -- what autoencoder,
tokenizer, super-resolution, inpainting and editing papers print beside rFID (rFID itself is plain ``fid_score`` on originals and
reconstructions) -- and MS-SSIM over random pairs of ONE directory, the diversity number of Odena et al. 2017.

    python -m tise_toolbox_amd.paired --path1 ORIG --path2 RECON [--ms-ssim] [--self-pairs N --seed S]
        [--per-pair OUT.csv] [--saved_file OUT.txt] [--batch-size 50] [--png-feed ring|dataloader] [--jpeg-feed native|pillow]
        [--num-workers 0] [--gpu_id 0]

DEFINITIONS (restated from the papers; no metric package and nothing of the reference toolbox is their source).  Images are 8-bit
RGB as the feeds decode them, values 0..255, L = 255.  Every quantity is computed per channel on R, G and B separately and then
averaged over the three channels.  Both images of a pair have one height and width; different pairs may differ in size.

  PSNR      SSE = sum (x - y)^2 over all H W 3 bytes, an exact integer; MSE = SSE / (3 H W); PSNR = 10 log10(255^2 / MSE) in
            fp64.  An identical pair gives inf.
  SSIM      Wang, Bovik, Sheikh & Simoncelli 2004, the form tf.image.ssim, pytorch-msssim and torchmetrics compute by default.
            Window g[i] ~ exp(-(i - 5)^2 / (2 1.5^2)), i = 0..10, normalised to sum 1 in fp64, applied as the outer product
            g g^T at the "valid" positions only: the maps are (H - 10) x (W - 10), nothing is padded.  mu_x, mu_y, E[x^2],
            E[y^2], E[xy] come from the window; s_x^2 = E[x^2] - mu_x^2, s_y^2 = E[y^2] - mu_y^2, s_xy = E[xy] - mu_x mu_y (the
            biased, weighted forms); C1 = (0.01 255)^2, C2 = (0.03 255)^2; cs = (2 s_xy + C2) / (s_x^2 + s_y^2 + C2),
            l = (2 mu_x mu_y + C1) / (mu_x^2 + mu_y^2 + C1), ssim = l cs.  SSIM of a pair: the mean of the ssim map over the
            valid positions, then the mean over the three channels.  An image with H < 11 or W < 11 is refused.
  MS-SSIM   Wang, Simoncelli & Bovik 2003: five scales, weights (0.0448, 0.2856, 0.3001, 0.2363, 0.1333); m_s = the mean of the
            cs map at scales 1..4 and of the ssim map at scale 5; per channel MS-SSIM = prod_s max(m_s, 0)^w_s (the clamp is
            pytorch-msssim's default), then the mean over the channels.  Between scales a 2 x 2 mean with stride 2; a last odd
            row or column is DROPPED (floor) -- this project's choice, packages differ (UNPINNED in README); for sizes divisible
            by 16 there is nothing to choose.  Level s holds multiples of 4^-s that are <= 255: exact in fp32, stored as fp32.
            The smaller side must be >= 176 (176 -> 88 -> 44 -> 22 -> 11); a smaller image is refused.

WHAT RUNS WHERE.  Side one goes through ``feeds.run`` on its file list (site PAIRED: every image used; the native JPEG feed, the
PNG ring or the DataLoader, as for IS*), side two -- decoded in step with it -- through ``feeds.u8_dataloader`` on ITS file list:
two concurrent ``feeds.run`` sessions would need the ragged-directory retry of one to restart the other, which ``feeds`` does not
do.  The two streams are re-chunked into batches of ``--batch-size`` pairs.  Per batch: ``device.pair_sse_u8`` (exact integers),
``device.ssim_pairs`` on the bytes and, under --ms-ssim, four ``device.pool2x2_pairs`` and four more ``device.ssim_pairs`` launches
on the fp32 levels (csrc/ssim.hip: fp64 in a fixed order, the same bits on every run, one launch for a ragged batch, no CPU
path).  log10, the five weighted powers and the channel mean run on the host in fp64, as do mean and population standard
deviation over the pairs, formed from ``{n, sum, sum of squares}`` per metric.  Under torchrun the PAIRS are sharded, one
all-reduce of those sums is the only exchange (--per-pair gathers its rows besides), rank 0 writes.  Identical pairs (PSNR = inf)
are counted and reported; they make the PSNR mean inf and its std nan, as numpy would.
"""
import argparse
import os

import numpy as np
import torch

from . import _lib, dist as tdist, feeds

IMAGE_EXTENSIONS = (".png", ".jpg", ".jpeg")
MS_WEIGHTS = np.array([0.0448, 0.2856, 0.3001, 0.2363, 0.1333], dtype=np.float64)
MS_MIN_SIDE = 176
SSIM_MIN_SIDE = 11
METRICS = ("psnr", "ssim", "ms_ssim")


# ---- host logic ------------------------------------------------------------------------------------------------------
def _stems(path):
    """{relative path without extension: file} of the image files under ``path``; two files of one stem are refused."""
    if not os.path.isdir(path):
        raise RuntimeError("Invalid path: %s" % path)
    out = {}
    for root, _, names in os.walk(path):
        for name in names:
            if name.lower().endswith(IMAGE_EXTENSIONS):
                full = os.path.join(root, name)
                stem = os.path.splitext(os.path.relpath(full, path))[0]
                if stem in out:
                    raise RuntimeError(f"{path} holds two images named {stem!r}: {os.path.relpath(out[stem], path)} and "
                                       f"{os.path.relpath(full, path)}")
                out[stem] = full
    return out


def pair_files(path1, path2):
    """Two directories -> ([file of side one], [file of side two]) paired by relative path WITHOUT extension (a/b.png pairs with
    a/b.jpg), in the order of the sorted stems.  A file present on one side only is refused, naming it."""
    a, b = _stems(path1), _stems(path2)
    for stem in sorted(a):
        if stem not in b:
            raise RuntimeError(f"missing image: {os.path.relpath(a[stem], path1)} of {path1} has no partner in {path2}")
    for stem in sorted(b):
        if stem not in a:
            raise RuntimeError(f"missing image: {os.path.relpath(b[stem], path2)} of {path2} has no partner in {path1}")
    if not a:
        raise RuntimeError(f"no image files in {path1}")
    order = sorted(a)
    return [a[s] for s in order], [b[s] for s in order]


def list_files(path):
    """The image files under ``path``, sorted by relative path without extension (pair_files' order)."""
    st = _stems(path)
    return [st[s] for s in sorted(st)]


def draw_self_pairs(n_files, n_pairs, seed=0):
    """``n_pairs`` index pairs (i, j), i != j, uniform over the ordered pairs of ``n_files`` files, from
    np.random.default_rng(seed): i uniform, j uniform over the other n_files - 1.  -> (n_pairs, 2) int64."""
    n_files, n_pairs = int(n_files), int(n_pairs)
    if n_files < 2:
        raise RuntimeError(f"--self-pairs needs at least two images (got {n_files})")
    if n_pairs < 1:
        raise RuntimeError(f"--self-pairs needs a positive number of pairs (got {n_pairs})")
    rng = np.random.default_rng(seed)
    i = rng.integers(0, n_files, size=n_pairs)
    j = rng.integers(0, n_files - 1, size=n_pairs)
    j = j + (j >= i)
    return np.stack([i, j], axis=1).astype(np.int64)


def psnr_from_sse(sse, h, w):
    """Exact integer SSEs of (h, w, 3) pairs -> fp64 PSNR, inf where the SSE is 0."""
    sse = np.asarray(sse, dtype=np.float64)
    n = 3.0 * np.asarray(h, dtype=np.float64) * np.asarray(w, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(255.0 ** 2 / (sse / n))


def ms_from_scale_means(m):
    """(n, 5, 3) fp64 scale means (cs at scales 1..4, ssim at scale 5) -> (n,) MS-SSIM: prod_s max(m_s, 0)^w_s per channel, then
    the channel mean."""
    m = np.maximum(np.asarray(m, dtype=np.float64), 0.0)
    return np.prod(m ** MS_WEIGHTS[None, :, None], axis=1).mean(axis=1)


def metric_sums(res):
    """Per-pair arrays of a shard (psnr, ssim, maybe ms_ssim) -> (10,) float64: [n, sum, sum of squares] per metric of METRICS
    (zeros for an absent one) and the number of identical pairs (PSNR = inf).  Additive over shards, an empty one included."""
    out = np.zeros(10, dtype=np.float64)
    for k, name in enumerate(METRICS):
        v = np.asarray(res.get(name, ()), dtype=np.float64).reshape(-1)
        out[3 * k:3 * k + 3] = (v.size, v.sum(), (v * v).sum())
    out[9] = np.isposinf(np.asarray(res.get("psnr", ()), dtype=np.float64)).sum()
    return out


def result_from_sums(sums):
    """metric_sums' (10,) totals -> dict: <metric> (mean) and <metric>_std (population std) for every metric with pairs, n,
    identical.  An inf among the PSNRs makes their mean inf and their std nan, as numpy's mean and std do."""
    sums = np.asarray(sums, dtype=np.float64)
    if int(sums[0]) < 1:
        raise RuntimeError("the paired metrics need at least one pair")
    res = {"n": int(sums[0]), "identical": int(sums[9])}
    for k, name in enumerate(METRICS):
        n, s, ss = sums[3 * k:3 * k + 3]
        if n > 0:
            res[name], res[name + "_std"] = mean_std_from_sums(n, s, ss)
    return res


def result_lines(res):
    lines = [f"PSNR: {res['psnr']} +- {res['psnr_std']}", f"SSIM: {res['ssim']} +- {res['ssim_std']}"]
    if "ms_ssim" in res:
        lines.append(f"MS-SSIM: {res['ms_ssim']} +- {res['ms_ssim_std']}")
    if res["identical"] > 0:
        lines.append(f"identical pairs: {res['identical']}")
    return lines


def per_pair_csv(files1, files2, res):
    """The --per-pair text: the header and one line per pair; the last field is empty without MS-SSIM."""
    rows = ["pair,file1,file2,h,w,psnr,ssim,ms_ssim"]
    ms = res.get("ms_ssim")
    for i, (f1, f2) in enumerate(zip(files1, files2)):
        rows.append(f"{i},{f1},{f2},{int(res['h'][i])},{int(res['w'][i])},{float(res['psnr'][i])!r},{float(res['ssim'][i])!r},"
                    + (repr(float(ms[i])) if ms is not None else ""))
    return "\n".join(rows) + "\n"


# ---- device ----------------------------------------------------------------------------------------------------------
def _as_list(t):
    return list(t) if isinstance(t, torch.Tensor) else [(c[0] if c.dim() == 4 and c.shape[0] == 1 else c) for c in t]


def psnr_ssim_from_images(xs, ys, ms_ssim=False):
    """Two (N,H,W,3) uint8 device tensors or two lists of (H_i,W_i,3) uint8 device tensors (pair by pair one size) -> dict of
    per-pair fp64 numpy arrays ``psnr``, ``ssim`` and, with ``ms_ssim``, ``ms_ssim`` and ``ms_scale_means`` (n, 5, 3); besides
    ``sse`` (int64), ``h``, ``w``.  The pyramid is built here: four pool2x2_pairs and five ssim_pairs launches per batch."""
    from . import device
    from .engine import require_gpu
    require_gpu()
    stacked = isinstance(xs, torch.Tensor) and isinstance(ys, torch.Tensor) and xs.dim() == 4 and ys.dim() == 4
    if stacked:                                              # a uniform batch stays one tensor: no per-image work on the host
        if xs.shape != ys.shape:
            raise ValueError(f"two (N,H,W,3) batches of one shape (got {tuple(xs.shape)} and {tuple(ys.shape)})")
        checks = [(xs, ys)] if len(xs) else []
    else:
        xs, ys = _as_list(xs), _as_list(ys)
        if len(xs) != len(ys):
            raise ValueError(f"{len(xs)} images on side one, {len(ys)} on side two")
        checks = list(zip(xs, ys))
    for i, (a, b) in enumerate(checks):
        if a.dtype != torch.uint8 or b.dtype != torch.uint8 or a.dim() != b.dim() or a.shape[-1] != 3 or b.shape[-1] != 3:
            raise ValueError(f"pair {i} must be two (H,W,3) uint8 images")
        if a.shape != b.shape:
            raise ValueError(f"pair {i} has two sizes ({a.shape[0]} x {a.shape[1]} and {b.shape[0]} x {b.shape[1]})")
        ah, aw = a.shape[-3], a.shape[-2]
        if min(ah, aw) < SSIM_MIN_SIDE:
            raise ValueError(f"SSIM needs both sides >= {SSIM_MIN_SIDE}: pair {i} is {ah} x {aw}")
        if ms_ssim and min(ah, aw) < MS_MIN_SIDE:
            raise ValueError(f"MS-SSIM needs the smaller side >= {MS_MIN_SIDE} (five scales, 176 -> 88 -> 44 -> 22 -> 11): "
                             f"pair {i} is {ah} x {aw}")
    if stacked:
        h, w = np.full(len(xs), xs.shape[1], dtype=np.int64), np.full(len(xs), xs.shape[2], dtype=np.int64)
    else:
        h, w = np.array([a.shape[0] for a in xs], dtype=np.int64), np.array([a.shape[1] for a in xs], dtype=np.int64)
    if len(xs) == 0:
        res = {"psnr": np.zeros(0), "ssim": np.zeros(0), "sse": np.zeros(0, dtype=np.int64), "h": h, "w": w}
        if ms_ssim:
            res["ms_ssim"], res["ms_scale_means"] = np.zeros(0), np.zeros((0, 5, 3))
        return res
    sse = device.pair_sse_u8(xs, ys)
    means = [device.ssim_pairs(xs, ys)]
    if ms_ssim:
        lx, ly = xs, ys
        for _ in range(4):
            lx, ly = device.pool2x2_pairs(lx, ly)
            means.append(device.ssim_pairs(lx, ly))
    sse = sse.cpu().numpy()
    means = [m.cpu().numpy() for m in means]
    res = {"psnr": psnr_from_sse(sse, h, w), "ssim": means[0][:, :, 0].mean(axis=1), "sse": sse, "h": h, "w": w}
    if ms_ssim:
        m = np.stack([means[s][:, :, 1] if s < 4 else means[s][:, :, 0] for s in range(5)], axis=1)
        res["ms_scale_means"], res["ms_ssim"] = m, ms_from_scale_means(m)
    return res


def _images(loader, dev):
    """The images of a loader's batches ((B,H,W,3) tensors or lists of (H,W,3)), one by one, on the device.  A device batch of
    the ring or of the JPEG feed lives in a buffer the loader reuses: its images are copied, because the re-chunking keeps some
    of them past the loader's next step."""
    for batch in loader:
        if isinstance(batch, (list, tuple)):
            for img in batch:
                img = img[0] if img.dim() == 4 else img
                yield img.clone() if img.is_cuda else img.to(dev, non_blocking=True)
        else:
            yield from (batch.clone() if batch.is_cuda else batch.to(dev, non_blocking=True)).unbind(0)


def _concat(parts, ms_ssim, per_batch=None):
    if per_batch is not None:
        parts = parts or [per_batch([], [])]
        return {k: np.concatenate([p[k] for p in parts], axis=0) for k in parts[0]}
    keys = ["psnr", "ssim", "sse", "h", "w"] + (["ms_ssim", "ms_scale_means"] if ms_ssim else [])
    if not parts:
        return psnr_ssim_from_images([], [], ms_ssim)
    return {k: np.concatenate([p[k] for p in parts], axis=0) for k in keys}


def paired_from_files(files1, files2, ms_ssim=False, batch_size=50, options=None, device=None, per_batch=None):
    """Per-pair arrays (psnr_ssim_from_images' dict) of files1[i] against files2[i], this process's lists as they are.
    ``per_batch``: a callable (xs, ys) -> dict of per-pair numpy arrays that takes psnr_ssim_from_images' place on every batch
    (two lists of (H,W,3) uint8 device tensors; called with two empty lists for an empty shard) -- lpips.py's use of this loop."""
    from .engine import require_gpu
    require_gpu()
    if len(files1) != len(files2):
        raise ValueError(f"{len(files1)} files on side one, {len(files2)} on side two")
    options = options or feeds.Options()
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    batch_size = max(1, int(batch_size))
    if not files1:
        return _concat([], ms_ssim, per_batch)
    workers = min(feeds.resolve_workers(options.num_workers, tdist.env_world()[1]), len(files2))

    def consume(loader):                                     # runs again from the start when the ring meets a ragged directory
        parts, xs, ys, base = [], [], [], 0
        other = feeds.u8_dataloader(files2, batch_size, workers, False)

        def flush():
            nonlocal xs, ys, base
            for k, (a, b) in enumerate(zip(xs, ys)):
                if a.shape != b.shape:
                    raise RuntimeError(f"pair {base + k}: {files1[base + k]} is {a.shape[0]} x {a.shape[1]}, "
                                       f"{files2[base + k]} is {b.shape[0]} x {b.shape[1]}; both images of a pair must have one size")
            parts.append(psnr_ssim_from_images(xs, ys, ms_ssim) if per_batch is None else per_batch(xs, ys))
            base += len(xs)
            xs, ys = [], []
        for a, b in zip(_images(loader, dev), _images(other, dev)):
            xs.append(a)
            ys.append(b)
            if len(xs) == batch_size:
                flush()
        if xs:
            flush()
        if base != len(files1):
            raise RuntimeError(f"the feeds delivered {base} pairs of {len(files1)}")
        return _concat(parts, ms_ssim, per_batch)
    return feeds.run(feeds.PAIRED, list(files1), options, consume, dev, batch_size,
                     loader_args={"ring": {"batch_size": 1, "group": batch_size}})


# ---- the scaffold of a pair-metric CLI (this one, lpips.py, dists.py) -----------------------------------------------------
def value_sums(values):
    """(3,) float64 {n, sum, sum of squares}: additive over shards, an empty one included."""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    return np.array([v.size, v.sum(), (v * v).sum()], dtype=np.float64)


def mean_std_from_sums(n, s, ss):
    """{n, sum, sum of squares}, n > 0 -> (mean, population standard deviation); an inf among the values makes the mean inf and the
    std nan, as numpy's mean and std do."""
    mean = s / n
    with np.errstate(invalid="ignore"):
        var = max(ss / n - mean * mean, 0.0) if np.isfinite(mean) else float("nan")
    return float(mean), float(np.sqrt(var))


def value_result(sums, name, what):
    """value_sums' totals of a one-number metric -> {n, <name>, <name>_std}."""
    sums = np.asarray(sums, dtype=np.float64)
    if int(sums[0]) < 1:
        raise RuntimeError(f"{what} needs at least one pair")
    mean, std = mean_std_from_sums(*sums)
    return {"n": int(sums[0]), name: mean, name + "_std": std}


def value_csv(name, files1, files2, per):
    """The --per-pair text of a one-number metric: the header and one line per pair."""
    rows = [f"pair,file1,file2,h,w,{name}"]
    for i, (f1, f2) in enumerate(zip(files1, files2)):
        rows.append(f"{i},{f1},{f2},{int(per['h'][i])},{int(per['w'][i])},{float(per[name][i])!r}")
    return "\n".join(rows) + "\n"


def value_per_batch(name, fn):
    """paired_from_files' per-batch hook of a one-number metric: ``fn(xs, ys)`` -> (n,) float64, not called on an empty shard."""
    def per_batch(xs, ys):
        return {name: fn(xs, ys) if len(xs) else np.zeros(0), "h": np.array([a.shape[0] for a in xs], dtype=np.int64),
                "w": np.array([a.shape[1] for a in xs], dtype=np.int64)}
    return per_batch


def self_pair_files(path, n_pairs, seed=0):
    """``n_pairs`` random pairs (draw_self_pairs) of ONE directory's sorted file list -> ([files[i]], [files[j]])."""
    files = list_files(path)
    idx = draw_self_pairs(len(files), n_pairs, seed)
    return [files[i] for i in idx[:, 0]], [files[j] for j in idx[:, 1]]


def evaluate_pairs(files1, files2, per_batch, sums_of, result_of, batch_size=50, options=None, device=None, ms_ssim=False):
    """This rank's shard of the pairs -> ``result_of`` (totals over all ranks) with per_pair (this rank's arrays), files1, files2
    and range [lo, hi).  ``sums_of``: per-pair arrays -> a float64 vector that is additive over shards."""
    rank, world, _ = tdist.env_world()
    lo, hi = tdist.shard_range(len(files1), rank, world)
    per = paired_from_files(files1[lo:hi], files2[lo:hi], ms_ssim, batch_size, options, device, per_batch=per_batch)
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    acc = torch.from_numpy(sums_of(per)).to(dev)
    tdist.all_reduce_sum_(acc)                               # {n, sum, sum of squares} per metric: the only exchange
    res = result_of(acc.cpu().numpy())
    res["per_pair"], res["files1"], res["files2"], res["range"] = per, list(files1), list(files2), (lo, hi)
    return res


def add_pair_arguments(parser, seed_help, saved_file_help, after_path2=None, after_batch_size=None):
    """The options every pair-metric CLI has, in the order of its --help; ``after_*``: callables that add the tool's own."""
    parser.add_argument("--path1", required=True, type=str, help="folder of originals (with --self-pairs: the one folder)")
    parser.add_argument("--path2", default=None, type=str, help="folder of reconstructions, paired by relative path without extension")
    if after_path2:
        after_path2(parser)
    parser.add_argument("--self-pairs", default=0, type=int, help="N random pairs (i != j) of --path1 instead of two folders")
    parser.add_argument("--seed", default=0, type=int, help=seed_help)
    parser.add_argument("--per-pair", default="", type=str, help="write one CSV line per pair here")
    parser.add_argument("--saved_file", default="", type=str, help=saved_file_help)
    parser.add_argument("--batch-size", default=50, type=int)
    if after_batch_size:
        after_batch_size(parser)
    parser.add_argument("--png-feed", default="ring", choices=["ring", "dataloader"])
    parser.add_argument("--jpeg-feed", default=None, choices=["native", "pillow"])
    parser.add_argument("--num-workers", default=0, type=int, help="image decode processes per side (0 = auto)")
    parser.add_argument("--gpu_id", default="0", type=str)


def check_pair_arguments(parser, args):
    if args.self_pairs:
        if args.path2:
            parser.error("--self-pairs takes --path1 only")
    elif not args.path2:
        parser.error("give --path2, or --self-pairs N")


def parse_model_pair_args(argv, description, flag, flag_help):
    """The parser of a pair metric on VGG-16: the common options, --weights, ``flag`` (the head's file) and --synthetic-weights."""
    def own(p):
        p.add_argument("--weights", default="", type=str, help="torchvision VGG-16 state_dict (vgg16-397923af.pth)")
        p.add_argument(flag, default="", type=str, help=flag_help)
        p.add_argument("--synthetic-weights", action="store_true",
                       help="seeded stand-in parameters: plumbing / throughput runs only (result lines are tagged)")
    parser = argparse.ArgumentParser(description=description)
    add_pair_arguments(parser, "seed of the --self-pairs draw and of the --synthetic-weights parameters",
                       "write the result line here as well", after_batch_size=own)
    args = parser.parse_args(argv)
    check_pair_arguments(parser, args)
    if args.synthetic_weights and (args.weights or getattr(args, flag[2:].replace("-", "_"))):
        parser.error(f"--synthetic-weights and --weights / {flag} are mutually exclusive")
    return args


def resolve_model_files(args, what, head_file, default_trunk, build_model, missing):
    """-> (model, tag) of a pair metric on VGG-16.  The trunk file: --weights, else ``default_trunk`` if it exists; the head's
    file has no default path.  Anything missing without --synthetic-weights is an error (``missing``), never a silent stand-in."""
    from . import weights as tweights
    if args.synthetic_weights:
        tweights.warn_synthetic(what)
        return build_model(synthetic=True, seed=args.seed), tweights.SYNTHETIC_TAG
    trunk = args.weights or (default_trunk if os.path.exists(default_trunk) else "")
    for path in (trunk, head_file):
        if path and not os.path.exists(path):
            raise RuntimeError("Invalid path: %s" % path)
    if not trunk or not head_file:
        raise RuntimeError(missing)
    return build_model(trunk, head_file), ""


def cli_device(args, tool, gpu="gpu_id"):
    """The device of this process (torchrun's local rank, else the option ``gpu``: --gpu_id, or --gpu where a CLI spells it so),
    made current."""
    if not torch.cuda.is_available():
        raise _lib.TiseLibraryError(f"{tool} needs an MI355X: there is no CPU path")
    rank, world, local_rank = tdist.init_from_env()
    dev = torch.device(f"cuda:{local_rank}" if world > 1 else f"cuda:{getattr(args, gpu)}")
    torch.cuda.set_device(dev)
    return dev


def feed_options(args):
    return feeds.Options(png_feed=args.png_feed, jpeg_feed=args.jpeg_feed, num_workers=args.num_workers)


def finish_cli(args, res, lines, columns, csv_of, dev):
    """--per-pair (the ranks' rows of h, w and ``columns`` gathered, ``csv_of(files1, files2, arrays)`` written by rank 0),
    --saved_file and the print."""
    if args.per_pair:
        per, (lo, hi) = res["per_pair"], res["range"]
        names = ["h", "w"] + list(columns)
        cols = [np.arange(lo, hi, dtype=np.float64)] + [per[c] for c in names]
        rows = tdist.all_gather_rows(torch.from_numpy(np.stack([np.asarray(c, dtype=np.float64) for c in cols], axis=1)).to(dev)).cpu().numpy()
        if tdist.is_main():
            with open(args.per_pair, "w") as f:
                f.write(csv_of(res["files1"], res["files2"], {c: rows[:, k + 1] for k, c in enumerate(names)}))
    tdist.write_lines(lines, args.saved_file)
    return res


# ---- this CLI --------------------------------------------------------------------------------------------------------
def _evaluate(files1, files2, ms_ssim, batch_size, options, device):
    return evaluate_pairs(files1, files2, None, metric_sums, result_from_sums, batch_size, options, device, ms_ssim)


def calculate_paired_given_paths(path1, path2, ms_ssim=False, batch_size=50, options=None, device=None):
    """PSNR, SSIM and (``ms_ssim``) MS-SSIM of every pair of two directories (pair_files) -> dict: psnr, psnr_std, ssim, ssim_std,
    [ms_ssim, ms_ssim_std,] n, identical; per_pair (this rank's arrays), files1, files2, range.  Under torchrun every rank
    returns the totals."""
    return _evaluate(*pair_files(path1, path2), ms_ssim, batch_size, options, device)


def calculate_self_pairs(path, n_pairs, seed=0, ms_ssim=False, batch_size=50, options=None, device=None):
    """The diversity use: ``n_pairs`` random pairs (draw_self_pairs) of ONE directory's sorted file list, side one files[i], side
    two files[j] -> calculate_paired_given_paths' dict (the diversity number is its ms_ssim: pass ``ms_ssim=True``)."""
    return _evaluate(*self_pair_files(path, n_pairs, seed), ms_ssim, batch_size, options, device)


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="PSNR, SSIM and MS-SSIM of image pairs")
    add_pair_arguments(parser, "seed of the --self-pairs draw", "write the result lines here as well", after_path2=lambda p: p.add_argument(
        "--ms-ssim", action="store_true", help="five-scale MS-SSIM as well (smaller side >= 176)"))
    args = parser.parse_args(argv)
    check_pair_arguments(parser, args)
    return args


def main(argv=None):
    args = parse_args(argv)
    dev = cli_device(args, "paired")
    if args.self_pairs:
        res = calculate_self_pairs(args.path1, args.self_pairs, args.seed, args.ms_ssim, args.batch_size, feed_options(args), dev)
    else:
        res = calculate_paired_given_paths(args.path1, args.path2, args.ms_ssim, args.batch_size, feed_options(args), dev)
    return finish_cli(args, res, result_lines(res), ["psnr", "ssim"] + (["ms_ssim"] if args.ms_ssim else []), per_pair_csv, dev)


if __name__ == "__main__":
    tdist.run_cli(main)
