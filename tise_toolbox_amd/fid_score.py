#!/usr/bin/env python3
"""FID on MI355X -- drop-in for the reference ``image_realism/FID/fid_score.py``.

Same module-level functions (names, argument meaning, return types, error behaviour) and the
same CLI flags / result-file text as the reference, so a caller switches by changing the import:

    get_activations                 fid_score.py:67      calculate_activation_statistics  :174
    calculate_frechet_distance      :121                 _compute_statistics_of_path      :199
    calculate_fid_given_paths       :223                 CLI                              :51-64,:241-254

What runs where: PNG decode on DataLoader workers (as the reference, :215-217); resize + input
affine, InceptionV3, fp64 mean/covariance accumulation and the Frechet distance on the GPU
(``engine.py`` -> ``libtise_hip.so`` + PyTorch-ROCm).  With ``torchrun --nproc-per-node N`` the file
list is sharded over N GPUs and the sufficient statistics are combined with one RCCL all-reduce.

Deviations from the reference, all deliberate (SURVEY.md notes N3-N5):
  * ``--gpu ""`` (CPU mode) is refused: this package is the MI355X path and has no CPU fallback.
  * ``--path1/--path2`` are required (upstream defaults them to the int 64 by a copy-paste slip).
  * extra flags: ``--weights`` (torchvision-format state_dict; there is no network to download it; without the flag
    the file the reference would read is looked up, see ``weights.py``), ``--synthetic-weights`` + ``--seed``
    (seeded stand-in parameters for plumbing / throughput runs: results are tagged), ``--save-stats`` (write
    mu/sigma .npz, the format upstream only reads; with ``--path1`` omitted this is the STATS-ONLY mode: no
    Frechet distance is solved), ``--label`` ("FID" | "O-FID", object_fidelity/O-FID/fid_score.py:216-222),
    ``--num-classes`` (80 for the O-FID fine-tune, O-FID/inception.py:58-64), ``--per-class`` (extension, BASELINE
    configs[4]: one FID per object class, crops grouped by the ``{class}`` token of ``{stem}_{class}_{k}.png``,
    object_fidelity/crop_object.py:45), ``--mode clean`` (extension: clean-fid's FID -- Inception-2015, every channel resized
    as a float32 image with Pillow's bicubic filter and not quantised, every image used; MODES below), ``--mode pytorch-fid``
    and ``--mode torch-fidelity`` (extensions: those packages' input routes on Inception-2015, every image used),
    ``--untagged-stats MODE`` (whose statistics a {mu, sigma} file without a mode tag holds).
"""
import contextlib
import os
import sys
import time
_T_IMPORT0 = time.time()
import warnings
from argparse import Action, ArgumentDefaultsHelpFormatter, ArgumentParser, ArgumentTypeError
from dataclasses import replace

import numpy as np
import torch

from . import _lib, device, dist as tdist, feeds, img_data, weights as tweights
from .engine import (RealismEngine, coalesce_batches, coalesce_u8, device_batch_images, frechet_solver, require_gpu,
                     run_with_exact_fallback)
from .inception import NETWORK_CLASSES, NETWORKS, InceptionV3

warnings.filterwarnings("ignore")          # fid_score.py:49
_T_IMPORT1 = time.time()


def _timing(label, t0=None):
    """TISE_TIMING=1: phase times of the process on stderr (tools/cli_probe.py reads them)."""
    if os.environ.get("TISE_TIMING") == "1" and tdist.is_main():
        now = time.time()
        try:
            # age of the process from the kernel's own clocks: start time in ticks since boot (/proc/self/stat field 22) against
            # /proc/uptime.  (psutil's create_time adds the start ticks to /proc/stat's btime, a WHOLE second: its phase stamps
            # were off by up to 1 s and could exceed the wall clock bench.py's cli_process leg measured around the process)
            start_ticks = int(open("/proc/self/stat").read().rsplit(")", 1)[1].split()[19])
            born = now - (float(open("/proc/uptime").read().split()[0]) - start_ticks / os.sysconf("SC_CLK_TCK"))
        except Exception:                                              # noqa: BLE001
            born = _T_IMPORT0
        extra = f" (+{now - t0:.2f} s)" if t0 is not None else ""
        print(f"[tise timing] {label}: {now - born:.2f} s after process start{extra}", file=sys.stderr, flush=True)
    return time.time()


# the networks FID is taken on: the reference never takes FID on the TF-slim bird network (it serves IS* for CUB only)
FID_NETWORKS = tuple(n for n in NETWORKS if n != "slim")


# --mode: what an image goes through before the network and which images count.  tise: the reference's -- Pillow's 8-bit bilinear
# resize (csrc/resize.hip), whole loader batches only.  clean: clean-fid's (Parmar et al. 2022) -- network inception-2015, every
# channel resized as a float32 image with Pillow's antialiased bicubic filter and NOT quantised, clipped to [0, 255], mapped
# (x - 128) / 128 (csrc/resize_f32.hip), every image used.  The file set is this module's os.walk either way (clean-fid globs and
# sorts: the same FID, other KID subsets).
# pytorch-fid: pytorch-fid's (Seitzer 2020) -- network inception-2015, byte / 255, torch's float32 bilinear interpolation
# (align_corners=False, no antialiasing), 2 x - 1 (csrc/resize_torch.hip), every image used.  torch-fidelity: torch-fidelity's
# (Obukhov et al. 2020; torchmetrics' FrechetInceptionDistance runs its extractor) -- network inception-2015, TensorFlow 1's legacy
# bilinear resize of the bytes as floats, (x - 128) * 2^-7 (csrc/resize_tf1.hip, the ADM suite's kernel), every image used; one
# image size per directory (that kernel has no ragged launch).
MODES = ("tise", "clean", "pytorch-fid", "torch-fidelity")
CLEAN_TAG = " [mode clean]"
MODE_RESIZE = {"tise": "reference", "clean": "clean", "pytorch-fid": "torch", "torch-fidelity": "tf1"}       # engine.RealismEngine(resize=...)
MODE_OWNER = {"clean": "clean-fid's", "pytorch-fid": "pytorch-fid's", "torch-fidelity": "torch-fidelity's"}
PACKAGE_MODES = ("pytorch-fid", "torch-fidelity")       # whose own packages write {mu, sigma} files without a tag: --untagged-stats


def mode_tag(mode):
    """What result lines carry behind the value: nothing under the default mode."""
    return "" if mode == "tise" else f" [mode {mode}]"


def resolve_mode(mode, network):
    """-> the network ``mode`` runs on; ``network`` None: the mode's own (tise: torchvision, every other mode: inception-2015)."""
    if mode not in MODES:
        raise ValueError(f"unknown mode {mode!r} (choose from {', '.join(MODES)})")
    if mode != "tise":
        if network not in (None, "inception-2015"):
            raise ValueError(f"--mode {mode} is {MODE_OWNER[mode]} FID and runs on --network inception-2015 only (got --network {network})")
        return "inception-2015"
    return "torchvision" if network is None else network


_UNTAGGED_STATS = None              # --untagged-stats MODE of this process (main sets it; set_untagged_stats for Python callers)


def set_untagged_stats(mode):
    """A statistics .npz WITHOUT a ``mode`` array is taken as ``mode``'s from now on (None: as the default mode's, the rule
    of every earlier version).  A tagged file is never overridden."""
    global _UNTAGGED_STATS
    if mode is not None and mode not in MODES:
        raise ValueError(f"unknown mode {mode!r} (choose from {', '.join(MODES)})")
    _UNTAGGED_STATS = mode


def _fid_network(value):
    if value == "slim":
        raise ArgumentTypeError("the slim network (TF-slim InceptionV3 of the reference's IS* for CUB birds) has no FID in the "
                                f"reference; choose from {', '.join(FID_NETWORKS)}")
    if value not in FID_NETWORKS:
        raise ArgumentTypeError(f"invalid choice: {value!r} (choose from {', '.join(FID_NETWORKS)})")
    return value


class _NetworkAction(Action):
    """--network, remembering that it was given: --mode clean has a network of its own and refuses an explicit other one."""
    def __call__(self, parser, namespace, values, option_string=None):
        namespace.network = values
        namespace.network_given = True


def _build_parser():
    parser = ArgumentParser(formatter_class=ArgumentDefaultsHelpFormatter)
    parser.add_argument("--batch-size", type=int, default=64, help="Batch size to use")
    parser.add_argument("--dims", type=int, default=2048, choices=list(InceptionV3.BLOCK_INDEX_BY_DIM),
                        help=("Dimensionality of Inception features to use. " "By default, uses pool3 features"))
    parser.add_argument("-c", "--gpu", default="0", type=str, help="GPU to use (CPU mode is not provided)")
    parser.add_argument("--path1", type=str, default=None, help="omit together with --save-stats: statistics of "
                        "--path2 only, no Frechet distance")
    parser.add_argument("--path2", type=str, required=True)
    parser.add_argument("--saved_file", type=str, default="")
    parser.add_argument("--weights", type=str, default=None, help="torchvision-format InceptionV3 state_dict (.pth)")
    parser.add_argument("--num-classes", type=int, default=None, help="classifier width (default: 1000, 1008 for --network inception-2015)")
    parser.add_argument("--network", type=_fid_network, default="torchvision", action=_NetworkAction, metavar="{" + ",".join(FID_NETWORKS) + "}",
                        help="torchvision: torchvision's InceptionV3 (the reference's FID wrapper); inception-2015: the "
                             "TensorFlow Inception-2015 graph pytorch-fid and TTUR take FID on (pt_inception-2015-12-05-6726825d.pth); "
                             "--save-stats then tags the .npz with network=inception-2015 (under --mode clean the default is inception-2015 "
                             "and any other choice is refused)")
    parser.set_defaults(network_given=False)
    parser.add_argument("--mode", type=str, default="tise", choices=list(MODES),
                        help="tise: the reference's FID (Pillow's 8-bit bilinear resize, the last N mod batch-size files dropped); "
                             "clean: clean-fid's FID -- --network inception-2015, every channel resized as a float32 image with "
                             "Pillow's bicubic filter and not quantised, every image used; "
                             "pytorch-fid: pytorch-fid's FID -- --network inception-2015, byte / 255, torch's float32 bilinear "
                             "interpolation (no antialiasing), 2 x - 1, every image used; "
                             "torch-fidelity: torch-fidelity's (and torchmetrics') FID -- --network inception-2015, TensorFlow 1's "
                             "legacy bilinear resize, (x - 128) / 128, every image used, one image size per directory.  --save-stats "
                             "tags the .npz with the mode; --kid keeps this project's subsets under every mode")
    parser.add_argument("--untagged-stats", type=str, default=None, choices=list(MODES), metavar="MODE",
                        help="take a statistics .npz WITHOUT a mode tag (the {mu, sigma} files pytorch-fid itself writes, for "
                             "instance) as MODE's; unset: such a file is the default mode's.  A tagged file is never overridden")
    parser.add_argument("--synthetic-weights", action="store_true",
                        help="seeded stand-in parameters (plumbing / throughput only; results are tagged)")
    parser.add_argument("--seed", type=int, default=0, help="seed of the --synthetic-weights parameters")
    parser.add_argument("--u8-cache", action="store_true",
                        help="decode each image directory once into <dir>/.tise_u8_cache.npy and feed later runs (and "
                             "all ranks) from it over a double-buffered pinned host->device pipeline")
    parser.add_argument("--per-class", action="store_true",
                        help="O-FID extension: one FID per object class ({stem}_{class}_{k}.png crops)")
    parser.add_argument("--save-stats", type=str, default="", help="write mu/sigma of --path2 to this .npz")
    parser.add_argument("--label", type=str, default="FID", choices=["FID", "O-FID"])
    parser.add_argument("--num-workers", type=int, default=0,
                        help="PNG decode processes (the reference hard-codes 8 DataLoader workers, fid_score.py:216); 0 = auto: "
                             "min(128, cpus / 2) shared by the ranks of the node")
    parser.add_argument("--conv", type=str, default=None, choices=["split", "exact"],
                        help="split: hand-written split-fp16 MFMA convolutions (fp32-class arithmetic, default); exact: fp32 "
                             "convolutions (MIOpen).  A split run whose range guard fires is finished on the exact path automatically")
    parser.add_argument("--png-feed", type=str, default="ring", choices=["ring", "dataloader"],
                        help="ring: decode workers write into one shared page-locked ring the parent copies from (png_ring.py); "
                             "dataloader: torch DataLoader workers + collate + pin_memory (round 1-4 path, also the fallback "
                             "for directories whose images differ in size)")
    parser.add_argument("--jpeg-feed", type=str, default=None, choices=["native", "pillow"],
                        help="native: a directory (shard) whose first file is a JPEG of the native subset is Huffman-decoded by threads "
                             "of this process and reconstructed on the GPU (jpeg_feed.py; images may differ in size); pillow: such "
                             "directories take the path of every other file (Pillow in the --png-feed workers).  Default: native for "
                             "directories whose images differ in size, pillow for directories of one size (the faster one of each, DESIGN.md)")
    parser.add_argument("--crop-feed", type=str, default=None, choices=["native", "dataloader"],
                        help="native: PNG directories whose images differ in size (object crops, O-FID) are inflated by threads of this "
                             "process and their row filters reversed on the GPU (crop_feed.py); dataloader: torch DataLoader workers, one "
                             "copy per crop.  Default: --per-class takes the native feed when the shard's first file is a PNG of the "
                             "native subset; a plain directory takes it only when asked (otherwise --png-feed decides)")
    parser.add_argument("--kid", action="store_true",
                        help="also report the Kernel Inception Distance (kid.py: unbiased MMD^2, kernel (x.y/d + 1)^3) from the "
                             "same pass over the images; --save-stats then also stores the feature rows, and an .npz input must hold them")
    parser.add_argument("--kid-subsets", type=int, default=100, help="number of random subsets of the KID estimate")
    parser.add_argument("--kid-subset-size", type=int, default=1000,
                        help="rows per subset and side (capped at the smaller set); 0 = the full-set estimator, no subsets")
    parser.add_argument("--kid-seed", type=int, default=0, help="seed of numpy.random.RandomState for the subsets")
    parser.add_argument("--kid-saved-file", type=str, default="", help="write the KID line(s) to this file")
    parser.add_argument("--prdc", action="store_true",
                        help="also report precision, recall, density and coverage (prdc.py: k-nearest-neighbour manifolds of the pool3 "
                             "rows) from the same pass over the images; --save-stats then also stores the feature rows, and an .npz "
                             "input must hold them.  Not available with --per-class")
    parser.add_argument("--prdc-k", type=int, default=5,
                        help="nearest neighbours of the manifold estimate, 1 .. 16: 5 is the density / coverage paper's value (the "
                             "prdc package), 3 the improved precision / recall paper's")
    parser.add_argument("--prdc-saved-file", type=str, default="", help="write the four precision / recall / density / coverage lines to this file")
    return parser


def _engine_for(model, dims):
    """Wrap a user-supplied reference-style model, or build the default one."""
    if isinstance(model, RealismEngine):
        return model
    eng = getattr(model, "_tise_engine", None)
    if eng is None:
        eng = RealismEngine(dims=dims, model=model, fold_bn=isinstance(model, InceptionV3),
                            resize=MODE_RESIZE[getattr(model, "fid_mode", "tise")])
        try:
            model._tise_engine = eng
        except Exception:
            pass
    return eng


def _forward_batch(engine, model, batch):
    """One batch -> (B, dims) fp32 features on the device, for either input convention."""
    if isinstance(batch, (list, tuple)):                 # ragged uint8 crops: resize each into one batch, ONE trunk pass
        if engine.resize == "tf1":                       # --mode torch-fidelity: a feed's list of equal-sized images is a dense batch
            return engine.features_from_u8(_one_size(engine, batch).to(engine.device, non_blocking=True))[0]
        return engine.features_from_u8_list(batch)[0]
    if batch.dtype == torch.uint8:                       # (B,H,W,3) decoded images: fused device resize
        if engine.resize == "tf1":
            _one_size(engine, batch)
        return engine.features_from_u8(batch.to(engine.device, non_blocking=True))[0]
    if isinstance(model, InceptionV3):
        return engine.features_from_float(batch)[0]
    # arbitrary nn.Module following the reference contract model(batch)[0] -> (B, dims, h, w)
    with torch.no_grad():
        pred = model(batch.to(engine.device))[0]
        if pred.shape[2] != 1 or pred.shape[3] != 1:     # fid_score.py:110-111
            pred = torch.nn.functional.adaptive_avg_pool2d(pred, output_size=(1, 1))
        return pred.reshape(pred.shape[0], -1).float().contiguous()


def _one_size(engine, images):
    """--mode torch-fidelity: a loader's batch -- (B,H,W,3), or a list of (H,W,3) images -- as one (B,H,W,3) batch of THE image
    size of the directory in work (``engine._one_size``, reset per directory by _compute_statistics_of_path); an image of
    another size is refused with the reason."""
    items = [images] if isinstance(images, torch.Tensor) else [(c[0] if c.dim() == 4 else c) for c in images]
    for c in items:
        hw = (int(c.shape[-3]), int(c.shape[-2]))
        seen = getattr(engine, "_one_size", None)
        if seen is None:
            engine._one_size = seen = hw
        if hw != seen:
            raise RuntimeError(f"--mode torch-fidelity: the images of this directory differ in size ({seen[0]} x {seen[1]} and "
                               f"{hw[0]} x {hw[1]}), and the TF1 resize of this mode has no ragged launch: one image size per "
                               "directory (resize or crop the images first, as torch-fidelity's own loader requires)")
    return images if isinstance(images, torch.Tensor) else torch.stack(items)


def _first(images, n):
    """The first n batches of a loader (fid_score.py:99 iterates all of them; n = its own batch count)."""
    import itertools
    return itertools.islice(iter(images), n)


def _check_cuda(cuda):
    if not cuda:
        raise _lib.TiseLibraryError(
            "cuda=False / --gpu '' requests the reference's CPU path; tise_toolbox_amd is MI355X-only "
            "and has no CPU fallback")
    require_gpu()


def get_activations(images, model, batch_size=64, dims=2048, cuda=True, verbose=True):
    """Activations of the pool_3 layer for all images (fid_score.py:67-118).

    ``images``: sized iterable of batches (``len`` = number of batches, :90) of either
    float (B,3,H,W) tensors in [0,1] (reference convention) or uint8 (B,H,W,3) tensors.
    Returns a float64 numpy array (n_used, dims) -- one device->host copy at the end instead of
    one per batch (:113).
    """
    _check_cuda(cuda)
    model.eval()                                          # :86
    d0 = images.__len__() * batch_size                    # :90
    if batch_size > d0:                                   # :91-93
        print(("Warning: batch size is bigger than the data size. " "Setting batch size to data size"))
        batch_size = d0
    n_batches = d0 // batch_size                          # :95  (ZeroDivisionError for an empty loader, as upstream)
    n_used_imgs = n_batches * batch_size                  # :96
    engine = _engine_for(model, dims)
    pred_dev = torch.empty((n_used_imgs, dims), dtype=torch.float32, device=engine.device)
    start = 0
    # the loader's batches are gathered into device batches (engine.device_batch_images): ``batch_size`` defines the
    # bookkeeping above, not the size of a trunk pass
    limit = device_batch_images(batch_size)
    engine.reserve_activations(min(n_used_imgs, limit))
    for batch in coalesce_u8(_first(images, n_batches), engine.device, limit, (n_used_imgs, batch_size)):   # :99
        f = _forward_batch(engine, model, batch)
        pred_dev[start:start + f.shape[0]] = f.reshape(f.shape[0], -1)                       # :113
        start += f.shape[0]
    if verbose:
        print(" done")                                    # :116
    engine.check_numerics(collective=False)               # split-fp16 range guard (no silent inf / NaN features)
    return pred_dev.cpu().numpy().astype(np.float64)      # :98 pred_arr is float64


def calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """Frechet distance d^2 = ||mu_1 - mu_2||^2 + Tr(C_1 + C_2 - 2*sqrt(C_1*C_2))  (fid_score.py:121-171).

    Accepts numpy arrays or CUDA tensors; evaluated on the device in fp64 (csrc/frechet.hip).
    Returns np.float64 like the reference.  The reference's rescue branch for a singular
    product (:156-160) is kept: when the device reports non-finite values the message is printed
    and the computation repeated with ``eps`` added to both diagonals.  The complex-residue
    ``ValueError`` (:163-167) cannot occur here: eigenvalues of a symmetric matrix are real.
    """
    require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())

    def prep(x, nd):
        if isinstance(x, torch.Tensor):
            x = x.to(dev, torch.float64)
            return torch.atleast_1d(x) if nd == 1 else torch.atleast_2d(x)
        x = np.atleast_1d(x) if nd == 1 else np.atleast_2d(x)             # :143-147
        return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device=dev)

    mu1, mu2 = prep(mu1, 1), prep(mu2, 1)
    sigma1, sigma2 = prep(sigma1, 2), prep(sigma2, 2)
    assert mu1.shape == mu2.shape, "Training and test mean vectors have different lengths"            # :149
    assert sigma1.shape == sigma2.shape, "Training and test covariances have different dimensions"    # :150
    d = mu1.shape[0]
    solver = frechet_solver(d, dev)
    res = solver.distance(mu1, sigma1, mu2, sigma2, 0.0)
    if res["flags"] & _lib.TISE_FLAG_NONFINITE:                                                        # :156-160
        msg = ("fid calculation produces singular product; " "adding %s to diagonal of cov estimates") % eps
        print(msg)
        res = solver.distance(mu1, sigma1, mu2, sigma2, float(eps))
    calculate_frechet_distance.last_result = res
    return np.float64(res["fid"])


def calculate_activation_statistics(images, model, batch_size=64, dims=2048, cuda=True, verbose=True,
                                    return_device=False, keep_features=False, n_images=None):
    """mu = mean(act), sigma = cov(act) of the pool_3 activations (fid_score.py:174-196).

    Unlike the reference no (N, dims) float64 array is ever materialised: every batch is folded
    into fp64 {n, sum x, sum x x^T} on the device and (mu, sigma) are finalised there.  Under
    torchrun each rank passes ITS shard of the batches; the sums are all-reduced over RCCL.
    Returns numpy float64 arrays (or CUDA tensors with ``return_device``).
    ``keep_features`` (KID, opt-in): the fp32 pool3 rows of the images used are also kept on the device (8 KB per image) and
    returned as a third value, in global index order on every rank (dist.all_gather_rows).  Without it nothing is retained.
    ``n_images`` (--mode clean): ``images`` delivers exactly this many images and EVERY one is used -- a short last batch
    included; the reference's whole-batch bookkeeping is not applied.
    """
    _check_cuda(cuda)
    model.eval()
    if n_images is not None:
        n_batches = images.__len__()
    elif tdist.world_size() > 1:
        # data-parallel: `images` is THIS rank's shard and may be empty (fewer batches than ranks).  The reference's
        # single-process bookkeeping below would divide by zero there while the other ranks wait in the all-reduce,
        # so an empty rank contributes zeros and the emptiness check is made once, on the global count.
        n_batches = images.__len__()
    else:
        d0 = images.__len__() * batch_size                # fid_score.py:90-96 bookkeeping
        if batch_size > d0:
            print(("Warning: batch size is bigger than the data size. " "Setting batch size to data size"))
            batch_size = d0
        n_batches = d0 // batch_size                      # ZeroDivisionError for an empty loader, as upstream
    engine = _engine_for(model, dims)
    stats = device.StatsAccumulator(dims, engine.device)
    n_rows = n_batches * batch_size if n_images is None else int(n_images)
    engine.reserve_activations(min(n_rows, device_batch_images(batch_size)))      # one allocation of the passes' peak
    if getattr(images, "pregrouped", False):              # img_data.U8CacheLoader(group=K): items are device batches already
        batches = iter(images)
    else:
        limit = device_batch_images(batch_size)
        batches = coalesce_u8(_first(images, n_batches), engine.device, limit, (n_rows, batch_size))
    err = None
    kept = []
    try:
        for batch in batches:
            f = _forward_batch(engine, model, batch)
            stats.update(f)
            if keep_features:
                kept.append(f.reshape(f.shape[0], -1).clone())
    except Exception as e:                                # noqa: BLE001 -- re-raised below, on EVERY rank
        err = e
    # A rank whose image loop failed (an unreadable file, a directory of ragged sizes, a dead decode worker) must not leave
    # the others waiting in the all-reduce below: the failure is agreed on collectively and every rank raises.
    if tdist.world_size() > 1:
        if tdist.any_rank(err is not None):
            if err is not None:
                raise err
            raise RuntimeError("the image loop failed on another rank (its own message says why)")
    elif err is not None:
        raise err
    engine.check_numerics()                               # split-fp16 range guard (no silent inf / NaN features)
    tdist.all_reduce_sum_(stats.buffer())
    if tdist.world_size() > 1 and stats.count() == 0:     # identical on every rank (read after the all-reduce)
        raise ZeroDivisionError("no complete batch in the image set (global N < batch size)")
    if n_images is not None and stats.count() == 0:
        raise ZeroDivisionError("no image in the image set")
    mu, sigma = stats.finalize()
    if verbose:
        print(" done")
    if not return_device:
        mu, sigma = mu.cpu().numpy(), sigma.cpu().numpy()
    if keep_features:
        rows = torch.cat(kept) if kept else torch.empty((0, dims), dtype=torch.float32, device=engine.device)
        return mu, sigma, tdist.all_gather_rows(rows)
    return mu, sigma


U8_CACHE_NAME = ".tise_u8_cache.npy"


_FEED = feeds.Options()             # --png-feed / --jpeg-feed / --crop-feed of this process (main sets them; --num-workers travels as an argument)


def prefetch_png_ring(path, batch_size, num_workers=0):
    """feeds.prefetch_png_ring under this module's flags: the decode workers start NOW, _compute_statistics_of_path picks them up."""
    return feeds.prefetch_png_ring(path, batch_size, replace(_FEED, num_workers=num_workers))


def kid_features_of_npz(path, flag="--kid"):
    """The ``features`` array of a statistics file (float32, n_used x dims, global walk order: what --kid --save-stats or
    --prdc --save-stats stores beside mu and sigma).  KID and the k-NN metrics need the rows themselves; a {mu, sigma} file
    cannot serve them.  ``flag`` names the metric that asks."""
    with np.load(path, allow_pickle=True) as f:
        if "features" not in f.files:
            raise RuntimeError(f"{path}: no 'features' array in this statistics file, and {flag} needs the feature rows; "
                               "make the file with --kid --save-stats or --prdc --save-stats")
        return np.ascontiguousarray(f["features"], dtype=np.float32)


def _compute_statistics_of_path(path, model, batch_size, dims, cuda, num_workers=8, u8_cache=False, keep_features=False):
    """fid_score.py:199-220: an .npz holds (mu, sigma); a directory is walked and pushed through the net.
    ``u8_cache``: decode the directory ONCE into ``<path>/.tise_u8_cache.npy`` ((N,H,W,3) uint8, walk order) and feed
    later runs -- and every rank of a data-parallel run -- from it through a double-buffered pinned host->device
    pipeline (img_data.U8CacheLoader) instead of PNG-decoding DataLoader workers.
    ``keep_features`` (KID, precision / recall / density / coverage): a third value, the fp32 feature rows of the n_used images
    in global walk order -- a device tensor from a directory, the ``features`` array of an .npz."""
    if path.endswith(".npz"):
        f = np.load(path, allow_pickle=True)              # :201-203
        m, s = f["mu"][:], f["sigma"][:]
        tag = str(f["network"]) if "network" in f.files else None
        untagged = "mode" not in f.files
        file_mode = str(f["mode"]) if not untagged else (_UNTAGGED_STATS or "tise")
        f.close()
        if untagged and _UNTAGGED_STATS is not None and tdist.is_main():
            print(f"[tise] {path}: no mode tag in this statistics file; taken as statistics of mode {_UNTAGGED_STATS} (--untagged-stats)",
                  file=sys.stderr, flush=True)
        check_stats_network(path, tag, getattr(model, "network", "torchvision"))
        check_stats_mode(path, file_mode, getattr(model, "fid_mode", "tise"), untagged)
        if keep_features:
            return m, s, kid_features_of_npz(path)
        return m, s
    files = img_data.get_filenames(path)                  # os.walk order (img_data.py:27-35)
    rank, world, _ = tdist.env_world()
    engine = _engine_for(model, dims)
    engine._one_size = None                               # --mode torch-fidelity: the image size of THIS directory (_one_size)

    if getattr(model, "fid_mode", "tise") != "tise":
        # every image is used: contiguous index ranges of the walk per rank (as cmmd.py), a short last loader batch; the PNG
        # ring forms whole batches of ITS batch size, so it runs on batches of one image (as the IS* feed, inception_score.py)
        if u8_cache:
            raise RuntimeError(f"--u8-cache holds whole loader batches only (the reference's drop-last rule); --mode {model.fid_mode} uses every image")
        lo, hi = tdist.shard_range(len(files), rank, world)
        shard = files[lo:hi]

        def consume_all(loader):
            return calculate_activation_statistics(loader, model, batch_size, dims, cuda, keep_features=keep_features, n_images=len(shard))
        return feeds.run(feeds.FID_ALL, shard, replace(_FEED, num_workers=num_workers), consume_all, engine.device, batch_size, world,
                         loader_args={"ring": {"batch_size": 1}})

    def consume(loader):
        return calculate_activation_statistics(loader, model, batch_size, dims, cuda, keep_features=keep_features)
    if u8_cache:
        loader, line = _u8_cache_loader(path, files, batch_size, engine.device, num_workers, rank, world)
        return feeds.session("u8cache", loader, consume, line)
    # jpeg / crop: items are loader batches as the DataLoader's collate_u8 makes them (dense or ragged): the DataLoader path's statistics
    # to the last bit, for images of any sizes.  ring: a ragged directory falls back to the DataLoader in one process; under torchrun the
    # rank that meets the odd file raises inside calculate_activation_statistics, which agrees on the failure collectively (feeds.run)
    shard, _ = tdist.shard_files(files, batch_size, rank, world)       # drop_last=True (:215-217), whole batches
    return feeds.run(feeds.FID, shard, replace(_FEED, num_workers=num_workers), consume, engine.device, batch_size, world, prefetch_key=path)


def _u8_cache_loader(path, files, batch_size, dev, num_workers, rank, world):
    """--u8-cache: (U8CacheLoader over this rank's rows of the cache, its feed line); rank 0 first builds a missing or stale cache."""
    cache = os.path.join(path, U8_CACHE_NAME)              # the name holds neither "png" nor "jpg": never walked
    # valid only for exactly these files as they are on disk now (relative path, size, mtime_ns of every file in
    # walk order, img_data.files_fingerprint): images regenerated under the same names rebuild it
    err = None
    if tdist.is_main() and not img_data.u8_cache_is_current(cache, files, path):
        try:
            img_data.build_u8_cache(files, cache, feeds.resolve_workers(num_workers, world), root=path)
        except Exception as e:                             # the other ranks must not wait in a barrier for a cache that never comes
            err = e
    failed = tdist.any_rank(err is not None)
    if err is not None:
        raise err
    if failed:
        raise RuntimeError(f"--u8-cache: rank 0 could not build {cache}")
    n_used = tdist.n_used_images(len(files), batch_size)
    lo, hi = tdist.shard_range(n_used // batch_size, rank, world)
    shape = np.load(cache, mmap_mode="r").shape
    group = device_batch_images(batch_size, int(np.prod(shape[1:]))) // batch_size
    loader = img_data.U8CacheLoader(cache, batch_size, dev, rows=(lo * batch_size, hi * batch_size), group=group)
    n_img = len(loader) * batch_size

    def line(wall):
        steady = ""
        sec = loader.steady_seconds()
        if sec and n_img > loader.first_item_rows:
            # without the first device batch (first-use costs of the process: code objects, allocator, resize plans):
            # device events at the end of the first and of the last device batch's work (the host time at
            # which the consumer came back for the second item still contained most of the first batch's device time)
            steady = f"; after the first device batch {(n_img - loader.first_item_rows) / sec:.0f} images/s"
        return (f"[tise] u8 cache feed: {n_img} images in {wall:.2f} s ({n_img / wall:.0f} images/s on this rank{steady}); host side "
                f"(page cache -> pinned buffer -> H2D enqueue) {loader.h2d_seconds:.2f} s, the rest is the device pipeline")
    return loader, (line if n_img else None)


def stats_network_tag(network):
    """Extra arrays of a statistics .npz: ``network`` for the Inception-2015 graph only, so that the default network's files
    stay exactly the {mu, sigma} files of the reference (and of pytorch-fid)."""
    return {} if network == "torchvision" else {"network": np.asarray(network)}


def check_stats_network(path, tag, network):
    """A tagged .npz was made on ``tag``'s network: statistics of one network do not compare with features of another.
    Untagged files (the reference's, pytorch-fid's, the default network's) load as they always did."""
    if tag is not None and tag != network:
        raise RuntimeError(f"{path}: statistics of network {tag!r}, this run uses --network {network}")


def stats_mode_tag(mode):
    """``mode`` for every mode but the default one, whose files stay exactly what they were."""
    return {} if mode == "tise" else {"mode": np.asarray(mode)}


def check_stats_mode(path, tag, mode, untagged=False):
    """Statistics of one mode (another resize, another set of images) do not compare with features of the other.  ``tag``: the
    file's ``mode`` array; for a file without one (``untagged``) what --untagged-stats says, else "tise"."""
    if tag != mode:
        hint = ""
        if untagged and mode in PACKAGE_MODES:
            hint = (f" (the file carries no mode tag and reads as the default mode's; if {MODE_OWNER[mode]} own package wrote it, "
                    f"pass --untagged-stats {mode})")
        raise RuntimeError(f"{path}: statistics of mode {tag!r}, this run uses --mode {mode}{hint}")


def save_stats_npz(path, mu, sigma, network="torchvision", features=None, mode="tise"):
    """``features`` (only under --kid or --prdc): the float32 rows those metrics need, beside mu and sigma; without it the file
    is exactly {mu, sigma[, network][, mode]}."""
    extra = {} if features is None else {"features": np.ascontiguousarray(
        features.cpu().numpy() if isinstance(features, torch.Tensor) else features, dtype=np.float32)}
    np.savez(path, mu=np.asarray(mu), sigma=np.asarray(sigma), **stats_network_tag(network), **stats_mode_tag(mode), **extra)


def _build_model(dims, weights, num_classes, seed, network="torchvision"):
    block_idx = InceptionV3.BLOCK_INDEX_BY_DIM[dims]
    model = InceptionV3([block_idx], weights=weights, num_classes=num_classes, seed=seed, network=network)
    from .inception import to_device_flat
    to_device_flat(model, torch.device("cuda", torch.cuda.current_device()))     # model.cuda() (fid_score.py:232-233) in one copy
    return model


@contextlib.contextmanager
def _own_model(dims, weights, num_classes, seed, network="torchvision", mode="tise"):
    """The model of ONE call of this module's path-level functions.

    _engine_for hangs the engine on the model and the engine holds the model: a reference cycle, so a finished call's ~1.4 GiB of
    device memory (weights, packed weights, statistics and staging buffers) stays until the garbage collector's next full pass
    (tools/soak_cli_loop.py: 16 calls in one process held 20 GiB; the reference's model dies when calculate_fid_given_paths
    returns, fid_score.py:229-238).  TISE_RELEASE_MODEL=1 cuts the cycle on the way out, and memory then stays flat
    (tests/test_gpu_pipeline.py::test_repeated_fid_calls_in_one_process_release_their_model).  It is NOT the default: with the
    prompt release in place two of thirteen runs of tests/test_gpu_pipeline.py failed in tests that had never failed before
     and the cause was not found in what was left of round 6 -- the collector-driven release is the
    behaviour of rounds 1-5."""
    network = resolve_mode(mode, network)
    model = _build_model(dims, weights, num_classes, seed, network)
    model.fid_mode = mode                                   # _engine_for picks the resize by it, _compute_statistics_of_path the images
    try:
        yield model
    finally:
        if os.environ.get("TISE_RELEASE_MODEL", "0") == "1":
            try:
                model._tise_engine = None
            except Exception:                                              # noqa: BLE001
                pass


def calculate_fid_given_paths(paths, batch_size, cuda, dims, weights=None, num_classes=None, seed=0,
                              save_stats="", num_workers=8, u8_cache=False, network=None, mode="tise"):
    """Calculates the FID of two paths (fid_score.py:223-238).  ``weights=None`` = seeded stand-in parameters (the
    CLI only allows that behind --synthetic-weights).  ``mode``: MODES ("clean": clean-fid's FID, "pytorch-fid": pytorch-fid's,
    "torch-fidelity": torch-fidelity's; ``network`` None = the mode's own network, resolve_mode)."""
    return _fid_kid_given_paths(paths, batch_size, cuda, dims, weights, num_classes, seed, save_stats, num_workers, u8_cache,
                                network, None, mode=mode)[0]


def calculate_fid_and_kid_given_paths(paths, batch_size, cuda, dims, weights=None, num_classes=None, seed=0, save_stats="",
                                      num_workers=8, u8_cache=False, network=None, subsets=100, subset_size=1000,
                                      kid_seed=0, mode="tise"):
    """FID and KID of two paths from ONE pass over each directory -> (fid, (kid_mean, kid_std)).  The pool3 rows of the images
    FID uses are kept on the device (8 KB per image) and handed to kid.kid_from_features; ``save_stats`` then also stores them
    (``features``), and an .npz path must hold them.  ``kid_seed`` seeds the subsets (``seed`` is the stand-in weights')."""
    return _fid_kid_given_paths(paths, batch_size, cuda, dims, weights, num_classes, seed, save_stats, num_workers, u8_cache,
                                network, {"subsets": subsets, "subset_size": subset_size, "seed": kid_seed}, mode=mode)[:2]


def calculate_kid_given_paths(paths, batch_size, cuda, dims, weights=None, num_classes=None, seed=0, save_stats="",
                              num_workers=8, u8_cache=False, network=None, subsets=100, subset_size=1000, kid_seed=0, mode="tise"):
    """Kernel Inception Distance of two paths -> (mean, std) over the subsets (kid.py; std is NaN for subset_size = 0).
    ``mode="clean"``: clean-fid's KID (its defaults are these: 100 subsets of at most 1000)."""
    return calculate_fid_and_kid_given_paths(paths, batch_size, cuda, dims, weights, num_classes, seed, save_stats, num_workers,
                                             u8_cache, network, subsets, subset_size, kid_seed, mode)[1]


def calculate_prdc_given_paths(paths, batch_size, cuda, dims, weights=None, num_classes=None, seed=0, save_stats="",
                               num_workers=8, u8_cache=False, network=None, nearest_k=5, mode="tise"):
    """Precision, recall, density and coverage of two paths (paths[0] the real side, paths[1] the generated side) -> OrderedDict
    (prdc.py).  One pass over each directory, as for KID: the pool3 rows are kept on the device; ``save_stats`` then also stores
    them (``features``), and an .npz path must hold them."""
    return _fid_kid_given_paths(paths, batch_size, cuda, dims, weights, num_classes, seed, save_stats, num_workers, u8_cache,
                                network, None, nearest_k, mode)[2]


def _fid_kid_given_paths(paths, batch_size, cuda, dims, weights, num_classes, seed, save_stats, num_workers, u8_cache, network,
                         kid_args, prdc_k=None, mode="tise"):
    """calculate_fid_given_paths; with ``kid_args`` (subsets, subset_size, seed) and / or ``prdc_k`` the feature rows of both
    sides are retained and the KID / the k-NN metrics are evaluated after the Frechet distance
    -> (fid, None | (mean, std), None | OrderedDict).  Without either: the launches of the FID alone."""
    network = resolve_mode(mode, network)
    for p in paths:
        if not os.path.exists(p):
            raise RuntimeError("Invalid path: %s" % p)    # :225-227
    keep = kid_args is not None or prdc_k is not None
    if prdc_k is not None and not 1 <= int(prdc_k) <= 16:
        raise ValueError(f"nearest_k must lie in 1 .. 16 (got {prdc_k})")
    if keep:
        for p in paths:                                   # a {mu, sigma} file cannot serve them: say so before anything is computed
            if p.endswith(".npz"):
                kid_features_of_npz(p, "--kid" if kid_args is not None else "--prdc")
    _check_cuda(cuda)
    if not u8_cache and mode == "tise":                    # (clean: the ring runs on batches of one image, started by feeds.run)
        # the decode workers of the first directory start now: PNG decode overlaps building the model (weights, BatchNorm
        # folding, split packing); the second directory's start when the first one's last chunk is decoded
        first = next((p for p in paths if os.path.isdir(p)), None)
        rest = [p for p in paths if os.path.isdir(p) and p != first]
        ld = prefetch_png_ring(first, batch_size, num_workers) if first else None
        if ld is not None and rest:
            ld.on_all_decoded = lambda: prefetch_png_ring(rest[0], batch_size, num_workers)
    t = _timing("decode workers started, building the model")
    if os.environ.get("TISE_PREALLOC_GB"):                 # probe (tools/cli_child_probe.py): what does the first big hipMalloc of a process cost?
        tp = time.perf_counter()
        _x = torch.empty(int(float(os.environ["TISE_PREALLOC_GB"]) * 2**30), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        print(f"[tise timing] prealloc {os.environ['TISE_PREALLOC_GB']} GB: {time.perf_counter() - tp:.3f} s", file=sys.stderr, flush=True)
        del _x
    with _own_model(dims, weights, num_classes, seed, network, mode) as model:
        _engine_for(model, dims)                               # fold BatchNorm, pack the split weights, load the code objects
        t = _timing("model + engine ready", t)
        m1, s1, *f1 = _compute_statistics_of_path(paths[0], model, batch_size, dims, cuda, num_workers, u8_cache, keep)
        t = _timing("first side done", t)
        # the first side's covariance is complete: factor it on a side stream while the second side's images are decoded
        # and pushed through the network (Tr sqrtm(S1 S2) is symmetric in its arguments; csrc/frechet.hip)
        dev = torch.device("cuda", torch.cuda.current_device())
        solver = frechet_solver(dims, dev)
        use_pf = tuple(np.shape(s1)) == (dims, dims) and tuple(np.shape(m1)) == (dims,)
        if use_pf:
            solver.prefactor(torch.as_tensor(np.ascontiguousarray(s1, dtype=np.float64), device=dev))
        m2, s2, *f2 = _compute_statistics_of_path(paths[1], model, batch_size, dims, cuda, num_workers, u8_cache, keep)
        t = _timing("second side done", t)
        if save_stats and tdist.is_main():
            save_stats_npz(save_stats, m2, s2, network, f2[0] if keep else None, mode)

        def solve():
            if not use_pf or np.shape(m1) != np.shape(m2) or np.shape(s1) != np.shape(s2):
                return calculate_frechet_distance(m1, s1, m2, s2)     # generic path (shape asserts :149-150 included)
            try:
                res = solver.distance_prefactored(np.atleast_1d(m1), np.atleast_1d(m2), np.atleast_2d(s2))
            except _lib.TiseStatusError:
                # the factor is gone: the process-wide solver of this (dims, device) served another distance / factorisation
                # between prefactor() and here (a model's forward hook, a second thread).  The one-call form needs nothing kept.
                return calculate_frechet_distance(m1, s1, m2, s2)
            if res["flags"] & _lib.TISE_FLAG_NONFINITE:          # :156-160 (eps retry) lives in calculate_frechet_distance
                return calculate_frechet_distance(m1, s1, m2, s2)
            calculate_frechet_distance.last_result = res
            return np.float64(res["fid"])

        fid = solve()
        if not keep:
            return fid, None, None
        # every rank holds the same rows in the same order (all_gather_rows) and evaluates the KID / the k-NN metrics itself: no broadcast
        kid_value = prdc_value = None
        if kid_args is not None:
            from . import kid
            kid_value = kid.kid_from_features(f1[0], f2[0], kid_args["subsets"], kid_args["subset_size"], kid_args["seed"])
        if prdc_k is not None:
            from . import prdc
            prdc_value = prdc.prdc_from_features(f1[0], f2[0], int(prdc_k))
        return fid, kid_value, prdc_value


def save_statistics_of_path(path, out_npz, batch_size, cuda, dims, weights=None, num_classes=None, seed=0,
                            num_workers=8, u8_cache=False, network=None, keep_features=False, mode="tise"):
    """STATS-ONLY mode: the step BEFORE the reference path -- write the ``.npz {mu, sigma}`` that
    ``_compute_statistics_of_path`` (fid_score.py:200-203) reads (the reference ships such files,
    download_evaluation_data.py:11-12, but no script that makes them).  No Frechet distance is solved."""
    if not os.path.exists(path):
        raise RuntimeError("Invalid path: %s" % path)
    network = resolve_mode(mode, network)
    _check_cuda(cuda)
    if not u8_cache and mode == "tise":
        prefetch_png_ring(path, batch_size, num_workers)   # decode overlaps building the model
    with _own_model(dims, weights, num_classes, seed, network, mode) as model:
        mu, sigma, *feats = _compute_statistics_of_path(path, model, batch_size, dims, cuda, num_workers, u8_cache, keep_features)
        if tdist.is_main():
            save_stats_npz(out_npz, mu, sigma, network, feats[0] if keep_features else None, mode)   # --kid / --prdc: the rows they need, too
        return mu, sigma


def class_of_crop(filename):
    """``{stem}_{class}_{count}.png`` (object_fidelity/crop_object.py:45) -> class name (may contain spaces; the
    image stem may contain underscores, so split from the right)."""
    base = os.path.basename(filename)
    base = base[:base.rfind(".")] if "." in base else base
    parts = base.rsplit("_", 2)
    if len(parts) != 3 or not parts[2].isdigit():
        raise ValueError(f"not a crop file name ({{stem}}_{{class}}_{{k}}.png): {filename}")
    return parts[1]


def _class_statistics(path, model, batch_size, dims, num_workers, owner=None, keep_features=False):
    """One pass over a crop directory -> {class: StatsAccumulator}.  Every crop is used (no drop-last: a class is
    not a DataLoader); batches are formed over the walk-ordered list and each row is folded into its class.
    ``keep_features`` (per-class KID): -> (accumulators, the fp32 rows of ALL crops in walk order, on every rank)."""
    files = img_data.get_filenames(path)
    classes = [class_of_crop(f) for f in files]
    names = sorted(set(classes))
    rank, world, _ = tdist.env_world()
    lo, hi = tdist.shard_range(len(files), rank, world)
    engine = _engine_for(model, dims)
    engine._one_size = None                               # --mode torch-fidelity: the image size of THIS directory (_one_size)
    accs = {c: device.StatsAccumulator(dims, engine.device) for c in names}
    # The pool3 rows of the directory stay on the device (8 KB per crop); once the walk is complete they are sorted by class
    # and folded into the 80 accumulators by ONE grouped launch (device.stats_update_grouped): every class's S is
    # read-modify-written once per directory.  Round 4 ran one index_select + one 528-workgroup covariance launch per class
    # present in a DEVICE BATCH, each a 2 x 33.5 MB read-modify-write of its S for a handful of rows.  Very large
    # directories are flushed every FLUSH_ROWS crops.
    FLUSH_ROWS = 1 << 18
    index_of = {c: i for i, c in enumerate(names)}
    acc_list = [accs[c] for c in names]
    kept, kept_rows = [], 0
    walk = []
    base = lo

    def flush():
        nonlocal kept, kept_rows
        if not kept_rows:
            return
        feats_all = torch.cat(kept) if len(kept) > 1 else kept[0]
        first = base - kept_rows
        cidx = np.fromiter((index_of[c] for c in classes[first:base]), dtype=np.int64, count=kept_rows)
        order = np.argsort(cidx, kind="stable")                       # walk order kept inside a class
        counts = np.bincount(cidx, minlength=len(names))
        offsets = np.concatenate([[0], np.cumsum(counts)])
        feats_sorted = feats_all.index_select(0, torch.from_numpy(order).to(feats_all.device))
        device.stats_update_grouped(acc_list, feats_sorted, offsets)
        kept, kept_rows = [], 0

    def consume(loader):
        nonlocal kept_rows, base
        for batch in coalesce_batches(loader, engine.device, device_batch_images(batch_size)):
            feats = _forward_batch(engine, model, batch)
            kept.append(feats)
            if keep_features:
                walk.append(feats.clone())
            kept_rows += feats.shape[0]
            base += feats.shape[0]
            if kept_rows >= FLUSH_ROWS:
                flush()
        flush()
    # the crop feed (crop_feed.py) forms the DataLoader's batches in its order, every crop used: the same class statistics to the last bit
    feeds.run(feeds.CROPS, files[lo:hi], replace(_FEED, num_workers=num_workers), consume, engine.device, batch_size, world)
    engine.check_numerics()                                # split-fp16 range guard, agreed on by all ranks before the reductions
    # every class is OWNED by one rank (``owner``: class -> rank, the same map on every rank and for both image sets):
    # its 33.57 MB buffer is reduced to that rank only, which alone finalises and solves it (calculate_per_class_fid) --
    # 80 classes on 8 GPUs: ten reduces and ten Frechet solves per rank instead of 80 all-reduces and 80 redundant
    # solves on every rank
    me = tdist.rank()
    parked = []
    for c in names:                                        # same class list on every rank (same walk)
        dst = owner[c] if owner is not None else 0
        tdist.reduce_sum_(accs[c].buffer(), dst=dst)
        if owner is not None and dst != me:
            # not this rank's class.  The buffer is the library's own hipMalloc memory, not the caching allocator's: it must
            # outlive the asynchronous reduce without relying on hipFree's implicit device-wide synchronisation (which would
            # also drain every reduce before the next is enqueued) -- so the accumulators are parked and dropped together
            parked.append(accs[c])
            accs[c] = None
    if parked:
        torch.cuda.current_stream(engine.device).synchronize()
        parked.clear()
    if keep_features:
        # shards are contiguous ranges of the walk (shard_range), so the gathered rows are the one-process walk order
        rows = torch.cat(walk) if walk else torch.empty((0, dims), dtype=torch.float32, device=engine.device)
        return accs, tdist.all_gather_rows(rows)
    return accs


def calculate_per_class_fid(paths, batch_size, cuda, dims, weights=None, num_classes=80, seed=0, num_workers=8,
                            min_count=2, network=None, mode="tise"):
    """EXTENSION (BASELINE configs[4]; the reference computes ONE O-FID over all crops): a Frechet
    distance per object class.  Returns (OrderedDict class -> fid, skipped) where ``skipped`` lists classes with
    fewer than ``min_count`` crops on either side (covariance undefined)."""
    return _per_class(paths, batch_size, cuda, dims, weights, num_classes, seed, num_workers, min_count, network, False, mode)[:2]


def calculate_per_class_kid(paths, batch_size, cuda, dims, weights=None, num_classes=80, seed=0, num_workers=8,
                            min_count=2, network=None, mode="tise"):
    """One full-set KID per object class (kid.per_class_kid: unbiased, so classes with different crop counts compare).
    Returns (OrderedDict class -> kid, skipped) like calculate_per_class_fid."""
    return _per_class(paths, batch_size, cuda, dims, weights, num_classes, seed, num_workers, min_count, network, True, mode)[2:]


def _class_sorted(feats_walk, path, names):
    """Walk-ordered rows of a crop directory -> (rows sorted by class, walk order kept inside a class; offsets over ``names``)."""
    index_of = {c: i for i, c in enumerate(names)}
    cidx = np.array([index_of[class_of_crop(f)] for f in img_data.get_filenames(path)], dtype=np.int64)
    order = np.argsort(cidx, kind="stable")
    offsets = np.concatenate([[0], np.cumsum(np.bincount(cidx, minlength=len(names)))]).astype(np.int64)
    return feats_walk.index_select(0, torch.from_numpy(order).to(feats_walk.device)), offsets


def _per_class(paths, batch_size, cuda, dims, weights, num_classes, seed, num_workers, min_count, network, with_kid, mode="tise"):
    """The per-class pass: -> (fids, skipped, kids | None, kid_skipped | None).  ``with_kid`` retains the crops' rows during
    the same pass (all-gathered in walk order under torchrun: every rank evaluates the 80 small groups itself)."""
    from collections import OrderedDict
    for p in paths:
        if not os.path.isdir(p):
            raise RuntimeError("Invalid path: %s" % p)
    network = resolve_mode(mode, network)
    _check_cuda(cuda)
    with _own_model(dims, weights, num_classes, seed, network, mode) as model:
        # the class list comes from the file names alone: the sorted union over both directories, identical on every rank,
        # dealt round-robin to the ranks
        present = [set(class_of_crop(f) for f in img_data.get_filenames(p)) for p in paths]
        names = sorted(present[0] | present[1])
        world, me = tdist.world_size(), tdist.rank()
        owner = tdist.class_owners(names, world)
        a1 = _class_statistics(paths[0], model, batch_size, dims, num_workers, owner, with_kid)
        a2 = _class_statistics(paths[1], model, batch_size, dims, num_workers, owner, with_kid)
        if with_kid:
            (a1, w1), (a2, w2) = a1, a2
        dev = torch.device("cuda", torch.cuda.current_device())
        mine = []
        status = torch.zeros((len(names), 3), dtype=torch.float64, device=dev)       # [fid, solved, skipped] per class
        for i, c in enumerate(names):
            if owner[c] != me:
                continue
            if c not in a1 or c not in a2 or a1[c].count() < min_count or a2[c].count() < min_count:
                status[i, 2] = 1.0
                continue
            mine.append((i, c))
        fids = _solve_classes([(a1[c], a2[c]) for _, c in mine], dims, dev)
        for (i, _), v in zip(mine, fids):
            status[i, 0], status[i, 1] = v, 1.0
        tdist.all_reduce_sum_(status)                                                 # 80 x 3 doubles: every rank gets every class
        st = status.cpu().numpy()
        out, skipped = OrderedDict(), []
        for i, c in enumerate(names):
            if st[i, 1] > 0:
                out[c] = float(st[i, 0])
            else:
                skipped.append(c)
        if not with_kid:
            return out, skipped, None, None
        from . import kid
        kids, kid_skipped = kid.per_class_kid(*_class_sorted(w1, paths[0], names), *_class_sorted(w2, paths[1], names), names,
                                              min_count)
        return out, skipped, kids, kid_skipped


_CLASS_SOLVERS = {}


def _solve_classes(pairs, dims, dev, eps=1e-6):
    """Frechet distances of [(StatsAccumulator side 1, side 2), ...] on this rank.  A solve at d = 2048 is ~4 000 short
    dependent launches (csrc/frechet.hip: one per column of the tridiagonalisation), i.e. launch-latency bound, so several
    host threads drive one solver and one stream each and the device interleaves them (TISE_PERCLASS_STREAMS, default 4;
    tools/perclass_probe.py, profiles/r04f_perclass_probe.txt: 80 full-rank solves 2.10 s on one stream, 1.38 / 1.22 / 1.14 s
    on 2 / 3 / 4; 80 rank-300 solves 0.57 -> 0.18 s)."""
    import threading
    n = len(pairs)
    out = [None] * n
    if n == 0:
        return out
    nthr = max(1, min(int(os.environ.get("TISE_PERCLASS_STREAMS", "4")), n))
    main_stream = torch.cuda.current_stream(dev)
    done = torch.cuda.Event()
    done.record(main_stream)
    errs = []

    def work(t):
        try:
            torch.cuda.set_device(dev)
            # one solver + stream per worker slot, kept for the life of the process like engine.frechet_solver: creating them
            # per call cost several d x d hipMallocs each, and closing a solver (hipFree = device-wide synchronisation) while
            # the sibling threads were still enqueueing their ~4000 launches per solve stalled the interleaving
            if nthr > 1:
                key = (int(dims), str(dev), t)
                if key not in _CLASS_SOLVERS:
                    _CLASS_SOLVERS[key] = (device.FrechetSolver(dims, dev), torch.cuda.Stream(device=dev))
                solver, stream = _CLASS_SOLVERS[key]
            else:
                solver, stream = frechet_solver(dims, dev), main_stream
            with torch.cuda.stream(stream):
                stream.wait_event(done)
                for j in range(t, n, nthr):
                    m1, s1 = pairs[j][0].finalize()
                    m2, s2 = pairs[j][1].finalize()
                    res = solver.distance(m1, s1, m2, s2, 0.0)
                    if res["flags"] & _lib.TISE_FLAG_NONFINITE:                    # fid_score.py:156-160
                        print(("fid calculation produces singular product; " "adding %s to diagonal of cov estimates") % eps)
                        res = solver.distance(m1, s1, m2, s2, float(eps))
                    out[j] = float(res["fid"])
                stream.synchronize()
        except BaseException as e:                                                 # noqa: BLE001 -- re-raised below
            errs.append(e)

    if nthr == 1:
        work(0)
    else:
        threads = [threading.Thread(target=work, args=(t,), name=f"tise-frechet-{t}") for t in range(nthr)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
    if errs:
        raise errs[0]
    return out


def main(argv=None):
    global _FEED
    parser = _build_parser()
    args = parser.parse_args(argv)
    try:
        args.network = resolve_mode(args.mode, args.network if args.network_given else None)
    except ValueError as e:
        parser.error(str(e))
    if args.mode != "tise" and args.u8_cache:
        parser.error(f"--mode {args.mode} --u8-cache is not available: the cache holds whole loader batches only, --mode {args.mode} uses every image")
    set_untagged_stats(args.untagged_stats)
    if args.num_classes is None:
        args.num_classes = NETWORK_CLASSES[args.network]
    _timing(f"imports done (this module's imports {_T_IMPORT1 - _T_IMPORT0:.2f} s)")
    if args.gpu == "":
        _check_cuda(False)
    if args.path1 is None and not args.save_stats:
        parser.error("--path1 is required (omit it only together with --save-stats: statistics-only mode)")
    if args.prdc and args.per_class:
        parser.error("--per-class --prdc is not available: a k-nearest-neighbour manifold of some 40 crops per class means nothing")
    if args.prdc and not 1 <= args.prdc_k <= 16:
        parser.error("--prdc-k must lie in 1 .. 16")
    rank, world, local_rank = tdist.init_from_env()
    if world == 1:
        os.environ.setdefault("HIP_VISIBLE_DEVICES", args.gpu)        # reference: CUDA_VISIBLE_DEVICES = args.gpu (:243)
    _FEED = feeds.Options(args.png_feed, args.jpeg_feed, args.crop_feed)
    if args.conv is not None:
        os.environ["TISE_CONV"] = "miopen" if args.conv == "exact" else "split"
    kind = tweights.inception_kind(args.network, args.label == "O-FID" and args.num_classes == 80)
    wpath, tag = tweights.resolve(args.weights, args.synthetic_weights, kind)
    tag = mode_tag(args.mode) + tag                                    # result lines name the mode (nothing under the default one)
    if args.path1 is None:                                             # statistics-only
        if tdist.is_main():
            print([args.path2])
        mu, sigma = run_with_exact_fallback(lambda: save_statistics_of_path(
            args.path2, args.save_stats, args.batch_size, args.gpu, args.dims, wpath, args.num_classes, args.seed, args.num_workers,
            args.u8_cache, args.network, args.kid or args.prdc, args.mode), "the statistics pass")
        if tdist.is_main():
            print(f"statistics of {args.path2} -> {args.save_stats}{tag}")
        return None
    paths = [args.path1, args.path2]
    if tdist.is_main():
        print(paths)                                                   # :247
    klabel = "O-KID" if args.label == "O-FID" else "KID"
    if args.per_class:
        per, skipped, kids, kid_skipped = run_with_exact_fallback(lambda: _per_class(
            paths, args.batch_size, args.gpu, args.dims, wpath, args.num_classes, args.seed, args.num_workers, 2,
            args.network, args.kid, args.mode), "the per-class FID")
        mean = float(np.mean(list(per.values()))) if per else float("nan")
        if tdist.is_main():
            lines = [f"{args.label}[{c}]: {v}{tag}" for c, v in per.items()]
            lines.append(f"{args.label} (mean of {len(per)} classes): {mean}{tag}")
            if skipped:
                lines.append("skipped (fewer than 2 crops on a side): " + ", ".join(skipped))
            if args.saved_file:
                with open(args.saved_file, "w") as f:
                    f.write("\n".join(lines))
            print("\n".join(lines))
            if args.kid:
                kmean = float(np.mean(list(kids.values()))) if kids else float("nan")
                klines = [f"O-KID[{c}]: {v}{tag}" for c, v in kids.items()]
                klines.append(f"O-KID (mean of {len(kids)} classes): {kmean}{tag}")
                if kid_skipped:
                    klines.append("skipped (fewer than 2 crops on a side): " + ", ".join(kid_skipped))
                if args.kid_saved_file:
                    with open(args.kid_saved_file, "w") as f:
                        f.write("\n".join(klines))
                print("\n".join(klines))
        return per
    kid_args = {"subsets": args.kid_subsets, "subset_size": args.kid_subset_size, "seed": args.kid_seed} if args.kid else None
    fid_value, kid_value, prdc_value = run_with_exact_fallback(lambda: _fid_kid_given_paths(
        paths, args.batch_size, args.gpu, args.dims, wpath, args.num_classes, args.seed, args.save_stats, args.num_workers,
        args.u8_cache, args.network, kid_args, args.prdc_k if args.prdc else None, args.mode), "the FID")
    fid_value = fid_value.item()
    if tdist.is_main():
        if args.saved_file:
            with open(args.saved_file, "w") as f:
                f.write(f"{args.label}: {fid_value}{tag}")             # :251-252 (no trailing newline)
        print(f"{args.label}: {fid_value}{tag}")                       # :254
        if args.kid:
            kline = f"{klabel}: {kid_value[0]} +- {kid_value[1]}{tag}"
            if args.kid_saved_file:
                with open(args.kid_saved_file, "w") as f:
                    f.write(kline)                                     # no trailing newline, like --saved_file
            print(kline)
        if args.prdc:
            prefix = "O-" if args.label == "O-FID" else ""
            plines = [f"{prefix}{name.capitalize()}: {prdc_value[name]}{tag}" for name in ("precision", "recall", "density", "coverage")]
            if args.prdc_saved_file:
                with open(args.prdc_saved_file, "w") as f:
                    f.write("\n".join(plines))                         # no trailing newline, like --saved_file
            print("\n".join(plines))
    return fid_value


if __name__ == "__main__":
    tdist.run_cli(main)
