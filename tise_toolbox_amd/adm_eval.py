"""The ADM sample-batch suite on MI355X: Inception Score, FID, sFID, Precision and Recall of two ``.npz`` image batches.

The protocol of the guided-diffusion evaluator (Dhariwal & Nichol 2021, "Diffusion Models Beat GANs on Image Synthesis",
evaluations/evaluator.py), whose five-number line diffusion-model result tables report:

    python -m tise_toolbox_amd.adm_eval REF.npz SAMPLE.npz [--weights PATH] [--batch-size 1000] [--save-stats OUT.npz]
                                        [--saved_file OUT.txt] [--synthetic-weights] [--seed S] [--is-split-size 5000]
                                        [--no-prdc] [--gpu 0]

Both sides are (N, H, W, 3) uint8 ``arr_0`` arrays, streamed (npz_batches.py).  One pass per side through
``RealismEngine(network="inception-2015", resize="tf1", spatial=True, with_logits=True)``: the images enter at their own size,
TensorFlow 1's legacy bilinear resize to 299 x 299 and (x - 128) / 128 (csrc/resize_tf1.hip), every image used.

    FID               Frechet distance of the pool3 rows (d = 2048)
    sFID              Frechet distance of the first 7 channels of mixed_6/conv:0 -- Mixed_6d's 1x1 branch after ReLU,
                      17 x 17 x 7 = 2023 numbers per image in h, w, c order (tise_split_tap_rows)
    Inception Score   SAMPLE only: softmax of pool3 @ W.T (no bias), chunks of --is-split-size images from index 0 (the last
                      one shorter), exp(mean KL) per chunk, the mean of the chunk scores
    Precision/Recall  prdc.prdc_from_features(ref rows, sample rows, nearest_k=3)

Known difference: the evaluator compares fp16-rounded distances with ``<=``, this project fp64 distances with ``<`` (prdc.py);
they part only at exact ties.  NOT pinned: the evaluator's printed numbers -- classify_image_graph_def.pb is not available to
this project, nor is TensorFlow; the resize is pinned to a numpy restatement of the CPU kernel (tests/_tf1_resize_ref.py).

REF.npz may be a statistics file instead: ``mu``, ``sigma``, ``mu_s``, ``sigma_s`` (the evaluator's key names) serve FID and
sFID; Precision and Recall also need a ``features`` array, which --save-stats writes (REF's statistics, the side a user keeps
across runs) together with ``network="inception-2015"`` and ``mode="adm"``.  One process only: sharding an .npz over ranks is
not offered.
"""
import argparse
import os

import numpy as np
import torch

from . import dist as tdist
from . import weights as tweights
from .npz_batches import NpzImageBatches, is_statistics_npz

NETWORK = "inception-2015"
MODE = "adm"
NEAREST_K = 3
LINES = ("Inception Score", "FID", "sFID", "Precision", "Recall")          # the evaluator's order
KEYS = ("inception_score", "fid", "sfid", "precision", "recall")


def is_chunks(n, split_size):
    """[(lo, hi)] of the evaluator's Inception Score chunks: from index 0, ``split_size`` images each, the last one shorter."""
    n, split_size = int(n), int(split_size)
    if split_size <= 0:
        raise ValueError("--is-split-size must be positive")
    return [(lo, min(lo + split_size, n)) for lo in range(0, n, split_size)]


def chunk_slices(idx_base, rows, n, split_size):
    """A device batch of ``rows`` images whose first has global index ``idx_base`` cut at the chunk borders ->
    [(chunk, row_lo, row_hi, index of row_lo inside its chunk)]."""
    out, lo, end = [], int(idx_base), min(int(idx_base) + int(rows), int(n))
    while lo < end:
        c = lo // split_size
        hi = min(end, (c + 1) * split_size)
        out.append((c, lo - idx_base, hi - idx_base, lo - c * split_size))
        lo = hi
    return out


class ChunkedInceptionScore:
    """The evaluator's Inception Score from logits that arrive in device batches: one device accumulator per chunk
    (``InceptionScoreAccumulator(..., splits=1)`` with the chunk's length as its image count, T = 1, bias-free rule), a batch
    that straddles a border sliced.  Takes the place of ``RealismEngine.is_acc`` (same ``update(logits, idx_base)``)."""

    def __init__(self, num_classes, n, split_size, dev):
        from . import device
        self.n, self.split_size = int(n), int(split_size)
        self.chunks = is_chunks(n, split_size)
        self.accs = [device.InceptionScoreAccumulator(num_classes, hi - lo, 1.0, 1, "coco", False, dev) for lo, hi in self.chunks]

    def update(self, logits, idx_base):
        for c, a, b, i0 in chunk_slices(idx_base, logits.shape[0], self.n, self.split_size):
            self.accs[c].update(logits[a:b], i0)

    def finalize(self):
        """-> (mean of the chunk scores, [chunk scores])."""
        scores = [float(acc.finalize()[2][0]) for acc in self.accs]
        return float(np.mean(scores)), scores


def load_statistics(path, need_features):
    """A statistics file as REF -> dict(mu, sigma, mu_s, sigma_s, features | None).  A file tagged with another ``mode`` or
    network is refused; an untagged file with ``mu_s`` is taken as the evaluator's own."""
    with np.load(path, allow_pickle=False) as f:
        names = set(f.files)
        mode = str(f["mode"]) if "mode" in names else None
        if mode is not None and mode != MODE:
            raise RuntimeError(f"{path}: statistics of mode {mode!r}; the ADM suite needs its own (mode {MODE!r}: another resize, "
                               "and the spatial statistics mu_s / sigma_s)")
        if "network" in names and str(f["network"]) != NETWORK:
            raise RuntimeError(f"{path}: statistics of network {str(f['network'])!r}, the ADM suite runs on {NETWORK}")
        missing = [k for k in ("mu", "sigma", "mu_s", "sigma_s") if k not in names]
        if missing:
            raise RuntimeError(f"{path}: no {', '.join(missing)} in this statistics file; the ADM suite needs mu, sigma, mu_s and "
                               "sigma_s (the evaluator's reference statistics, or a file made with adm_eval --save-stats)")
        if need_features and "features" not in names:
            raise RuntimeError(f"{path}: no 'features' array in this statistics file, and Precision / Recall need the feature "
                               "rows; make the file with adm_eval --save-stats, or pass --no-prdc for Inception Score, FID and sFID alone")
        out = {k: np.ascontiguousarray(f[k], dtype=np.float64) for k in ("mu", "sigma", "mu_s", "sigma_s")}
        out["features"] = np.ascontiguousarray(f["features"], dtype=np.float32) if (need_features and "features" in names) else None
    return out


def save_statistics(path, side):
    feats = side["features"]
    np.savez(path, mu=_host(side["mu"]), sigma=_host(side["sigma"]), mu_s=_host(side["mu_s"]), sigma_s=_host(side["sigma_s"]),
             features=np.ascontiguousarray(_host(feats), dtype=np.float32), network=np.asarray(NETWORK), mode=np.asarray(MODE))


def _host(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _refuse_multi_rank():
    if tdist.env_world()[1] > 1 or tdist.world_size() > 1:
        raise RuntimeError("adm_eval runs in one process: sharding an .npz image batch over the ranks of a torchrun job is not "
                           "offered (run it without torchrun)")


def _pass(engine, path, batch_size, want_is, is_split_size):
    """One pass over an image batch -> dict(mu, sigma, mu_s, sigma_s, features (device rows), n[, inception_score, is_chunks])."""
    feed = NpzImageBatches(path, batch=batch_size)
    n = feed.n_images
    if n < 2:
        raise RuntimeError(f"{path}: {n} image{'s' if n != 1 else ''}; statistics need at least 2")
    engine.begin(n_total=n, temperature=1.0, splits=1, rule="coco")
    engine.is_acc = ChunkedInceptionScore(engine.model.fc.out_features, n, is_split_size, engine.device) if want_is else None
    engine.reserve_activations(min(batch_size, n))
    rows, base = [], 0
    for b in feed:
        x = b.to(engine.device, non_blocking=True)
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(engine.device))
        feed.in_flight(done)
        rows.append(engine.step_u8(x, base))
        base += b.shape[0]
    mu, sigma = engine.statistics()
    mu_s, sigma_s = engine.statistics_spatial()
    out = dict(mu=mu, sigma=sigma, mu_s=mu_s, sigma_s=sigma_s, features=torch.cat(rows), n=n)
    if want_is:
        out["inception_score"], out["is_chunks"] = engine.is_acc.finalize()
    engine.is_acc = None
    return out


def evaluate(ref, sample, weights=None, batch_size=1000, save_stats="", seed=0, is_split_size=5000, prdc=True, device_index=None):
    """The suite of ``ref`` (an image batch or a statistics file) and ``sample`` (an image batch) -> dict with the keys
    ``inception_score``, ``fid``, ``sfid`` and, with ``prdc``, ``precision`` and ``recall`` (Python floats; ``n_ref``,
    ``n_sample`` and ``is_chunks`` ride along).  ``weights=None``: seeded stand-in parameters (the CLI allows that only
    behind --synthetic-weights).  ``save_stats``: write REF's statistics and feature rows there."""
    from .engine import RealismEngine, require_gpu
    from .fid_score import calculate_frechet_distance
    _refuse_multi_rank()
    for p in (ref, sample):
        if not os.path.exists(p):
            raise RuntimeError("Invalid path: %s" % p)
        if os.path.isdir(p):
            raise RuntimeError(f"{p}: a directory; the ADM suite takes .npz image batches (fid_score serves directories of image files)")
    if int(batch_size) <= 0:
        raise ValueError("batch_size must be positive")
    is_chunks(1, is_split_size)                                        # (refuses a non-positive split size before any work)
    if is_statistics_npz(sample):
        raise RuntimeError(f"{sample}: a statistics file; SAMPLE.npz must be an image batch (the Inception Score needs the images)")
    ref_stats = None
    if is_statistics_npz(ref):
        if save_stats:
            raise RuntimeError(f"{ref}: already a statistics file; --save-stats stores the statistics of an image batch given as REF.npz")
        ref_stats = load_statistics(ref, need_features=prdc)
    else:
        NpzImageBatches(ref, batch=batch_size)                         # a malformed batch is refused before the model is built
    NpzImageBatches(sample, batch=batch_size)
    require_gpu()
    engine = RealismEngine(dims=2048, device_index=device_index, weights=weights, seed=seed, with_logits=True, network=NETWORK,
                           resize="tf1", spatial=True)
    with torch.no_grad():
        r = ref_stats if ref_stats is not None else _pass(engine, ref, batch_size, False, is_split_size)
        if save_stats:
            save_statistics(save_stats, r)
        s = _pass(engine, sample, batch_size, True, is_split_size)
    out = {"inception_score": s["inception_score"]}
    out["fid"] = float(calculate_frechet_distance(r["mu"], r["sigma"], s["mu"], s["sigma"]))
    out["sfid"] = float(calculate_frechet_distance(r["mu_s"], r["sigma_s"], s["mu_s"], s["sigma_s"]))
    if prdc:
        from .prdc import prdc_from_features
        pr = prdc_from_features(r["features"], s["features"], nearest_k=NEAREST_K)
        out["precision"], out["recall"] = pr["precision"], pr["recall"]
    out["n_ref"] = int(r["n"]) if "n" in r else None
    out["n_sample"] = int(s["n"])
    out["is_chunks"] = s["is_chunks"]
    return out


def result_lines(result, tag=""):
    """The evaluator's lines, in its order, for the numbers ``result`` holds."""
    return [f"{label}: {result[key]}{tag}" for label, key in zip(LINES, KEYS) if key in result]


def _build_parser():
    p = argparse.ArgumentParser(prog="python -m tise_toolbox_amd.adm_eval", description=__doc__.split("\n\n")[0],
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("ref", metavar="REF.npz", help="reference side: an (N,H,W,3) uint8 arr_0 batch, or a statistics file (mu, sigma, mu_s, sigma_s)")
    p.add_argument("sample", metavar="SAMPLE.npz", help="sample side: an (N,H,W,3) uint8 arr_0 batch")
    p.add_argument("--weights", default=None, help="Inception-2015 parameters (pytorch-fid's pt_inception-2015-12-05 state_dict)")
    p.add_argument("--synthetic-weights", action="store_true", help="seeded stand-in parameters: plumbing / throughput runs only")
    p.add_argument("--seed", type=int, default=0, help="seed of the stand-in parameters")
    p.add_argument("--batch-size", type=int, default=1000, help="images per device pass")
    p.add_argument("--is-split-size", type=int, default=5000, help="images per Inception Score chunk (the evaluator's split_size)")
    p.add_argument("--save-stats", default="", help="write REF's mu, sigma, mu_s, sigma_s and feature rows to this .npz")
    p.add_argument("--saved_file", default="", help="write the result lines to this file")
    p.add_argument("--no-prdc", action="store_true", help="skip Precision and Recall (a statistics file without feature rows can then serve as REF)")
    p.add_argument("--gpu", default="0", help="HIP device to use")
    return p


def main(argv=None):
    args = _build_parser().parse_args(argv)
    _refuse_multi_rank()
    os.environ.setdefault("HIP_VISIBLE_DEVICES", args.gpu)
    wpath, tag = tweights.resolve(args.weights, args.synthetic_weights, tweights.inception_kind(NETWORK))
    print([args.ref, args.sample])
    result = evaluate(args.ref, args.sample, wpath, args.batch_size, args.save_stats, args.seed, args.is_split_size, not args.no_prdc)
    tdist.write_lines(result_lines(result, tag), args.saved_file)
    return result


if __name__ == "__main__":
    tdist.run_cli(main)
