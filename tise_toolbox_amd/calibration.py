#!/usr/bin/env python3
"""IS* temperature calibration on MI355X: fit the T that IS* divides the logits by, for the model this project runs.

Drop-in for the reference's ``classifier_calibration/temperature_scaling.py`` (``ModelWithTemperature.set_temperature``
:34-77, ``_ECELoss`` :80-119) as its notebook drives it: cached validation logits + labels in, the NLL-optimal T out.
The reference's T_COCO / T_BIRD / T_OIS (engine.py) were fitted for other networks; this fits T to the
logits that ``inception_score`` actually forms -- same engine, feed, classifier bias rule and dropped background class
(``collect_logits``) -- and the printed T goes unchanged into ``inception_score --temperature``.

What is reproduced of the reference:
  * T is an fp32 parameter (``torch.ones(1) * init_temp``, :16-18) optimised by ``torch.optim.LBFGS([T], lr=0.01,
    max_iter=50)`` with torch's defaults (:62).
  * The loss is the MEAN cross-entropy of logits / T (:41, :65).
  * The closure calls ``loss.backward()`` and never zeroes ``T.grad`` (:64-67), so the k-th evaluation hands LBFGS the
    SUM of the k gradients so far.  The fitted T depends on it; ``fit_temperature`` accumulates the same way.
  * Before: NLL / ECE of the raw logits (T = 1); after: at the fitted T.  The three printed lines, in its format.
  * ECE: 15 bins with fp32 edges ``torch.linspace(0, 1, 16)``; a row is in a bin when lower < conf <= upper; empty bins
    are skipped; ece = sum |mean conf - accuracy| * share of rows.
What differs: every loss / gradient / ECE evaluation is one pass of csrc/calibrate.hip over the resident logits in fp64
(the reference evaluates in fp32 on its GPU); the loss and gradient handed to LBFGS are rounded to fp32 as the
reference's are.  Labels index the classes AFTER a dropped background column (``--drop-first-class``, c0 = 1).

    python -m tise_toolbox_amd.calibration --features val_logits.npz
    python -m tise_toolbox_amd.calibration --image_dir VAL --labels subdirs --rule coco [--save-features f.npz]
"""
import os
import sys
from argparse import ArgumentDefaultsHelpFormatter, ArgumentParser

import numpy as np
import torch

from . import device, dist as tdist, weights as tweights
from .engine import require_gpu
from .inception import NETWORKS, network_classes

N_BINS = 15


# ---- LBFGS with the reference's accumulated gradient ---------------------------------------------------------------------
def fit_temperature(evaluate, init_temp=1.0, lr=0.01, max_iter=50):
    """``evaluate(T) -> (mean nll, d mean nll / dT)`` (Python floats, T the fp32 parameter's value) -> fitted T (float).

    torch.optim.LBFGS on a CPU fp32 parameter exactly as temperature_scaling.py:62-69 sets it up; the closure adds each
    new gradient (rounded to fp32) to ``T.grad`` without zeroing it, as ``loss.backward()`` does there."""
    t = torch.nn.Parameter(torch.ones(1) * init_temp)
    opt = torch.optim.LBFGS([t], lr=lr, max_iter=max_iter)

    def closure():
        loss, grad = evaluate(float(t.detach()[0]))
        g = torch.tensor([grad], dtype=torch.float32)
        if t.grad is None:
            t.grad = g
        else:
            t.grad.add_(g)
        return torch.tensor(loss, dtype=torch.float32)

    opt.step(closure)
    return float(t.detach()[0])


def ece_from_bins(count, conf_sum, correct_sum, n_rows):
    """_ECELoss (:107-119) from per-bin sums: sum over non-empty bins of |mean conf - accuracy| * count / N (fp64)."""
    ece = 0.0
    for k, c, a in zip(count, conf_sum, correct_sum):
        if k > 0:
            ece += abs(c / k - a / k) * (k / n_rows)
    return float(ece)


def _summary(ev, temperature):
    r = ev(temperature)
    n = ev.rows
    bins = [((a / k) if k else 0.0, (c / k) if k else 0.0, int(k))
            for k, c, a in zip(r["count"], r["conf_sum"], r["correct_sum"])]
    return {"nll": r["nll_sum"] / n, "ece": ece_from_bins(r["count"], r["conf_sum"], r["correct_sum"], n),
            "bins": bins}


def _device_logits(logits):
    require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    if not isinstance(logits, torch.Tensor):
        logits = torch.from_numpy(np.ascontiguousarray(logits))
    logits = logits.to(dev, torch.float32)
    if logits.dim() != 2 or logits.stride(1) != 1:
        logits = logits.contiguous()
    return logits


def _evaluator(logits, labels, c0, n_bins):
    logits = _device_logits(logits)
    if logits.shape[0] == 0:
        raise ValueError("no logits to calibrate on")
    return device.CalibrationEvaluator(logits, torch.as_tensor(np.asarray(labels) if not isinstance(labels, torch.Tensor)
                                                               else labels), c0=c0, n_bins=n_bins)


def expected_calibration_error(logits, labels, T=1.0, n_bins=N_BINS, c0=0):
    """_ECELoss()(logits / T, labels) (temperature_scaling.py:80-119), evaluated on the device."""
    return _summary(_evaluator(logits, labels, c0, n_bins), T)["ece"]


def set_temperature_from_logits(logits, labels, init_temp=1.0, lr=0.01, max_iter=50, n_bins=N_BINS, c0=0, verbose=True):
    """set_temperature (temperature_scaling.py:34-77) on cached logits: (N, c0 + C) fp32 logits (CUDA tensor or numpy),
    (N,) labels in [0, C) -> dict(temperature, before, after, lines); before / after = dict(nll, ece, bins), bins = per
    bin (accuracy, mean confidence, count).  Prints the reference's three lines when ``verbose``."""
    ev = _evaluator(logits, labels, c0, n_bins)
    n = ev.rows
    before = _summary(ev, 1.0)

    def evaluate(t):
        r = ev(t)
        return r["nll_sum"] / n, r["grad_sum"] / n
    if verbose:
        print("Before temperature - NLL: %.3f, ECE: %.3f" % (before["nll"], before["ece"]), flush=True)
    t = fit_temperature(evaluate, init_temp, lr, max_iter)
    after = _summary(ev, t)
    lines = ["Before temperature - NLL: %.3f, ECE: %.3f" % (before["nll"], before["ece"]),
             "Optimal temperature: {}".format(t),
             "After temperature - NLL: %.10f, ECE: %.10f" % (after["nll"], after["ece"])]
    if verbose:
        print(lines[1])
        print(lines[2], flush=True)
    return {"temperature": t, "before": before, "after": after, "lines": lines}


# ---- labelled images -> logits ---------------------------------------------------------------------------------------------
def _is_image(name):
    return name.rfind("jpg") != -1 or name.rfind("png") != -1      # img_data.get_filenames' rule


def labels_from_subdirs(root):
    """ImageFolder / ImageNet-val convention: class i = the i-th of the SORTED subfolders of ``root``; every image below
    it (any depth, sorted) has label i.  -> (files, labels int64, class names)."""
    classes = sorted(d for d in os.listdir(root) if os.path.isdir(os.path.join(root, d)))
    if not classes:
        raise ValueError(f"{root}: no class subfolders")
    files, labels = [], []
    for i, cls in enumerate(classes):
        for dirpath, dirnames, names in os.walk(os.path.join(root, cls)):
            dirnames.sort()
            for name in sorted(names):
                p = os.path.join(dirpath, name)
                if _is_image(name) and os.path.isfile(p):
                    files.append(p)
                    labels.append(i)
    return files, np.asarray(labels, dtype=np.int64), classes


def labels_from_file(root, label_file, num_classes=None):
    """One ``relative/path<TAB>label`` per line (empty lines skipped), paths relative to ``root``.  A path that is not a
    file, a label that is not an integer or (with ``num_classes``) outside [0, num_classes) raises ValueError naming the
    line.  -> (files, labels int64)."""
    files, labels = [], []
    with open(label_file) as f:
        for lineno, line in enumerate(f, 1):
            line = line.rstrip("\r\n")
            if not line.strip():
                continue
            parts = line.split("\t")
            if len(parts) != 2:
                raise ValueError(f"{label_file}:{lineno}: expected 'relative/path<TAB>label', got {line!r}")
            rel, lab = parts
            p = os.path.join(root, rel)
            if not os.path.isfile(p):
                raise ValueError(f"{label_file}:{lineno}: no such image {p!r}")
            try:
                y = int(lab)
            except ValueError:
                raise ValueError(f"{label_file}:{lineno}: label {lab!r} is not an integer") from None
            if y < 0 or (num_classes is not None and y >= num_classes):
                raise ValueError(f"{label_file}:{lineno}: label {y} outside [0, {num_classes})")
            files.append(p)
            labels.append(y)
    if not files:
        raise ValueError(f"{label_file}: no labelled images")
    return files, np.asarray(labels, dtype=np.int64)


class _LogitSink:
    """Stands where the engine keeps its IS* accumulator: ``update(logits, idx_base)`` receives exactly the logits IS*
    would reduce, and stores them in rows idx_base.. of one preallocated buffer."""

    def __init__(self, out):
        self.out = out

    def update(self, logits, idx_base):
        self.out[idx_base:idx_base + logits.shape[0]].copy_(logits)


class _NoStats:
    def update(self, feats):
        pass


def collect_logits(files, rule="coco", drop_first_class=False, fc_bias="auto", weights=None, num_classes=None, seed=0,
                   batch_size=50, network="torchvision"):
    """Image files -> (N, num_classes) fp32 logits on the device (one preallocated buffer) and c0 (1 with
    ``drop_first_class``, else 0).  The images go through inception_score's engine and feed (PNG ring, the rule's
    classifier bias -- inception.fc_bias_for_rule), so the logits are bitwise those IS* divides by T."""
    from . import inception_score as isc
    isc.configure(weights=weights, num_classes=num_classes, seed=seed, rule=rule, drop_first_class=drop_first_class,
                  fc_bias=fc_bias, batch_size=batch_size, network=network)
    eng = isc._engine()
    n = len(files)
    out = torch.empty((n, eng.model.fc.out_features), dtype=torch.float32, device=eng.device)

    def begin():
        eng.begin(n_total=max(n, 1), rule=rule, drop_first_class=drop_first_class)
        eng.stats = _NoStats()                       # only the logits are wanted
        eng.is_acc = _LogitSink(out)
    isc.feed_images(eng, list(files), 0, n, begin)
    eng.check_numerics(collective=False)
    return out, (1 if drop_first_class else 0)


# ---- CLI ---------------------------------------------------------------------------------------------------------------------
def _build_parser():
    parser = ArgumentParser(formatter_class=ArgumentDefaultsHelpFormatter,
                            description="Fit the IS* temperature (temperature_scaling.py) to this project's model.")
    src = parser.add_mutually_exclusive_group(required=True)
    src.add_argument("--features", type=str, default=None,
                     help="npz with 'features' (N x C logits) and 'labels' (N ints), the calibration notebook's input")
    src.add_argument("--image_dir", type=str, default=None, help="labelled validation images")
    parser.add_argument("--labels", type=str, default="subdirs",
                        help="with --image_dir: 'subdirs' (class = sorted subfolder index) or a file of "
                             "'relative/path<TAB>label' lines")
    parser.add_argument("--rule", type=str, default="coco", choices=["coco", "bird", "ois"],
                        help="the IS* rule the temperature is for (decides the classifier bias, as in inception_score)")
    parser.add_argument("--drop-first-class", action="store_true", help="bird: class 0 is background (labels index the rest)")
    parser.add_argument("--fc-bias", type=str, default="auto", choices=["auto", "on", "off"],
                        help="classifier bias in the logits; auto follows --rule as inception_score does")
    parser.add_argument("--weights", type=str, default=None, help="torchvision-format InceptionV3 state_dict (.pth)")
    parser.add_argument("--synthetic-weights", action="store_true",
                        help="seeded stand-in parameters (plumbing only; results are tagged)")
    parser.add_argument("--num-classes", type=int, default=None,
                        help="classifier width (default: 1000, 1008 for --network inception-2015, 51 for --network slim)")
    parser.add_argument("--network", type=str, default="torchvision", choices=list(NETWORKS),
                        help="torchvision: torchvision's InceptionV3; inception-2015: the TensorFlow Inception-2015 graph of the "
                             "reference's IS* for COCO (pytorch-fid's pt_inception-2015-12-05-6726825d.pth: 1008 classes, "
                             "exclude-padding average pools, max-pool branch in Mixed_7c, input (v - 128) / 128); slim: the "
                             "TF-slim InceptionV3 of the reference's IS* for CUB birds (a TensorFlow checkpoint: 51 classes, "
                             "exclude-padding average pools, no BatchNorm gamma, input v / 127.5 - 1)")
    parser.add_argument("--seed", type=int, default=0, help="seed of the --synthetic-weights parameters")
    parser.add_argument("--batch-size", type=int, default=50)
    parser.add_argument("--init-temp", type=float, default=1.0)
    parser.add_argument("--lr", type=float, default=0.01)
    parser.add_argument("--max-iter", type=int, default=50)
    parser.add_argument("--n-bins", type=int, default=N_BINS)
    parser.add_argument("--save-features", type=str, default="", help="write the collected logits + labels (npz)")
    parser.add_argument("--saved_file", type=str, default="", help="write T and the NLL / ECE before and after")
    parser.add_argument("--gpu", type=int, default=0)
    return parser


def main(argv=None):
    args = _build_parser().parse_args(argv)
    if args.num_classes is None:
        args.num_classes = network_classes(args.network)
    if args.network == "slim" and args.rule == "bird":
        args.drop_first_class = True          # the bird head's class 0 is background (inception_score_star_bird.py:180-189)
    if tdist.env_world()[1] > 1:
        raise SystemExit("tise_toolbox_amd.calibration runs in one process: start it without torchrun "
                         "(the logits of a validation set fit one GPU)")
    os.environ.setdefault("HIP_VISIBLE_DEVICES", str(args.gpu))
    tag = ""
    if args.features:
        with np.load(args.features) as f:
            logits = np.asarray(f["features"], dtype=np.float32)
            labels = np.asarray(f["labels"]).astype(np.int64)
        c0 = 1 if args.drop_first_class else 0
    else:
        wpath, tag = tweights.resolve(args.weights, args.synthetic_weights,
                                      tweights.inception_kind(args.network, args.rule == "ois" and args.num_classes == 80))
        n_cls = args.num_classes - (1 if args.drop_first_class else 0)
        if args.labels == "subdirs":
            files, labels, _ = labels_from_subdirs(args.image_dir)
        else:
            files, labels = labels_from_file(args.image_dir, args.labels, n_cls)
        if labels.size and (labels.min() < 0 or labels.max() >= n_cls):
            raise ValueError(f"labels must lie in [0, {n_cls}) for a {args.num_classes}-class head")
        print("[Data] [{}] labelled images ...".format(len(files)), flush=True)
        from .engine import run_with_exact_fallback
        logits, c0 = run_with_exact_fallback(
            lambda: collect_logits(files, args.rule, args.drop_first_class, args.fc_bias, wpath, args.num_classes,
                                   args.seed, args.batch_size, args.network), "the logit collection")
        if args.save_features:
            np.savez(args.save_features, features=logits.cpu().numpy(), labels=labels)
    res = set_temperature_from_logits(logits, labels, args.init_temp, args.lr, args.max_iter, args.n_bins, c0, verbose=False)
    for line in res["lines"]:
        print(line)
    if tag:
        print(tag.strip())
    if args.saved_file:
        with open(args.saved_file, "w") as f:
            f.write("\n".join(res["lines"]) + tag + "\n")
    sys.stdout.flush()
    return res


if __name__ == "__main__":
    tdist.run_cli(main)
