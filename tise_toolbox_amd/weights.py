"""Where the networks' parameters come from.

The reference always evaluates with PRETRAINED parameters: torchvision's ``inception_v3(pretrained=True)`` download
(image_realism/FID/inception.py:57 -> ``$TORCH_HOME/hub/checkpoints/inception_v3_google-1a9a5a14.pth``), the 80-class
fine-tune ``weights/inceptionv3_fine_to_with_80_coco_classes.pth`` (object_fidelity/O-IS/object_centric_inception_score.py:45,
O-FID/inception.py:63) and ``clip.load("ViT-B/32")`` (text_relevance/RP_coco.py:33 -> ``~/.cache/clip/ViT-B-32.pt``).
There is no network here, so the CLIs resolve, in order:

  1. ``--weights PATH``                       (torchvision / OpenAI-format state_dict)
  2. the path the reference itself would read (the cache file / relative path above), if it exists
  3. ``--synthetic-weights``: seeded stand-in parameters -- throughput and plumbing runs only.  A warning goes to
     stderr and every result line / file carries ``SYNTHETIC_TAG`` so that it cannot pass for a real score
     (``ranking_score --collect`` refuses tagged files).
  4. otherwise: ``RuntimeError`` -- never a silent stand-in.
"""
import os
import sys

SYNTHETIC_TAG = " [synthetic weights: not a real score]"

_KINDS = {
    "inception": ("InceptionV3 (torchvision inception_v3_google-1a9a5a14.pth)",
                  lambda: [os.path.join(_torch_home(), "hub", "checkpoints", "inception_v3_google-1a9a5a14.pth"),
                           os.path.join(_torch_home(), "checkpoints", "inception_v3_google-1a9a5a14.pth")]),
    "inception80": ("80-class fine-tuned InceptionV3",
                    lambda: [os.path.join("weights", "inceptionv3_fine_to_with_80_coco_classes.pth")]),
    # the Inception-2015 graph (--network inception-2015): pytorch-fid's conversion of classify_image_graph_def.pb, at the
    # path pytorch-fid caches it under
    "inception2015": ("Inception-2015 graph (pytorch-fid pt_inception-2015-12-05-6726825d.pth)",
                      lambda: [os.path.join(_torch_home(), "hub", "checkpoints", "pt_inception-2015-12-05-6726825d.pth")]),
    # the TF-slim InceptionV3 of the reference's IS* for CUB birds: a TensorFlow checkpoint (V1 file or V2 prefix) at the
    # path of inception_score_star_bird.py:35-39, relative to the working directory as there
    "slim": ("TF-slim InceptionV3 fine-tuned on CUB birds (TensorFlow checkpoint birds_valid299/model.ckpt)",
             lambda: [os.path.join("IS", "bird", "inception_finetuned_models", "birds_valid299", "model.ckpt")]),
    "clip": ("CLIP ViT-B/32", lambda: [os.path.expanduser(os.path.join("~", ".cache", "clip", "ViT-B-32.pt"))]),
    # the tower of the published CMMD figures (cmmd --tower ViT-L/14@336), under the name the OpenAI package caches it
    "clip-l14-336": ("CLIP ViT-L/14@336", lambda: [os.path.expanduser(os.path.join("~", ".cache", "clip", "ViT-L-14-336px.pt"))]),
    # the towers of FD-DINOv2 (fd_dinov2 --arch), under the names torch.hub caches the released files
    "dinov2-vits14": ("DINOv2 ViT-S/14", lambda: [os.path.join(_torch_home(), "hub", "checkpoints", "dinov2_vits14_pretrain.pth")]),
    "dinov2-vitb14": ("DINOv2 ViT-B/14", lambda: [os.path.join(_torch_home(), "hub", "checkpoints", "dinov2_vitb14_pretrain.pth")]),
    "dinov2-vitl14": ("DINOv2 ViT-L/14", lambda: [os.path.join(_torch_home(), "hub", "checkpoints", "dinov2_vitl14_pretrain.pth")]),
    # the trunk of FD-SwAV (fd_swav), under the name torch.hub's facebookresearch/swav caches the released file (from memory: UNPINNED)
    "swav-resnet50": ("SwAV ResNet-50 (800 epochs)", lambda: [os.path.join(_torch_home(), "hub", "checkpoints", "swav_800ep_pretrain.pth.tar")]),
    # the counter of counting alignment (CA), at the relative path counting_alignment/CA.py:139 loads
    "countseg": ("CountSeg ResNet-50 (coco14.pt)", lambda: [os.path.join("weights", "coco14.pt")]),
}


def _torch_home():
    return os.path.expanduser(os.environ.get("TORCH_HOME", os.path.join(os.environ.get("XDG_CACHE_HOME", "~/.cache"), "torch")))


def warn_synthetic(what):
    print(f"[tise] WARNING: {what} runs with SEEDED STAND-IN parameters (no pretrained file given): scores are "
          f"meaningless except for comparing code paths on identical inputs", file=sys.stderr, flush=True)


def inception_kind(network, label_80=False):
    """The ``_KINDS`` entry of an InceptionV3 run: ``label_80`` = the 80-class fine-tune (O-IS / O-FID with 80 classes)."""
    if network == "inception-2015":
        return "inception2015"
    if network == "slim":
        return "slim"
    return "inception80" if label_80 else "inception"


def _exists(path, kind):
    """A TensorFlow checkpoint path names a V1 file or the prefix of a V2 checkpoint (``path.index`` + data shards)."""
    return os.path.exists(path) or (kind == "slim" and os.path.exists(path + ".index"))


def resolve(weights, synthetic, kind, what=None):
    """-> (path or None, tag).  ``None`` means seeded stand-in parameters (only with ``synthetic``).  ``kind`` None: a
    network without a default file (``what`` names it), so ``--weights`` or ``--synthetic-weights`` it has to be."""
    if kind is None:
        defaults = lambda: []
    else:
        what, defaults = _KINDS[kind][0] if what is None else what, _KINDS[kind][1]
    if synthetic:
        # an explicit request always wins: a seeded plumbing / throughput run must not pick up a file that happens to
        # sit in ~/.cache or the working directory on one machine and not on another
        if weights:
            raise RuntimeError("--synthetic-weights and --weights are mutually exclusive")
        warn_synthetic(what)
        return None, SYNTHETIC_TAG
    if weights:
        if not _exists(weights, kind):
            raise RuntimeError("Invalid path: %s" % weights)
        return weights, ""
    for p in defaults():
        if _exists(p, kind):
            print(f"[tise] {what}: parameters from {p}", file=sys.stderr, flush=True)
            return p, ""
    if kind is None:
        raise RuntimeError(f"no parameters for {what}, which has no default file: pass --weights PATH, or --synthetic-weights "
                           f"for a plumbing/throughput run with seeded stand-ins")
    raise RuntimeError(
        f"no parameters for {what}: the reference downloads them, this machine cannot.  Pass --weights PATH, put the "
        f"file at {defaults()[0]!r}, or pass --synthetic-weights for a plumbing/throughput run with seeded stand-ins")
