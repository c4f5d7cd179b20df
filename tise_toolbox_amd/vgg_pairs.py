"""The VGG-16 trunk that the pair metrics share (lpips_model.LpipsVGG16, dists_model.DistsVGG16): torchvision's thirteen 3 x 3 /
stride 1 / padding 1 convolutions, the five ReLU taps, the (3, 256) input table, the trunk file's loader with its refusals and the
seeded stand-in trunk.  A metric adds its table, its pool, its head and the head's parameters.
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

MIN_SIDE = 16
CONV_INDICES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)            # torchvision vgg16().features
CONV_CHANNELS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
                 (512, 512), (512, 512), (512, 512))
TAP_AFTER = (1, 3, 6, 9, 12)                                                # conv number (0-based) whose ReLU is a tap
POOL_BEFORE = (2, 4, 7, 10)                                                 # conv number that reads a pooled map
TAP_NAMES = ("relu1_2", "relu2_2", "relu3_3", "relu4_3", "relu5_3")
TAP_CHANNELS = (64, 128, 256, 512, 512)
DEFAULT_FILE = "vgg16-397923af.pth"


def default_weights_path():
    from .weights import _torch_home
    return os.path.join(_torch_home(), "hub", "checkpoints", DEFAULT_FILE)


def _guess_trunk(sd):
    """What network a torchvision-style state_dict looks like, by its first convolution and its keys."""
    w0 = sd.get("features.0.weight")
    shape = tuple(w0.shape) if hasattr(w0, "shape") else None
    if shape == (64, 3, 11, 11):
        return "AlexNet"
    if any(".squeeze." in k or ".expand" in k for k in sd):
        return "SqueezeNet"
    convs = sorted(int(k.split(".")[1]) for k in sd if k.startswith("features.") and k.endswith(".weight") and sd[k].dim() == 4)
    if shape == (64, 3, 3, 3) and convs and tuple(convs) != CONV_INDICES:
        return f"another VGG variant ({len(convs)} convolutions at features {convs})"
    return "an unknown network"


def load_file(path):
    try:
        sd = torch.load(path, map_location="cpu", weights_only=True)
    except TypeError:                                                      # a torch without weights_only
        sd = torch.load(path, map_location="cpu")
    if isinstance(sd, dict) and "state_dict" in sd and isinstance(sd["state_dict"], dict):
        sd = sd["state_dict"]
    if not isinstance(sd, dict):
        raise ValueError(f"{path}: not a state_dict")
    return sd


def named_source(source):
    """A file or a dict -> (its name in messages, the dict)."""
    if isinstance(source, (str, os.PathLike)):
        return source, load_file(source)
    return "state_dict", source


class VGG16Pairs(nn.Module):
    """The trunk of a pair metric.  A subclass calls ``__init__`` with its input table, adds the head's parameters and then
    calls ``freeze``; it supplies ``check_size`` for ``table_lookup``."""

    def __init__(self, table):
        super().__init__()
        self.convs = nn.ModuleList([nn.Conv2d(ci, co, 3, stride=1, padding=1) for ci, co in CONV_CHANNELS])
        self.register_buffer("table", table)
        self.synthetic = False

    def freeze(self):
        for p in self.parameters():
            p.requires_grad_(False)

    # ---- parameters --------------------------------------------------------------------------------------------------
    def load_trunk(self, source):
        """A torchvision ``vgg16`` state_dict (``features.N.weight`` / ``.bias``; classifier entries are ignored) or its file.
        A file whose shapes say another network is refused, naming both."""
        path, sd = named_source(source)
        for k, idx in enumerate(CONV_INDICES):
            ci, co = CONV_CHANNELS[k]
            for part, want in (("weight", (co, ci, 3, 3)), ("bias", (co,))):
                key = f"features.{idx}.{part}"
                got = tuple(sd[key].shape) if key in sd and hasattr(sd[key], "shape") else None
                if got != want:
                    raise ValueError(f"{path}: {key} is {got if got else 'missing'}, VGG-16 has {want}: the file looks like "
                                     f"{_guess_trunk(sd)}, this loader takes torchvision's VGG-16")
        for k, idx in enumerate(CONV_INDICES):
            self.convs[k].weight.copy_(sd[f"features.{idx}.weight"].to(self.convs[k].weight.dtype))
            self.convs[k].bias.copy_(sd[f"features.{idx}.bias"].to(self.convs[k].bias.dtype))
        return self

    def init_synthetic_trunk(self, generator):
        """Seeded stand-in convolutions (weights.py's rules): He-scaled normal weights, small normal biases, drawn in fp64 per
        convolution, weight then bias.  The head's parameters are drawn from the same generator after these."""
        for conv in self.convs:
            fan_in = conv.in_channels * 9
            conv.weight.copy_((torch.randn(conv.weight.shape, generator=generator, dtype=torch.float64) * (2.0 / fan_in) ** 0.5).to(conv.weight.dtype))
            conv.bias.copy_((torch.randn(conv.bias.shape, generator=generator, dtype=torch.float64) * 0.05).to(conv.bias.dtype))
        self.synthetic = True

    # ---- arithmetic --------------------------------------------------------------------------------------------------
    @property
    def dtype(self):
        return self.convs[0].weight.dtype

    def table_lookup(self, img):
        """(N,H,W,3) uint8 -> (the bytes as (N,3,H,W) int64, the network input (N,3,H,W) in the module's dtype)."""
        if img.dtype != torch.uint8 or img.dim() != 4 or img.shape[3] != 3:
            raise ValueError(f"images must be (N,H,W,3) uint8 (got {tuple(img.shape)} {img.dtype})")
        self.check_size(img.shape[1], img.shape[2])
        idx = img.long().permute(0, 3, 1, 2)
        t = self.table.to(self.dtype)
        return idx, torch.stack([t[c][idx[:, c]] for c in range(3)], dim=1)

    def features(self, x, pool, amax=None):
        """(N,3,H,W) -> the five tap tensors, ``pool`` between the blocks.  ``amax``: a list that receives the largest
        |activation| of every convolution."""
        out = []
        for k, conv in enumerate(self.convs):
            if k in POOL_BEFORE:
                x = pool(x)
            x = F.relu(conv(x))
            if amax is not None:
                amax.append(float(x.abs().max()))
            if k in TAP_AFTER:
                out.append(x)
        return out

    @staticmethod
    def check_pair(a, b):
        if a.shape != b.shape:
            raise ValueError(f"both images of a pair must have one size (got {tuple(a.shape)} and {tuple(b.shape)})")
