"""CountSeg as a plain torch module: the counter of counting alignment (CA.py), the definition the HIP route (countseg_hip.py) is
compared against, its parameter loader and the seeded stand-in parameters.

LAYOUT, RESTATED from Cholakkal, Sun, Khan & Shao 2019 ("Object Counting and Instance Segmentation with Image-level Supervision") and,
FROM MEMORY, the PRM package of Zhou et al. 2018 -- ``nest.modules.fc_resnet50(channels=240)`` under ``peak_response_mapping(..,
enable_peak_stimulation=True, peak_stimulation="addedmodule5", sub_pixel_locating_factor=1)``; neither package is installed here and
parity with their numbers is UNPINNED (README).  With C = 80 classes and P = 120:

  trunk    resnet_model.ResNet50 without its final mean: the last map (n, 2048, h, w), h = ceil(H / 32)
  mix      1 x 1 convolution 2048 -> 2 P with bias, no activation; channels [0, P) feed the class branch, [P, 2 P) the density branch
  cls      1 x 1 convolution P -> C with bias: the class maps M
  den      1 x 1 convolution P -> C with bias: the density maps D
  peaks    ``peak_stimulation``: the local maxima of a class map (``max_pool2d(3, stride 1, padding 1, return_indices)`` returns the
           pixel's own index: the first maximum of a window wins its tie) that reach the map's lower median (``torch.median``)
  output   confidence_c = the mean of M_c over its peaks, density_mean_c = the mean of D_c, n_peaks_c

The backward pass of the reference's model (peak back-propagation, instance masks, its third return value) is not built: CA.py
drops it.
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import resnet_model

N_CLASSES = 80
WIDTH = 120                                   # P; the reference's ``channels`` argument is 2 P = 240
NETWORK = "countseg-resnet50"
_FEATURES = {"0": "conv1", "1": "bn1", "4": "layer1", "5": "layer2", "6": "layer3", "7": "layer4"}      # nest's fc_resnet50.features
_HEAD = ("mix", "cls", "den")


def peak_stimulation(maps):
    """(n, C, h, w) class maps -> (confidence (n, C), n_peaks (n, C) int64), as PRM writes it.  A class map holding a NaN gives
    confidence NaN and 0 peaks."""
    n, c, h, w = maps.shape
    _, idx = F.max_pool2d(maps, 3, 1, 1, return_indices=True)
    own = torch.arange(h * w, device=maps.device).view(1, 1, h, w)
    med = torch.median(maps.flatten(2), 2).values
    peak = (idx == own) & (maps >= med[..., None, None])
    cnt = peak.sum((2, 3))
    conf = torch.where(peak, maps, torch.zeros_like(maps)).sum((2, 3)) / cnt
    bad = torch.isnan(maps).flatten(2).any(2)
    return torch.where(bad, torch.full_like(conf, float("nan")), conf), torch.where(bad, torch.zeros_like(cnt), cnt)


class CountSeg(nn.Module):
    """The definition above.  ``forward``: (n, H, W, 3) uint8 -> (confidence (n, C), density_mean (n, C), n_peaks (n, C)) in the
    module's dtype (fp32 as built, fp64 after ``.double()``)."""

    def __init__(self, n_classes=N_CLASSES, width=WIDTH):
        super().__init__()
        self.trunk = resnet_model.ResNet50()
        self.mix = nn.Conv2d(resnet_model.OUT_DIM, 2 * width, 1)
        self.cls = nn.Conv2d(width, n_classes, 1)
        self.den = nn.Conv2d(width, n_classes, 1)
        self.n_classes, self.width = n_classes, width
        self.synthetic = False
        for p in self.parameters():
            p.requires_grad_(False)
        self.eval()

    @property
    def dtype(self):
        return self.mix.weight.dtype

    def maps(self, img):
        """-> (class maps, density maps), each (n, C, h, w)."""
        t = self.mix(self.trunk.feature_map(img))
        return self.cls(t[:, :self.width]), self.den(t[:, self.width:])

    def forward(self, img):
        m, d = self.maps(img)
        conf, cnt = peak_stimulation(m)
        return conf, d.mean((2, 3)), cnt

    # ---- parameters ------------------------------------------------------------------------------------------------------
    def load_countseg(self, source):
        """A checkpoint ``{"model": state_dict}`` or a bare state dict, or the file of either.  ``module.`` and PRM's leading ``0.``
        are stripped; the trunk comes as ``features.{0,1,4,5,6,7}.*`` (nest's fc_resnet50) or under ``conv1, bn1, layer1..4``; the head
        under THIS project's names ``mix``, ``cls``, ``den`` only (the head's names in the released coco14.pt are not known here: a
        converter is separate work).  Any other key is refused by name, any wrong shape naming both shapes."""
        path, sd = (source, _load_file(source)) if isinstance(source, (str, os.PathLike)) else ("state_dict", source)
        if isinstance(sd, dict) and isinstance(sd.get("model"), dict):
            sd = sd["model"]
        trunk, head = {}, {}
        for key, v in sd.items():
            k = key
            if k.startswith("module."):
                k = k[len("module."):]
            if k.startswith("0."):
                k = k[2:]
            parts = k.split(".")
            if parts[0] == "features" and len(parts) > 2 and parts[1] in _FEATURES:
                k = ".".join([_FEATURES[parts[1]]] + parts[2:])
                parts = k.split(".")
            if k.endswith("num_batches_tracked"):
                continue
            if parts[0] in _HEAD and len(parts) == 2 and parts[1] in ("weight", "bias"):
                head[k] = v
            elif parts[0] in ("conv1", "bn1", "layer1", "layer2", "layer3", "layer4"):
                trunk[k] = v
            else:
                raise ValueError(f"{path}: {key} is {tuple(getattr(v, 'shape', ()))}, CountSeg has no such entry: this loader takes "
                                 f"the trunk as features.{{0,1,4,5,6,7}}.* or conv1, bn1, layer1..4 and the head as mix, cls, den")
        own = {k: v for k, v in self.state_dict().items() if k.split(".")[0] in _HEAD}
        for k, t in own.items():
            got = tuple(head[k].shape) if k in head and hasattr(head[k], "shape") else None
            if got != tuple(t.shape):
                raise ValueError(f"{path}: {k} is {got if got else 'missing'}, CountSeg has {tuple(t.shape)}")
        try:
            self.trunk.load_resnet50(trunk)
        except ValueError as e:
            raise ValueError(f"{path}: the trunk: {str(e)[len('state_dict: '):]}") from None
        for k, t in own.items():
            t.copy_(head[k].to(t.dtype))
        self.synthetic = False
        return self

    def init_synthetic(self, seed=0):
        """Seeded stand-in parameters (weights.py's rules: plumbing and throughput runs only, result lines are tagged).  The trunk's
        stand-ins as they are; then, from a generator of its own in fp64: mix, cls and den weights N(0, 2 / fan_in), mix bias 0.1 N,
        b_cls N(0, 1) -- on the trunk's stand-in features the class maps have a spread of about five around zero, so both
        signs of the confidence occur -- and b_den U(-0.5, 3.5); with the density maps' own spread the rounded counts take many
        values (tests/test_countseg_host.py holds both)."""
        self.trunk.init_synthetic(seed)
        g = torch.Generator().manual_seed(int(seed) + 0x43534547)
        rn = lambda shape: torch.randn(shape, generator=g, dtype=torch.float64)
        for conv in (self.mix, self.cls, self.den):
            conv.weight.copy_((rn(conv.weight.shape) * (2.0 / conv.in_channels) ** 0.5).to(conv.weight.dtype))
        self.mix.bias.copy_((0.1 * rn(self.mix.bias.shape)).to(self.mix.bias.dtype))
        self.cls.bias.copy_((B_CLS_MEAN + B_CLS_STD * rn(self.cls.bias.shape)).to(self.cls.bias.dtype))
        self.den.bias.copy_((-0.5 + 4.0 * torch.rand(self.den.bias.shape, generator=g, dtype=torch.float64)).to(self.den.bias.dtype))
        self.synthetic = True
        return self


B_CLS_MEAN, B_CLS_STD = 0.0, 1.0              # init_synthetic: checked on the CPU against the trunk's stand-in features


def _load_file(path):
    sd = torch.load(path, map_location="cpu")
    if not isinstance(sd, dict):
        raise ValueError(f"{path}: not a state dict")
    return sd


def build_model(weights=None, synthetic=False, seed=0):
    """CountSeg from a file, or seeded stand-ins under ``synthetic`` (never silently)."""
    if synthetic:
        if weights:
            raise RuntimeError("--synthetic-weights and --weights are mutually exclusive")
        return CountSeg().init_synthetic(seed)
    if not weights:
        raise RuntimeError("CountSeg needs a parameter file (--weights: a checkpoint with the trunk as features.* and the head as mix, "
                           "cls, den); or --synthetic-weights for a plumbing run")
    return CountSeg().load_countseg(weights)


def preprocess_u8(img, size=448):
    """CA.py's transform before normalising: RGB, ``transforms.Resize((448, 448))`` = Pillow's 8-bit BILINEAR resize straight to
    size x size, the bytes kept.  Returns a (size, size, 3) uint8 tensor."""
    import numpy as np
    from PIL import Image
    return torch.from_numpy(np.asarray(img.convert("RGB").resize((size, size), Image.BILINEAR), dtype=np.uint8).copy())
