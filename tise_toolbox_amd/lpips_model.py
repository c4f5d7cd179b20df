"""LPIPS with the VGG-16 trunk as a plain torch module: the definition the HIP route (lpips_hip.py) is compared against, the
parameter loaders and the seeded stand-in parameters.

DEFINITION (restated from Zhang, Isola, Efros, Shechtman & Wang 2018 and the ``lpips`` package v0.1, net = "vgg"; the package is
not installed here and nothing of it is this file's source -- parity with its numbers is UNPINNED, see README).

  images   8-bit RGB as the feeds decode them; both images of a pair have one size, H and W >= 16 (four floor pools must leave
           one pixel).
  input    x = b / 127.5 - 1, then (x - shift_c) / scale_c with shift = (-0.030, -0.088, -0.188), scale = (0.458, 0.448, 0.450),
           computed in fp32 and tabulated: ``input_table()`` is the (3, 256) table every route reads.
  network  torchvision VGG-16 ``features``: 3 x 3 / stride 1 / padding 1 convolutions at the indices CONV_INDICES, each followed by
           ReLU, MaxPool2d(2, 2) (floor) after blocks 1..4.
  taps     relu1_2, relu2_2, relu3_3, relu4_3, relu5_3: 64, 128, 256, 512, 512 channels.
  head     per tap and pixel n(a) = sqrt(sum_c a_c^2) + 1e-10, d = sum_c w_c (a_c / n(a) - b_c / n(b))^2; the tap's value is the
           mean of d over the pixels; LPIPS is the sum over the five taps.  No resize, no spatial map.
"""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
MIN_SIDE = 16
EPS = 1e-10

CONV_INDICES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)            # torchvision vgg16().features
CONV_CHANNELS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
                 (512, 512), (512, 512), (512, 512))
TAP_AFTER = (1, 3, 6, 9, 12)                                                # conv number (0-based) whose ReLU is a tap
POOL_BEFORE = (2, 4, 7, 10)                                                 # conv number that reads a pooled map
TAP_NAMES = ("relu1_2", "relu2_2", "relu3_3", "relu4_3", "relu5_3")
TAP_CHANNELS = (64, 128, 256, 512, 512)

CONFIGS = {"vgg": {"conv_indices": CONV_INDICES, "conv_channels": CONV_CHANNELS, "tap_after": TAP_AFTER, "pool_before": POOL_BEFORE,
                   "tap_channels": TAP_CHANNELS, "default_file": "vgg16-397923af.pth"}}
# the linear layers of the package's other two networks: what a file of theirs looks like (the loaders name it)
_OTHER_LINS = {"alex": (64, 192, 384, 256, 256), "squeeze": (64, 128, 256, 384, 384, 512, 512)}


def config(net):
    """CONFIGS[net]; ``alex`` and ``squeeze`` are refused with the reason."""
    if net in CONFIGS:
        return CONFIGS[net]
    if net in _OTHER_LINS:
        raise ValueError(f"LPIPS network {net!r} is not built here: only 'vgg' (VGG-16) is -- its thirteen convolutions are all "
                         "3 x 3 / stride 1 / padding 1, the shape family the split-precision kernels serve; AlexNet's 11 x 11 / "
                         "stride 4 stem and SqueezeNet's fire modules are out of scope (README)")
    raise ValueError(f"unknown LPIPS network {net!r}: 'vgg' is the one built here")


def input_table():
    """(3, 256) float32: table[c][b] = ((b / 127.5 - 1) - shift_c) / scale_c, every step in fp32."""
    b = np.arange(256, dtype=np.float32)
    x = b / np.float32(127.5) - np.float32(1.0)
    t = (x[None, :] - np.asarray(SHIFT, dtype=np.float32)[:, None]) / np.asarray(SCALE, dtype=np.float32)[:, None]
    return torch.from_numpy(np.ascontiguousarray(t.astype(np.float32)))


def check_size(h, w, what="LPIPS"):
    if min(int(h), int(w)) < MIN_SIDE:
        raise ValueError(f"{what} needs both sides >= {MIN_SIDE} (four 2 x 2 floor pools must leave one pixel): got {int(h)} x {int(w)}")


def default_weights_path():
    from .weights import _torch_home
    return os.path.join(_torch_home(), "hub", "checkpoints", CONFIGS["vgg"]["default_file"])


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


def _guess_lin(chans):
    for name, c in _OTHER_LINS.items():
        if tuple(chans) == c:
            return {"alex": "AlexNet", "squeeze": "SqueezeNet"}[name]
    return "an unknown network"


def _load_file(path):
    try:
        sd = torch.load(path, map_location="cpu", weights_only=True)
    except TypeError:                                                      # a torch without weights_only
        sd = torch.load(path, map_location="cpu")
    if isinstance(sd, dict) and "state_dict" in sd and isinstance(sd["state_dict"], dict):
        sd = sd["state_dict"]
    if not isinstance(sd, dict):
        raise ValueError(f"{path}: not a state_dict")
    return sd


class LpipsVGG16(nn.Module):
    """The definition above in plain torch.  ``forward(a, b)``: two (N,H,W,3) uint8 tensors -> (N,) LPIPS in the module's dtype
    (fp32 as built, fp64 after ``.double()``)."""

    def __init__(self, net="vgg"):
        super().__init__()
        cfg = config(net)
        self.net = net
        self.convs = nn.ModuleList([nn.Conv2d(ci, co, 3, stride=1, padding=1) for ci, co in cfg["conv_channels"]])
        self.lins = nn.ParameterList([nn.Parameter(torch.zeros(c), requires_grad=False) for c in cfg["tap_channels"]])
        self.register_buffer("table", input_table())
        self.synthetic = False
        for p in self.parameters():
            p.requires_grad_(False)

    # ---- parameters --------------------------------------------------------------------------------------------------
    def load_trunk(self, source):
        """A torchvision ``vgg16`` state_dict (``features.N.weight`` / ``.bias``; classifier entries are ignored) or its file.
        A file whose shapes say another network is refused, naming both."""
        path = source if isinstance(source, (str, os.PathLike)) else "state_dict"
        sd = _load_file(source) if isinstance(source, (str, os.PathLike)) else source
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

    def load_lins(self, source):
        """The package's linear-layer file (``lin0.model.1.weight`` .. ``lin4.model.1.weight``, each (1, C, 1, 1)) or its dict.
        A file whose shapes say another network is refused, naming both."""
        path = source if isinstance(source, (str, os.PathLike)) else "state_dict"
        sd = _load_file(source) if isinstance(source, (str, os.PathLike)) else source
        keys = sorted(k for k in sd if k.startswith("lin") and k.endswith(".model.1.weight"))
        chans = [int(sd[k].shape[1]) if sd[k].dim() == 4 else -1 for k in keys]
        want = [f"lin{k}.model.1.weight" for k in range(len(TAP_CHANNELS))]
        if keys != want or tuple(chans) != TAP_CHANNELS or any(tuple(sd[k].shape) != (1, c, 1, 1) for k, c in zip(keys, chans)):
            raise ValueError(f"{path}: linear layers {keys} with {chans} channels; VGG-16 has {want} with {list(TAP_CHANNELS)}: "
                             f"the file looks like {_guess_lin(chans)}'s, this loader takes the VGG-16 one (vgg.pth)")
        for k, key in enumerate(want):
            self.lins[k].copy_(sd[key].reshape(-1).to(self.lins[k].dtype))
        return self

    def init_synthetic(self, seed=0):
        """Seeded stand-in parameters (weights.py's rules: plumbing and throughput runs only, result lines are tagged):
        He-scaled normal convolutions, small normal biases, non-negative linear weights."""
        g = torch.Generator().manual_seed(int(seed))
        for conv in self.convs:
            fan_in = conv.in_channels * 9
            conv.weight.copy_((torch.randn(conv.weight.shape, generator=g, dtype=torch.float64) * (2.0 / fan_in) ** 0.5).to(conv.weight.dtype))
            conv.bias.copy_((torch.randn(conv.bias.shape, generator=g, dtype=torch.float64) * 0.05).to(conv.bias.dtype))
        for lin in self.lins:
            lin.copy_(torch.rand(lin.shape, generator=g, dtype=torch.float64).to(lin.dtype))
        self.synthetic = True
        return self

    # ---- arithmetic --------------------------------------------------------------------------------------------------
    def prepare(self, img):
        """(N,H,W,3) uint8 -> (N,3,H,W) in the module's dtype: the table look-up."""
        if img.dtype != torch.uint8 or img.dim() != 4 or img.shape[3] != 3:
            raise ValueError(f"images must be (N,H,W,3) uint8 (got {tuple(img.shape)} {img.dtype})")
        check_size(img.shape[1], img.shape[2])
        idx = img.long().permute(0, 3, 1, 2)
        t = self.table.to(self.convs[0].weight.dtype)
        return torch.stack([t[c][idx[:, c]] for c in range(3)], dim=1)

    def taps(self, x, amax=None):
        """(N,3,H,W) -> the five tap tensors.  ``amax``: a list that receives the largest |activation| of every convolution."""
        out = []
        for k, conv in enumerate(self.convs):
            if k in POOL_BEFORE:
                x = F.max_pool2d(x, 2, 2)
            x = F.relu(conv(x))
            if amax is not None:
                amax.append(float(x.abs().max()))
            if k in TAP_AFTER:
                out.append(x)
        return out

    @staticmethod
    def head(a, b, w):
        """Two (N,C,h,w) tap tensors and (C,) weights -> (N,): the mean over the pixels of sum_c w_c (a_c / n(a) - b_c / n(b))^2."""
        na = a.pow(2).sum(1, keepdim=True).sqrt() + EPS
        nb = b.pow(2).sum(1, keepdim=True).sqrt() + EPS
        d = ((a / na - b / nb).pow(2) * w.view(1, -1, 1, 1)).sum(1)
        return d.mean((1, 2))

    def forward(self, a, b, amax=None):
        if a.shape != b.shape:
            raise ValueError(f"both images of a pair must have one size (got {tuple(a.shape)} and {tuple(b.shape)})")
        n = a.shape[0]
        ta = self.taps(self.prepare(torch.cat([a, b], 0)), amax)
        total = None
        for t, w in zip(ta, self.lins):
            v = self.head(t[:n], t[n:], w)
            total = v if total is None else total + v
        return total


def build_model(weights=None, lpips_weights=None, synthetic=False, seed=0, net="vgg"):
    """LpipsVGG16 from the two files, or seeded stand-ins under ``synthetic`` (never silently)."""
    model = LpipsVGG16(net)
    if synthetic:
        if weights or lpips_weights:
            raise RuntimeError("--synthetic-weights and --weights / --lpips-weights are mutually exclusive")
        return model.init_synthetic(seed)
    if not weights or not lpips_weights:
        raise RuntimeError("LPIPS needs two files: the VGG-16 trunk (--weights, torchvision's vgg16-397923af.pth) and the linear "
                           "layers (--lpips-weights, the lpips package's vgg.pth); or --synthetic-weights for a plumbing run")
    return model.load_trunk(weights).load_lins(lpips_weights)
