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
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .vgg_pairs import (CONV_CHANNELS, CONV_INDICES, DEFAULT_FILE, MIN_SIDE, POOL_BEFORE, TAP_AFTER, TAP_CHANNELS, TAP_NAMES,  # noqa: F401
                        VGG16Pairs, default_weights_path, named_source)

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
EPS = 1e-10

CONFIGS = {"vgg": {"conv_indices": CONV_INDICES, "conv_channels": CONV_CHANNELS, "tap_after": TAP_AFTER, "pool_before": POOL_BEFORE,
                   "tap_channels": TAP_CHANNELS, "default_file": DEFAULT_FILE}}
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


def _guess_lin(chans):
    for name, c in _OTHER_LINS.items():
        if tuple(chans) == c:
            return {"alex": "AlexNet", "squeeze": "SqueezeNet"}[name]
    return "an unknown network"


class LpipsVGG16(VGG16Pairs):
    """The definition above in plain torch.  ``forward(a, b)``: two (N,H,W,3) uint8 tensors -> (N,) LPIPS in the module's dtype
    (fp32 as built, fp64 after ``.double()``)."""
    check_size = staticmethod(check_size)

    def __init__(self, net="vgg"):
        cfg = config(net)
        super().__init__(input_table())
        self.net = net
        self.lins = nn.ParameterList([nn.Parameter(torch.zeros(c), requires_grad=False) for c in cfg["tap_channels"]])
        self.freeze()

    # ---- parameters --------------------------------------------------------------------------------------------------
    def load_lins(self, source):
        """The package's linear-layer file (``lin0.model.1.weight`` .. ``lin4.model.1.weight``, each (1, C, 1, 1)) or its dict.
        A file whose shapes say another network is refused, naming both."""
        path, sd = named_source(source)
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
        self.init_synthetic_trunk(g)
        for lin in self.lins:
            lin.copy_(torch.rand(lin.shape, generator=g, dtype=torch.float64).to(lin.dtype))
        return self

    # ---- arithmetic --------------------------------------------------------------------------------------------------
    def prepare(self, img):
        """(N,H,W,3) uint8 -> (N,3,H,W) in the module's dtype: the table look-up."""
        return self.table_lookup(img)[1]

    def taps(self, x, amax=None):
        """(N,3,H,W) -> the five tap tensors.  ``amax``: a list that receives the largest |activation| of every convolution."""
        return self.features(x, lambda t: F.max_pool2d(t, 2, 2), amax)

    @staticmethod
    def head(a, b, w):
        """Two (N,C,h,w) tap tensors and (C,) weights -> (N,): the mean over the pixels of sum_c w_c (a_c / n(a) - b_c / n(b))^2."""
        na = a.pow(2).sum(1, keepdim=True).sqrt() + EPS
        nb = b.pow(2).sum(1, keepdim=True).sqrt() + EPS
        d = ((a / na - b / nb).pow(2) * w.view(1, -1, 1, 1)).sum(1)
        return d.mean((1, 2))

    def forward(self, a, b, amax=None):
        self.check_pair(a, b)
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
