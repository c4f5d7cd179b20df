"""CountSeg on MI355X: the counter of counting alignment (CA.py) on the ResNet-50 trunk of resnet_hip.py.

``HipCountSeg(model)`` takes a ``countseg_model.CountSeg`` (real parameters or the seeded stand-ins) and offers
``rows_from_u8((n, H, W, 3) uint8) -> (n, 2 C) fp64``: per image ``[confidence_0 .. confidence_{C-1} | density_mean_0 ..
density_mean_{C-1}]``.  Per batch:

  trunk   ``HipResNet50.map_from_u8``: the last map as a split tensor (n, h, w, 4096), h = ceil(H / 32); chunked under the trunk's
          activation budget
  mix     ONE ``SplitConv`` 2048 -> 240 in mode 1 into fp32 (scale * conv; the bias is left to the consumer, as with conv3 of a
          bottleneck); kernel choice left to "auto"
  head    ONE ``device.countseg_head`` (csrc/countseg.hip): both 1 x 1 branches in fp64, 3 x 3 local maxima, the median by rank
          counting, the mean of the surviving peaks and the mean of the density map, the maps never leaving the LDS
  guard   the range guard of the split format, read once; a non-finite row raises ``FloatingPointError``

There is no CPU path and no library convolution.  A row's bits do not depend on its batch, chunk or position.  ``last_peaks`` keeps
the (n, C) int32 peak counts of the last call.  ``TISE_COUNTSEG=torch`` (``build_counter``) runs the fp32 module itself on library
kernels: the A/B route.  The map is at most 1024 pixels (tise_countseg_head): an image of up to 1024 x 1024; CA runs at 448 x 448.
"""
import os

import torch

from . import countseg_model, device, resnet_hip
from .conv_split import SplitConv


class HipCountSeg:
    resolution = 448                                                        # what CA resizes to

    def __init__(self, model, device_=None, budget=resnet_hip.ACTIVATION_BUDGET_BYTES):
        if not isinstance(model, countseg_model.CountSeg):
            raise TypeError("HipCountSeg takes a countseg_model.CountSeg")
        self.trunk = resnet_hip.HipResNet50(model.trunk, device_, budget)
        self.dev = self.trunk.dev
        self.synthetic = bool(model.synthetic)
        self.n_classes, self.width = model.n_classes, model.width
        p, c = self.width, self.n_classes
        f32 = lambda t: t.detach().float().cpu().contiguous()
        head = [f32(model.mix.weight), f32(model.mix.bias), f32(model.cls.weight).reshape(c, p), f32(model.cls.bias),
                f32(model.den.weight).reshape(c, p), f32(model.den.bias)]
        if not all(bool(torch.isfinite(t).all()) for t in head):
            raise ValueError("CountSeg: non-finite value (NaN or Inf) in the parameters of the head")
        self.mix = SplitConv(head[0], torch.zeros(2 * p), (1, 1), (0, 0), self.dev, name="mix", check=False)
        self.b_mix, self.w_cls, self.b_cls, self.w_den, self.b_den = (t.to(self.dev).contiguous() for t in head[1:])
        self.last_peaks = None

    @torch.no_grad()
    def rows_from_u8(self, batch):
        """(n, H, W, 3) uint8 device batch of one size, H and W >= 32, ceil(H / 32) ceil(W / 32) <= 1024 -> (n, 2 C) fp64 rows
        [conf | den].  Raises FloatingPointError when an activation left the fp16 range of the split format or a row is not finite."""
        x = self.trunk.map_from_u8(batch)
        n, h, w, _ = x.shape
        if h * w > device.COUNTSEG_MAX_PIXELS:
            raise ValueError(f"CountSeg: the last map of a {batch.shape[1]} x {batch.shape[2]} image is {h} x {w}: more than "
                             f"{device.COUNTSEG_MAX_PIXELS} pixels")
        c = self.n_classes
        raw = torch.empty((n, h, w, 2 * self.width), dtype=torch.float32, device=self.dev)
        if n:
            self.mix(x, [(0, 2 * self.width, raw, 0, 1)])
        conf, den, self.last_peaks = device.countseg_head(raw, self.b_mix, self.w_cls, self.b_cls, self.w_den, self.b_den)
        rows = torch.cat([conf, den], 1)
        if n and device.read_split_overflow():
            raise FloatingPointError("CountSeg: an activation exceeded the fp16 range of the split-precision format (|v| > 65504); the "
                                     "result is not usable")
        if not bool(torch.isfinite(rows).all()):
            raise FloatingPointError("CountSeg: a confidence or density mean is not finite")
        return rows


class TorchCountSeg:
    """``TISE_COUNTSEG=torch``: the fp32 module itself on library kernels, with HipCountSeg's interface.  ``autocast``: under
    torch.autocast(fp16) (tools/countseg_probe.py's third side)."""
    resolution = 448

    def __init__(self, model, device_, autocast=False):
        self.model = model.to(device_).float().eval()
        self.dev = torch.device(device_)
        self.synthetic, self.n_classes, self.width, self.autocast = bool(model.synthetic), model.n_classes, model.width, bool(autocast)
        self.last_peaks = None

    @torch.no_grad()
    def rows_from_u8(self, batch):
        with torch.autocast("cuda", dtype=torch.float16, enabled=self.autocast):
            m, d = self.model.maps(batch.to(self.dev))
        conf, cnt = countseg_model.peak_stimulation(m.float())              # the decisions in fp32 on both sides of the A/B
        self.last_peaks = cnt.to(torch.int32)
        rows = torch.cat([conf.double(), d.float().mean((2, 3)).double()], 1)
        if not bool(torch.isfinite(rows).all()):
            raise FloatingPointError("CountSeg: a confidence or density mean is not finite")
        return rows


def build_counter(weights, dev, seed=0):
    """The counter the CLI runs: HipCountSeg over countseg_model.build_model, or TorchCountSeg with TISE_COUNTSEG=torch.
    ``weights=None``: seeded stand-ins (the CLI only allows that behind --synthetic-weights)."""
    from .engine import require_gpu
    require_gpu()
    model = countseg_model.build_model(weights, synthetic=not weights, seed=seed)
    route = os.environ.get("TISE_COUNTSEG", "hip")
    if route == "torch":
        return TorchCountSeg(model, dev)
    if route != "hip":
        raise ValueError(f"TISE_COUNTSEG={route!r}: 'hip' (default) or 'torch'")
    return HipCountSeg(model, dev)
