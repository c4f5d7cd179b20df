"""LPIPS (VGG-16) on MI355X: lpips_model.LpipsVGG16's definition on vgg_pairs_hip's runner -- LPIPS's input table,
``device.maxpool2s2_split`` after blocks 1..4 and ``device.lpips_layer`` right after each tap.
"""
import torch

from . import device, lpips_model
from .vgg_pairs_hip import ACTIVATION_BUDGET_BYTES, HipVGG16Pairs


class HipLpips(HipVGG16Pairs):
    name, model_class, takes = "LPIPS", lpips_model.LpipsVGG16, "HipLpips takes an lpips_model.LpipsVGG16"
    pool = staticmethod(device.maxpool2s2_split)

    def __init__(self, model, device_=None, budget=ACTIVATION_BUDGET_BYTES):
        super().__init__(model, device_, budget)
        self.lins = [lin.detach().float().contiguous().to(self.dev) for lin in model.lins]

    def _chunk(self, xs, ys):
        out = torch.zeros(len(xs), dtype=torch.float64, device=self.dev)
        self._trunk(xs, ys, lambda k, x: device.lpips_layer(x, self.lins[k], out))
        return (out,)
