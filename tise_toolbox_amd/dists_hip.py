"""DISTS on MI355X: dists_model.DistsVGG16's definition on the split-precision convolutions.

Per chunk of pairs of ONE size: ``device.dists_image_sums`` (stage 0: the exact integer sums of the bytes), then vgg_pairs_hip's
runner with DISTS's input table, ``device.l2pool3s2_split`` before blocks 2..5 and ``device.dists_layer`` right after each tap.
The integers of stage 0 are read back together with the result; the host forms the three colours' S1 and S2 from them (variance
and covariance numerators in exact integer arithmetic, rounded once) and adds them in fp64.
"""
import numpy as np
import torch

from . import device, dists_model
from .vgg_pairs_hip import ACTIVATION_BUDGET_BYTES, HipVGG16Pairs


def stage0_value(sums, h, w, alpha, beta):
    """(n,3,5) integer sums {bx, by, bx^2, by^2, bx by} of h x w images, alpha and beta of the 3 colours -> (n,) float64: the
    stage-0 part of DISTS with x = b / 255.  The means are correctly rounded quotients of integers; the variance and covariance
    numerators N sum b^2 - (sum b)^2 and N sum bx by - sum bx sum by are exact Python integers, rounded once by the division."""
    npix = int(h) * int(w)
    den = npix * npix * 255 * 255
    out = np.zeros(len(sums), dtype=np.float64)
    for i, pair in enumerate(np.asarray(sums).tolist()):
        total = 0.0
        for c in range(3):
            sx, sy, sxx, syy, sxy = (int(v) for v in pair[c])
            mx, my = sx / (255 * npix), sy / (255 * npix)
            vx, vy, cxy = (npix * sxx - sx * sx) / den, (npix * syy - sy * sy) / den, (npix * sxy - sx * sy) / den
            s1 = (2.0 * mx * my + dists_model.C1) / (mx * mx + my * my + dists_model.C1)
            s2 = (2.0 * cxy + dists_model.C2) / (vx + vy + dists_model.C2)
            total += float(alpha[c]) * (1.0 - s1) + float(beta[c]) * (1.0 - s2)
        out[i] = total
    return out


class HipDists(HipVGG16Pairs):
    name, model_class, takes = "DISTS", dists_model.DistsVGG16, "HipDists takes a dists_model.DistsVGG16"
    pool = staticmethod(device.l2pool3s2_split)

    def __init__(self, model, device_=None, budget=ACTIVATION_BUDGET_BYTES):
        super().__init__(model, device_, budget)
        alpha, beta = model.normalized_weights()                 # fp64, divided by sum alpha + sum beta on the host
        if not bool(torch.isfinite(torch.cat([alpha, beta])).all()):
            raise ValueError("DISTS VGG-16: alpha / beta do not normalise (sum alpha + sum beta is zero or not finite)")
        self.alpha0, self.beta0 = alpha[:3].numpy().copy(), beta[:3].numpy().copy()
        self.alphas, self.betas, at = [], [], 3
        for c in dists_model.STAGE_CHANNELS[1:]:
            self.alphas.append(alpha[at:at + c].contiguous().to(self.dev))
            self.betas.append(beta[at:at + c].contiguous().to(self.dev))
            at += c

    def _chunk(self, xs, ys):
        """-> ((n,) float64: stages 1..5, (n,3,5) int64: the sums of stage 0), both on the device."""
        out = torch.zeros(len(xs), dtype=torch.float64, device=self.dev)
        sums = device.dists_image_sums(xs, ys)
        self._trunk(xs, ys, lambda k, x: device.dists_layer(x, self.alphas[k], self.betas[k], out))
        return out, sums

    def _results(self, n):
        return super()._results(n) + [torch.zeros((n, 3, 5), dtype=torch.int64, device=self.dev)]

    def _value(self, host, chunks):
        value, ints = host                                       # the integers of stage 0 come back with the result
        for part, xp, _ in chunks:
            value[part] = stage0_value(ints[part], xp[0].shape[0], xp[0].shape[1], self.alpha0, self.beta0) + value[part]
        return value
