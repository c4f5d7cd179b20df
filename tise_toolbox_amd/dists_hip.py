"""DISTS on MI355X: dists_model.DistsVGG16's definition on the split-precision convolutions.

Per chunk of pairs of ONE size: ``device.dists_image_sums`` (stage 0: the exact integer sums of the bytes),
``device.lpips_input_split`` with DISTS's table (bytes -> the 32-channel split tensor of both sides, 2n images), thirteen
``SplitConv`` launches (lpips_hip.vgg_convs: conv1_1 as a 32-channel layer with 29 zero weight columns, kernel choice left to
"auto"), ``device.l2pool3s2_split`` before blocks 2..5, and ``device.dists_layer`` right after each tap, so that a tap is freed
before the next block runs.  The integers of stage 0 are read back together with the result; the host forms the three colours' S1
and S2 from them (variance and covariance numerators in exact integer arithmetic, rounded once) and adds them in fp64.  The range
guard of the split format is read once per call.  There is no CPU path and no library convolution.

A pair's bits do not depend on its group, chunk or position: every convolution output element is a fixed-order sum over K, the
pools and the head work per image resp. per pair, and the head's workgroup cut depends on the stage's size only.
"""
import numpy as np
import torch

from . import device, dists_model
from .lpips_hip import ACTIVATION_BUDGET_BYTES, chunks_by_size, vgg_convs


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


class HipDists:
    def __init__(self, model, device_=None, budget=ACTIVATION_BUDGET_BYTES):
        from .engine import require_gpu
        require_gpu()
        if not isinstance(model, dists_model.DistsVGG16):
            raise TypeError("HipDists takes a dists_model.DistsVGG16")
        self.dev = torch.device(device_) if device_ is not None else torch.device("cuda", torch.cuda.current_device())
        self.budget = int(budget)
        self.synthetic = bool(model.synthetic)
        flat = torch.cat([p.detach().float().reshape(-1) for p in model.parameters()] + [model.table.detach().float().reshape(-1)])
        if not bool(torch.isfinite(flat).all()):                 # one check for all layers (SplitConv check=False below)
            raise ValueError("DISTS VGG-16: non-finite value (NaN or Inf) in the parameters")
        if float(model.table.abs().max()) > 65504.0:
            raise ValueError("DISTS VGG-16: the input table leaves the fp16 range of the split format")
        self.table = model.table.detach().float().contiguous().to(self.dev)
        self.convs = vgg_convs(model.convs, self.dev)
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
        """n pairs of one size (two lists of (H,W,3) uint8 device tensors, or two (n,H,W,3) tensors) -> ((n,) float64: stages 1..5,
        (n,3,5) int64: the sums of stage 0), both on the device."""
        n = len(xs)
        out = torch.zeros(n, dtype=torch.float64, device=self.dev)
        sums = device.dists_image_sums(xs, ys)
        x = device.lpips_input_split(xs, ys, self.table)
        tap = 0
        for k, conv in enumerate(self.convs):
            if k in dists_model.POOL_BEFORE:
                x = device.l2pool3s2_split(x)
            m, h, w, _ = x.shape
            y = torch.empty((m, h, w, 2 * conv.cout), dtype=torch.float16, device=self.dev)
            conv(x, [(0, conv.cout, y, 0, 0)])
            x = y
            if k in dists_model.TAP_AFTER:
                device.dists_layer(x, self.alphas[tap], self.betas[tap], out)
                tap += 1
        return out, sums

    def __call__(self, xs, ys):
        """Two (N,H,W,3) uint8 device tensors or two lists of (H_i,W_i,3) uint8 device tensors (pair by pair one size, every side
        >= 16) -> (N,) float64 numpy array.  Raises FloatingPointError when an activation left the fp16 range of the split format."""
        n, chunks = chunks_by_size(xs, ys, dists_model.check_size, "DISTS", self.budget)
        res = torch.zeros(n, dtype=torch.float64, device=self.dev)
        ints = torch.zeros((n, 3, 5), dtype=torch.int64, device=self.dev)
        for part, xp, yp in chunks:
            where = torch.as_tensor(part, device=self.dev)
            res[where], ints[where] = self._chunk(xp, yp)
        if n and device.read_split_overflow():
            raise FloatingPointError("DISTS VGG-16 trunk: an activation exceeded the fp16 range of the split-precision format "
                                     "(|v| > 65504); the result is not usable")
        value, ints = res.cpu().numpy(), ints.cpu().numpy()         # the integers of stage 0 come back with the result
        for part, xp, _ in chunks:
            value[part] = stage0_value(ints[part], xp[0].shape[0], xp[0].shape[1], self.alpha0, self.beta0) + value[part]
        return value
