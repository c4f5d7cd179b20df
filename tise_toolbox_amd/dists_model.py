"""DISTS with the VGG-16 trunk as a plain torch module: the definition the HIP route (dists_hip.py) is compared against, the
parameter loaders and the seeded stand-in parameters.

DEFINITION (restated from Ding, Ma, Wang & Simoncelli 2020, "Image Quality Assessment: Unifying Structure and Texture Similarity",
and the ``DISTS_pytorch`` package from memory; the package is not installed here and nothing of it is this file's source -- parity
with its numbers is UNPINNED, see README).

  images   8-bit RGB as the feeds decode them; both images of a pair have one size, H and W >= 16 (the route is pinned from 16 up,
           like LPIPS).  No resize.
  stage 0  the image itself, x = b / 255 in the module's dtype: 3 channels.
  input    (x - mean_c) / std_c with mean = (0.485, 0.456, 0.406), std = (0.229, 0.224, 0.225), computed in fp32 from fp32(b / 255)
           and tabulated: ``input_table()`` is the (3, 256) table every route, the fp64 module included, reads.
  network  torchvision VGG-16 ``features``: the thirteen 3 x 3 / stride 1 / padding 1 convolutions of vgg_pairs.CONV_INDICES, each
           followed by ReLU; each of the four max-pools replaced by the L2 pool y = sqrt(conv(x^2, g, stride 2, padding 1,
           depthwise) + 1e-12), g = a a^T / sum with a = (0.5, 1, 0.5), zero padding: the output is ceil(H/2) x ceil(W/2).
  taps     relu1_2, relu2_2, relu3_3, relu4_3, relu5_3; channels of the six stages 3, 64, 128, 256, 512, 512 = 1475.
  head     per stage, pair and channel over the pixels: mx, my the means, vx, vy = mean (x - mx)^2, cxy = mean (x - mx)(y - my);
           S1 = (2 mx my + c1) / (mx^2 + my^2 + c1), S2 = (2 cxy + c2) / (vx + vy + c2), c1 = c2 = 1e-6.
  score    alpha, beta (1, 1475, 1, 1), divided by (sum alpha + sum beta) in fp64; DISTS = sum over stages and channels of
           alpha_c (1 - S1_c) + beta_c (1 - S2_c) -- the package's 1 - (sum alpha S1 + sum beta S2) written so that nothing cancels:
           an identical pair is exactly 0.0.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .vgg_pairs import (CONV_CHANNELS, CONV_INDICES, MIN_SIDE, POOL_BEFORE, TAP_AFTER, VGG16Pairs, default_weights_path,  # noqa: F401
                        named_source)

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
C1 = C2 = 1e-6
POOL_EPS = 1e-12
POOL_TAPS = (0.25, 0.5, 0.25)                                               # a / sum(a), a = (0.5, 1, 0.5): g = a a^T / sum
STAGE_CHANNELS = (3, 64, 128, 256, 512, 512)
N_CHANNELS = sum(STAGE_CHANNELS)                                            # 1475


def input_table():
    """(3, 256) float32: table[c][b] = (fp32(b / 255) - mean_c) / std_c, every step in fp32."""
    x = np.arange(256, dtype=np.float32) / np.float32(255.0)
    t = (x[None, :] - np.asarray(MEAN, dtype=np.float32)[:, None]) / np.asarray(STD, dtype=np.float32)[:, None]
    return torch.from_numpy(np.ascontiguousarray(t.astype(np.float32)))


def check_size(h, w, what="DISTS"):
    if min(int(h), int(w)) < MIN_SIDE:
        raise ValueError(f"{what} needs both sides >= {MIN_SIDE} (the route is pinned from {MIN_SIDE} up, like LPIPS): "
                         f"got {int(h)} x {int(w)}")


def pooled_size(s):
    """The side after one L2 pool: ceil(s / 2)."""
    return (int(s) + 1) // 2


def l2pool(x):
    """(N,C,H,W) -> (N,C,ceil(H/2),ceil(W/2)): sqrt(conv(x^2, g, stride 2, padding 1, depthwise) + 1e-12).  The depthwise
    convolution is written out as its nine weighted, strided slices of the zero-padded squares, added in row-major tap order: a
    sum of non-negative terms in every dtype and on every backend (a library convolution that goes through a transform can
    return a small negative sum where the map is zero, and the square root of that is NaN)."""
    oh, ow = pooled_size(x.shape[2]), pooled_size(x.shape[3])
    sq = F.pad(x * x, (1, 2 * ow - x.shape[3], 1, 2 * oh - x.shape[2]))        # (N,C,2 oh + 1,2 ow + 1)
    acc = None
    for dh in range(3):
        for dw in range(3):
            term = sq[:, :, dh:dh + 2 * oh:2, dw:dw + 2 * ow:2] * (POOL_TAPS[dh] * POOL_TAPS[dw])
            acc = term if acc is None else acc + term
    return (acc + POOL_EPS).sqrt()


def stage_terms(x, y):
    """Two (N,C,h,w) stage tensors -> (S1, S2), each (N,C)."""
    mx, my = x.mean((2, 3), keepdim=True), y.mean((2, 3), keepdim=True)
    dx, dy = x - mx, y - my
    vx, vy, cxy = (dx * dx).mean((2, 3)), (dy * dy).mean((2, 3)), (dx * dy).mean((2, 3))
    mx, my = mx[:, :, 0, 0], my[:, :, 0, 0]
    s1 = (2 * mx * my + C1) / (mx * mx + my * my + C1)
    s2 = (2 * cxy + C2) / (vx + vy + C2)
    return s1, s2


class DistsVGG16(VGG16Pairs):
    """The definition above in plain torch.  ``forward(a, b)``: two (N,H,W,3) uint8 tensors -> (N,) DISTS in the module's dtype
    (fp32 as built, fp64 after ``.double()``)."""
    check_size = staticmethod(check_size)

    def __init__(self):
        super().__init__(input_table())
        self.alpha = nn.Parameter(torch.full((1, N_CHANNELS, 1, 1), 0.1), requires_grad=False)
        self.beta = nn.Parameter(torch.full((1, N_CHANNELS, 1, 1), 0.1), requires_grad=False)
        self.freeze()

    # ---- parameters --------------------------------------------------------------------------------------------------
    def load_dists_weights(self, source):
        """The package's parameter file (keys ``alpha`` and ``beta``, each (1, 1475, 1, 1)) or its dict.  Any other shape is
        refused, naming both."""
        path, sd = named_source(source)
        want = (1, N_CHANNELS, 1, 1)
        for key in ("alpha", "beta"):
            got = tuple(sd[key].shape) if key in sd and hasattr(sd[key], "shape") else None
            if got != want:
                raise ValueError(f"{path}: {key} is {got if got else 'missing'}, DISTS on VGG-16 has {want} "
                                 f"(3 + 64 + 128 + 256 + 512 + 512 channels): this loader takes the DISTS_pytorch package's weights.pt")
        self.alpha.copy_(sd["alpha"].to(self.alpha.dtype))
        self.beta.copy_(sd["beta"].to(self.beta.dtype))
        return self

    def init_synthetic(self, seed=0):
        """Seeded stand-in parameters (weights.py's rules: plumbing and throughput runs only, result lines are tagged):
        He-scaled normal convolutions and small normal biases as LPIPS's stand-ins, alpha and beta = |N(0.1, 0.01)|."""
        g = torch.Generator().manual_seed(int(seed))
        self.init_synthetic_trunk(g)
        for p in (self.alpha, self.beta):
            p.copy_((0.1 + 0.01 * torch.randn(p.shape, generator=g, dtype=torch.float64)).abs().to(p.dtype))
        return self

    def normalized_weights(self):
        """(alpha, beta) / (sum alpha + sum beta), two (1475,) float64 tensors: formed in fp64 on the host."""
        a, b = self.alpha.detach().double().reshape(-1), self.beta.detach().double().reshape(-1)
        total = a.sum() + b.sum()
        return a / total, b / total

    # ---- arithmetic --------------------------------------------------------------------------------------------------
    def prepare(self, img):
        """(N,H,W,3) uint8 -> (stage 0 (N,3,H,W) = b / 255, the network input (N,3,H,W): the table look-up), module's dtype."""
        idx, x = self.table_lookup(img)
        return idx.to(self.dtype) / 255, x

    def stages(self, img, amax=None):
        """(N,H,W,3) uint8 -> the six stage tensors.  ``amax``: a list that receives the largest |activation| of every convolution."""
        x0, x = self.prepare(img)
        return [x0] + self.features(x, l2pool, amax)

    def similarities(self, a, b, amax=None):
        """-> (S1, S2, alpha, beta): S (N,1475) in the module's dtype, the normalised weights (1475,) in the module's dtype."""
        self.check_pair(a, b)
        n = a.shape[0]
        st = self.stages(torch.cat([a, b], 0), amax)
        terms = [stage_terms(t[:n], t[n:]) for t in st]
        al, be = (w.to(self.dtype) for w in self.normalized_weights())
        return torch.cat([t[0] for t in terms], 1), torch.cat([t[1] for t in terms], 1), al, be

    def forward(self, a, b, amax=None):
        s1, s2, al, be = self.similarities(a, b, amax)
        total, at = None, 0
        for c in STAGE_CHANNELS:                                             # stage by stage, as the device adds them
            v = (al[at:at + c] * (1 - s1[:, at:at + c]) + be[at:at + c] * (1 - s2[:, at:at + c])).sum(1)
            total = v if total is None else total + v
            at += c
        return total

    def forward_package_form(self, a, b):
        """1 - (sum alpha S1 + sum beta S2): the package's form, which cancels near 0 (kept for the comparison in the tests)."""
        s1, s2, al, be = self.similarities(a, b)
        return 1 - ((al * s1).sum(1) + (be * s2).sum(1))


def build_model(weights=None, dists_weights=None, synthetic=False, seed=0):
    """DistsVGG16 from the two files, or seeded stand-ins under ``synthetic`` (never silently)."""
    model = DistsVGG16()
    if synthetic:
        if weights or dists_weights:
            raise RuntimeError("--synthetic-weights and --weights / --dists-weights are mutually exclusive")
        return model.init_synthetic(seed)
    if not weights or not dists_weights:
        raise RuntimeError("DISTS needs two files: the VGG-16 trunk (--weights, torchvision's vgg16-397923af.pth) and alpha / beta "
                           "(--dists-weights, the DISTS_pytorch package's weights.pt); or --synthetic-weights for a plumbing run")
    return model.load_trunk(weights).load_dists_weights(dists_weights)
