"""LPIPS (VGG-16) on MI355X: lpips_model.LpipsVGG16's definition on the split-precision convolutions.

Per chunk of pairs of ONE size: ``device.lpips_input_split`` (bytes -> the 32-channel split tensor of both sides, 2n images),
thirteen ``SplitConv`` launches (conv1_1 as a 32-channel layer with 29 zero weight columns; kernel choice left to "auto": the
row-window kernel where its window fits and its row-length reciprocal is exact, the default kernel elsewhere -- conv_split.py),
``device.maxpool2s2_split`` after blocks 1..4, and ``device.lpips_layer`` right after each tap, so that a tap is freed before the
next block runs.  The range guard of the split format is read once per call.  There is no CPU path and no library convolution.

A pair's bits do not depend on its group, chunk or position: every convolution output element is a fixed-order sum over K, the
pools and the head work per image resp. per pair, and the head's workgroup cut depends on the tap's size only.
"""
import numpy as np
import torch

from . import device, lpips_model
from .conv_split import SplitConv

# Bytes the LARGEST activation of a chunk may take: conv1_1's / conv1_2's output, (2n, H, W, 64) split = 512 n H W bytes (two of
# them and the 256 n H W byte input are alive at once).  2 GiB: 64 pairs of 256 x 256 per chunk.
ACTIVATION_BUDGET_BYTES = 2 << 30


def pairs_per_chunk(h, w, budget=ACTIVATION_BUDGET_BYTES):
    return int(max(1, min(device.LPIPS_MAX_PAIRS, budget // (512 * int(h) * int(w)))))


def vgg_convs(convs, dev):
    """The thirteen convolutions of a torch VGG-16 trunk as ``SplitConv``s left to "auto"; conv1_1 becomes a 32-channel layer with 29
    zero weight columns.  The caller has checked the parameters (check=False)."""
    out = []
    for k, conv in enumerate(convs):
        w, b = conv.weight.detach().float(), conv.bias.detach().float()
        if k == 0:                                           # conv1_1 as a 32-channel layer: 29 zero weight columns
            w = torch.cat([w, torch.zeros((w.shape[0], 29, 3, 3), dtype=w.dtype)], 1)
        out.append(SplitConv(w, b, (1, 1), (1, 1), dev, name=f"features.{lpips_model.CONV_INDICES[k]}", check=False))
    return out


def chunks_by_size(xs, ys, check_size, what, budget):
    """Two (N,H,W,3) uint8 device tensors or two lists of (H_i,W_i,3) uint8 device tensors -> (N, [(indices, x side, y side), ..]):
    the pairs grouped by size and every group cut under the activation budget; a side of a chunk is a slice of the stacked
    tensor where the chunk is contiguous in it, else a list.  Wrong dtypes, shapes and sizes raise before anything is enqueued."""
    stacked = isinstance(xs, torch.Tensor) and isinstance(ys, torch.Tensor) and xs.dim() == 4 and ys.dim() == 4
    if stacked:
        if xs.shape != ys.shape:
            raise ValueError(f"two (N,H,W,3) batches of one shape (got {tuple(xs.shape)} and {tuple(ys.shape)})")
    else:
        xs = [(c[0] if c.dim() == 4 and c.shape[0] == 1 else c) for c in xs]
        ys = [(c[0] if c.dim() == 4 and c.shape[0] == 1 else c) for c in ys]
        if len(xs) != len(ys):
            raise ValueError(f"{len(xs)} images on side one, {len(ys)} on side two")
    groups = {}
    for i, (a, b) in enumerate(zip(xs, ys)):
        if a.dtype != torch.uint8 or b.dtype != torch.uint8 or a.dim() != 3 or b.dim() != 3 or a.shape[-1] != 3 or b.shape[-1] != 3:
            raise ValueError(f"pair {i} must be two (H,W,3) uint8 images")
        if a.shape != b.shape:
            raise ValueError(f"pair {i} has two sizes ({a.shape[0]} x {a.shape[1]} and {b.shape[0]} x {b.shape[1]})")
        check_size(a.shape[0], a.shape[1], f"{what}: pair {i}")
        groups.setdefault((a.shape[0], a.shape[1]), []).append(i)
    chunks = []
    for (h, w), idx in groups.items():
        step = pairs_per_chunk(h, w, budget)
        for at in range(0, len(idx), step):
            part = idx[at:at + step]
            if stacked and part == list(range(part[0], part[0] + len(part))):
                chunks.append((part, xs[part[0]:part[0] + len(part)], ys[part[0]:part[0] + len(part)]))
            else:
                chunks.append((part, [xs[i] for i in part], [ys[i] for i in part]))
    return len(xs), chunks


class HipLpips:
    def __init__(self, model, device_=None, budget=ACTIVATION_BUDGET_BYTES):
        from .engine import require_gpu
        require_gpu()
        if not isinstance(model, lpips_model.LpipsVGG16):
            raise TypeError("HipLpips takes an lpips_model.LpipsVGG16")
        self.dev = torch.device(device_) if device_ is not None else torch.device("cuda", torch.cuda.current_device())
        self.budget = int(budget)
        self.synthetic = bool(model.synthetic)
        params = [p.detach().float().reshape(-1) for p in model.parameters()] + [model.table.detach().float().reshape(-1)]
        flat = torch.cat(params)
        if not bool(torch.isfinite(flat).all()):                 # one check for all layers (SplitConv check=False below)
            raise ValueError("LPIPS VGG-16: non-finite value (NaN or Inf) in the parameters")
        if float(model.table.abs().max()) > 65504.0:
            raise ValueError("LPIPS VGG-16: the input table leaves the fp16 range of the split format")
        self.table = model.table.detach().float().contiguous().to(self.dev)
        self.convs = vgg_convs(model.convs, self.dev)
        self.lins = [lin.detach().float().contiguous().to(self.dev) for lin in model.lins]

    def _chunk(self, xs, ys):
        """n pairs of one size (two lists of (H,W,3) uint8 device tensors, or two (n,H,W,3) tensors) -> (n,) float64 on the device."""
        n = len(xs)
        out = torch.zeros(n, dtype=torch.float64, device=self.dev)
        x = device.lpips_input_split(xs, ys, self.table)
        tap = 0
        for k, conv in enumerate(self.convs):
            if k in lpips_model.POOL_BEFORE:
                x = device.maxpool2s2_split(x)
            m, h, w, _ = x.shape
            y = torch.empty((m, h, w, 2 * conv.cout), dtype=torch.float16, device=self.dev)
            conv(x, [(0, conv.cout, y, 0, 0)])
            x = y
            if k in lpips_model.TAP_AFTER:
                device.lpips_layer(x, self.lins[tap], out)
                tap += 1
        return out

    def __call__(self, xs, ys):
        """Two (N,H,W,3) uint8 device tensors or two lists of (H_i,W_i,3) uint8 device tensors (pair by pair one size, every side
        >= 16) -> (N,) float64 numpy array.  Raises FloatingPointError when an activation left the fp16 range of the split format."""
        n, chunks = chunks_by_size(xs, ys, lpips_model.check_size, "LPIPS", self.budget)
        res = torch.zeros(n, dtype=torch.float64, device=self.dev)
        for part, xp, yp in chunks:
            res[torch.as_tensor(part, device=self.dev)] = self._chunk(xp, yp)
        if n and device.read_split_overflow():
            raise FloatingPointError("LPIPS VGG-16 trunk: an activation exceeded the fp16 range of the split-precision format "
                                     "(|v| > 65504); the result is not usable")
        return res.cpu().numpy()
