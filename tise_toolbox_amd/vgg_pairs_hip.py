"""The VGG-16 pair metrics on MI355X: what lpips_hip.HipLpips and dists_hip.HipDists share, on the split-precision convolutions.

Per chunk of pairs of ONE size: ``device.lpips_input_split`` with the metric's table (bytes -> the 32-channel split tensor of both
sides, 2n images), thirteen ``SplitConv`` launches (conv1_1 as a 32-channel layer with 29 zero weight columns; kernel choice left
to "auto": the row-window kernel where its window fits and its row-length reciprocal is exact, the default kernel elsewhere --
conv_split.py), the metric's pool before blocks 2..5, and the metric's head right after each tap, so that a tap is freed before
the next block runs.  Nothing inside a chunk waits for the device; the range guard of the split format is read once per call.
There is no CPU path and no library convolution.

A pair's bits do not depend on its group, chunk or position: every convolution output element is a fixed-order sum over K, the
pools and the heads work per image resp. per pair, and a head's workgroup cut depends on the tap's size only.
"""
import torch

from . import device, vgg_pairs
from .conv_split import SplitConv

# Bytes the LARGEST activation of a chunk may take: conv1_1's / conv1_2's output, (2n, H, W, 64) split = 512 n H W bytes (two of
# them and the 256 n H W byte input are alive at once).  2 GiB: 64 pairs of 256 x 256 per chunk.
ACTIVATION_BUDGET_BYTES = 2 << 30
MAX_PAIRS = min(device.LPIPS_MAX_PAIRS, device.DISTS_MAX_PAIRS)           # a chunk goes through launches of both files


def pairs_per_chunk(h, w, budget=ACTIVATION_BUDGET_BYTES):
    return int(max(1, min(MAX_PAIRS, budget // (512 * int(h) * int(w)))))


def vgg_convs(convs, dev):
    """The thirteen convolutions of a torch VGG-16 trunk as ``SplitConv``s left to "auto"; conv1_1 becomes a 32-channel layer with 29
    zero weight columns.  The caller has checked the parameters (check=False)."""
    out = []
    for k, conv in enumerate(convs):
        w, b = conv.weight.detach().float(), conv.bias.detach().float()
        if k == 0:                                           # conv1_1 as a 32-channel layer: 29 zero weight columns
            w = torch.cat([w, torch.zeros((w.shape[0], 29, 3, 3), dtype=w.dtype)], 1)
        out.append(SplitConv(w, b, (1, 1), (1, 1), dev, name=f"features.{vgg_pairs.CONV_INDICES[k]}", check=False))
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


class HipVGG16Pairs:
    """A metric sets ``name`` ("LPIPS"), ``model_class``, ``takes`` (the TypeError's text) and ``pool`` (a ``device`` function), and
    writes ``_chunk``: n pairs of one size -> the chunk's device tensors, (n,) float64 first, through ``_trunk``."""

    def __init__(self, model, device_=None, budget=ACTIVATION_BUDGET_BYTES):
        from .engine import require_gpu
        require_gpu()
        if not isinstance(model, self.model_class):
            raise TypeError(self.takes)
        self.dev = torch.device(device_) if device_ is not None else torch.device("cuda", torch.cuda.current_device())
        self.budget = int(budget)
        self.synthetic = bool(model.synthetic)
        flat = torch.cat([p.detach().float().reshape(-1) for p in model.parameters()] + [model.table.detach().float().reshape(-1)])
        if not bool(torch.isfinite(flat).all()):                 # one check for all layers (SplitConv check=False below)
            raise ValueError(f"{self.name} VGG-16: non-finite value (NaN or Inf) in the parameters")
        if float(model.table.abs().max()) > 65504.0:
            raise ValueError(f"{self.name} VGG-16: the input table leaves the fp16 range of the split format")
        self.table = model.table.detach().float().contiguous().to(self.dev)
        self.convs = vgg_convs(model.convs, self.dev)

    def _trunk(self, xs, ys, on_tap):
        """The trunk on n pairs of one size (two lists of (H,W,3) uint8 device tensors, or two (n,H,W,3) tensors);
        ``on_tap(k, x)`` enqueues the head on tap k, the split tensor (2n,h,w,2C)."""
        x = device.lpips_input_split(xs, ys, self.table)
        tap = 0
        for k, conv in enumerate(self.convs):
            if k in vgg_pairs.POOL_BEFORE:
                x = self.pool(x)
            m, h, w, _ = x.shape
            y = torch.empty((m, h, w, 2 * conv.cout), dtype=torch.float16, device=self.dev)
            conv(x, [(0, conv.cout, y, 0, 0)])
            x = y
            if k in vgg_pairs.TAP_AFTER:
                on_tap(tap, x)
                tap += 1

    def _results(self, n):
        """The device tensors a call's chunks are scattered into, ``_chunk``'s tensors for all n pairs."""
        return [torch.zeros(n, dtype=torch.float64, device=self.dev)]

    def _value(self, host, chunks):
        """``_results``' tensors as numpy arrays, read back after the last chunk -> the (N,) float64 values."""
        return host[0]

    def __call__(self, xs, ys):
        """Two (N,H,W,3) uint8 device tensors or two lists of (H_i,W_i,3) uint8 device tensors (pair by pair one size, every side
        >= 16) -> (N,) float64 numpy array.  Raises FloatingPointError when an activation left the fp16 range of the split format."""
        n, chunks = chunks_by_size(xs, ys, self.model_class.check_size, self.name, self.budget)
        results = self._results(n)
        for part, xp, yp in chunks:
            where = torch.as_tensor(part, device=self.dev)
            for all_pairs, of_chunk in zip(results, self._chunk(xp, yp)):
                all_pairs[where] = of_chunk
        if n and device.read_split_overflow():
            raise FloatingPointError(f"{self.name} VGG-16 trunk: an activation exceeded the fp16 range of the split-precision format "
                                     "(|v| > 65504); the result is not usable")
        return self._value([t.cpu().numpy() for t in results], chunks)
