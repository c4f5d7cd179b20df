"""ResNet-50 on MI355X: the trunk of FD-SwAV (fd_swav.py) on the split-precision convolutions.

``HipResNet50(model)`` takes a ``resnet_model.ResNet50`` (real parameters or the seeded stand-ins) and offers
``features_from_u8((n, H, W, 3) uint8) -> (n, 2048) fp32``.  Per chunk of images under an activation budget:

  stem    ``device.stem_conv7x7s2_split_u8`` (csrc/conv_pipe.hip, stem7_mfma_u8_kernel): 7 x 7 / stride 2 / zero padding 3 on the
          matrix cores straight from the bytes, K = 7 x 32; or route "padded" (below)
  pool    ``device.maxpool3s2p1_split`` (csrc/resnet.hip)
  blocks  sixteen bottlenecks: conv1 and conv2 as ``SplitConv`` mode 0 (BatchNorm folded, ReLU in the epilogue, kernel choice left
          to "auto"), conv3 -- and the downsample convolution where there is one -- as ``SplitConv`` mode 1 into fp32 (scale *
          conv, no bias), then ``device.residual_relu_split``: split(max((raw + bias) + identity, 0))
  mean    ``tise_split_mean_nhwc``

Nothing inside a call waits for the device; the range guard of the split format is read once per call and raises
``FloatingPointError``.  There is no CPU path and no library convolution.  A row's bits do not depend on its chunk or position:
every convolution output element is a fixed-order sum over K and every other kernel works per pixel.

Route "padded" (``TISE_RESNET_STEM=padded``, and wherever the matrix-core stem refuses a batch): ``device.resnet_input_split``
writes the table values as a 32-channel split tensor and conv1 runs as a 32-channel ``SplitConv`` with 29 zero weight columns, as
LPIPS's conv1_1 does -- 1.26 GMAC for 118 MMAC of work at 224 x 224.  It is the stem the tests compare the matrix-core stem
against, and the other side of the A/B (tools/resnet_probe.py).

``TISE_RESNET=torch`` (``build_tower``) runs the fp32 module itself on library kernels: the A/B route.
"""
import ctypes
import os

import torch

from . import _lib, device, resnet_model
from .conv_split import SplitConv, split_planes

# Bytes the activations of a chunk may take.  The widest moment of an image is layer1's first block: conv3's and the downsample's
# fp32 results and the block's output, 3 x (H/4)(W/4) x 256 x 4 = 192 H W bytes, next to route "padded"'s 128 H W byte input:
# 256 H W bytes per image are budgeted.  2 GiB: 167 images of 224 x 224 per chunk.
ACTIVATION_BUDGET_BYTES = 2 << 30
BYTES_PER_PIXEL = 256
MAX_IMAGES = 65535                                                          # tise_split_mean_nhwc's grid
STEMS = ("mfma", "padded")
DEFAULT_STEM = "mfma"


def images_per_chunk(h, w, budget=ACTIVATION_BUDGET_BYTES):
    return int(max(1, min(MAX_IMAGES, int(budget) // (BYTES_PER_PIXEL * int(h) * int(w)))))


def pack_stem7_mfma(w, dev):
    """BatchNorm-folded stem weights (64, 3, 7, 7) [cout][cin][kh][kw] -> (28672 fp16 in the order of stem7_mfma_u8_kernel, fp32 (64,)
    un-scaling).  Per cout a power-of-two pre-scale keeps both halves normal fp16 (as conv_split.SplitConv: frexp, exact).  K =
    7 filter rows x 32 slots, slot s < 21 = tap (kw = s // 3, c = s % 3), slots 21..31 zero; the fragment order is
    [kh][s2][plane hi / lo][cout tile t][lane][j] with cout = 32 t + lane % 32 and s = 16 s2 + 8 (lane // 32) + j."""
    w = w.detach().float().cpu()
    assert tuple(w.shape) == (64, 3, 7, 7)
    amax = w.abs().reshape(64, -1).amax(1).clamp_min(1e-30)
    _, ex = torch.frexp(amax)
    pre = torch.ldexp(torch.ones_like(amax), 1 - ex)                        # max |w pre| in [1, 2)
    wk = torch.zeros((64, 7, 32), dtype=torch.float32)
    wk[:, :, :21] = (w * pre.view(-1, 1, 1, 1)).permute(0, 2, 3, 1).reshape(64, 7, 21)      # [cout][kh][3 kw + c]
    planes = split_planes(wk)                                               # (2, 64, 7, 32)
    frag = planes.reshape(2, 2, 32, 7, 2, 2, 8)                             # [plane][t][cout % 32][kh][s2][half][j]
    frag = frag.permute(3, 4, 0, 1, 5, 2, 6).contiguous()                   # [kh][s2][plane][t][half][cout % 32][j]
    return frag.reshape(-1).to(dev).contiguous(), torch.ldexp(torch.ones_like(amax), ex - 1).to(dev).contiguous()


class _Block:
    def __init__(self, name, blk, folded, dev):
        conv = lambda part, stride, pad: SplitConv(*folded[f"{name}.{part}"], (stride, stride), (pad, pad), dev, name=f"{name}.{part}",
                                                   check=False)
        self.conv1 = conv("conv1", 1, 0)
        self.conv2 = conv("conv2", blk.stride, 1)
        self.conv3 = conv("conv3", 1, 0)
        self.down = conv("downsample.0", blk.stride, 0) if blk.downsample is not None else None

    def __call__(self, x):
        """x: split tensor (n, h, w, 2 Cin) -> split tensor (n, h', w', 2 Cout)."""
        dev = x.device
        n, h, w, _ = x.shape
        a = torch.empty((n, h, w, 2 * self.conv1.cout), dtype=torch.float16, device=dev)
        self.conv1(x, [(0, self.conv1.cout, a, 0, 0)])
        oh, ow = self.conv2.out_hw(h, w)
        b = torch.empty((n, oh, ow, 2 * self.conv2.cout), dtype=torch.float16, device=dev)
        self.conv2(a, [(0, self.conv2.cout, b, 0, 0)])
        c = self.conv3.cout
        raw = torch.empty((n, oh, ow, c), dtype=torch.float32, device=dev)
        self.conv3(b, [(0, c, raw, 0, 1)])
        if self.down is None:
            return device.residual_relu_split(raw, self.conv3.bias[:c], x)
        idr = torch.empty((n, oh, ow, c), dtype=torch.float32, device=dev)
        self.down(x, [(0, c, idr, 0, 1)])
        return device.residual_relu_split(raw, self.conv3.bias[:c], idr, self.down.bias[:c])


class HipResNet50:
    resolution = 224                                                        # what fd_swav resizes to; any size >= 32 is taken

    def __init__(self, model, device_=None, budget=ACTIVATION_BUDGET_BYTES, stem=None):
        from .engine import require_gpu
        require_gpu()
        if not isinstance(model, resnet_model.ResNet50):
            raise TypeError("HipResNet50 takes a resnet_model.ResNet50")
        self.dev = torch.device(device_) if device_ is not None else torch.device("cuda", torch.cuda.current_device())
        self.budget = int(budget)
        self.synthetic = bool(model.synthetic)
        self.out_dim = model.out_dim
        stem = stem or os.environ.get("TISE_RESNET_STEM", DEFAULT_STEM)
        if stem not in STEMS:
            raise ValueError(f"TISE_RESNET_STEM={stem!r}: one of {STEMS}")
        self.stem = stem
        folded = model.folded()
        table = model.table.detach().float().cpu()
        flat = torch.cat([t.reshape(-1) for wb in folded.values() for t in wb] + [table.reshape(-1)])
        if not bool(torch.isfinite(flat).all()):                            # one check for all layers (SplitConv check=False below)
            raise ValueError("ResNet-50: non-finite value (NaN or Inf) in the BatchNorm-folded parameters or the input table")
        if float(table.abs().max()) > 65504.0:
            raise ValueError("ResNet-50: the input table leaves the fp16 range of the split format")
        self.table = table.contiguous().to(self.dev)
        w1, b1 = folded["conv1"]
        self.stem_w, self.stem_scale = pack_stem7_mfma(w1, self.dev)
        self.stem_bias = b1.to(self.dev).contiguous()
        self._stem_params = (w1, b1)
        self._stem_padded = None                                            # built on first use
        self.blocks = [_Block(name, blk, folded, self.dev) for name, blk in model.blocks()]
        self.last_stem = None                                               # the route the last chunk's stem took

    def _padded_stem(self):
        if self._stem_padded is None:
            w1, b1 = self._stem_params                                      # conv1 as a 32-channel layer: 29 zero weight columns
            w32 = torch.cat([w1, torch.zeros((64, 29, 7, 7), dtype=w1.dtype)], 1)
            self._stem_padded = SplitConv(w32, b1, (2, 2), (3, 3), self.dev, name="conv1", check=False)
        return self._stem_padded

    def stem_forward(self, u8):
        """A dense (n, H, W, 3) uint8 device batch -> conv1 + bn1 + ReLU as a split tensor (n, H', W', 128)."""
        if self.stem == "mfma" and device.stem_conv7x7s2_supported(u8):
            self.last_stem = "mfma"
            return device.stem_conv7x7s2_split_u8(u8, self.table, self.stem_w, self.stem_scale, self.stem_bias)
        self.last_stem = "padded"
        conv = self._padded_stem()
        x = device.resnet_input_split(u8, self.table)
        n, h, w, _ = x.shape
        oh, ow = conv.out_hw(h, w)
        y = torch.empty((n, oh, ow, 128), dtype=torch.float16, device=self.dev)
        conv(x, [(0, 64, y, 0, 0)])
        return y

    def _chunk_map(self, u8):
        x = device.maxpool3s2p1_split(self.stem_forward(u8))
        for blk in self.blocks:
            x = blk(x)
        return x

    def _chunk(self, u8):
        x = self._chunk_map(u8)
        n, h, w, c2 = x.shape
        out = torch.empty((n, c2 // 2), dtype=torch.float32, device=self.dev)
        _lib.call("tise_split_mean_nhwc", device._ptr(x), n, h * w, c2 // 2, device._ptr(out),
                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        return out

    def _check_batch(self, batch):
        if not isinstance(batch, torch.Tensor) or batch.dtype != torch.uint8 or batch.dim() != 4 or batch.shape[3] != 3:
            raise ValueError(f"HipResNet50 takes a (n, H, W, 3) uint8 batch (got {tuple(getattr(batch, 'shape', ()))} "
                             f"{getattr(batch, 'dtype', type(batch).__name__)})")
        if not batch.is_cuda:
            raise _lib.TiseLibraryError("HipResNet50 runs on MI355X only: the batch is not on a HIP device")
        n, h, w, _ = batch.shape
        resnet_model.check_size(h, w)
        return n, h, w

    def _guard(self, n):
        if n and device.read_split_overflow():
            raise FloatingPointError("ResNet-50 trunk: an activation exceeded the fp16 range of the split-precision format "
                                     "(|v| > 65504); the result is not usable")

    @torch.no_grad()
    def features_from_u8(self, batch):
        """(n, H, W, 3) uint8 device batch of one size, H and W >= 32 -> (n, 2048) fp32.  Raises FloatingPointError when an
        activation left the fp16 range of the split format."""
        n, h, w = self._check_batch(batch)
        out = torch.empty((n, self.out_dim), dtype=torch.float32, device=self.dev)
        step = images_per_chunk(h, w, self.budget)
        for at in range(0, n, step):
            out[at:at + step] = self._chunk(batch[at:at + step].contiguous())
        self._guard(n)
        return out

    @torch.no_grad()
    def map_from_u8(self, batch):
        """(n, H, W, 3) uint8 device batch of one size, H and W >= 32 -> the last map as a split tensor (n, h, w, 4096), (h, w) =
        resnet_model.output_hw(H, W): features_from_u8 without the mean (the trunk used fully convolutionally: countseg_hip.py), with
        its chunking, budget and guard."""
        n, h, w = self._check_batch(batch)
        oh, ow = resnet_model.output_hw(h, w)
        step = images_per_chunk(h, w, self.budget)
        if 0 < n <= step:                                                   # one chunk: its map is the result
            out = self._chunk_map(batch.contiguous())
        else:
            out = torch.empty((n, oh, ow, 2 * self.out_dim), dtype=torch.float16, device=self.dev)
            for at in range(0, n, step):
                out[at:at + step] = self._chunk_map(batch[at:at + step].contiguous())
        self._guard(n)
        return out


class TorchResNet50:
    """``TISE_RESNET=torch``: the fp32 module itself on library kernels, with HipResNet50's interface.  ``autocast``: under
    torch.autocast(fp16) (tools/resnet_probe.py's third side)."""
    resolution = 224

    def __init__(self, model, device_, autocast=False):
        self.model = model.to(device_).float().eval()
        self.dev = torch.device(device_)
        self.synthetic, self.out_dim, self.autocast = bool(model.synthetic), model.out_dim, bool(autocast)

    @torch.no_grad()
    def features_from_u8(self, batch):
        if self.autocast:
            with torch.autocast("cuda", dtype=torch.float16):
                return self.model(batch.to(self.dev)).float()
        return self.model(batch.to(self.dev)).float()


def build_tower(weights, dev, seed=0):
    """The tower the CLI runs: HipResNet50 over resnet_model.build_model, or TorchResNet50 with TISE_RESNET=torch.
    ``weights=None``: seeded stand-ins (the CLI only allows that behind --synthetic-weights)."""
    model = resnet_model.build_model(weights, synthetic=not weights, seed=seed)
    route = os.environ.get("TISE_RESNET", "hip")
    if route == "torch":
        return TorchResNet50(model, dev)
    if route != "hip":
        raise ValueError(f"TISE_RESNET={route!r}: 'hip' (default) or 'torch'")
    return HipResNet50(model, dev)
