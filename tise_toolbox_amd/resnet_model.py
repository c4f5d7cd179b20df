"""ResNet-50 as a plain torch module: the definition the HIP route (resnet_hip.py) is compared against, the parameter loaders
and the seeded stand-in parameters.  It is the trunk of FD-SwAV (fd_swav.py).

LAYOUT: torchvision's ``resnet50``, RESTATED FROM MEMORY -- torchvision is not installed here and nothing of it is this file's
source; parity with its numbers is UNPINNED (README).

  conv1    64 x 3 x 7 x 7, stride 2, padding 3, no bias; bn1; ReLU; MaxPool2d(3, stride 2, padding 1)
  layer1-4 3, 4, 6, 3 bottleneck blocks of planes 64, 128, 256, 512: conv1 1 x 1, conv2 3 x 3 padding 1 WITH THE BLOCK'S STRIDE
           (torchvision >= 1.5 and SwAV's own file: stride 2 in the first block of layers 2..4), conv3 1 x 1 to 4 planes; a
           BatchNorm after each, ReLU after bn1 and bn2; ``downsample.0`` / ``.1`` (1 x 1 at the block's stride, BatchNorm) in
           the first block of every layer; out = relu(bn3(conv3) + identity)
  BatchNorm in eval mode, eps 1e-5
  output   the mean over the last map: (n, 2048) in the module's dtype.  There is no ``fc``.

INPUT: (n, H, W, 3) uint8.  The network input is (b / 255 - mean_c) / std_c with the ImageNet constants, computed in fp32 and
tabulated: ``input_table()`` is the (3, 256) table every route, the fp64 module included, reads.  H or W < 32 is refused: five
halvings must leave one pixel, and the route is pinned from 32 up.
"""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
MIN_SIDE = 32
LAYERS = (3, 4, 6, 3)
PLANES = (64, 128, 256, 512)
OUT_DIM = 2048
BN_EPS = 1e-5
NETWORK = "swav-resnet50"
BN3_GAIN = 0.25                              # init_synthetic: keeps the residual stream of the stand-ins inside the fp16 range


def input_table():
    """(3, 256) float32: table[c][b] = (fp32(b / 255) - mean_c) / std_c, every step in fp32."""
    x = np.arange(256, dtype=np.float32) / np.float32(255.0)
    t = (x[None, :] - np.asarray(MEAN, dtype=np.float32)[:, None]) / np.asarray(STD, dtype=np.float32)[:, None]
    return torch.from_numpy(np.ascontiguousarray(t.astype(np.float32)))


def check_size(h, w, what="ResNet-50"):
    if min(int(h), int(w)) < MIN_SIDE:
        raise ValueError(f"{what} needs both sides >= {MIN_SIDE} (five halvings must leave one pixel, and the route is pinned from "
                         f"{MIN_SIDE} up): got {int(h)} x {int(w)}")


def halved(s):
    """The side after a stride-2 layer with 'same'-style padding (7 x 7 / padding 3, 3 x 3 / padding 1, 1 x 1): floor((s - 1) / 2) + 1."""
    return (int(s) - 1) // 2 + 1


def output_hw(h, w):
    """The size of the last map: five halvings."""
    for _ in range(5):
        h, w = halved(h), halved(w)
    return h, w


class Bottleneck(nn.Module):
    def __init__(self, inplanes, planes, stride, downsample):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes, eps=BN_EPS)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes, eps=BN_EPS)
        self.conv3 = nn.Conv2d(planes, 4 * planes, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(4 * planes, eps=BN_EPS)
        self.downsample = None
        if downsample:
            self.downsample = nn.Sequential(nn.Conv2d(inplanes, 4 * planes, 1, stride=stride, bias=False),
                                            nn.BatchNorm2d(4 * planes, eps=BN_EPS))
        self.stride = stride

    def forward(self, x, amax=None):
        def seen(t):
            if amax is not None:
                amax.append(float(t.abs().max()))
            return t
        identity = x if self.downsample is None else seen(self.downsample(x))
        out = seen(F.relu(self.bn1(self.conv1(x))))
        out = seen(F.relu(self.bn2(self.conv2(out))))
        out = seen(self.bn3(self.conv3(out)))
        return F.relu(seen(out + identity))


class ResNet50(nn.Module):
    """The definition above.  ``forward``: (n, H, W, 3) uint8 -> (n, 2048) in the module's dtype (fp32 as built, fp64 after
    ``.double()``)."""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64, eps=BN_EPS)
        inplanes = 64
        for i, (blocks, planes) in enumerate(zip(LAYERS, PLANES)):
            layer = []
            for b in range(blocks):
                layer.append(Bottleneck(inplanes, planes, 2 if (b == 0 and i > 0) else 1, b == 0))
                inplanes = 4 * planes
            setattr(self, f"layer{i + 1}", nn.Sequential(*layer))
        self.register_buffer("table", input_table(), persistent=False)
        self.synthetic = False
        self.out_dim = OUT_DIM
        for p in self.parameters():
            p.requires_grad_(False)
        self.eval()

    @property
    def dtype(self):
        return self.conv1.weight.dtype

    def blocks(self):
        """The sixteen bottleneck blocks with their names, in order."""
        for i in range(4):
            for b, blk in enumerate(getattr(self, f"layer{i + 1}")):
                yield f"layer{i + 1}.{b}", blk

    def conv_bn_pairs(self):
        """(name of the convolution, convolution, its BatchNorm) of the 53 convolutions, in ``named_modules()`` order."""
        yield "conv1", self.conv1, self.bn1
        for name, blk in self.blocks():
            yield f"{name}.conv1", blk.conv1, blk.bn1
            yield f"{name}.conv2", blk.conv2, blk.bn2
            yield f"{name}.conv3", blk.conv3, blk.bn3
            if blk.downsample is not None:
                yield f"{name}.downsample.0", blk.downsample[0], blk.downsample[1]

    # ---- parameters ------------------------------------------------------------------------------------------------------
    def load_resnet50(self, source):
        """A SwAV checkpoint (keys with a ``module.`` prefix; ``projection_head.*`` and ``prototypes.*`` dropped) or a plain
        torchvision-style ResNet-50 state dict (``fc.*`` and ``num_batches_tracked`` dropped), or the file of either.  A file whose
        shapes say another network is refused, naming the first offending key with both shapes."""
        path, sd = (source, load_file(source)) if isinstance(source, (str, os.PathLike)) else ("state_dict", source)
        sd = clean_state_dict(sd)
        want = {k: tuple(v.shape) for k, v in self.state_dict().items() if not k.endswith("num_batches_tracked")}
        for key, shape in want.items():
            got = tuple(sd[key].shape) if key in sd and hasattr(sd[key], "shape") else None
            if got != shape:
                raise ValueError(f"{path}: {key} is {got if got else 'missing'}, ResNet-50 has {shape}: the file looks like "
                                 f"{_guess_network(sd)}, this loader takes SwAV's or torchvision's ResNet-50")
        for key in sd:
            if key not in want:
                raise ValueError(f"{path}: {key} is {tuple(getattr(sd[key], 'shape', ()))}, ResNet-50 has no such entry: the file "
                                 f"looks like {_guess_network(sd)}, this loader takes SwAV's or torchvision's ResNet-50")
        own = self.state_dict()
        for key in want:
            own[key].copy_(sd[key].to(own[key].dtype))
        self.synthetic = False
        return self

    def init_synthetic(self, seed=0):
        """Seeded stand-in parameters (weights.py's rules: plumbing and throughput runs only, result lines are tagged), drawn in
        fp64 from ONE generator in ``named_modules()`` order: convolutions N(0, 2 / fan_in); BatchNorm weight g (1 + 0.1 N) with
        g = 0.25 for every bn3 and 1 elsewhere (the downsample BatchNorm included), bias 0.1 N, running_mean 0.1 N, running_var
        U(0.5, 1.5).  With g = 1 the residual stream reaches 3.2e4 at 224 x 224, half the fp16 range of the split format."""
        g = torch.Generator().manual_seed(int(seed))
        rn = lambda shape: torch.randn(shape, generator=g, dtype=torch.float64)
        for name, m in self.named_modules():
            if isinstance(m, nn.Conv2d):
                fan_in = m.in_channels * m.kernel_size[0] * m.kernel_size[1]
                m.weight.copy_((rn(m.weight.shape) * (2.0 / fan_in) ** 0.5).to(m.weight.dtype))
            elif isinstance(m, nn.BatchNorm2d):
                gain = BN3_GAIN if name.endswith(".bn3") else 1.0
                m.weight.copy_((gain * (1 + 0.1 * rn(m.weight.shape))).to(m.weight.dtype))
                m.bias.copy_((0.1 * rn(m.bias.shape)).to(m.bias.dtype))
                m.running_mean.copy_((0.1 * rn(m.running_mean.shape)).to(m.running_mean.dtype))
                m.running_var.copy_((0.5 + torch.rand(m.running_var.shape, generator=g, dtype=torch.float64)).to(m.running_var.dtype))
        self.synthetic = True
        return self

    def folded(self):
        """{convolution's name: (weight, bias)} with the BatchNorm folded in: w gamma / sqrt(var + eps) and beta - mean gamma /
        sqrt(var + eps), formed in fp64 on the host and rounded once to fp32."""
        out = {}
        for name, conv, bn in self.conv_bn_pairs():
            s = bn.weight.detach().double().cpu() / torch.sqrt(bn.running_var.detach().double().cpu() + bn.eps)
            w = conv.weight.detach().double().cpu() * s.view(-1, 1, 1, 1)
            b = bn.bias.detach().double().cpu() - bn.running_mean.detach().double().cpu() * s
            out[name] = (w.float(), b.float())
        return out

    # ---- arithmetic ------------------------------------------------------------------------------------------------------
    def network_input(self, img):
        """(n, H, W, 3) uint8 -> (n, 3, H, W) in the module's dtype: the table look-up."""
        if not isinstance(img, torch.Tensor) or img.dtype != torch.uint8 or img.dim() != 4 or img.shape[3] != 3:
            raise ValueError(f"ResNet-50 takes a (n, H, W, 3) uint8 batch (got {tuple(getattr(img, 'shape', ()))} "
                             f"{getattr(img, 'dtype', type(img).__name__)})")
        check_size(img.shape[1], img.shape[2])
        idx = img.permute(0, 3, 1, 2).long()
        table = self.table.to(img.device)
        x = torch.stack([table[c][idx[:, c]] for c in range(3)], 1)
        return x.to(self.dtype)

    def forward(self, img, amax=None):
        """``amax``: a list that receives the largest |activation| of every layer's output."""
        return self.feature_map(img, amax).mean((2, 3))

    def feature_map(self, img, amax=None):
        """The last map, (n, 2048, h, w) with (h, w) = output_hw(H, W): the trunk used fully convolutionally (countseg_model.py)."""
        x = self.network_input(img)
        x = F.relu(self.bn1(self.conv1(x)))
        if amax is not None:
            amax.append(float(x.abs().max()))
        x = F.max_pool2d(x, 3, 2, 1)
        for _, blk in self.blocks():
            x = blk(x, amax)
        return x


def load_file(path):
    sd = torch.load(path, map_location="cpu")
    if isinstance(sd, dict) and "state_dict" in sd and isinstance(sd["state_dict"], dict):
        sd = sd["state_dict"]
    if not isinstance(sd, dict):
        raise ValueError(f"{path}: not a state dict")
    return sd


def clean_state_dict(sd):
    """Both layouts -> plain ResNet-50 keys: the ``module.`` prefix removed; ``projection_head.*``, ``prototypes.*``, ``fc.*`` and
    ``num_batches_tracked`` dropped."""
    out = {}
    for k, v in sd.items():
        if k.startswith("module."):
            k = k[len("module."):]
        if k.startswith(("projection_head.", "prototypes.", "fc.")) or k.endswith("num_batches_tracked"):
            continue
        out[k] = v
    return out


def _guess_network(sd):
    keys = list(sd)
    if any(k.startswith("features.") for k in keys):
        return "a VGG or AlexNet"
    if any(k.startswith(("Mixed_", "Conv2d_")) for k in keys):
        return "an InceptionV3"
    if any(k.startswith("layer1.") for k in keys):
        if not any(".conv3." in k for k in keys):
            return "a ResNet-18 / 34 (basic blocks: no conv3)"
        n3 = len({k.split(".")[1] for k in keys if k.startswith("layer3.")})
        w = sd.get("conv1.weight")
        if n3 != 6:
            return f"a ResNet with {n3} blocks in layer3 (ResNet-101 / 152?)"
        if w is not None and hasattr(w, "shape") and tuple(w.shape) != (64, 3, 7, 7):
            return "a wide ResNet-50 (SwAV's w2 / w4 / w5?)"
        return "a ResNet of another width"
    return "another network"


def load_state_dict_file(path):
    """-> ResNet50 with the parameters of ``path`` (either layout of ``load_resnet50``)."""
    return ResNet50().load_resnet50(path)


def build_model(weights=None, synthetic=False, seed=0):
    """ResNet50 from a file, or seeded stand-ins under ``synthetic`` (never silently)."""
    if synthetic:
        if weights:
            raise RuntimeError("--synthetic-weights and --weights are mutually exclusive")
        return ResNet50().init_synthetic(seed)
    if not weights:
        raise RuntimeError("ResNet-50 needs a parameter file (--weights: SwAV's swav_800ep_pretrain.pth.tar or a torchvision-style "
                           "ResNet-50 state dict); or --synthetic-weights for a plumbing run")
    return load_state_dict_file(weights)


def preprocess_u8(img, size=224):
    """What dgm-eval's ``swav`` encoder does to an image before normalising, RESTATED FROM MEMORY (UNPINNED): RGB, Pillow's 8-bit
    BICUBIC resize straight to size x size, the bytes kept.  Returns a (size, size, 3) uint8 tensor."""
    from PIL import Image
    return torch.from_numpy(np.asarray(img.convert("RGB").resize((size, size), Image.BICUBIC), dtype=np.uint8).copy())
