"""DINOv2 ViT-S/B/L-14 for FD-DINOv2 (fd_dinov2.py): the fp32 module (parameters, position table, preprocessing) and its
PyTorch-ROCm forward.  The default forward of the CLI is dinov2_hip.HipDino (csrc/clip_ops.hip) built FROM this module.

FD-DINOv2 is the Frechet distance in the space of DINOv2 ViT-L/14's class token (Stein et al. 2023, "Exposing flaws of
generative model evaluation metrics and their fair treatment of diffusion models", the `dgm-eval` package; the tower: Oquab et
al. 2023, "DINOv2: Learning Robust Visual Features without Supervision").  Neither package, nor a parameter file, is
available to this project, so this module RESTATES the published architecture under the official state-dict key names --
``cls_token``, ``pos_embed``, ``patch_embed.proj.{weight,bias}``, ``blocks.{i}.norm1 / attn.qkv / attn.proj / ls1.gamma /
norm2 / mlp.fc1 / mlp.fc2 / ls2.gamma``, ``norm`` -- so that ``dinov2_vit{s,b,l}14_pretrain.pth`` loads with ``strict=True``
(``mask_token`` is accepted and ignored: it only replaces masked patches in training).  What differs from a CLIP tower
(clip_model.VisionTransformer): LayerScale on both branches, exact (erf) GELU, a bias on the patch embedding, no ``ln_pre``
and no projection, LayerNorm eps 1e-6, and a position table stored for 37 x 37 patches (518 px) that is interpolated to the
input's grid.

    tokens  = cat(cls_token, patch_embed(x)) + pos
    block   : x += ls1 * attn(norm1 x);  x += ls2 * mlp(norm2 x)        (F.gelu, erf)
    feature = norm(x)[:, 0]                                              (``x_norm_clstoken``; width = embedding width)

RESTATED FROM MEMORY, so UNPINNED (the README says the same): the position-table rule (``interpolate_pos_table``) and the
preprocessing (``preprocess``).  Parity with the real `dinov2` package and with dgm-eval's numbers is UNPINNED as well: there
are no weights here, the towers are tested against this module in fp32 on seeded parameters only.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
PATCH = 14
TABLE_GRID = 37                      # the released tables hold 37 x 37 patch rows (518 px) + the class row
RESOLUTION = 224                     # dgm-eval feeds 224 x 224
LN_EPS = 1e-6

# The released ViT towers without registers (Oquab et al. 2023, table of architectures): head width 64, MLP ratio 4.
CONFIGS = {
    "vits14": dict(width=384, layers=12, heads=6, patch=PATCH, resolution=RESOLUTION),
    "vitb14": dict(width=768, layers=12, heads=12, patch=PATCH, resolution=RESOLUTION),
    "vitl14": dict(width=1024, layers=24, heads=16, patch=PATCH, resolution=RESOLUTION),
}
DEFAULT_ARCH = "vitl14"


def get_config(arch=None):
    """A name of ``CONFIGS`` (None: vitl14) or a configuration dict itself -> the dict.  Tests register tiny towers in
    ``CONFIGS`` at run time, as clip_model.CONFIGS allows."""
    if arch is None:
        arch = DEFAULT_ARCH
    if isinstance(arch, dict):
        return arch
    if arch not in CONFIGS:
        raise ValueError(f"unknown DINOv2 tower {arch!r}: one of {sorted(CONFIGS)}")
    return CONFIGS[arch]


def config_name(cfg):
    for name, c in CONFIGS.items():
        if c == cfg:
            return name
    return "unnamed(" + ", ".join(f"{k}={v}" for k, v in cfg.items()) + ")"


class LayerScale(nn.Module):
    def __init__(self, width):
        super().__init__()
        self.gamma = nn.Parameter(torch.ones(width))

    def forward(self, x):
        return x * self.gamma


class Attention(nn.Module):
    def __init__(self, width, heads):
        super().__init__()
        self.heads = heads
        self.qkv = nn.Linear(width, 3 * width)
        self.proj = nn.Linear(width, width)

    def forward(self, x):
        b, s, w = x.shape
        q, k, v = self.qkv(x).view(b, s, 3, self.heads, w // self.heads).permute(2, 0, 3, 1, 4)
        o = F.scaled_dot_product_attention(q, k, v)
        return self.proj(o.transpose(1, 2).reshape(b, s, w))


class Mlp(nn.Module):
    def __init__(self, width):
        super().__init__()
        self.fc1 = nn.Linear(width, 4 * width)
        self.fc2 = nn.Linear(4 * width, width)

    def forward(self, x):
        return self.fc2(F.gelu(self.fc1(x)))


class Block(nn.Module):
    def __init__(self, width, heads):
        super().__init__()
        self.norm1 = nn.LayerNorm(width, eps=LN_EPS)
        self.attn = Attention(width, heads)
        self.ls1 = LayerScale(width)
        self.norm2 = nn.LayerNorm(width, eps=LN_EPS)
        self.mlp = Mlp(width)
        self.ls2 = LayerScale(width)

    def forward(self, x):
        x = x + self.ls1(self.attn(self.norm1(x)))
        return x + self.ls2(self.mlp(self.norm2(x)))


class PatchEmbed(nn.Module):
    def __init__(self, width, patch):
        super().__init__()
        self.proj = nn.Conv2d(3, width, patch, patch)                 # with a bias, unlike CLIP's conv1

    def forward(self, x):
        return self.proj(x).flatten(2).transpose(1, 2)


def interpolate_pos_table(table, grid):
    """The (1 + T*T, D) position table of a checkpoint -> (1 + grid*grid, D) for an input of grid x grid patches, ONCE at load.
    RESTATED FROM MEMORY of the released DINOv2 code's ``interpolate_pos_encoding`` (UNPINNED): the class row as it is; the patch
    rows as a (1, D, T, T) image through ``F.interpolate(scale_factor=((grid + 0.1) / T, (grid + 0.1) / T), mode="bicubic",
    antialias=False)`` in fp32 -- the 0.1 is the released code's guard against the floor of a scale factor times T falling one
    short.  The table itself when grid == T."""
    n, d = table.shape
    t = int(round((n - 1) ** 0.5))
    if t * t + 1 != n:
        raise RuntimeError(f"pos_embed has {n} rows: not a square grid plus the class row")
    if grid == t:
        return table
    tab = table.detach().float()
    patch = tab[1:].reshape(1, t, t, d).permute(0, 3, 1, 2)
    s = (grid + 0.1) / t
    patch = F.interpolate(patch, scale_factor=(s, s), mode="bicubic", antialias=False)
    assert patch.shape[-2:] == (grid, grid), (tuple(patch.shape), grid)
    return torch.cat([tab[:1], patch.permute(0, 2, 3, 1).reshape(grid * grid, d)], 0)


class DinoVisionTransformer(nn.Module):
    def __init__(self, config=None, table_grid=TABLE_GRID):
        """``config``: a name of ``CONFIGS`` or a configuration dict.  ``pos_embed`` has the checkpoint's shape (1, 1 +
        table_grid^2, width); ``finalize()`` -- called by ``build_dinov2`` after the parameters are in -- interpolates it once
        to the grid of ``resolution`` into the buffer ``pos`` that ``forward`` adds."""
        super().__init__()
        cfg = get_config(config)
        self.config = dict(cfg)
        w = cfg["width"]
        self.patch, self.resolution, self.out_dim = cfg["patch"], cfg["resolution"], w
        self.patch_embed = PatchEmbed(w, cfg["patch"])
        self.cls_token = nn.Parameter(torch.zeros(1, 1, w))
        self.pos_embed = nn.Parameter(torch.zeros(1, 1 + table_grid * table_grid, w))
        self.blocks = nn.ModuleList([Block(w, cfg["heads"]) for _ in range(cfg["layers"])])
        self.norm = nn.LayerNorm(w, eps=LN_EPS)
        self.register_buffer("pos", torch.zeros(1 + (self.resolution // self.patch) ** 2, w), persistent=False)

    def finalize(self):
        with torch.no_grad():
            self.pos = interpolate_pos_table(self.pos_embed[0], self.resolution // self.patch).to(self.pos_embed).contiguous()
        return self

    def forward(self, x):
        """(B, 3, resolution, resolution) preprocessed images -> (B, width): the normalised class token."""
        if x.shape[-2:] != (self.resolution, self.resolution):
            raise ValueError(f"input of {tuple(x.shape[-2:])}, the position table was interpolated for {self.resolution}")
        x = self.patch_embed(x)
        x = torch.cat([self.cls_token.expand(x.shape[0], -1, -1), x], 1) + self.pos
        for blk in self.blocks:
            x = blk(x)
        return self.norm(x)[:, 0]

    encode_image = forward


def seeded_init_(model, seed=0):
    """Stand-in parameters: truncated-normal (std 0.02, +-2 std) weights and tables, LayerScale gammas drawn in [0.5, 1.5] (not
    the initial 1, nor the released 1e-5: a missing or misplaced gamma must show), NONZERO biases, LayerNorm weights around 1."""
    g = torch.Generator().manual_seed(seed)

    def trunc_(p, std=0.02, mean=0.0):
        v = torch.randn(p.shape, generator=g)
        for _ in range(8):                                             # redraw what fell outside two standard deviations
            bad = v.abs() > 2
            if not bad.any():
                break
            v = torch.where(bad, torch.randn(p.shape, generator=g), v)
        p.data.copy_(mean + std * v.clamp_(-2, 2))

    trunc_(model.patch_embed.proj.weight)
    trunc_(model.patch_embed.proj.bias)
    trunc_(model.cls_token)
    trunc_(model.pos_embed)
    for blk in model.blocks:
        for lin in (blk.attn.qkv, blk.attn.proj, blk.mlp.fc1, blk.mlp.fc2):
            trunc_(lin.weight)
            trunc_(lin.bias)
        for ls in (blk.ls1, blk.ls2):
            ls.gamma.data.copy_(0.5 + torch.rand(ls.gamma.shape, generator=g))
        for ln in (blk.norm1, blk.norm2):
            trunc_(ln.weight, 0.1, 1.0)
            trunc_(ln.bias)
    trunc_(model.norm.weight, 0.1, 1.0)
    trunc_(model.norm.bias)
    return model


def config_from_state_dict(sd):
    """The configuration a DINOv2 ``state_dict`` was built with, read off its tensor SHAPES.  Refused, with the reason: the
    register models (``register_tokens``: the ``_reg4`` files; their extra tokens are not implemented) and the SwiGLU MLP of
    ``vitg14`` (``mlp.w12``)."""
    if "register_tokens" in sd:
        raise RuntimeError("a DINOv2 model WITH REGISTERS (the _reg4 files: 'register_tokens' in the state dict): FD-DINOv2 is "
                           "defined on the models without registers, and the register tokens are not implemented here")
    if any(k.endswith("mlp.w12.weight") for k in sd):
        raise RuntimeError("a DINOv2 ViT-g/14 (SwiGLU MLP: 'mlp.w12' in the state dict): only vits14, vitb14 and vitl14 (fc1 / "
                           "GELU / fc2) are implemented")
    try:
        conv = sd["patch_embed.proj.weight"]
    except KeyError:
        raise RuntimeError("not a DINOv2 state_dict: no 'patch_embed.proj.weight'") from None
    width, patch = conv.shape[0], conv.shape[-1]
    layers = len({k.split(".")[1] for k in sd if k.startswith("blocks.")})
    return dict(width=width, layers=layers, heads=width // 64, patch=patch, resolution=RESOLUTION)


def build_dinov2(weights=None, seed=0, arch=None):
    """The module of tower ``arch`` (a name of ``CONFIGS`` or a configuration dict; None: vitl14) with the parameters of the file
    ``weights`` -- refused when its shapes say another tower -- or, without one, the seeded stand-ins; position table
    interpolated to the tower's resolution."""
    cfg = get_config(arch)
    if weights:
        sd = torch.load(weights, map_location="cpu")
        sd = dict(sd.get("state_dict", sd))
        found = config_from_state_dict(sd)
        shape_keys = ("width", "layers", "heads", "patch")                 # the input resolution is not a property of the file
        if [found[k] for k in shape_keys] != [cfg[k] for k in shape_keys]:
            raise RuntimeError(f"{weights}: parameters of {config_name(found)}, but the tower asked for is {config_name(cfg)}")
        sd.pop("mask_token", None)
        grid = int(round((sd["pos_embed"].shape[1] - 1) ** 0.5))
        model = DinoVisionTransformer(cfg, table_grid=grid)
        model.load_state_dict(sd, strict=True)
    else:
        model = seeded_init_(DinoVisionTransformer(cfg), seed)
    return model.finalize().eval()


def preprocess(img, size=RESOLUTION):
    """What dgm-eval's DINOv2 encoder does to an image, RESTATED FROM MEMORY (UNPINNED): convert to RGB, Pillow's 8-bit BICUBIC
    resize STRAIGHT to size x size (no aspect preservation, no crop), /255, ImageNet mean and std, all in float32.  Returns a
    (3, size, size) fp32 tensor."""
    from PIL import Image
    img = img.convert("RGB").resize((size, size), Image.BICUBIC)
    a = np.asarray(img, dtype=np.float32) / 255.0
    a = (a - np.array(IMAGENET_MEAN, dtype=np.float32)) / np.array(IMAGENET_STD, dtype=np.float32)
    return torch.from_numpy(a).permute(2, 0, 1).contiguous()


def preprocess_lut():
    """3 x 256 fp32 table byte -> network input value with preprocess()'s own op order, all in float32."""
    a = np.arange(256, dtype=np.float32) / 255.0
    return np.ascontiguousarray(np.stack([(a - np.float32(IMAGENET_MEAN[c])) / np.float32(IMAGENET_STD[c]) for c in range(3)]).astype(np.float32))


def preprocess_device(batch_u8, size=RESOLUTION):
    """preprocess() for a (N, H, W, 3) uint8 CUDA batch of equally sized RGB images, on the device: Pillow-exact BICUBIC 8-bit
    resample (csrc/resize.hip) and the look-up of preprocess_lut().  Returns (N, 3, size, size) fp32 -- the values of
    torch.stack([preprocess(img, size) for img in batch]) bit for bit."""
    from . import device
    return device.resize_u8_lut(batch_u8, (size, size), preprocess_lut(), filter="bicubic")
