"""The DINOv2 ViT tower of FD-DINOv2 on the hand-written kernels of csrc/clip_ops.hip, with an FP32 RESIDUAL STREAM.

``HipDino(model)`` takes a ``dinov2_model.DinoVisionTransformer`` (real parameters or the seeded stand-ins) and offers
``encode_image((B, 3, R, R)) -> (B, width) fp32``.  dgm-eval runs this tower in fp32; clip_hip.HipTowers' arithmetic -- the
stream itself in fp16, which is what `clip.load` serves -- would round the stream after each of its 2 x layers additions, on a
network known for very large activations on a few tokens and channels.  So this tower computes what ``torch.autocast(fp16)``
computes: fp16 operands on the matrix cores, fp32 accumulation, the stream, LayerNorm statistics and the features in fp32.

Per block (x: the fp32 stream, updated in place):
    y   = tise_layernorm_f32(x) -> fp16                      norm1
    qkv = tise_gemm_f16(y, qkv)                              fp16
    o   = tise_attention_long_f16 / tise_attention_f16       fp16 (257 tokens at 224: the long kernel)
    x   = tise_gemm_f16_res32(o, proj, scale=ls1, res=x)     fp32: x + ls1 * (o W^T + b), nothing rounded to fp16
    y   = tise_layernorm_f32(x) -> fp16                      norm2
    f   = tise_gemm_f16_act(y, fc1, act=2)                   exact GELU in the epilogue, fp16
    x   = tise_gemm_f16_res32(f, fc2, scale=ls2, res=x)      fp32
Tokens: tise_patchify_pad_f16 (588 -> 640 columns) + tise_gemm_f16 with the patch embedding's bias (fp16 rows), then
tise_vit_tokens_f32 adds the fp32 position table (interpolated once at load, dinov2_model.interpolate_pos_table) and sets the
fp32 class row.  Features: tise_gather_rows_f32 takes the class row of every image and tise_layernorm_f32 normalises it to
fp32.  The gather is a kernel of its own rather than a row-index argument of the LayerNorm: B rows of 4 KB cost nothing, and
tise_layernorm_f32 stays the plain strided sibling of tise_layernorm_f16 that every block calls.

Weights and Linear biases are kept in fp16 (the matrix cores' operands; autocast rounds them the same way), LayerNorm
parameters, LayerScale, the class token and the position table in fp32.  PyTorch only allocates.

``TISE_DINO=torch`` (``build_tower``) runs the module itself under ``torch.autocast(fp16)`` on library kernels: the A/B route.
"""
import ctypes
import os

import torch

from . import _lib, clip_hip, dinov2_model
from .clip_hip import _p, _stream


def gemm_res32(a, w, bias, scale, res, out=None):
    """out32 = res + scale * (a @ w.T + bias);  a (M, K), w (N, K), bias (N) fp16; scale (N) fp32 or None; res (M, N) fp32.
    ``out=None``: in place, into ``res``."""
    assert a.dtype == w.dtype == torch.float16 and res.dtype == torch.float32 and a.is_cuda
    assert a.dim() == 2 and w.dim() == 2 and a.shape[1] == w.shape[1] and a.stride(1) == 1 and w.stride(1) == 1 and res.stride(1) == 1
    m, k = a.shape
    n = w.shape[0]
    assert res.shape == (m, n) and (scale is None or (scale.dtype == torch.float32 and scale.shape == (n,)))
    if out is None:
        out = res
    assert out.dtype == torch.float32 and out.shape == (m, n) and out.stride(1) == 1
    _lib.call("tise_gemm_f16_res32", _p(a), a.stride(0), _p(w), w.stride(0), _p(bias), _p(scale), _p(res), res.stride(0), _p(out),
              out.stride(0), m, n, k, _stream())
    return out


def layernorm32(x, gamma, beta, eps, out_dtype=torch.float16, out=None):
    """LayerNorm of fp32 rows with fp32 gamma / beta -> fp16 rows (for a GEMM) or fp32 rows (the features)."""
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and out_dtype in (torch.float16, torch.float32)
    if out is None:
        out = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    _lib.call("tise_layernorm_f32", _p(x), x.stride(0), _p(gamma), _p(beta), _p(out), out.stride(0), x.shape[0], x.shape[1],
              ctypes.c_float(eps), 1 if out.dtype == torch.float32 else 0, _stream())
    return out


class _Block:
    def __init__(self, blk, dev):
        h = lambda t: t.detach().to(dev, torch.float16).contiguous()
        f = lambda t: t.detach().to(dev, torch.float32).contiguous()
        self.ln1 = (f(blk.norm1.weight), f(blk.norm1.bias), blk.norm1.eps)
        self.ln2 = (f(blk.norm2.weight), f(blk.norm2.bias), blk.norm2.eps)
        self.w_qkv, self.b_qkv = h(blk.attn.qkv.weight), h(blk.attn.qkv.bias)
        self.w_proj, self.b_proj = h(blk.attn.proj.weight), h(blk.attn.proj.bias)
        self.w_fc1, self.b_fc1 = h(blk.mlp.fc1.weight), h(blk.mlp.fc1.bias)
        self.w_fc2, self.b_fc2 = h(blk.mlp.fc2.weight), h(blk.mlp.fc2.bias)
        self.ls1, self.ls2 = f(blk.ls1.gamma), f(blk.ls2.gamma)
        self.heads = blk.attn.heads

    def __call__(self, x, batch, seq):
        """x (batch*seq, width) fp32, updated in place (module docstring)."""
        y = layernorm32(x, *self.ln1)
        qkv = clip_hip.gemm(y, self.w_qkv, self.b_qkv)
        o = clip_hip.attention(qkv, batch, seq, self.heads, causal=False)
        gemm_res32(o, self.w_proj, self.b_proj, self.ls1, x)
        y = layernorm32(x, *self.ln2, out=y)
        f = clip_hip.gemm(y, self.w_fc1, self.b_fc1, act=2)           # exact GELU in the epilogue
        return gemm_res32(f, self.w_fc2, self.b_fc2, self.ls2, x)


class HipDino:
    def __init__(self, model, device=None):
        if not torch.cuda.is_available():
            raise _lib.TiseLibraryError("HipDino needs an MI355X: there is no CPU path")
        _lib.load()
        dev = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.device = dev
        h = lambda t: t.detach().to(dev, torch.float16).contiguous()
        f = lambda t: t.detach().to(dev, torch.float32).contiguous()
        self.patch, self.width = model.patch, model.out_dim
        self.resolution, self.out_dim = model.resolution, model.out_dim
        if self.width > 1024 or self.width % 64 != 0:
            raise ValueError(f"width {self.width}: the kernels take widths up to 1024 in multiples of 64")
        kcols = 3 * self.patch * self.patch
        self.kpad = (kcols + 63) // 64 * 64                          # 588 -> 640: tise_gemm_f16 steps K by 64
        w = torch.zeros((self.width, self.kpad), dtype=torch.float16, device=dev)
        w[:, :kcols] = h(model.patch_embed.proj.weight.flatten(1))   # columns (c, ky, kx)
        self.w_patch, self.b_patch = w, h(model.patch_embed.proj.bias)
        self.cls, self.pos = f(model.cls_token.reshape(-1)), f(model.pos)
        assert self.pos.shape == (1 + (self.resolution // self.patch) ** 2, self.width)
        self.norm = (f(model.norm.weight), f(model.norm.bias), model.norm.eps)
        self.blocks = [_Block(b, dev) for b in model.blocks]

    # what RP_coco.encode_paths preprocesses with (plain functions: the DataLoader's workers pickle ``preprocess``)
    preprocess_device = staticmethod(dinov2_model.preprocess_device)
    preprocess = staticmethod(dinov2_model.preprocess)

    @torch.no_grad()
    def encode_image(self, image):
        """(B, 3, resolution, resolution) preprocessed images -> (B, width) fp32: norm(x)[:, 0] of the module."""
        x = image.to(self.device, torch.float16).contiguous()
        b, _, r, r2 = x.shape
        if (r, r2) != (self.resolution, self.resolution):
            raise ValueError(f"input of {r} x {r2}, the position table was interpolated for {self.resolution}")
        if b == 0:
            return torch.empty((0, self.width), dtype=torch.float32, device=self.device)
        g = r // self.patch
        npatch, seq = g * g, g * g + 1
        pm = torch.empty((b * npatch, self.kpad), dtype=torch.float16, device=self.device)
        _lib.call("tise_patchify_pad_f16", _p(x), b, r, self.patch, self.kpad, _p(pm), _stream())
        pe = clip_hip.gemm(pm, self.w_patch, self.b_patch)
        xs = torch.empty((b * seq, self.width), dtype=torch.float32, device=self.device)
        _lib.call("tise_vit_tokens_f32", _p(pe), _p(self.cls), _p(self.pos), b, npatch, self.width, _p(xs), _stream())
        for blk in self.blocks:
            blk(xs, b, seq)
        idx = torch.arange(b, device=self.device, dtype=torch.int64) * seq          # the class token of every image
        c = torch.empty((b, self.width), dtype=torch.float32, device=self.device)
        _lib.call("tise_gather_rows_f32", _p(xs), _p(idx), b, self.width, _p(c), _stream())
        return layernorm32(c, *self.norm, out_dtype=torch.float32)

    def parameters(self):                                            # so that callers can ask for the dtype
        yield self.w_patch


class AutocastDino:
    """``TISE_DINO=torch``: the module itself under torch.autocast(fp16) on library kernels, with HipDino's interface."""

    def __init__(self, model, device):
        self.model = model.to(device).float().eval()
        self.device = torch.device(device)
        self.resolution, self.out_dim = model.resolution, model.out_dim

    preprocess_device = staticmethod(dinov2_model.preprocess_device)
    preprocess = staticmethod(dinov2_model.preprocess)

    @torch.no_grad()
    def encode_image(self, image):
        with torch.autocast("cuda", dtype=torch.float16):
            return self.model(image.to(self.device, torch.float32)).float()

    def parameters(self):
        return self.model.parameters()


def build_tower(weights, dev, arch=None, seed=0):
    """The tower the CLI runs: HipDino over dinov2_model.build_dinov2, or AutocastDino with TISE_DINO=torch."""
    model = dinov2_model.build_dinov2(weights, seed, arch)
    route = os.environ.get("TISE_DINO", "hip")
    if route == "torch":
        return AutocastDino(model, dev)
    if route != "hip":
        raise ValueError(f"TISE_DINO={route!r}: 'hip' (default) or 'torch'")
    return HipDino(model, dev)
