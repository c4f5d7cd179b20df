"""The CLIP towers (ViT-B/32; ViT-L/14@336 for CMMD) on the hand-written kernels of csrc/clip_ops.hip;
also towers of openclip_model.py's kind: head width 80 on the long-sequence attention and the exact GELU are read off the module.
A tower wider than 1024 columns (open_clip's ViT-H/14 itself: 1280) is refused when HipTowers is built -- the LayerNorm entry point
the towers launch holds 1024 -- and runs on the library route (RP_coco.build_towers).

``HipTowers(model)`` takes a ``clip_model.CLIP`` (real OpenAI parameters or the seeded stand-ins), keeps fp16 copies
of its parameters in the layouts the kernels read, and offers ``encode_image`` / ``encode_text`` with the signatures
of the module's own methods.  Every matrix product -- the patch embedding (as a GEMM over ``tise_patchify_f16``'s
patch matrix), the q/k/v, output, MLP and final projections -- is ``tise_gemm_f16`` with bias / QuickGELU / residual
fused in its epilogue; LayerNorm, attention (``tise_attention_f16`` up to 96 tokens, ``tise_attention_long_f16`` beyond: the
577 tokens of L/14@336) and the token assembly are the other kernels of that file.  PyTorch only
allocates the buffers.  Arithmetic: fp16 tensors, fp32 accumulation and statistics, i.e. what the fp16 model
``clip.load`` serves on a GPU computes (third-party `clip`, model.py: ``convert_weights`` + fp32 LayerNorm).
Parity of the towers themselves stays UNPINNED (no `clip` package, weights or vocabulary here); the tests compare
against ``clip_model.CLIP`` run in fp32 through PyTorch-ROCm.
"""
import ctypes

import torch

from . import _lib


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def gemm(a, w, bias=None, residual=None, act=0, out=None):
    """out = act(a @ w.T + bias) + residual;  a (M, K), w (N, K) fp16 CUDA, row strides arbitrary multiples of 8.
    act: 0 none, 1 QuickGELU (tise_gemm_f16, the CLIP towers' entry), 2 exact (erf) GELU (tise_gemm_f16_act: the DINOv2 tower)."""
    assert a.dtype == w.dtype == torch.float16 and a.is_cuda and a.dim() == 2 and w.dim() == 2 and a.shape[1] == w.shape[1]
    assert a.stride(1) == 1 and w.stride(1) == 1
    m, k = a.shape
    n = w.shape[0]
    if out is None:
        out = torch.empty((m, n), dtype=torch.float16, device=a.device)
    _lib.call("tise_gemm_f16_act" if int(act) == 2 else "tise_gemm_f16", _p(a), a.stride(0), _p(w), w.stride(0), _p(bias), _p(residual),
              residual.stride(0) if residual is not None else 0, _p(out), out.stride(0), m, n, k, int(act), _stream())
    return out


def layernorm(x, gamma, beta, eps=1e-5, out=None):
    assert x.dtype == torch.float16 and x.dim() == 2 and x.stride(1) == 1
    if out is None:
        out = torch.empty_like(x)
    if x.shape[1] > LAYERNORM_MAX_C:
        raise ValueError(f"the towers' LayerNorm kernel holds rows of up to {LAYERNORM_MAX_C} columns (got {x.shape[1]})")
    _lib.call("tise_layernorm_f16", _p(x), x.stride(0), _p(gamma), _p(beta), _p(out), out.stride(0), x.shape[0], x.shape[1],
              ctypes.c_float(eps), _stream())
    return out


LAYERNORM_MAX_C = 1024           # tise_layernorm_f16 holds a row as 2 x 8 values per lane
ATTN_LONG_HEAD_DIMS = (64, 80)   # tise_attention_long_f16's instances; tise_attention_f16 (short / causal) is 64 only
GEMM_K_STEP = 64                 # tise_gemm_f16 steps K by 64 columns
ATTN_LONG_KEY_TILE = 64          # keys per LDS tile of tise_attention_long_f16 (= tise_attention_long_key_tile(), csrc/clip_ops.hip)
ATTN_SHORT_MAX_SEQ = 96          # tise_attention_f16 keeps a (sequence, head)'s scores in registers up to here


def attention(qkv, batch, seq, heads, causal, head_dim=64):
    """qkv (batch*seq, 3*heads*head_dim) fp16 contiguous -> (batch*seq, heads*head_dim).  seq <= 96: tise_attention_f16 (one wave
    per (sequence, head); head_dim 64 only); longer sequences: tise_attention_long_f16 (streamed keys, online softmax),
    non-causal only, head_dim 64 or 80."""
    if seq > ATTN_SHORT_MAX_SEQ:
        if causal:
            raise ValueError(f"causal attention runs up to {ATTN_SHORT_MAX_SEQ} tokens (got {seq}): the long-sequence kernel has no mask")
        return attention_long(qkv, batch, seq, heads, head_dim)
    if head_dim != 64:
        raise ValueError(f"the short / causal attention kernel runs at head width 64 only (got {head_dim}, {seq} tokens"
                         f"{', causal' if causal else ''})")
    assert qkv.dtype == torch.float16 and qkv.is_contiguous() and qkv.shape == (batch * seq, 3 * heads * head_dim)
    out = torch.empty((batch * seq, heads * head_dim), dtype=torch.float16, device=qkv.device)
    _lib.call("tise_attention_f16", _p(qkv), batch, seq, heads, head_dim, 1 if causal else 0, _p(out), _stream())
    return out


def attention_long(qkv, batch, seq, heads, head_dim=64):
    """attention(..., causal=False) on tise_attention_long_f16 whatever the length (any seq >= 1), at head width 64 or 80."""
    if head_dim not in ATTN_LONG_HEAD_DIMS:
        raise ValueError(f"the long-sequence attention kernel runs at head widths {ATTN_LONG_HEAD_DIMS} (got {head_dim})")
    assert qkv.dtype == torch.float16 and qkv.is_contiguous() and qkv.shape == (batch * seq, 3 * heads * head_dim)
    out = torch.empty((batch * seq, heads * head_dim), dtype=torch.float16, device=qkv.device)
    _lib.call("tise_attention_long_f16", _p(qkv), batch, seq, heads, head_dim, _p(out), _stream())
    return out


def mlp_act(module):
    """The GEMM epilogue's activation code of a block's MLP activation module: 1 QuickGELU, 2 exact (erf) GELU."""
    from . import clip_model
    if isinstance(module, clip_model.QuickGELU):
        return 1
    if isinstance(module, torch.nn.GELU) and getattr(module, "approximate", "none") == "none":
        return 2
    raise ValueError(f"no GEMM epilogue for the MLP activation {module!r}: QuickGELU or the exact nn.GELU")


def _k_padded(cols):
    return (cols + GEMM_K_STEP - 1) // GEMM_K_STEP * GEMM_K_STEP


def _pad_cols(t, kp):
    """A GEMM operand (rows, K) with zero columns up to kp = _k_padded(K), as the patch matrix of patch 14 has them: a width that
    is no multiple of the K-step (a tower of 2 heads of 80: 160) still runs, on exact zeros.  kp == K: the tensor itself."""
    return t if t.shape[1] == kp else torch.nn.functional.pad(t, (0, kp - t.shape[1])).contiguous()


def _layernorm_k(x, ln, kp):
    """layernorm(x, *ln) as the next GEMM's operand: (rows, kp) with zeros behind the C columns (kp == C: layernorm's own output)."""
    if x.shape[1] == kp:
        return layernorm(x, *ln)
    buf = torch.zeros((x.shape[0], kp), dtype=torch.float16, device=x.device)
    layernorm(x, *ln, out=buf[:, :x.shape[1]])
    return buf


class _Block:
    def __init__(self, blk, dev):
        h = lambda t: t.detach().to(dev, torch.float16).contiguous()
        self.kp = kp = _k_padded(blk.attn.in_proj_weight.shape[1])
        self.ln1 = (h(blk.ln_1.weight), h(blk.ln_1.bias), blk.ln_1.eps)
        self.ln2 = (h(blk.ln_2.weight), h(blk.ln_2.bias), blk.ln_2.eps)
        self.w_in, self.b_in = _pad_cols(h(blk.attn.in_proj_weight), kp), h(blk.attn.in_proj_bias)
        self.w_out, self.b_out = _pad_cols(h(blk.attn.out_proj.weight), kp), h(blk.attn.out_proj.bias)
        self.w_fc, self.b_fc = _pad_cols(h(blk.mlp.c_fc.weight), kp), h(blk.mlp.c_fc.bias)
        self.w_pr, self.b_pr = h(blk.mlp.c_proj.weight), h(blk.mlp.c_proj.bias)
        self.heads = blk.attn.heads
        self.head_dim = blk.attn.in_proj_weight.shape[1] // self.heads
        self.act = mlp_act(blk.mlp.gelu)

    def __call__(self, x, batch, seq, causal):
        """x (batch*seq, width) -> x + attn(ln_1(x)); then + mlp(ln_2(.))   (clip model.py ResidualAttentionBlock)."""
        y = _layernorm_k(x, self.ln1, self.kp)
        qkv = gemm(y, self.w_in, self.b_in)
        o = attention(qkv, batch, seq, self.heads, causal, self.head_dim)
        x = gemm(_pad_cols(o, self.kp), self.w_out, self.b_out, residual=x)
        y = _layernorm_k(x, self.ln2, self.kp)
        f = gemm(y, self.w_fc, self.b_fc, act=self.act)             # QuickGELU (1) or exact GELU (2) in the epilogue
        return gemm(f, self.w_pr, self.b_pr, residual=x)


class HipTowers:
    def __init__(self, model, device=None):
        if not torch.cuda.is_available():
            raise _lib.TiseLibraryError("HipTowers needs an MI355X: there is no CPU path")
        _lib.load()
        dev = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.device = dev
        h = lambda t: t.detach().to(dev, torch.float16).contiguous()
        v = model.visual
        self.patch = v.conv1.kernel_size[0]
        self.width_v = v.conv1.out_channels
        self.resolution, self.out_dim = model.resolution, model.out_dim
        self.w_patch = h(v.conv1.weight.flatten(1))                 # (width, 3 * P * P): columns (c, ky, kx)
        kcols = 3 * self.patch * self.patch
        # tise_patchify_f16 moves 8 halves (patch % 8 == 0) and tise_gemm_f16 steps K by 64: any other patch size (L/14:
        # 588 columns) takes tise_patchify_pad_f16 and a weight matrix with zero columns up to the next multiple of 64
        self.kpad = 0 if (kcols % 64 == 0 and self.patch % 8 == 0) else (kcols + 63) // 64 * 64
        if self.kpad:
            w = torch.zeros((self.width_v, self.kpad), dtype=torch.float16, device=dev)
            w[:, :kcols] = self.w_patch
            self.w_patch = w
        self.cls, self.pos_v = h(v.class_embedding), h(v.positional_embedding)
        self.ln_pre = (h(v.ln_pre.weight), h(v.ln_pre.bias), v.ln_pre.eps)
        self.ln_post = (h(v.ln_post.weight), h(v.ln_post.bias), v.ln_post.eps)
        self.proj_v = _pad_cols(h(v.proj.t()), _k_padded(self.width_v))      # (out_dim, width): features @ proj
        self.blocks_v = [_Block(b, dev) for b in v.transformer.resblocks]
        self.table = h(model.token_embedding.weight)
        self.pos_t = h(model.positional_embedding)
        self.ln_final = (h(model.ln_final.weight), h(model.ln_final.bias), model.ln_final.eps)
        self.proj_t = _pad_cols(h(model.text_projection.t()), _k_padded(self.table.shape[1]))
        self.blocks_t = [_Block(b, dev) for b in model.transformer.resblocks]
        self.width_t = self.table.shape[1]
        self.logit_scale = model.logit_scale
        # a head width the kernels of a tower's sequences do not have is an error here, before anything is launched: the text
        # tower (causal) and an image tower of up to 96 tokens run on the short kernel, head width 64 only
        for name, width in (("image", self.width_v), ("text", self.width_t)):
            if width > LAYERNORM_MAX_C:
                raise ValueError(f"the {name} tower is {width} columns wide: HipTowers' LayerNorm kernel holds rows of up to "
                                 f"{LAYERNORM_MAX_C}; this tower runs on the library route (TISE_CLIP=torch)")
        seq_v = self.pos_v.shape[0]
        for name, blocks, long_seq in (("image", self.blocks_v, seq_v > ATTN_SHORT_MAX_SEQ), ("text", self.blocks_t, False)):
            for blk in blocks:
                if blk.head_dim != 64 and not (long_seq and blk.head_dim in ATTN_LONG_HEAD_DIMS):
                    raise ValueError(f"the {name} tower has head width {blk.head_dim}: the "
                                     f"{'long-sequence' if long_seq else 'short / causal'} attention kernel does not run it")

    @torch.no_grad()
    def encode_image(self, image):
        """(B, 3, resolution, resolution) preprocessed images -> (B, out_dim) fp16 (clip model.py VisionTransformer.forward)."""
        x = image.to(self.device, torch.float16).contiguous()
        b, _, r, _ = x.shape
        g = r // self.patch
        npatch = g * g
        if self.kpad:
            pm = torch.empty((b * npatch, self.kpad), dtype=torch.float16, device=self.device)
            _lib.call("tise_patchify_pad_f16", _p(x), b, r, self.patch, self.kpad, _p(pm), _stream())
        else:
            pm = torch.empty((b * npatch, 3 * self.patch * self.patch), dtype=torch.float16, device=self.device)
            _lib.call("tise_patchify_f16", _p(x), b, r, self.patch, _p(pm), _stream())
        pe = gemm(pm, self.w_patch)                                  # conv1 (no bias)
        seq = npatch + 1
        tok = torch.empty((b * seq, self.width_v), dtype=torch.float16, device=self.device)
        _lib.call("tise_vit_tokens_f16", _p(pe), _p(self.cls), _p(self.pos_v), b, npatch, self.width_v, _p(tok), _stream())
        xs = layernorm(tok, *self.ln_pre)
        for blk in self.blocks_v:
            xs = blk(xs, b, seq, causal=False)
        idx = torch.arange(b, device=self.device, dtype=torch.int64) * seq          # the class token of every image
        c = torch.empty((b, self.width_v), dtype=torch.float16, device=self.device)
        _lib.call("tise_gather_rows_f16", _p(xs), _p(idx), b, self.width_v, _p(c), _stream())
        return gemm(_layernorm_k(c, self.ln_post, self.proj_v.shape[1]), self.proj_v)

    @torch.no_grad()
    def encode_text(self, text):
        """(B, 77) int token ids -> (B, out_dim) fp16 (clip model.py CLIP.encode_text: features at the end-of-text token =
        the position of the largest id)."""
        text = text.to(self.device)
        b, seq = text.shape
        tok32 = text.to(torch.int32).contiguous()
        x = torch.empty((b * seq, self.width_t), dtype=torch.float16, device=self.device)
        _lib.call("tise_text_tokens_f16", _p(tok32), _p(self.table), _p(self.pos_t), b * seq, seq, self.width_t, _p(x), _stream())
        for blk in self.blocks_t:
            x = blk(x, b, seq, causal=True)
        idx = (torch.arange(b, device=self.device, dtype=torch.int64) * seq + text.argmax(-1).to(torch.int64)).contiguous()
        e = torch.empty((b, self.width_t), dtype=torch.float16, device=self.device)
        _lib.call("tise_gather_rows_f16", _p(x), _p(idx), b, self.width_t, _p(e), _stream())
        return gemm(_layernorm_k(e, self.ln_final, self.proj_t.shape[1]), self.proj_t)

    def parameters(self):                                            # so that callers can ask for the dtype
        yield self.table
