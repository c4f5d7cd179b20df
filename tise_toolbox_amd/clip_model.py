"""CLIP ViT-B/32 for RP-COCO / PA and ViT-L/14@336 for CMMD (``CONFIGS``): the module (parameters, tokenizers, preprocessing) and its
PyTorch-ROCm forward.  The default forward of the CLIs is clip_hip.HipTowers (csrc/clip_ops.hip) built FROM this module.

The reference calls the third-party `clip` package (`clip.load("ViT-B/32")`, text_relevance/RP_coco.py:31,
positional_alignment/PA.py:30), which is not in /root/reference, not in this image, and whose weights and BPE
vocabulary cannot be fetched.  This module restates the published architecture (Radford et al. 2021; ViT-B/32:
patch 32, width 768, 12 layers, 12 heads, 512-d joint space; text: 77 tokens, width 512, 12 layers, 8 heads,
vocab 49408, QuickGELU, causal mask, features taken at the end-of-text token) with the parameter names of the
OpenAI checkpoint, so a real `state_dict` loads with `strict=True`; without one the weights are seeded
stand-ins (throughput and plumbing only).  This module's own forward runs on PyTorch-ROCm library kernels (hipBLASLt
GEMMs, SDPA; selected by TISE_CLIP=torch) and is the fp32 reference the hand-written towers are tested against
(tests/test_gpu_clip.py).  PARITY of either forward against the real `clip` package: UNPINNED; what is pinned for this
row is the host logic and the retrieval reduction around the towers (tests/golden/rp_stub_*.npz).
"""
import gzip
import html
import math
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
CONTEXT_LENGTH = 77
VOCAB_SIZE = 49408
SOT, EOT = 49406, 49407

# The published towers (Radford et al. 2021, table 20; the OpenAI package's build_model reads the same numbers off a
# checkpoint's shapes).  Heads are width // 64 in every published ViT tower.  ViT-B/32 serves RP-COCO, PA, CLIP-FID and the
# default CMMD; ViT-L/14@336 is the tower of the published CMMD figures (Jayasumana et al. 2024).
CONFIGS = {
    "ViT-B/32": dict(resolution=224, patch=32, width=768, layers=12, heads=12, embed_dim=512,
                     text_width=512, text_layers=12, text_heads=8),
    "ViT-L/14@336": dict(resolution=336, patch=14, width=1024, layers=24, heads=16, embed_dim=768,
                         text_width=768, text_layers=12, text_heads=12),
}
DEFAULT_ARCH = "ViT-B/32"


def get_config(arch=None):
    """A name of ``CONFIGS`` (None: ViT-B/32) or a configuration dict itself -> the dict."""
    if arch is None:
        arch = DEFAULT_ARCH
    if isinstance(arch, dict):
        return arch
    if arch not in CONFIGS:
        raise ValueError(f"unknown CLIP tower {arch!r}: one of {sorted(CONFIGS)}")
    return CONFIGS[arch]


def config_name(cfg):
    """The ``CONFIGS`` name of a configuration, or its numbers when it has none (error messages)."""
    for name, c in CONFIGS.items():
        if c == cfg:
            return name
    return "unnamed(" + ", ".join(f"{k}={v}" for k, v in cfg.items()) + ")"


class QuickGELU(nn.Module):
    def forward(self, x):
        return x * torch.sigmoid(1.702 * x)


class Attention(nn.Module):
    """Parameter-name compatible with nn.MultiheadAttention (in_proj_weight / in_proj_bias / out_proj)."""

    def __init__(self, width, heads):
        super().__init__()
        self.heads = heads
        self.in_proj_weight = nn.Parameter(torch.empty(3 * width, width))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * width))
        self.out_proj = nn.Linear(width, width)

    def forward(self, x, causal):
        b, s, w = x.shape
        qkv = F.linear(x, self.in_proj_weight, self.in_proj_bias).view(b, s, 3, self.heads, w // self.heads)
        q, k, v = qkv.permute(2, 0, 3, 1, 4)
        o = F.scaled_dot_product_attention(q, k, v, is_causal=causal)
        return self.out_proj(o.transpose(1, 2).reshape(b, s, w))


def make_act(act):
    """The MLP activation of a tower: "quick_gelu" (every OpenAI tower) or "gelu" (exact erf GELU: openclip_model's towers)."""
    if act == "quick_gelu":
        return QuickGELU()
    if act == "gelu":
        return nn.GELU()
    raise ValueError(f"unknown MLP activation {act!r}: 'quick_gelu' or 'gelu'")


class Block(nn.Module):
    def __init__(self, width, heads, act="quick_gelu"):
        super().__init__()
        self.attn = Attention(width, heads)
        self.ln_1 = nn.LayerNorm(width)
        self.mlp = nn.Sequential(OrderedDict([("c_fc", nn.Linear(width, 4 * width)), ("gelu", make_act(act)),
                                              ("c_proj", nn.Linear(4 * width, width))]))
        self.ln_2 = nn.LayerNorm(width)

    def forward(self, x, causal):
        x = x + self.attn(self.ln_1(x), causal)
        return x + self.mlp(self.ln_2(x))


class Transformer(nn.Module):
    def __init__(self, width, layers, heads, act="quick_gelu"):
        super().__init__()
        self.resblocks = nn.ModuleList([Block(width, heads, act) for _ in range(layers)])

    def forward(self, x, causal=False):
        for blk in self.resblocks:
            x = blk(x, causal)
        return x


class VisionTransformer(nn.Module):
    def __init__(self, resolution=224, patch=32, width=768, layers=12, heads=12, out_dim=512, act="quick_gelu"):
        super().__init__()
        self.conv1 = nn.Conv2d(3, width, patch, patch, bias=False)
        scale = width ** -0.5
        self.class_embedding = nn.Parameter(scale * torch.randn(width))
        self.positional_embedding = nn.Parameter(scale * torch.randn((resolution // patch) ** 2 + 1, width))
        self.ln_pre = nn.LayerNorm(width)
        self.transformer = Transformer(width, layers, heads, act)
        self.ln_post = nn.LayerNorm(width)
        self.proj = nn.Parameter(scale * torch.randn(width, out_dim))

    def forward(self, x):
        x = self.conv1(x).flatten(2).transpose(1, 2)                       # (B, patches, width)
        cls = self.class_embedding.to(x.dtype).expand(x.shape[0], 1, -1)
        x = torch.cat([cls, x], 1) + self.positional_embedding.to(x.dtype)
        x = self.transformer(self.ln_pre(x))
        return self.ln_post(x[:, 0]) @ self.proj


class CLIP(nn.Module):
    def __init__(self, embed_dim=512, text_width=512, text_layers=12, text_heads=8, config=None):
        """``config``: a name of ``CONFIGS`` or a configuration dict (then the other arguments are not read); None: ViT-B/32
        with the text tower of the arguments, as before the configurations existed."""
        super().__init__()
        act = "quick_gelu"
        if config is not None:
            cfg = get_config(config)
            act = cfg.get("act", act)                          # only openclip_model's configurations carry one
            embed_dim, text_width, text_layers, text_heads = cfg["embed_dim"], cfg["text_width"], cfg["text_layers"], cfg["text_heads"]
            self.visual = VisionTransformer(cfg["resolution"], cfg["patch"], cfg["width"], cfg["layers"], cfg["heads"], embed_dim, act)
        else:
            self.visual = VisionTransformer(out_dim=embed_dim)
        # what callers preprocess to and allocate for (clip_hip.HipTowers and RP_coco.encode_paths read both)
        self.resolution = self.visual.conv1.kernel_size[0] * int(round((self.visual.positional_embedding.shape[0] - 1) ** 0.5))
        self.out_dim = embed_dim
        self.transformer = Transformer(text_width, text_layers, text_heads, act)
        self.token_embedding = nn.Embedding(VOCAB_SIZE, text_width)
        self.positional_embedding = nn.Parameter(torch.empty(CONTEXT_LENGTH, text_width))
        self.ln_final = nn.LayerNorm(text_width)
        self.text_projection = nn.Parameter(torch.empty(text_width, embed_dim))
        self.logit_scale = nn.Parameter(torch.ones([]) * math.log(1 / 0.07))

    def encode_image(self, image):
        return self.visual(image)

    def encode_text(self, text):
        x = self.token_embedding(text) + self.positional_embedding.to(self.token_embedding.weight.dtype)
        x = self.ln_final(self.transformer(x, causal=True))
        return x[torch.arange(x.shape[0], device=x.device), text.argmax(-1)] @ self.text_projection


def seeded_init_(model, seed=0):
    """Stand-in weights (the published initialisation scheme, seeded)."""
    g = torch.Generator().manual_seed(seed)

    def normal_(p, std):
        p.data.copy_(torch.randn(p.shape, generator=g) * std)

    normal_(model.token_embedding.weight, 0.02)
    normal_(model.positional_embedding, 0.01)
    tw, vw = model.token_embedding.weight.shape[1], model.visual.conv1.out_channels       # B/32: 512 and 768
    for tower, width, layers in ((model.transformer, tw, len(model.transformer.resblocks)),
                                 (model.visual.transformer, vw, len(model.visual.transformer.resblocks))):
        proj_std = (width ** -0.5) * ((2 * layers) ** -0.5)
        for blk in tower.resblocks:
            normal_(blk.attn.in_proj_weight, width ** -0.5)
            normal_(blk.attn.out_proj.weight, proj_std)
            normal_(blk.mlp.c_fc.weight, (2 * width) ** -0.5)
            normal_(blk.mlp.c_proj.weight, proj_std)
            for b in (blk.attn.in_proj_bias, blk.attn.out_proj.bias, blk.mlp.c_fc.bias, blk.mlp.c_proj.bias):
                b.data.zero_()
    normal_(model.text_projection, tw ** -0.5)
    normal_(model.visual.conv1.weight, 0.02)
    normal_(model.visual.class_embedding, vw ** -0.5)
    normal_(model.visual.positional_embedding, vw ** -0.5)
    normal_(model.visual.proj, vw ** -0.5)
    return model


def config_from_state_dict(sd):
    """The configuration an OpenAI-format ``state_dict`` was built with, read off its tensor SHAPES as the OpenAI package's
    ``build_model`` does (meta-device tensors are enough).  Heads are not in the shapes: ``width // 64``."""
    try:
        conv = sd["visual.conv1.weight"]
    except KeyError:
        raise RuntimeError("not a CLIP ViT state_dict: no 'visual.conv1.weight' (the ResNet towers are not supported)") from None
    width, patch = conv.shape[0], conv.shape[-1]
    grid = int(round((sd["visual.positional_embedding"].shape[0] - 1) ** 0.5))
    if grid * grid + 1 != sd["visual.positional_embedding"].shape[0]:
        raise RuntimeError(f"visual.positional_embedding has {sd['visual.positional_embedding'].shape[0]} rows: not a square grid plus one")
    blocks = lambda prefix: len({k[len(prefix):].split(".")[0] for k in sd if k.startswith(prefix)})
    text_width = sd["ln_final.weight"].shape[0]
    return dict(resolution=grid * patch, patch=patch, width=width, layers=blocks("visual.transformer.resblocks."),
                heads=width // 64, embed_dim=sd["text_projection"].shape[1], text_width=text_width,
                text_layers=blocks("transformer.resblocks."), text_heads=text_width // 64)


def build_clip(weights=None, seed=0, arch=None):
    """The module of tower ``arch`` (a name of ``CONFIGS`` or a configuration dict; None: ViT-B/32) with the parameters of the
    file ``weights`` -- refused when its shapes say another tower -- or, without one, the seeded stand-ins."""
    cfg = get_config(arch)
    model = CLIP(config=cfg)
    if weights:
        sd = torch.load(weights, map_location="cpu")
        sd = sd.get("state_dict", sd)
        for k in ("input_resolution", "context_length", "vocab_size"):
            sd.pop(k, None)
        found = config_from_state_dict(sd)
        if found != cfg:
            raise RuntimeError(f"{weights}: parameters of {config_name(found)}, but the tower asked for is {config_name(cfg)}")
        model.load_state_dict(sd, strict=True)
    else:
        seeded_init_(model, seed)
    return model.eval()


def preprocess(img, size=224):
    """clip._transform: Resize(size, bicubic) -> CenterCrop(size) -> RGB -> ToTensor -> Normalize (size = the tower's input
    resolution: 224, or 336 for ViT-L/14@336).  PIL on the host (as the reference), returns a (3, size, size) fp32 tensor."""
    from PIL import Image
    w, h = img.size
    nh, nw, top, left = preprocess_geometry(h, w, size)
    img = img.resize((nw, nh), Image.BICUBIC)
    a = np.asarray(img.crop((left, top, left + size, top + size)).convert("RGB"), dtype=np.float32) / 255.0
    a = (a - np.array(CLIP_MEAN, dtype=np.float32)) / np.array(CLIP_STD, dtype=np.float32)
    return torch.from_numpy(a).permute(2, 0, 1).contiguous()


def preprocess_lut():
    """3 x 256 fp32 table byte -> network input value with preprocess()'s own op order: float32(v) / 255.0, minus the mean,
    divided by the std, all in float32 -- the ToTensor + Normalize of clip._transform as a look-up."""
    a = np.arange(256, dtype=np.float32) / 255.0
    return np.ascontiguousarray(np.stack([(a - np.float32(CLIP_MEAN[c])) / np.float32(CLIP_STD[c]) for c in range(3)]).astype(np.float32))


def preprocess_geometry(h, w, size=224):
    """(resized height, resized width, top, left) of clip._transform for an h x w image, with torchvision's own integer
    rules (third-party; clip/clip.py _transform -> torchvision.transforms.Resize(size) + CenterCrop(size), size 224 unless
    the tower says otherwise): the shorter side becomes ``size`` and the longer one ``int(size * long / short)`` -- TRUNCATED,
    not rounded (640 x 480 -> 298, not 299, at 224) -- and the crop starts at ``int(round((n - size) / 2.0))`` (Python's
    round: halves go to the even integer).  Square images -- the toolbox's 256 x 256 -- are unaffected; ADVICE r5 caught the
    one-pixel difference on other shapes."""
    if w <= h:
        nw, nh = size, int(size * h / w)
    else:
        nw, nh = int(size * w / h), size
    return nh, nw, int(round((nh - size) / 2.0)), int(round((nw - size) / 2.0))


def preprocess_device(batch_u8, size=224):
    """preprocess() for a (N, H, W, 3) uint8 CUDA batch of equally sized RGB images, on the device: Pillow-exact BICUBIC
    8-bit resample (csrc/resize.hip, tise_resize_u8), the crop as a slice, ToTensor + Normalize through preprocess_lut().
    Returns (N, 3, size, size) fp32 -- the values of torch.stack([preprocess(img, size) for img in batch]) bit for bit."""
    from . import device
    n, h, w, _ = batch_u8.shape
    nh, nw, top, left = preprocess_geometry(h, w, size)
    x = device.resize_u8_lut(batch_u8, (nh, nw), preprocess_lut(), filter="bicubic")
    if (nh, nw) != (size, size):
        x = x[:, :, top:top + size, left:left + size].contiguous()
    return x


# ---- tokenizers -----------------------------------------------------------------------------------------
def _bytes_to_unicode():
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("\xa1"), ord("\xac") + 1)) + list(range(ord("\xae"), ord("\xff") + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return dict(zip(bs, (chr(c) for c in cs)))


class BPETokenizer:
    """The published CLIP byte-pair tokenizer, driven by the user's `bpe_simple_vocab_16e6.txt.gz` (not shipped;
    restated from the algorithm's description, exercised here only on a synthetic merge table; `ftfy` text repair
    is skipped because the package is absent)."""

    def __init__(self, bpe_path):
        import regex
        self.byte_encoder = _bytes_to_unicode()
        merges = gzip.open(bpe_path).read().decode("utf-8").split("\n")
        merges = [tuple(m.split()) for m in merges[1:49152 - 256 - 2 + 1] if m]
        vocab = list(self.byte_encoder.values())
        vocab = vocab + [v + "</w>" for v in vocab] + ["".join(m) for m in merges] + ["<|startoftext|>", "<|endoftext|>"]
        self.encoder = dict(zip(vocab, range(len(vocab))))
        self.bpe_ranks = dict(zip(merges, range(len(merges))))
        self.cache = {}
        self.pat = regex.compile(r"""<\|startoftext\|>|<\|endoftext\|>|'s|'t|'re|'ve|'m|'ll|'d|[\p{L}]+|[\p{N}]|[^\s\p{L}\p{N}]+""",
                                 regex.IGNORECASE)

    def _bpe(self, token):
        if token in self.cache:
            return self.cache[token]
        word = tuple(token[:-1]) + (token[-1] + "</w>",)
        while len(word) > 1:
            pairs = {(word[i], word[i + 1]) for i in range(len(word) - 1)}
            best = min(pairs, key=lambda p: self.bpe_ranks.get(p, float("inf")))
            if best not in self.bpe_ranks:
                break
            out, i = [], 0
            while i < len(word):
                if i < len(word) - 1 and (word[i], word[i + 1]) == best:
                    out.append(word[i] + word[i + 1]); i += 2
                else:
                    out.append(word[i]); i += 1
            word = tuple(out)
        self.cache[token] = word
        return word

    def encode(self, text):
        text = " ".join(html.unescape(html.unescape(text)).split()).strip().lower()
        ids = []
        for tok in self.pat.findall(text):
            tok = "".join(self.byte_encoder[b] for b in tok.encode("utf-8"))
            ids.extend(self.encoder[t] for t in self._bpe(tok))
        return ids

    def __call__(self, texts, context_length=CONTEXT_LENGTH):
        """clip.tokenize: (len(texts), context_length) int64, zero padded.  Rows are written into ONE numpy array (no tensor
        per caption) and whole captions are memoised next to the per-word merge cache: the RP / PA pickles repeat their
        mismatched captions many times and the host tokeniser was the longest stage of the RP-COCO job."""
        import numpy as np
        sot, eot = self.encoder["<|startoftext|>"], self.encoder["<|endoftext|>"]
        out = np.zeros((len(texts), context_length), dtype=np.int64)
        memo = self.__dict__.setdefault("_caption_memo", {})
        for i, t in enumerate(texts):
            ids = memo.get(t)
            if ids is None:
                ids = [sot] + self.encode(t) + [eot]
                if len(memo) < 1 << 20:
                    memo[t] = ids
            if len(ids) > context_length:
                raise RuntimeError(f"Input {t} is too long for context length {context_length}")    # clip.tokenize
            out[i, :len(ids)] = ids
        return torch.from_numpy(out)


class HashTokenizer:
    """Stand-in when no vocabulary file is given: one id per lower-cased word (stable hash), same framing
    (start token, end token = largest id so that argmax finds it, zero padding)."""

    def __call__(self, texts, context_length=CONTEXT_LENGTH):
        """Rows are written into ONE numpy array and word ids are memoised (crc32 per distinct word once): 4x the rate of
        building a tensor per caption -- the host tokeniser was the longest stage of the 30 k-item RP-COCO job."""
        import zlib
        import numpy as np
        out = np.zeros((len(texts), context_length), dtype=np.int64)
        words = self.__dict__.setdefault("_word_ids", {})
        for i, t in enumerate(texts):
            ids = [SOT]
            for w in t.lower().split()[:context_length - 2]:
                k = words.get(w)
                if k is None:
                    k = words[w] = 1 + zlib.crc32(w.encode()) % (SOT - 1)
                ids.append(k)
            ids.append(EOT)
            out[i, :len(ids)] = ids
        return torch.from_numpy(out)
