"""open_clip ViT-H/14 for CLIPScore and the human-preference scores built on it (HPS v2): the module, its registry and its loader.

The tower is ``clip_model.CLIP`` -- the same blocks, tokenizers and preprocessing -- with the two things the OpenAI towers never
needed: an explicit head count (width 1280 over 16 heads is 80 columns per head; ``clip_model.config_from_state_dict`` infers
``width // 64``) and the exact (erf) GELU in the MLP instead of QuickGELU.  Its registry is its own: ``clip_model.CONFIGS`` holds
the OpenAI towers only.

EVERYTHING about open_clip here is restated from memory of its ``ViT-H-14.json`` and of its model code: the numbers of
``CONFIGS``, LayerNorm eps 1e-5, ``ln_pre`` present, a patch convolution without bias, the OpenAI mean / std, a bicubic
short-side resize plus centre crop, a 77-token causal text tower read at the end-of-text token, and the OpenAI BPE vocabulary.
There is no ``open_clip`` package and no parameter file here, so PARITY with it is UNPINNED; the tests compare
clip_hip.HipTowers against this module in fp32 on seeded parameters, at towers of up to 1024 columns (``default_route``).

Files: open_clip's native ``state_dict`` uses the OpenAI key names (``visual.conv1.weight``, ``transformer.resblocks...``), with
a stored ``attn_mask`` buffer that is dropped.  The Hugging Face ``CLIPModel`` layout (keys under ``vision_model.`` /
``text_model.``; the layout of PickScore's published file) is refused: a converter is out of scope.
"""
import torch

from . import clip_model

# open_clip model_configs/ViT-H-14.json, from memory (module docstring).  Heads are part of the configuration: 1280 / 16 = 80.
CONFIGS = {
    "ViT-H-14": dict(resolution=224, patch=14, width=1280, layers=32, heads=16, embed_dim=1024,
                     text_width=1024, text_layers=24, text_heads=16, act="gelu"),
}

HIP_MAX_WIDTH = 1024             # clip_hip.LAYERNORM_MAX_C: the widest LayerNorm row of the towers' hand-written kernels


def default_route(cfg):
    """The default route of RP_coco.build_towers for a configuration of this registry: "hip" (clip_hip.HipTowers: attention at
    head width 80, exact GELU in the GEMM epilogue) while both towers are at most HIP_MAX_WIDTH columns wide, "torch" (the fp16
    module on library kernels) beyond -- ViT-H-14's image tower is 1280 wide, which HipTowers refuses."""
    return "hip" if max(cfg["width"], cfg["text_width"]) <= HIP_MAX_WIDTH else "torch"


def get_config(arch):
    """A name of ``CONFIGS`` or a configuration dict itself -> the dict, checked: both widths divide into their heads."""
    if isinstance(arch, dict):
        cfg = arch
    elif arch in CONFIGS:
        cfg = CONFIGS[arch]
    else:
        raise ValueError(f"unknown open_clip tower {arch!r}: one of {sorted(CONFIGS)}")
    for w, h in (("width", "heads"), ("text_width", "text_heads")):
        if cfg[h] <= 0 or cfg[w] % cfg[h] != 0:
            raise ValueError(f"{w} {cfg[w]} is not a multiple of {h} {cfg[h]}")
    return cfg


def is_config(arch):
    """Whether ``arch`` names a tower of this registry, or is a configuration dict of this module's kind (it says its ``act``)."""
    return (isinstance(arch, dict) and "act" in arch) or (isinstance(arch, str) and arch in CONFIGS)


def config_name(cfg):
    for name, c in CONFIGS.items():
        if c == cfg:
            return name
    return "unnamed(" + ", ".join(f"{k}={v}" for k, v in cfg.items()) + ")"


def build_model(arch="ViT-H-14"):
    """The module of ``arch`` with PyTorch's default initialisation (seeded_init_ or load_state_dict follow)."""
    return clip_model.CLIP(config=get_config(arch))


seeded_init_ = clip_model.seeded_init_


def shapes_of(sd):
    """What a native-layout ``state_dict`` says about its tower: everything of a configuration but heads and activation, which
    no shape shows."""
    found = clip_model.config_from_state_dict(sd)
    return {k: v for k, v in found.items() if k not in ("heads", "text_heads")}


def load_state_dict_(model, sd, cfg, what="state_dict"):
    """Load a native open_clip ``state_dict`` into ``model`` (built from ``cfg``), strictly.  The heads come from ``cfg``, never
    from ``width // 64``; a file of another tower and the Hugging Face layout are refused with the reason."""
    sd = dict(sd.get("state_dict", sd))
    if any(k.startswith(("vision_model.", "text_model.")) for k in sd):
        raise RuntimeError(f"{what}: Hugging Face CLIPModel layout (keys under 'vision_model.' / 'text_model.'); this loader reads "
                           f"open_clip's native state_dict only, and a converter is out of scope")
    if any(k.startswith("module.") for k in sd):                 # a checkpoint saved from DistributedDataParallel
        sd = {k[len("module."):] if k.startswith("module.") else k: v for k, v in sd.items()}
    for k in ("attn_mask", "input_resolution", "context_length", "vocab_size"):
        sd.pop(k, None)
    found = shapes_of(sd)
    want = {k: v for k, v in cfg.items() if k in found}
    if found != want:
        theirs = next((n for n, c in list(CONFIGS.items()) + list(clip_model.CONFIGS.items())
                       if {k: v for k, v in c.items() if k in found} == found), None)
        theirs = theirs or "unnamed(" + ", ".join(f"{k}={v}" for k, v in found.items()) + ")"
        raise RuntimeError(f"{what}: parameters of {theirs}, but the tower asked for is {config_name(cfg)}")
    model.load_state_dict(sd, strict=True)
    return model


def build_openclip(weights=None, seed=0, arch="ViT-H-14"):
    """``clip_model.build_clip`` for this registry: the parameters of the file ``weights``, or the seeded stand-ins."""
    cfg = get_config(arch)
    model = build_model(cfg)
    if weights:
        load_state_dict_(model, torch.load(weights, map_location="cpu"), cfg, weights)
    else:
        seeded_init_(model, seed)
    return model.eval()
