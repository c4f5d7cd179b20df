"""CPU: openclip_model -- the ViT-H-14 numbers, a tiny tower of the same kind (heads of 80, exact GELU) built, run and round-tripped
through a saved file, and the loader's refusals."""
import pytest
import torch

TINY = dict(resolution=154, patch=14, width=160, layers=2, heads=2, embed_dim=64, text_width=128, text_layers=2, text_heads=2,
            act="gelu")


def test_vit_h_14_numbers_and_registries():
    from tise_toolbox_amd import clip_model, openclip_model
    assert openclip_model.get_config("ViT-H-14") == dict(resolution=224, patch=14, width=1280, layers=32, heads=16, embed_dim=1024,
                                                         text_width=1024, text_layers=24, text_heads=16, act="gelu")
    cfg = openclip_model.CONFIGS["ViT-H-14"]
    assert cfg["width"] // cfg["heads"] == 80 and cfg["text_width"] // cfg["text_heads"] == 64
    assert (cfg["resolution"] // cfg["patch"]) ** 2 + 1 == 257
    assert "ViT-H-14" not in clip_model.CONFIGS and "ViT-H/14" not in clip_model.CONFIGS
    with pytest.raises(ValueError):
        clip_model.get_config("ViT-H/14")
    with pytest.raises(ValueError, match="ViT-H-14"):
        openclip_model.get_config("ViT-B/32")
    assert openclip_model.is_config("ViT-H-14") and openclip_model.is_config(TINY)
    assert not openclip_model.is_config("ViT-B/32") and not openclip_model.is_config(None)
    assert not openclip_model.is_config(clip_model.CONFIGS["ViT-B/32"])


def test_tiny_tower_builds_runs_and_round_trips(tmp_path):
    from tise_toolbox_amd import clip_model, openclip_model
    model = openclip_model.build_openclip(None, 0, TINY)
    blk = model.visual.transformer.resblocks[0]
    assert blk.attn.heads == 2 and blk.attn.in_proj_weight.shape == (480, 160)           # heads from the configuration: 80 wide
    assert isinstance(blk.mlp.gelu, torch.nn.GELU) and isinstance(model.transformer.resblocks[0].mlp.gelu, torch.nn.GELU)
    assert model.visual.ln_pre.eps == 1e-5 and model.visual.conv1.bias is None and model.resolution == 154
    img = torch.randn((2, 3, 154, 154), generator=torch.Generator().manual_seed(1))
    tok = clip_model.HashTokenizer()(["a cat on a mat", "two dogs"])
    with torch.no_grad():
        fi, ft = model.encode_image(img), model.encode_text(tok)
    assert fi.shape == (2, 64) and ft.shape == (2, 64) and torch.isfinite(fi).all() and torch.isfinite(ft).all()
    # exact GELU, not QuickGELU: the same parameters under clip_model's default activation give other features
    quick = clip_model.CLIP(config={k: v for k, v in TINY.items() if k != "act"})
    quick.load_state_dict(model.state_dict())
    with torch.no_grad():
        assert not torch.allclose(quick.eval().encode_image(img), fi)
    # a native open_clip file: the OpenAI key names plus a stored attn_mask
    sd = dict(model.state_dict())
    sd["attn_mask"] = torch.full((77, 77), float("-inf")).triu_(1)
    path = str(tmp_path / "tiny.pt")
    torch.save(sd, path)
    again = openclip_model.build_openclip(path, 5, TINY)
    with torch.no_grad():
        assert torch.equal(again.encode_image(img), fi) and torch.equal(again.encode_text(tok), ft)
    torch.save({"state_dict": {"module." + k: v for k, v in sd.items()}}, path)
    with torch.no_grad():
        assert torch.equal(openclip_model.build_openclip(path, 5, TINY).encode_image(img), fi)
    assert openclip_model.seeded_init_ is clip_model.seeded_init_
    other = openclip_model.build_openclip(None, 1, TINY)
    assert not torch.equal(other.visual.proj, model.visual.proj)


def test_refusals(tmp_path):
    from tise_toolbox_amd import clip_model, openclip_model
    # a file of another tower: both are named
    other = dict(TINY, width=320, heads=4)
    path = str(tmp_path / "other.pt")
    torch.save(openclip_model.build_openclip(None, 0, other).state_dict(), path)
    with pytest.raises(RuntimeError, match=r"parameters of unnamed\(.*width=320.*but the tower asked for is unnamed\(.*width=160"):
        openclip_model.build_openclip(path, 0, TINY)
    tiny_b32 = dict(clip_model.CONFIGS["ViT-B/32"], layers=1, text_layers=1)
    torch.save(clip_model.build_clip(None, 0, tiny_b32).state_dict(), path)
    with pytest.raises(RuntimeError, match="but the tower asked for is ViT-H-14"):
        openclip_model.build_openclip(path, 0, "ViT-H-14")
    # the Hugging Face CLIPModel layout (PickScore's file), with the reason
    hf = {"vision_model.embeddings.patch_embedding.weight": torch.zeros(4, 3, 2, 2), "text_model.final_layer_norm.weight": torch.zeros(4),
          "logit_scale": torch.zeros(())}
    torch.save(hf, path)
    with pytest.raises(RuntimeError, match="Hugging Face CLIPModel layout"):
        openclip_model.build_openclip(path, 0, TINY)
    # width % heads != 0, on either tower
    with pytest.raises(ValueError, match="width 160 is not a multiple of heads 3"):
        openclip_model.get_config(dict(TINY, heads=3))
    with pytest.raises(ValueError, match="text_width 128 is not a multiple of text_heads 3"):
        openclip_model.build_openclip(None, 0, dict(TINY, text_heads=3))
    with pytest.raises(ValueError):
        clip_model.make_act("relu")
