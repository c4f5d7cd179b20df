"""CPU: the host side of the ViT-L/14@336 tower: configurations read back off tensor shapes, the refusal of a parameter file of
another tower, clip._transform's integer rules at 336 pixels, the ViT-B/32 seeded parameters unchanged bit for bit, the new C
entries' argument checks (no GPU: fake aligned addresses, one defect per call) and the CLI's defaults."""
import ctypes
import hashlib
import os

import pytest
import torch

TINY = dict(resolution=154, patch=14, width=128, layers=2, heads=2, embed_dim=64, text_width=64, text_layers=1, text_heads=1)


def _meta_state_dict(cfg):
    """The shapes of an OpenAI-format state_dict of ``cfg`` as meta tensors (no storage)."""
    from tise_toolbox_amd import clip_model
    m = lambda *s: torch.empty(s, device="meta")
    w, tw = cfg["width"], cfg["text_width"]
    sd = {"visual.conv1.weight": m(w, 3, cfg["patch"], cfg["patch"]), "visual.class_embedding": m(w),
          "visual.positional_embedding": m((cfg["resolution"] // cfg["patch"]) ** 2 + 1, w), "visual.proj": m(w, cfg["embed_dim"]),
          "visual.ln_pre.weight": m(w), "visual.ln_post.weight": m(w), "token_embedding.weight": m(clip_model.VOCAB_SIZE, tw),
          "positional_embedding": m(clip_model.CONTEXT_LENGTH, tw), "ln_final.weight": m(tw),
          "text_projection": m(tw, cfg["embed_dim"]), "logit_scale": m()}
    for prefix, width, layers in (("visual.transformer", w, cfg["layers"]), ("transformer", tw, cfg["text_layers"])):
        for i in range(layers):
            sd[f"{prefix}.resblocks.{i}.attn.in_proj_weight"] = m(3 * width, width)
            sd[f"{prefix}.resblocks.{i}.mlp.c_fc.weight"] = m(4 * width, width)
    return sd


def test_configs_hold_the_published_towers():
    from tise_toolbox_amd import clip_model
    assert clip_model.CONFIGS["ViT-B/32"] == dict(resolution=224, patch=32, width=768, layers=12, heads=12, embed_dim=512,
                                                  text_width=512, text_layers=12, text_heads=8)
    assert clip_model.CONFIGS["ViT-L/14@336"] == dict(resolution=336, patch=14, width=1024, layers=24, heads=16, embed_dim=768,
                                                      text_width=768, text_layers=12, text_heads=12)
    with pytest.raises(ValueError, match="ViT-H"):
        clip_model.get_config("ViT-H/14")


def test_config_from_state_dict_reads_the_shapes():
    from tise_toolbox_amd import clip_model
    for name in ("ViT-B/32", "ViT-L/14@336"):                          # 428 M parameters are never built here: meta tensors
        assert clip_model.config_from_state_dict(_meta_state_dict(clip_model.CONFIGS[name])) == clip_model.CONFIGS[name]
    model = clip_model.build_clip(arch=TINY)                           # and a real (tiny) module's own state_dict
    assert clip_model.config_from_state_dict(model.state_dict()) == TINY
    assert (model.resolution, model.out_dim) == (154, 64)
    assert model.visual.positional_embedding.shape == (122, 128) and len(model.visual.transformer.resblocks) == 2
    b32 = clip_model.CLIP()
    assert (b32.resolution, b32.out_dim) == (224, 512) and clip_model.config_from_state_dict(b32.state_dict()) == clip_model.CONFIGS["ViT-B/32"]
    with pytest.raises(RuntimeError, match="visual.conv1.weight"):
        clip_model.config_from_state_dict({"visual.layer1.0.conv1.weight": torch.empty(1, device="meta")})


def test_build_clip_refuses_a_file_of_another_tower(tmp_path, monkeypatch):
    from tise_toolbox_amd import clip_model
    other = dict(TINY, resolution=140)
    monkeypatch.setitem(clip_model.CONFIGS, "tiny/14@154", TINY)
    path = str(tmp_path / "tiny.pt")
    model = clip_model.build_clip(arch=TINY, seed=3)
    torch.save(model.state_dict(), path)
    loaded = clip_model.build_clip(path, arch="tiny/14@154")
    assert all(torch.equal(a, b) for a, b in zip(loaded.state_dict().values(), model.state_dict().values()))
    with pytest.raises(RuntimeError, match=r"tiny/14@154.*ViT-B/32"):   # names what the file holds and what was asked for
        clip_model.build_clip(path)
    with pytest.raises(RuntimeError, match="resolution=140"):
        clip_model.build_clip(path, arch=other)


def test_preprocess_geometry_at_336():
    """clip._transform's integer rules with 336 in place of 224, worked by hand:
    640 x 480 (w x h): short side 480 -> 336, long side int(336 * 640 / 480) = int(448.0) = 448, left = round(112 / 2) = 56;
    500 x 375: int(336 * 500 / 375) = int(448.0) = 448;  333 x 500 (h = 500): int(336 * 500 / 333) = int(504.504...) = 504
    (truncated; rounding gives 505), top = round(168 / 2) = 84;  w 337, h 336: int(336 * 337 / 336) = 337, left = round(0.5) = 0
    (half to even; half up gives 1);  w 339, h 336: 339, left = round(1.5) = 2;  w 341: left = round(2.5) = 2 (half up: 3);
    1000 x 999 (h = 999): int(336 * 1000 / 999) = int(336.336...) = 336: no crop at all."""
    from tise_toolbox_amd.clip_model import preprocess_geometry as geo
    assert geo(480, 640, 336) == (336, 448, 0, 56)
    assert geo(375, 500, 336) == (336, 448, 0, 56)
    assert geo(500, 333, 336) == (504, 336, 84, 0)
    assert geo(336, 337, 336) == (336, 337, 0, 0)
    assert geo(336, 339, 336) == (336, 339, 0, 2)
    assert geo(336, 341, 336) == (336, 341, 0, 2)
    assert geo(999, 1000, 336) == (336, 336, 0, 0)
    assert geo(256, 256, 336) == (336, 336, 0, 0)
    assert geo(480, 640) == geo(480, 640, 224) == (224, 298, 0, 37)     # the default is 224 as before


def test_preprocess_takes_the_size():
    from PIL import Image
    import numpy as np
    from tise_toolbox_amd import clip_model
    img = Image.fromarray(np.random.default_rng(0).integers(0, 256, (50, 70, 3), dtype=np.uint8))
    assert clip_model.preprocess(img).shape == (3, 224, 224) and clip_model.preprocess(img, size=336).shape == (3, 336, 336)


# SHA-256 of seeded ViT-B/32 parameters (build_clip(), seed 0) recorded at the commit before the configurations existed
B32_DIGESTS = {
    "token_embedding.weight": "e90bdd3b22f7cbdbacc31235d85cb598c43d7877b626a91c6b13f235a3934de0",
    "positional_embedding": "aeb1861af76fa50cc078562d2f06fb0260be73dcf797c4f943b3135672e0ecc2",
    "transformer.resblocks.0.attn.in_proj_weight": "02f0b2eeb6fa02ea1d4dd914b734a49f5cb31c539e1dacb096d4394203d9a841",
    "transformer.resblocks.11.mlp.c_proj.weight": "87784d96ab6969012ad0193db9bd2a5012aafc57ae81653506765bf7647cb311",
    "visual.transformer.resblocks.0.attn.in_proj_weight": "d20558ff8134434a89e6487d3c8dba5098496d4f625a95834cf8012218f91df4",
    "visual.transformer.resblocks.11.mlp.c_fc.weight": "26b6ae24f52aa3c8bed3aefb451df6a15a5a0153248f276bc58e8d5c23f2a038",
    "text_projection": "0a96f1b615e89c29825e30d43cda5457863e4621d44d389cf6cfdcce3fa84c93",
    "visual.conv1.weight": "54af4242d094801f58e7b79e6ed055bcc888417ee80ba879c5022ee2462a14ad",
    "visual.class_embedding": "f0b4833adfe7bd1cc491dbfffa13ee631653a85cf61e7b72330308ef285d211c",
    "visual.positional_embedding": "9cb2815b49518db36efebdb964e4db7ac795ca616ae7b3cdfdab6cb7c7d8f079",
    "visual.proj": "72cb48688c2672d6bad0f1b819444fd40e18180b8fd4233d8aa4546be72073db",
}


def test_b32_seeded_parameters_are_unchanged():
    """Same generator, same draw order: the first and the last tensor drawn, and some of both towers between them."""
    from tise_toolbox_amd import clip_model
    sd = clip_model.build_clip().state_dict()
    for k, want in B32_DIGESTS.items():
        assert hashlib.sha256(sd[k].numpy().tobytes()).hexdigest() == want, k
    named = clip_model.build_clip(arch="ViT-B/32").state_dict()
    assert all(torch.equal(sd[k], named[k]) for k in B32_DIGESTS)


def test_new_entries_reject_every_single_defect_without_a_gpu():
    """tise_attention_long_f16 and tise_patchify_pad_f16 check their arguments before any HIP call: fake device addresses,
    exactly one defect per call, each TISE_ERR_INVALID_ARG; batch 0 is TISE_OK without a launch; a grid beyond 2^31 - 1
    workgroups is TISE_ERR_UNSUPPORTED."""
    from tise_toolbox_amd import _lib, build, clip_hip
    build.build(force=False, verbose=False)
    lib = _lib.load()
    bad = _lib.TISE_ERR_INVALID_ARG
    A, O = 0x7f0000000000, 0x7f0000400000

    def attn(qkv=A, out=O, batch=0, seq=577, heads=16, hd=64):
        return lib.tise_attention_long_f16(qkv, batch, seq, heads, hd, out, None)
    assert attn() == _lib.TISE_OK and attn(seq=1) == _lib.TISE_OK and attn(seq=1 << 30) == _lib.TISE_OK    # no length limit
    for kw in (dict(qkv=None), dict(out=None), dict(seq=0), dict(seq=-5), dict(hd=32), dict(hd=128), dict(heads=0), dict(batch=-1),
               dict(qkv=A + 8), dict(qkv=A + 2), dict(out=O + 8), dict(out=O + 2)):
        assert attn(**kw) == bad, kw
    assert attn(batch=1 << 20, seq=1 << 20, heads=1) == _lib.TISE_ERR_UNSUPPORTED       # 2^13 blocks x 2^20 sequences = 2^33
    assert lib.tise_attention_long_key_tile() == clip_hip.ATTN_LONG_KEY_TILE

    def patchify(img=A, out=O, batch=0, res=336, patch=14, kpad=640):
        return lib.tise_patchify_pad_f16(img, batch, res, patch, kpad, out, None)
    assert patchify() == _lib.TISE_OK and patchify(img=A + 2) == _lib.TISE_OK and patchify(res=7, patch=7, kpad=192) == _lib.TISE_OK
    for kw in (dict(img=None), dict(out=None), dict(batch=-1), dict(res=0), dict(patch=0), dict(res=337), dict(kpad=576), dict(kpad=600),
               dict(kpad=0), dict(img=A + 1), dict(out=O + 8), dict(out=O + 2)):
        assert patchify(**kw) == bad, kw


def test_cli_defaults_and_the_l14_weight_file(monkeypatch):
    from tise_toolbox_amd import clip_model, cmmd, weights
    a = cmmd.parse_args(["--path1", "ref", "--path2", "gen"])
    assert a.tower == "ViT-B/32" == cmmd.TOWER and (cmmd.DIMS, cmmd.NETWORK) == (512, "clip-vit-b32")
    assert cmmd.parse_args(["--path1", "r", "--path2", "g", "--tower", "ViT-L/14@336"]).tower == "ViT-L/14@336"
    with pytest.raises(SystemExit):
        cmmd.parse_args(["--path1", "r", "--path2", "g", "--tower", "ViT-H/14"])
    assert cmmd.tower_info("ViT-B/32") == (512, "clip-vit-b32", "clip")
    assert cmmd.tower_info("ViT-L/14@336") == (768, "clip-vit-l14-336", "clip-l14-336")
    monkeypatch.setitem(clip_model.CONFIGS, "tiny/14@154", TINY)       # the choices are built inside parse_args
    assert cmmd.parse_args(["--path1", "r", "--path2", "g", "--tower", "tiny/14@154"]).tower == "tiny/14@154"
    assert cmmd.tower_info("tiny/14@154") == (64, "clip-tiny-14-154", None)
    monkeypatch.setenv("HOME", "/nonexistent-home")
    want = os.path.join("/nonexistent-home", ".cache", "clip", "ViT-L-14-336px.pt")
    assert weights._KINDS["clip-l14-336"][1]() == [want]
    with pytest.raises(RuntimeError) as e:
        weights.resolve(None, False, "clip-l14-336")
    assert want in str(e.value) and "ViT-L/14@336" in str(e.value)
    assert weights.resolve(None, True, "clip-l14-336") == (None, weights.SYNTHETIC_TAG)
    with pytest.raises(RuntimeError, match="tiny/14@154"):
        weights.resolve(None, False, None, "CLIP tiny/14@154")


def test_feature_files_are_per_tower(tmp_path):
    import numpy as np
    from tise_toolbox_amd import cmmd
    feats = np.random.default_rng(1).standard_normal((5, 768)).astype(np.float32)
    mu, sigma = feats.astype(np.float64).mean(0), np.cov(feats.astype(np.float64), rowvar=False)
    l14, b32 = str(tmp_path / "l14.npz"), str(tmp_path / "b32.npz")
    cmmd.save_features_npz(l14, feats, mu, sigma, "ViT-L/14@336")
    cmmd.save_features_npz(b32, feats[:, :512], mu[:512], sigma[:512, :512])
    with np.load(l14) as f:
        assert str(f["network"]) == "clip-vit-l14-336"
    got = cmmd.load_features_npz(l14, "ViT-L/14@336")
    assert np.array_equal(got[0], feats)
    with pytest.raises(RuntimeError, match="clip-vit-l14-336"):
        cmmd.load_features_npz(l14)                                    # under the default ViT-B/32
    with pytest.raises(RuntimeError, match="clip-vit-b32"):
        cmmd.load_features_npz(b32, "ViT-L/14@336")
    wrong = str(tmp_path / "wrong_width.npz")
    cmmd.save_features_npz(wrong, feats[:, :512], mu[:512], sigma[:512, :512], "ViT-L/14@336")
    with pytest.raises(RuntimeError, match=r"expected \(n, 768\)"):
        cmmd.load_features_npz(wrong, "ViT-L/14@336")
