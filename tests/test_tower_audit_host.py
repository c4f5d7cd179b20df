"""CPU: what tests/_tower_audit.py (the launch audit of the CLIP and DINOv2 towers) can state without a GPU: every ``tise_*``
entry point the towers' sources name is one the recorder knows, the helper's tiny configurations are the tower tests', and
the plans it derives from a module have the graph's launch sequence."""
import os
import re

import torch

from tests import _tower_audit as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_entry_point_of_the_towers_sources_is_known_to_the_recorder():
    """Every ``tise_*`` name in clip_hip.py and dinov2_hip.py is in _tower_audit.KNOWN or in the stated list of entry points that
    launch nothing (A.LAUNCH_NOTHING), and KNOWN holds no name the sources do not: a new kernel cannot slip past the audit."""
    names = set()
    for f in ("clip_hip.py", "dinov2_hip.py"):
        names |= set(re.findall(r"\btise_[a-z0-9_]+\b", open(os.path.join(ROOT, "tise_toolbox_amd", f)).read()))
    assert A.LAUNCH_NOTHING == ("tise_attention_long_key_tile",)
    assert names - set(A.LAUNCH_NOTHING) == set(A.KNOWN), (names - set(A.KNOWN), set(A.KNOWN) - names)
    assert len(A.KNOWN) == 14 and set(A.LAUNCH_NOTHING) <= names
    for name, (ins, outs) in A.KNOWN.items():                          # positions inside the argument list, none twice
        assert len(set(ins + outs)) == len(ins + outs) and max(ins + outs) < len(A.ARGS[name]), name


def test_signatures_agree_with_the_recorders_argument_names():
    """_lib.SIGNATURES has one argument more than A.ARGS (the stream) for every known entry point, pointers where KNOWN says."""
    import ctypes
    from tise_toolbox_amd import _lib
    for name, labels in A.ARGS.items():
        args = _lib.SIGNATURES[name][1]
        assert len(args) == len(labels) + 1, name
        ptrs = {i for i, a in enumerate(args[:-1]) if a in (ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64))}
        assert ptrs == set(A.KNOWN[name][0] + A.KNOWN[name][1]), (name, ptrs)


def test_tiny_configurations_are_the_tower_tests():
    from tests import test_gpu_clip_l14, test_gpu_dinov2
    assert A.TINY154 == test_gpu_dinov2.TINY154 and A.TINY84 == test_gpu_dinov2.TINY84 and A.TINY_CLIP == test_gpu_clip_l14.TINY


def test_plans_state_the_modules_graph():
    """The DINOv2 plan of the issue: patchify_pad, gemm, vit_tokens_f32, per block ln32, gemm, attention(_long), res32, ln32,
    gemm_act (act = 2), res32, then gather_f32 and ln32 with out_fp32 = 1; the CLIP image and text plans likewise; parameters
    rounded as the towers document; fill_defaults_ leaves no all-zero bias and no all-one LayerNorm weight."""
    from tise_toolbox_amd import clip_model, dinov2_model
    for cfg, att in ((A.TINY154, "tise_attention_long_f16"), (A.TINY84, "tise_attention_f16")):
        model = dinov2_model.build_dinov2(None, 0, cfg)
        plan = A.dino_plan(model, torch.zeros(3, 3, cfg["resolution"], cfg["resolution"]), "cpu")
        block = ["tise_layernorm_f32", "tise_gemm_f16", att, "tise_gemm_f16_res32", "tise_layernorm_f32", "tise_gemm_f16_act", "tise_gemm_f16_res32"]
        assert [s.name for s in plan] == ["tise_patchify_pad_f16", "tise_gemm_f16", "tise_vit_tokens_f32"] + 2 * block + ["tise_gather_rows_f32", "tise_layernorm_f32"]
        assert [s.scalars["act"] for s in plan if s.name == "tise_gemm_f16_act"] == [2, 2]
        assert [s.scalars["out_fp32"] for s in plan if s.name == "tise_layernorm_f32"] == [0, 0, 0, 0, 1]
        assert all(s.scalars["eps"] == 9.999999974752427e-07 for s in plan if s.name == "tise_layernorm_f32")      # fp32(1e-6)
        assert plan[1].scalars["k"] == 640 and plan[1].params["w"].shape == (128, 640) and not plan[1].params["w"][:, 588:].any()
        assert plan[6].params["scale"].dtype == torch.float32 and plan[6].params["bias"].dtype == torch.float16
        assert torch.equal(plan[6].params["scale"], model.blocks[0].ls1.gamma) and torch.equal(plan[9].params["scale"], model.blocks[0].ls2.gamma)
    model = A.fill_defaults_(clip_model.build_clip(None, 0, A.TINY_CLIP))
    for name, p in model.named_parameters():
        if p.dim() == 1:
            assert not bool((p == 0).all()) and not bool((p == 1).all()), name
    plan = A.clip_image_plan(model, torch.zeros(2, 3, 154, 154), "cpu")
    assert [s.name for s in plan][:4] == ["tise_patchify_pad_f16", "tise_gemm_f16", "tise_vit_tokens_f16", "tise_layernorm_f16"]
    assert len(plan) == 7 + 7 * 2 and plan[-1].params["w"].shape == (64, 128) and plan[5].scalars["n"] == 384
    assert [s.scalars["act"] for s in plan if s.name == "tise_gemm_f16"] == [0] + [0, 0, 1, 0] * 2 + [0]
    text = clip_model.HashTokenizer()(list(A.CAPTIONS))
    plan = A.clip_text_plan(model, text[:, :15], "cpu")
    assert len(plan) == 1 + 7 + 3 and plan[3].scalars == dict(batch=5, seq=15, heads=1, head_dim=64, causal=1)
    assert plan[-3].given["index"].tolist() == [15 * i + int(text[i].argmax()) for i in range(5)]
    b32 = clip_model.build_clip(None, 0, dict(clip_model.CONFIGS["ViT-B/32"], layers=1, text_layers=1))
    plan = A.clip_image_plan(b32, torch.zeros(1, 3, 224, 224), "cpu")
    assert plan[0].name == "tise_patchify_f16" and plan[1].scalars["k"] == 3072
