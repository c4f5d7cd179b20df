"""GPU: every launch of the CLIP and DINOv2 towers against fp64, and the towers' wiring against the module's graph.

tests/test_gpu_clip_kernels.py, test_gpu_attention_long.py and test_gpu_dinov2_kernels.py pin the kernels on operands the tests
make themselves; tests/test_gpu_clip.py, test_gpu_clip_l14.py and test_gpu_dinov2.py pin the class token's cosine.  Everything
clip_hip.py and dinov2_hip.py decide in between -- which tensor goes into which argument, which of ls1 / ls2, b_proj / b_fc2,
ln1 / ln2 a launch gets, eps, act, out_fp32, causal, the row strides, the reuse of ``y``, the in-place update of the fp32 stream,
the kpad columns, the gather index, the short / long attention switch, the GEMM instance -- is checked here, launch by launch:
a recorder (tests/_tower_audit.py) keeps the operands of every launch of a real forward as that launch saw them, each launch
is compared with fp64 computed from ITS OWN recorded input and the MODULE's parameters at the bound the project derived for that
kernel (none taken from what a tower gives), and the launch sequence, every scalar and every input's bits are compared with
the module's graph.  The forwards are small: the product's widths (N, K, heads and LayerNorm C are the product's), few layers
and few images; every configuration is registered at run time and every parameter is seeded.

First run on an MI355X (launches audited; worst |out - fp64| / bound per entry point, every one <= 1; exact kernels 0):
  DINOv2 tiny154 / tiny84 / vits14-2l / vitb14-2l / vitl14-2l: 19 launches each; gemm_f16 0.90 / 0.89 / 0.71 / 0.56 / 0.55,
    gemm_f16_act 0.85 / 0.83 / 0.67 / 0.48 / 0.37, gemm_f16_res32 0.13 / 0.10 / 0.02 / 0.004 / 0.002, layernorm_f32 0.99 each,
    attention_long 0.31 / - / 0.29 / 0.36 / 0.40, attention (tiny84) 0.48
  outliers, tiny154 / vitl14-2l: 19 each; gemm_f16 0.94 / 0.75, act 0.91 / 0.69, res32 0.68 / 0.38, layernorm_f32 0.99 / 0.99,
    attention_long 0.43 / 0.39; stream maximum 3003 / 3005, median 0.29 / 0.47; 1 - cos HipDino 3.2e-11 / 1.4e-08 against
    autocast 3.0e-10 / 1.9e-08
  CLIP b32-2l image 21: gemm 0.88, layernorm_f16 0.99, attention 0.55; l14-336-1l / l14-154-1l 14 each: gemm 0.86 / 0.81,
    layernorm 0.99, attention_long 0.20 / 0.31; text at 77 / 14 tokens 18 each: gemm 0.70 / 0.69, layernorm 0.99, attention 0.73 / 0.74
  tiny audits in four processes (one per GEMM instance), 19 + 19 + 21 + 11 launches each: the same figures on every instance
    (gemm 0.97, act 0.85, res32 0.13); b32-1l at 328 images 14 launches: gemm 0.87, layernorm 0.99, attention 0.64
Wall time: the four processes 8.3 s, the tiny outliers condition 4.8 s (the first autocast forward), every other test 0.02-1.3 s.
No launch exceeded its bound, so no kernel and no derivation changed.
"""
import collections
import json
import os
import subprocess
import sys
import time

import pytest
import torch

from tests import _tower_audit as A

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _report(name, chk, t0):
    for k, entry, where, ratio, inst in chk.rows:
        print(f"{name} launch {k:3d} {entry:26s} {where:40s} ratio {ratio:.4f} {inst or ''}")
    print(f"{name}: {len(chk.names)} launches audited, worst ratio per entry point {chk.summary()['worst']}, instances "
          f"{sorted(chk.instances)}, checks {chk.seconds:.1f} s, wall {time.time() - t0:.1f} s")
    assert not chk.failures, f"{name}: {len(chk.failures)} failures:\n" + "\n".join(m for _, _, m in chk.failures)


# ------------------------------------------------------------------------------------------------------------ DINOv2
def _dino_cfg(case):
    from tise_toolbox_amd import dinov2_model
    return {"tiny154": A.TINY154, "tiny84": A.TINY84,
            "vits14-2l": dict(dinov2_model.CONFIGS["vits14"], layers=2), "vitb14-2l": dict(dinov2_model.CONFIGS["vitb14"], layers=2),
            "vitl14-2l": dict(dinov2_model.CONFIGS["vitl14"], layers=2)}[case.replace("-outliers", "")]


def _dino_model(case, monkeypatch, dev):
    """The seeded module of a configuration registered for the test; ``-outliers``: A.make_outliers_ on top."""
    from tise_toolbox_amd import dinov2_model
    name = "audit-" + case
    monkeypatch.setitem(dinov2_model.CONFIGS, name, _dino_cfg(case))
    model = dinov2_model.build_dinov2(None, 0, name)
    if case.endswith("-outliers"):
        A.make_outliers_(model)
    return model.to(dev)


DINO_CASES = ["tiny154", "tiny84", "vits14-2l", "vitb14-2l", "vitl14-2l", "tiny154-outliers", "vitl14-2l-outliers"]


@pytest.mark.timeout(120)
@pytest.mark.parametrize("case", DINO_CASES)
def test_dinov2_every_launch_matches_fp64_and_the_modules_graph(cuda_device, monkeypatch, case):
    """HipDino: the tiny towers (122 tokens: the long attention kernel; 37: the short one) on 3 images, ViT-S / B / L widths
    (384 / 6 heads, 768 / 12, 1024 / 16) with 2 layers at 224 on 2 images, and the ``outliers`` parameter sets (the stream
    beyond 1e3 on a few tokens and channels with its median below 10: a condition on the construction, asserted).  3 + 7 x
    layers + 2 launches each; every check of tests/_tower_audit.Checker; the recorded forward gives the bits of a plain one."""
    from tise_toolbox_amd import clip_hip, dinov2_hip
    t0 = time.time()
    model = _dino_model(case, monkeypatch, cuda_device)
    cfg = _dino_cfg(case)
    image = A.seeded_images(3 if case.startswith("tiny") else 2, cfg["resolution"], 5, cuda_device)
    chk, feat = A.audit_dino(model, image, cuda_device)
    _report(case, chk, t0)
    assert len(chk.names) == 5 + 7 * cfg["layers"]
    seq = (cfg["resolution"] // 14) ** 2 + 1
    long = seq > clip_hip.ATTN_SHORT_MAX_SEQ
    assert chk.names.count("tise_attention_long_f16") == (cfg["layers"] if long else 0)
    assert chk.names.count("tise_attention_f16") == (0 if long else cfg["layers"])
    assert torch.equal(feat, dinov2_hip.HipDino(model, cuda_device).encode_image(image.half()))
    big, median = chk.stream_stats
    print(f"{case}: the fp32 stream's largest |x| {big:.1f}, median |x| after the last update {median:.3f}")
    if case.endswith("-outliers"):
        assert big >= 1e3 and median < 10, (big, median)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("case", ["tiny154-outliers", "vitl14-2l-outliers"])
def test_dinov2_end_to_end_condition_holds_on_outliers(cuda_device, monkeypatch, case):
    """tests/test_gpu_dinov2.py's condition on the ``outliers`` parameters: 1 - cos(HipDino, fp32 module) <= 2 x (1 -
    cos(autocast module, fp32 module)).  tests/test_dinov2_host.py shows on the same parameters and images that an fp16 stream
    misses it by more than a factor 10 (tiny154)."""
    from tests.test_gpu_dinov2 import _compare
    from tise_toolbox_amd import dinov2_hip
    t0 = time.time()
    model = _dino_model(case, monkeypatch, cuda_device)
    n = 3 if case.startswith("tiny") else 2
    trio = (dinov2_hip.HipDino(model, cuda_device), dinov2_hip.AutocastDino(model, cuda_device), model)
    _, _, e_hip, e_auto = _compare(trio, n, cuda_device, 5)
    print(f"{case}: 1 - cos HipDino {e_hip:.3e}, autocast {e_auto:.3e}, wall {time.time() - t0:.1f} s")
    assert e_hip <= 2 * e_auto, (e_hip, e_auto)


# -------------------------------------------------------------------------------------------------------------- CLIP
def _clip_cfg(case):
    from tise_toolbox_amd import clip_model
    b32, l14 = clip_model.CONFIGS["ViT-B/32"], clip_model.CONFIGS["ViT-L/14@336"]
    return {"b32-2l": dict(b32, layers=2, text_layers=2), "b32-1l": dict(b32, layers=1, text_layers=1),
            "l14-336-1l": dict(l14, layers=1, text_layers=1), "l14-154-1l": dict(l14, layers=1, text_layers=1, resolution=154)}[case]


def _clip_model(case, monkeypatch, dev):
    from tise_toolbox_amd import clip_model
    name = "audit-" + case
    monkeypatch.setitem(clip_model.CONFIGS, name, _clip_cfg(case))
    return A.fill_defaults_(clip_model.build_clip(None, 0, name)).to(dev)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("case,images,seq,patchify", [("b32-2l", 3, 50, "tise_patchify_f16"), ("l14-336-1l", 2, 577, "tise_patchify_pad_f16"),
                                                      ("l14-154-1l", 2, 122, "tise_patchify_pad_f16")])
def test_clip_image_every_launch_matches_fp64_and_the_modules_graph(cuda_device, monkeypatch, case, images, seq, patchify):
    """HipTowers.encode_image: ViT-B/32 shapes with 2 layers on 3 images (50 tokens, tise_patchify_f16, kpad = 0, the short
    attention kernel) and an L/14-shaped tower of width 1024 with 1 layer on 2 images at 336 (577 tokens) and at 154 (122): the
    padded patch matrix and the long attention kernel.  4 + 7 x layers + 3 launches."""
    from tise_toolbox_amd import clip_hip
    t0 = time.time()
    model = _clip_model(case, monkeypatch, cuda_device)
    cfg = _clip_cfg(case)
    towers = clip_hip.HipTowers(model, cuda_device)
    assert (towers.kpad == 0) == (patchify == "tise_patchify_f16")
    image = A.seeded_images(images, cfg["resolution"], 7, cuda_device)
    chk, feat = A.audit_clip_image(model, image, cuda_device, towers)
    _report(case, chk, t0)
    assert len(chk.names) == 7 + 7 * cfg["layers"] and chk.names[0] == patchify
    assert chk.names.count("tise_attention_long_f16" if seq > clip_hip.ATTN_SHORT_MAX_SEQ else "tise_attention_f16") == cfg["layers"]
    assert (cfg["resolution"] // cfg["patch"]) ** 2 + 1 == seq
    assert torch.equal(feat, towers.encode_image(image))


@pytest.mark.timeout(120)
def test_clip_text_every_launch_at_77_tokens_and_truncated(cuda_device, monkeypatch):
    """HipTowers.encode_text on ViT-B/32's text shapes (width 512, 8 heads) with 2 layers: 5 captions at the full 77 tokens, and
    the same captions through RP_coco.embed_texts, which encodes a batch at its longest caption (14 tokens here): causal
    short-attention launches at seq < 32 and at 77, the end-of-text gather index, the position table's first rows."""
    from tise_toolbox_amd import RP_coco, clip_hip, clip_model
    t0 = time.time()
    monkeypatch.delenv("TISE_CLIP_TRUNCATE", raising=False)
    model = _clip_model("b32-2l", monkeypatch, cuda_device)
    towers = clip_hip.HipTowers(model, cuda_device)
    tok = clip_model.HashTokenizer()
    text = tok(list(A.CAPTIONS)).to(cuda_device)
    assert text.shape == (5, 77)
    chk, feat = A.audit_clip_text(model, text, cuda_device, towers)
    _report("b32-2l text at 77 tokens", chk, t0)
    assert len(chk.names) == 1 + 7 * 2 + 3 and chk.names.count("tise_attention_f16") == 2
    assert torch.equal(feat, towers.encode_text(text))
    # through embed_texts: every encode_text call it makes is audited against the plan of the ids it was handed
    seen = []
    plain = towers.encode_text

    def audited(ids):
        c, out = A.check_assembly(A.clip_text_plan(model, ids, cuda_device), lambda: plain(ids))
        seen.append((tuple(ids.shape), c))
        return out
    towers.encode_text = audited                                      # on the instance: the class keeps its method
    emb = RP_coco.embed_texts(towers, tok, list(A.CAPTIONS), cuda_device, 8)
    del towers.encode_text
    longest = int(text.argmax(-1).max()) + 1                          # the end-of-text token of the longest caption
    assert [s for s, _ in seen] == [(5, longest)] and longest == 14
    _report("b32-2l text truncated to 14 tokens", seen[0][1], t0)
    assert len(seen[0][1].names) == 18
    full = feat.float() / feat.float().norm(dim=-1, keepdim=True)
    cos = (emb.float() * full).sum(-1)
    print(f"truncated against 77 tokens: smallest cosine {cos.min().item():.6f}")
    assert cos.min().item() > 0.999                                  # nothing behind the end-of-text token reaches the feature


# --------------------------------------------------------------------------------------------------- GEMM instances
# tests/test_gpu_dinov2_kernels._CHILD_ENVS: gemm_f16_big_kernel, gemm16_f16_kernel<true>, gemm_f16_kernel
@pytest.mark.timeout(500)
def test_every_gemm_instance_runs_on_a_towers_operands(cuda_device):
    """The tiny DINOv2 and CLIP audits (A.run_tiny_audits) in this process (gemm16_f16_kernel<false>) and in fresh child
    processes under the three environments of tests/test_gpu_dinov2_kernels.py, ONE AT A TIME, each under that test's time limit;
    no child is started after one fails.  Every launch of every child passes the same audit; together the four kernel instances
    ran on tower launches, each with the three epilogues (fp16, act = 2, res32)."""
    from tests.test_gpu_dinov2_kernels import _CHILD_ENVS
    t0 = time.time()
    here = A.run_tiny_audits(cuda_device)
    seen = collections.Counter()
    for name, rec in here.items():
        assert not rec["failures"], (name, rec["failures"])
        assert rec["instances"] == ["gemm16_f16_kernel<false>"], (name, rec)
        seen.update(rec["instances"])
    print(f"default: {json.dumps(here)}")
    torch.cuda.empty_cache()
    for extra, instance in _CHILD_ENVS:
        env = {k: v for k, v in os.environ.items() if k not in ("TISE_GEMM_SHAPE", "TISE_GEMM_BIG")}
        env.update(extra)
        try:
            p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_tower_audit.py")], env=env, cwd=ROOT, capture_output=True,
                               text=True, timeout=120)
        except subprocess.TimeoutExpired as e:
            pytest.fail(f"child {extra} timed out; stderr:\n{e.stderr}")
        assert p.returncode == 0, f"child {extra} exit {p.returncode}; stderr:\n{p.stderr[-6000:]}"
        res = json.loads(p.stdout.strip().splitlines()[-1])
        assert res["env"] == extra and sorted(res["audits"]) == sorted(here)
        print(f"child {extra}: {json.dumps(res['audits'])}")
        for name, rec in res["audits"].items():
            assert not rec["failures"], (extra, name, rec["failures"])
            assert rec["launches"] == here[name]["launches"] and rec["instances"] == [instance], (extra, name, rec)
            assert all(v <= 1.0 for v in rec["worst"].values()), (extra, name, rec)
            seen.update(rec["instances"])
    print(f"instances on tower launches: {dict(seen)}; wall {time.time() - t0:.1f} s")
    assert set(seen) == A.ALL_INSTANCES, seen


@pytest.mark.timeout(300)
def test_the_instance_rule_inside_one_forward(cuda_device, monkeypatch):
    """ViT-B/32 image shapes, 1 layer, 328 images = 16 400 rows: c_fc (N = 3072: 65 x 12 = 780 tiles of 256 x 256) crosses the
    768-tile rule and runs on gemm_f16_big_kernel; in_proj (N = 2304: 585 tiles), out_proj, c_proj (N = 768: 195) and the patch
    and projection GEMMs stay on gemm16_f16_kernel<false>: two instances inside one forward, every launch audited."""
    from tise_toolbox_amd import clip_hip
    t0 = time.time()
    model = _clip_model("b32-1l", monkeypatch, cuda_device)
    towers = clip_hip.HipTowers(model, cuda_device)
    image = A.seeded_images(328, 224, 9, cuda_device)
    chk, feat = A.audit_clip_image(model, image, cuda_device, towers)
    _report("b32-1l at 328 images", chk, t0)
    where = {w: inst for _, _, w, _, inst in chk.rows if inst}
    assert where["visual.transformer.resblocks.0.mlp.c_fc"] == "gemm_f16_big_kernel"
    assert {w for w, inst in where.items() if inst != "gemm16_f16_kernel<false>"} == {"visual.transformer.resblocks.0.mlp.c_fc"}
    assert len(where) == 6 and set(chk.instances) == {"gemm_f16_big_kernel", "gemm16_f16_kernel<false>"}
    assert torch.equal(feat, towers.encode_image(image))
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ the audit has teeth
def _swap_layerscales(tower):
    blk = tower.blocks[1]
    blk.ls1, blk.ls2 = blk.ls2, blk.ls1


def _bias_of_the_neighbour(tower):
    blk = tower.blocks[0]
    blk.b_proj = blk.b_fc2.clone()                                   # the same shape: (width,)


def _final_eps(tower):
    tower.norm = (tower.norm[0], tower.norm[1], 1e-5)


# launches of the tiny tower: 0 patchify, 1 patch GEMM, 2 tokens; block i from 3 + 7 i: norm1, qkv, attention, proj (res32),
# norm2, fc1, fc2 (res32); 17 gather, 18 norm
@pytest.mark.timeout(120)
@pytest.mark.parametrize("mutate,launches,reasons", [
    (_swap_layerscales, {13, 16}, {(13, "input:scale"), (13, "numeric"), (16, "input:scale"), (16, "numeric")}),
    (_bias_of_the_neighbour, {6}, {(6, "input:bias"), (6, "numeric")}),
    (_final_eps, {18}, {(18, "scalar:eps")}),
], ids=["ls1-ls2-swapped", "b_proj-from-b_fc2", "final-eps-1e-5"])
def test_a_wrong_tower_fails_the_audit_at_that_launch(cuda_device, monkeypatch, mutate, launches, reasons):
    """Three mistakes made on a built HipDino INSTANCE (never in product code), wrong numerics only: block 1's ls1 and ls2
    swapped; block 0's b_proj with the values of b_fc2; the final norm's eps 1e-5.  Each fails the audit at exactly the launches
    that read the wrong operand, for the stated reasons, and at no other: every later launch is checked on its own recorded
    input.  The unmutated tower passes (test_dinov2_every_launch_...[tiny154])."""
    model = _dino_model("tiny154", monkeypatch, cuda_device)
    image = A.seeded_images(3, 154, 5, cuda_device)
    chk, _ = A.audit_dino(model, image, cuda_device, mutate=mutate)
    got = {(k, r) for k, r, _ in chk.failures}
    for _, _, m in chk.failures:
        print(m)
    assert {k for k, _ in got} == launches, got
    assert reasons <= got, (reasons - got, got)
    assert min(k for k, _ in got) == min(launches)
