"""GPU: the DINOv2 tower on the hand-written kernels (dinov2_hip.HipDino: an fp32 residual stream over tise_gemm_f16_res32,
tise_layernorm_f32 and tise_gemm_f16_act's exact GELU) against dinov2_model.DinoVisionTransformer in fp32 on the same seeded
parameters: two tiny registered towers (patch 14; 122 tokens: the long attention kernel, 37 tokens: the short one), the full
seeded vitl14 at 224 once, the preprocessing on the device, and fd_dinov2's command line end to end.

THE CONDITION on the tower, as tests/test_gpu_clip_l14.py words it: for the worst image,
    1 - cos(HipDino, fp32 module) <= 2 x (1 - cos(the module under torch.autocast(fp16), fp32 module)),
both measured here and printed, and cos >= 0.9995.  The yardstick is PyTorch's own autocast forward of the same graph on the same
parameters -- its residual stream is fp32 -- not the code under test; the factor 2 allows two evaluation orders of one graph to
differ by O(1).  An fp16-stream implementation is not expected to meet this at 24 layers; that is the point.  Cosines are taken
in float64.

Figures of the first run on an MI355X (1 - cos against the fp32 module, worst image; HipDino / autocast module):
tiny 154 px (122 tokens) 9.655e-08 / 1.628e-07, tiny 84 px (37 tokens) 1.215e-07 / 1.796e-07, full vitl14 at 224 on 2 images
4.049e-07 / 7.413e-07 (ratio 0.55 against the allowed 2)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TINY154 = dict(width=128, layers=2, heads=2, patch=14, resolution=154)      # 11 x 11 + 1 = 122 tokens: tise_attention_long_f16
TINY84 = dict(width=128, layers=2, heads=2, patch=14, resolution=84)        # 6 x 6 + 1 = 37 tokens: tise_attention_f16
TINY_NAME = "tiny-test14"


def _one_minus_cos(a, b):
    a, b = a.double(), b.double()
    return 1 - (a * b).sum(-1) / (a.norm(dim=-1) * b.norm(dim=-1))


def _trio(arch, dev, seed=0):
    """-> (HipDino, the autocast route over the same module, the fp32 module)."""
    from tise_toolbox_amd import dinov2_hip, dinov2_model
    model = dinov2_model.build_dinov2(None, seed, arch).to(dev)
    return dinov2_hip.HipDino(model, dev), dinov2_hip.AutocastDino(model, dev), model


def _compare(trio, n, dev, seed):
    hip, auto, ref = trio
    g = torch.Generator(device="cpu").manual_seed(seed)
    img = torch.randn((n, 3, hip.resolution, hip.resolution), generator=g).to(dev).half()   # what encode_paths hands over
    with torch.no_grad():
        fi = hip.encode_image(img)
        ri = ref(img.float())
        ai = auto.encode_image(img)
    assert fi.shape == (n, hip.out_dim) and fi.dtype == torch.float32 and torch.isfinite(fi).all()
    assert ai.shape == fi.shape and ai.dtype == torch.float32
    e_hip, e_auto = _one_minus_cos(fi, ri).max().item(), _one_minus_cos(ai, ri).max().item()
    print(f"1 - cos against the fp32 module, worst of {n} images: HipDino {e_hip:.3e}, autocast module {e_auto:.3e}")
    assert torch.equal(hip.encode_image(img), fi)                                           # repeatable bits
    return img, fi, e_hip, e_auto


@pytest.mark.parametrize("cfg,kernel_seq", [(TINY154, 122), (TINY84, 37)], ids=["154px-122tok-long", "84px-37tok-short"])
def test_tiny_tower_matches_fp32_module(cuda_device, cfg, kernel_seq):
    """Patch 14, width 128, 2 heads, 2 layers, 3 images: the condition of the module docstring, cos >= 0.9995, repeatable bits,
    and batch 1 equals the row of batch 3."""
    from tise_toolbox_amd import clip_hip
    trio = _trio(cfg, cuda_device)
    hip = trio[0]
    assert (hip.kpad, hip.resolution, hip.out_dim) == (640, cfg["resolution"], 128)
    assert hip.pos.shape[0] == kernel_seq and (kernel_seq > clip_hip.ATTN_SHORT_MAX_SEQ) == (cfg is TINY154)
    assert hip.pos.dtype == hip.cls.dtype == hip.blocks[0].ls1.dtype == hip.norm[0].dtype == torch.float32
    assert hip.blocks[0].w_fc2.dtype == hip.blocks[0].b_fc2.dtype == torch.float16
    img, fi, e_hip, e_auto = _compare(trio, 3, cuda_device, 5)
    assert e_hip <= 2 * e_auto, (e_hip, e_auto)
    assert 1 - e_hip >= 0.9995
    one = torch.cat([hip.encode_image(img[k:k + 1]) for k in range(3)])
    assert torch.equal(one, fi)
    assert hip.encode_image(img[:0]).shape == (0, 128)


@pytest.mark.timeout(600)
def test_full_vitl14_matches_fp32_module(cuda_device):
    """The full seeded vitl14 (24 layers, width 1024, 16 heads, 257 tokens at 224) on 2 images: the module docstring's
    condition and cos >= 0.9995; shape (2, 1024), fp32, repeatable bits; image k alone gives the bits of image k in the batch."""
    trio = _trio("vitl14", cuda_device)
    img, fi, e_hip, e_auto = _compare(trio, 2, cuda_device, 6)
    assert fi.shape == (2, 1024)
    assert e_hip <= 2 * e_auto, (e_hip, e_auto)
    assert 1 - e_hip >= 0.9995
    one = torch.cat([trio[0].encode_image(img[k:k + 1]) for k in range(2)])
    assert torch.equal(one, fi)


@pytest.mark.parametrize("h,w", [(256, 256), (301, 203)])
def test_preprocess_device_equals_pillow(cuda_device, h, w):
    """preprocess_device(x) == torch.stack([preprocess(img) ...]) bit for bit on 3 images: a down-sample of a square and an odd
    size stretched to the square."""
    from PIL import Image
    from tise_toolbox_amd import dinov2_model
    rng = np.random.default_rng(h + w)
    batch = rng.integers(0, 256, (3, h, w, 3), dtype=np.uint8)
    got = dinov2_model.preprocess_device(torch.from_numpy(batch).to(cuda_device))
    want = torch.stack([dinov2_model.preprocess(Image.fromarray(im)) for im in batch])
    assert got.shape == (3, 3, 224, 224) and got.dtype == torch.float32
    assert torch.equal(got.cpu(), want)


def _png_dir(path, n, seed):
    from PIL import Image
    from tests import _cases
    os.makedirs(path)
    pool = _cases.smooth_images(12, 64, 64, seed=seed)
    for k in range(n):
        Image.fromarray(np.ascontiguousarray(np.roll(pool[k % 12], 3 * k + seed, axis=1))).save(os.path.join(path, f"{k:04d}.png"))
    return str(path)


_PREFIXES = ("FD-DINOv2 (", "KD-DINOv2 (", "Precision-DINOv2 (", "Recall-DINOv2 (", "Density-DINOv2 (", "Coverage-DINOv2 (")


@pytest.mark.timeout(300)
def test_cli_end_to_end_under_a_registered_tiny_tower(cuda_device, tmp_path, capfd, monkeypatch):
    """fd_dinov2.main on two directories of 12 seeded 64 x 64 PNGs under a tiny tower registered for the test, with
    --synthetic-weights --kd --prdc --save-features: the FD line equals calculate_frechet_distance of np.mean / np.cov of the
    saved rows within 1e-6 relative; KD and PRDC equal kid_from_features / prdc_from_features on the same rows exactly; a rerun
    from the feature file prints identical lines; the file is refused under another arch."""
    from tise_toolbox_amd import dinov2_model, fd_dinov2, fid_score, kid, prdc
    from tise_toolbox_amd.weights import SYNTHETIC_TAG
    monkeypatch.setitem(dinov2_model.CONFIGS, TINY_NAME, TINY154)
    monkeypatch.delenv("TISE_DINO", raising=False)
    ref, gen = _png_dir(tmp_path / "ref", 12, 3), _png_dir(tmp_path / "gen", 12, 4)
    out_npz, out_txt = str(tmp_path / "ref.npz"), str(tmp_path / "lines.txt")
    tail = ["--path2", gen, "--batch-size", "5", "--num-workers", "2", "--synthetic-weights", "--kd", "--prdc", "--arch", TINY_NAME]
    capfd.readouterr()
    res = fd_dinov2.main(["--path1", ref] + tail + ["--save-features", out_npz, "--saved_file", out_txt])
    lines = [ln for ln in capfd.readouterr().out.splitlines() if ln.startswith(_PREFIXES)]
    assert len(lines) == 6 and all(ln.endswith(SYNTHETIC_TAG) for ln in lines) and open(out_txt).read() == "\n".join(lines)
    assert [ln.split(":")[0] for ln in lines] == [p + TINY_NAME + ")" for p in _PREFIXES]
    with np.load(out_npz) as f:
        assert str(f["network"]) == "dinov2-" + TINY_NAME
        r1 = np.array(f["features"])
    assert r1.shape == (12, 128) and r1.dtype == np.float32 and np.isfinite(r1).all() and np.unique(r1, axis=0).shape[0] == 12
    # the generated side's rows, through the Python entry points
    from tise_toolbox_amd import cmmd, dinov2_hip
    tower = dinov2_hip.build_tower(None, cuda_device, TINY_NAME, 0)
    assert isinstance(tower, dinov2_hip.HipDino)
    assert np.array_equal(cmmd.embed_image_dir(tower, ref, cuda_device, 5, workers=2).cpu().numpy(), r1)
    r2 = cmmd.embed_image_dir(tower, gen, cuda_device, 5, workers=2).cpu().numpy()
    want_fd = float(fid_score.calculate_frechet_distance(np.mean(r1.astype(np.float64), 0), np.cov(r1.astype(np.float64), rowvar=False),
                                                         np.mean(r2.astype(np.float64), 0), np.cov(r2.astype(np.float64), rowvar=False)))
    assert abs(res["fd"] - want_fd) <= 1e-6 * abs(want_fd), (res["fd"], want_fd)
    assert lines[0] == f"FD-DINOv2 ({TINY_NAME}): {res['fd']}{SYNTHETIC_TAG}"
    assert abs(fd_dinov2.fd_dinov2_from_features(r1, r2) - want_fd) <= 1e-6 * abs(want_fd)
    want_kd = kid.kid_from_features(r1, r2, subsets=100, subset_size=1000)
    want_prdc = prdc.prdc_from_features(r1, r2, nearest_k=5)
    assert res["kd"] == want_kd and dict(res["prdc"]) == dict(want_prdc)
    assert lines[1] == f"KD-DINOv2 ({TINY_NAME}): {want_kd[0]} +- {want_kd[1]}{SYNTHETIC_TAG}"
    assert lines[2:] == [f"{k.capitalize()}-DINOv2 ({TINY_NAME}): {want_prdc[k]}{SYNTHETIC_TAG}" for k in ("precision", "recall", "density", "coverage")]
    # the feature file in place of the directory: the same lines
    fd_dinov2.main(["--path1", out_npz] + tail)
    assert [ln for ln in capfd.readouterr().out.splitlines() if ln.startswith(_PREFIXES)] == lines
    # another architecture refuses it; no parameters and no --synthetic-weights is refused too
    monkeypatch.setitem(dinov2_model.CONFIGS, "tiny-other14", TINY84)
    with pytest.raises(RuntimeError, match="dinov2-" + TINY_NAME):
        fd_dinov2.main(["--path1", out_npz, "--path2", gen, "--synthetic-weights", "--arch", "tiny-other14"])
    with pytest.raises(RuntimeError, match="no parameters for DINOv2"):
        fd_dinov2.main(["--path1", ref, "--path2", gen, "--arch", TINY_NAME])
    # the A/B route gives the same metric up to the towers' difference
    monkeypatch.setenv("TISE_DINO", "torch")
    auto = dinov2_hip.build_tower(None, cuda_device, TINY_NAME, 0)
    assert isinstance(auto, dinov2_hip.AutocastDino)
    ra = cmmd.embed_image_dir(auto, ref, cuda_device, 5, workers=2)
    assert _one_minus_cos(ra.cpu(), torch.from_numpy(r1)).max().item() < 1e-5
