"""GPU: the ViT-L/14@336 image tower on the hand-written kernels (clip_hip.HipTowers over tise_attention_long_f16 and
tise_patchify_pad_f16) against clip_model.CLIP in fp32 on the same fp16-rounded seeded parameters: two tiny configurations of
the same shape family (patch 14: 122 and 577 tokens), the full seeded tower once, the 336-pixel preprocess on the device, and
cmmd's command line under a tower registered for the test.

THE CONDITION on the towers: for the worst image, 1 - cos(HipTowers, fp32 module) <= 2 x (1 - cos(library fp16 module, fp32
module)).  The yardstick is PyTorch's own fp16 forward of the same graph on the same parameters, not the code under test; the
factor 2 allows two fp16 evaluation orders of one graph to differ by O(1).  Cosines are taken in float64 (the differences are
of the order of fp32's own rounding).  The tiny towers (2 layers) also meet tests/test_gpu_clip.py's 0.9995.

Figures of the first run on an MI355X (1 - cos against the fp32 module, worst image; HipTowers / library fp16 module):
tiny 154 px 2.907e-07 / 3.197e-07, tiny 336 px 2.417e-07 / 2.294e-07, full ViT-L/14@336 1.423e-06 / 1.367e-06."""
import copy
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TINY = dict(resolution=154, patch=14, width=128, layers=2, heads=2, embed_dim=64, text_width=64, text_layers=1, text_heads=1)
TINY336 = dict(TINY, resolution=336)
TINY_NAME = "tiny-test/14@154"


def _one_minus_cos(a, b):
    a, b = a.double(), b.double()
    return 1 - (a * b).sum(-1) / (a.norm(dim=-1) * b.norm(dim=-1))


def _trio(arch, dev, seed=0):
    """-> (HipTowers, the fp16 library module it was built from, the fp32 module on the fp16-rounded parameters)."""
    from tise_toolbox_amd import clip_hip, clip_model
    model_h = clip_model.build_clip(None, seed, arch).to(dev).half()
    ref = copy.deepcopy(model_h).float()
    return clip_hip.HipTowers(model_h, dev), model_h, ref


def _compare(trio, n, dev, seed):
    towers, model_h, ref = trio
    g = torch.Generator(device="cpu").manual_seed(seed)
    img = torch.randn((n, 3, towers.resolution, towers.resolution), generator=g).to(dev)
    with torch.no_grad():
        fi = towers.encode_image(img)
        ri = ref.encode_image(img.half().float())
        li = model_h.encode_image(img.half())
    assert fi.shape == (n, towers.out_dim) and fi.dtype == torch.float16 and torch.isfinite(fi).all()
    hip, lib = _one_minus_cos(fi, ri).max().item(), _one_minus_cos(li, ri).max().item()
    print(f"1 - cos against the fp32 module, worst of {n} images: HipTowers {hip:.3e}, library fp16 module {lib:.3e}")
    assert torch.equal(towers.encode_image(img), fi)                                   # repeatable bits
    return img, fi, hip, lib


@pytest.mark.parametrize("cfg", [TINY, TINY336], ids=["154px-122tok", "336px-577tok"])
def test_tiny_l14_shaped_tower_matches_fp32_module(cuda_device, cfg):
    """Resolution 154 / 336, patch 14, width 128, 2 layers, 2 heads, 64-d: 122 / 577 tokens through the long-sequence
    attention, the padded patch GEMM (588 -> 640 columns) and the token kernels; 8 images.  The condition of the module
    docstring, and cos >= 0.9995 as tests/test_gpu_clip.py::test_towers_match_fp32_module."""
    trio = _trio(cfg, cuda_device)
    assert trio[0].kpad == 640 and trio[0].resolution == cfg["resolution"] and trio[0].out_dim == 64
    img, fi, hip, lib = _compare(trio, 8, cuda_device, 5)
    assert hip <= 2 * lib, (hip, lib)
    assert 1 - hip >= 0.9995
    one = torch.cat([trio[0].encode_image(img[k:k + 1]) for k in range(8)])            # batch invariance
    assert torch.equal(one, fi)


@pytest.fixture(scope="module")
def full_l14(cuda_device):
    return _trio("ViT-L/14@336", cuda_device)


@pytest.mark.timeout(600)
def test_full_l14_336_tower_matches_fp32_module(cuda_device, full_l14):
    """The full seeded ViT-L/14@336 (24 layers, width 1024, 16 heads, 577 tokens, 768-d) on 4 images: the module docstring's
    condition; shape (n, 768), fp16, repeatable bits; image k alone gives the bits of image k in the batch of 4.
    First run on an MI355X: HipTowers 1.423e-06, library fp16 module 1.367e-06 (ratio 1.04 against the allowed 2)."""
    img, fi, hip, lib = _compare(full_l14, 4, cuda_device, 6)
    assert fi.shape == (4, 768)
    assert hip <= 2 * lib, (hip, lib)
    towers = full_l14[0]
    one = torch.cat([towers.encode_image(img[k:k + 1]) for k in range(4)])
    assert torch.equal(one, fi)


@pytest.mark.parametrize("h,w", [(256, 256), (400, 300), (300, 500)])
def test_preprocess_device_at_336_equals_pillow(cuda_device, h, w):
    """preprocess_device(x, size=336) == torch.stack([preprocess(img, size=336) ...]) bit for bit: an up-sample (256 x 256),
    a tall and a wide image with a crop."""
    from PIL import Image
    from tise_toolbox_amd import clip_model
    rng = np.random.default_rng(h + w)
    batch = rng.integers(0, 256, (3, h, w, 3), dtype=np.uint8)
    got = clip_model.preprocess_device(torch.from_numpy(batch).to(cuda_device), size=336)
    want = torch.stack([clip_model.preprocess(Image.fromarray(im), size=336) for im in batch])
    assert got.shape == (3, 3, 336, 336) and got.dtype == torch.float32
    assert torch.equal(got.cpu(), want)


def _png_dir(path, n, seed):
    from PIL import Image
    from tests import _cases
    os.makedirs(path)
    pool = _cases.smooth_images(12, 64, 64, seed=seed)
    for k in range(n):
        Image.fromarray(np.ascontiguousarray(np.roll(pool[k % 12], 3 * k + seed, axis=1))).save(os.path.join(path, f"{k:04d}.png"))
    return str(path)


@pytest.mark.timeout(300)
def test_cmmd_cli_under_a_registered_tower(cuda_device, tmp_path, capfd, monkeypatch):
    """cmmd.main end to end with --tower naming a tiny patch-14 configuration registered for the test: the result lines name
    the tower, the value is cmmd_from_features of embed_image_dir's rows, the feature file carries the tower's tag, reproduces
    the lines under the same tower and is refused under ViT-B/32."""
    from tise_toolbox_amd import RP_coco, clip_hip, clip_model, cmmd, fid_score
    from tise_toolbox_amd.weights import SYNTHETIC_TAG
    monkeypatch.setitem(clip_model.CONFIGS, TINY_NAME, TINY)
    ref, gen = _png_dir(tmp_path / "ref", 12, 3), _png_dir(tmp_path / "gen", 12, 4)
    out_npz = str(tmp_path / "ref.npz")
    tail = ["--path2", gen, "--batch-size", "5", "--num-workers", "2", "--synthetic-weights", "--clip-fid", "--tower", TINY_NAME]
    capfd.readouterr()
    value, fid = cmmd.main(["--path1", ref] + tail + ["--save-features", out_npz])
    lines = [ln for ln in capfd.readouterr().out.splitlines() if ln.startswith(("CMMD (", "CLIP-FID ("))]
    towers = RP_coco.build_towers(None, cuda_device, TINY_NAME)[0]
    assert isinstance(towers, clip_hip.HipTowers) and (towers.resolution, towers.out_dim) == (154, 64)
    r1 = cmmd.embed_image_dir(towers, ref, cuda_device, 5, workers=2)
    r2 = cmmd.embed_image_dir(towers, gen, cuda_device, 5, workers=2)
    assert r1.shape == (12, 64) and r2.shape == (12, 64)
    want = cmmd.cmmd_from_features(r1, r2)
    (m1, s1), (m2, s2) = cmmd.clip_statistics(r1), cmmd.clip_statistics(r2)
    want_fid = float(fid_score.calculate_frechet_distance(m1, s1, m2, s2))
    assert lines == [f"CMMD ({TINY_NAME}): {want}{SYNTHETIC_TAG}", f"CLIP-FID ({TINY_NAME}): {want_fid}{SYNTHETIC_TAG}"]
    assert (value, fid) == (want, want_fid)
    empty = RP_coco.encode_paths(towers, [], cuda_device, 5, 0, "ring", True, lambda f: f.float(), torch.float32)
    assert empty.shape == (0, 64)
    with np.load(out_npz) as f:
        assert str(f["network"]) == "clip-tiny-test-14-154" and np.array_equal(f["features"], r1.cpu().numpy())
    again = cmmd.main(["--path1", out_npz] + tail)
    lines_npz = [ln for ln in capfd.readouterr().out.splitlines() if ln.startswith(("CMMD (", "CLIP-FID ("))]
    assert lines_npz == lines and again == (value, fid)
    assert cmmd.calculate_cmmd_given_paths([out_npz, gen], 5, num_workers=2, tower=TINY_NAME) == value
    with pytest.raises(RuntimeError, match="clip-tiny-test-14-154"):
        cmmd.main(["--path1", out_npz, "--path2", gen, "--batch-size", "5", "--synthetic-weights", "--tower", "ViT-B/32"])
