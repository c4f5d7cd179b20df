"""GPU: the whole ResNet-50 route (resnet_hip.HipResNet50) against the seeded module's fp64 CPU forward, its invariances, the range
guard, and the fd_swav CLI end to end.

The bound of the route: per row ||dev - ref||_2 / ||ref||_2 <= 4 delta, delta = the module's OWN fp32-vs-fp64 distance on the same
image (computed here, asserted > 0 first) -- the margin LPIPS and DISTS use.  Measured on MI355X (this file's printout): see the
README's FD-SwAV entry."""
import os

import numpy as np
import pytest
import torch

from tests._trunk_audit import CONV_TOL

pytestmark = pytest.mark.gpu

SIZES = ((32, 32, 2), (33, 47, 2), (64, 64, 2), (224, 224, 2))


def seeded_bytes(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)


def rel_rows(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm(dim=1) / b.norm(dim=1)).numpy()


@pytest.fixture(scope="module")
def world(cuda_device):
    """The seeded module, its fp64 twin, the device tower, and per size (images, fp64 rows, delta per row): computed once."""
    from tise_toolbox_amd import resnet_hip, resnet_model

    class World:
        pass
    w = World()
    w.dev = cuda_device
    w.model = resnet_model.ResNet50().init_synthetic(0)
    w.model64 = resnet_model.ResNet50().init_synthetic(0).double()
    w.tower = resnet_hip.HipResNet50(w.model, cuda_device, stem="mfma")
    w.cases = {}
    for h, wd, n in SIZES:
        img = seeded_bytes(n, h, wd, 31 * h + wd)
        ref = w.model64(img)
        w.cases[(h, wd)] = (img, ref, rel_rows(w.model(img), ref))
    return w


@pytest.mark.parametrize("h,w", [s[:2] for s in SIZES])
def test_route_against_fp64_module(world, h, w):
    img, ref, delta = world.cases[(h, w)]
    assert (delta > 0).all(), delta
    got = world.tower.features_from_u8(img.to(world.dev))
    assert world.tower.last_stem == "mfma" and got.shape == (img.shape[0], 2048) and got.dtype == torch.float32
    err = rel_rows(got.cpu(), ref)
    print(f"route {h}x{w}: device error per row {err}, delta {delta}, share of the bound {err / (4 * delta)}")
    assert (err <= 4 * delta).all(), (err, delta)


def test_row_bits_do_not_depend_on_batch_chunk_or_call(world):
    from tise_toolbox_amd import resnet_hip
    img = torch.cat([world.cases[(64, 64)][0], seeded_bytes(3, 64, 64, 77)]).to(world.dev)
    whole = world.tower.features_from_u8(img)
    assert torch.equal(world.tower.features_from_u8(img), whole)                         # a second call
    for i in (0, 4):
        assert torch.equal(world.tower.features_from_u8(img[i:i + 1]), whole[i:i + 1])   # alone
    tiny = resnet_hip.HipResNet50(world.model, world.dev, budget=1, stem="mfma")
    assert resnet_hip.images_per_chunk(64, 64, 1) == 1
    assert torch.equal(tiny.features_from_u8(img), whole)                                # one image per chunk


def test_both_stems_agree(world):
    from tise_toolbox_amd import resnet_hip
    padded = resnet_hip.HipResNet50(world.model, world.dev, stem="padded")
    for (h, w) in ((33, 47), (224, 224)):
        img, ref, _ = world.cases[(h, w)]
        a = world.tower.features_from_u8(img.to(world.dev)).cpu().double()
        b = padded.features_from_u8(img.to(world.dev)).cpu().double()
        assert padded.last_stem == "padded" and world.tower.last_stem == "mfma"
        scale = ref.abs().max().item()
        diff = (a - b).abs().max().item()
        print(f"stems {h}x{w}: |mfma - padded| / scale = {diff / scale:.3e}")
        assert diff <= 2 * CONV_TOL * scale, (h, w, diff, scale)


def test_stem_choice_from_the_environment(world, monkeypatch):
    from tise_toolbox_amd import resnet_hip
    monkeypatch.setenv("TISE_RESNET_STEM", "padded")
    assert resnet_hip.HipResNet50(world.model, world.dev).stem == "padded"
    monkeypatch.setenv("TISE_RESNET_STEM", "other")
    with pytest.raises(ValueError, match="TISE_RESNET_STEM"):
        resnet_hip.HipResNet50(world.model, world.dev)
    monkeypatch.delenv("TISE_RESNET_STEM")
    assert resnet_hip.HipResNet50(world.model, world.dev).stem == resnet_hip.DEFAULT_STEM
    with pytest.raises(ValueError, match="five halvings"):
        world.tower.features_from_u8(torch.zeros((1, 31, 40, 3), dtype=torch.uint8, device=world.dev))
    with pytest.raises(ValueError, match="uint8"):
        world.tower.features_from_u8(torch.zeros((1, 32, 32, 3), dtype=torch.float32, device=world.dev))


def test_range_guard_fires(world):
    from tise_toolbox_amd import device, resnet_hip, resnet_model
    big = resnet_model.ResNet50().init_synthetic(0)
    big.layer1[0].conv1.weight.mul_(2.0 ** 15)
    tower = resnet_hip.HipResNet50(big, world.dev)
    device.read_split_overflow()
    with pytest.raises(FloatingPointError, match="65504"):
        tower.features_from_u8(world.cases[(32, 32)][0].to(world.dev))
    assert not device.read_split_overflow()                                              # read and cleared by the call
    nan = resnet_model.ResNet50().init_synthetic(0)
    nan.layer2[1].bn2.bias[5] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        resnet_hip.HipResNet50(nan, world.dev)


def _png_dir(path, sizes, seed):
    from PIL import Image
    from tests import _cases
    os.makedirs(path)
    pools = {}
    for k, (h, w) in enumerate(sizes):
        if (h, w) not in pools:
            pools[(h, w)] = _cases.smooth_images(12, h, w, seed=seed + h)
        Image.fromarray(np.ascontiguousarray(np.roll(pools[(h, w)][k % 12], 3 * k + seed, axis=1))).save(os.path.join(path, f"{k:04d}.png"))
    return str(path)


_PREFIXES = ("FD-SwAV:", "KD-SwAV:", "Precision-SwAV:", "Recall-SwAV:", "Density-SwAV:", "Coverage-SwAV:")


@pytest.mark.timeout(600)
def test_cli_end_to_end(world, tmp_path, capfd, monkeypatch):
    """fd_swav.main on 23 PNGs of one size (the ring, resized on the device) against 27 PNGs of two sizes (the DataLoader, resized by
    Pillow), --batch-size 10 --synthetic-weights --kd --prdc --save-features."""
    from PIL import Image
    from oracle import fid_oracle
    from tise_toolbox_amd import fd_swav, fid_score, img_data, kid, prdc, resnet_hip, resnet_model
    from tise_toolbox_amd.weights import SYNTHETIC_TAG
    monkeypatch.delenv("TISE_RESNET", raising=False)
    monkeypatch.delenv("TISE_RESNET_STEM", raising=False)
    ref = _png_dir(tmp_path / "ref", [(64, 64)] * 23, 3)
    gen = _png_dir(tmp_path / "gen", [(64, 64)] * 20 + [(48, 80)] * 7, 4)
    out_npz, out_txt = str(tmp_path / "ref.npz"), str(tmp_path / "lines.txt")
    tail = ["--path2", gen, "--batch-size", "10", "--num-workers", "2", "--synthetic-weights", "--kd", "--prdc"]
    capfd.readouterr()
    res = fd_swav.main(["--path1", ref] + tail + ["--save-features", out_npz, "--saved_file", out_txt])
    lines = [ln for ln in capfd.readouterr().out.splitlines() if ln.startswith(_PREFIXES)]
    assert len(lines) == 6 and all(ln.endswith(SYNTHETIC_TAG) for ln in lines) and open(out_txt).read() == "\n".join(lines)
    assert [ln.split(":")[0] + ":" for ln in lines] == list(_PREFIXES)
    with np.load(out_npz) as f:
        assert sorted(f.files) == ["features", "mu", "network", "sigma"] and str(f["network"]) == "swav-resnet50"
        r1 = np.array(f["features"])
    assert r1.shape == (23, 2048) and r1.dtype == np.float32 and np.isfinite(r1).all() and np.unique(r1, axis=0).shape[0] == 23
    # the saved rows against the fp64 module on Pillow-resized bytes, within 4 delta per row
    files = img_data.get_filenames(ref)
    u8 = torch.stack([resnet_model.preprocess_u8(Image.open(p)) for p in files])
    assert u8.shape == (23, 224, 224, 3) and u8.dtype == torch.uint8
    want = torch.cat([world.model64(u8[i:i + 6]) for i in range(0, 23, 6)])
    delta = rel_rows(torch.cat([world.model(u8[i:i + 6]) for i in range(0, 23, 6)]), want)
    err = rel_rows(torch.from_numpy(r1), want)
    with capfd.disabled():                                                               # (a later readouterr would swallow it)
        print(f"cli rows: device error {err.max():.3e} (largest share of 4 delta: {(err / (4 * delta)).max():.3f}), delta {delta.min():.3e} .. {delta.max():.3e}")
    assert (delta > 0).all() and (err <= 4 * delta).all(), (err, delta)
    # the generated side through the Python entry points (a ragged directory: Pillow in the DataLoader's workers)
    tower = resnet_hip.build_tower(None, world.dev, 0)
    assert isinstance(tower, resnet_hip.HipResNet50) and tower.synthetic
    r2 = fd_swav.embed_image_dir(tower, gen, world.dev, 10, workers=2).cpu().numpy()
    assert r2.shape == (27, 2048)
    a1, a2 = r1.astype(np.float64), r2.astype(np.float64)
    s1, s2 = np.cov(a1, rowvar=False), np.cov(a2, rowvar=False)
    oracle = float(fid_oracle.calculate_frechet_distance_symmetric(a1.mean(0), s1, a2.mean(0), s2))
    # N < d.  The solver's documented rank-deficient bound (tests/test_gpu_frechet_kernels.py, DESIGN.md "Frechet"): an eigenvalue
    # that should be 0 is found within delta = 2 d eps tr(S1) ||S2||_F of it, and the square root turns that into sqrt(delta); at
    # most 32 such eigenvalues are computed (r - rank <= 32), and tr_covmean enters the distance twice.  Nothing is added for the
    # oracle's own eigvalsh.  Measured on MI355X: FD-SwAV 138.46435 against 138.46415, difference 2.0e-4, margin 6.6e-3 (tr S1 80.6).
    eps, d = 2.0 ** -52, 2048
    margin_dev = 2 * 32 * np.sqrt(2 * d * eps * np.trace(s1) * np.linalg.norm(s2))
    with capfd.disabled():
        print(f"FD-SwAV {res['fd']!r} vs oracle {oracle!r}: difference {abs(res['fd'] - oracle):.3e}, margin {margin_dev:.3e}, "
              f"tr S1 {np.trace(s1):.3e}")
    assert abs(res["fd"] - oracle) <= margin_dev
    assert lines[0] == f"FD-SwAV: {res['fd']}{SYNTHETIC_TAG}"
    assert abs(fd_swav.fd_swav_from_features(r1, r2) - res["fd"]) <= 1e-6 * abs(res["fd"])
    want_kd = kid.kid_from_features(r1, r2, subsets=100, subset_size=1000)
    want_prdc = prdc.prdc_from_features(r1, r2, nearest_k=5)
    assert res["kd"] == want_kd and dict(res["prdc"]) == dict(want_prdc)
    assert lines[1] == f"KD-SwAV: {want_kd[0]} +- {want_kd[1]}{SYNTHETIC_TAG}"
    assert lines[2:] == [f"{k.capitalize()}-SwAV: {want_prdc[k]}{SYNTHETIC_TAG}" for k in ("precision", "recall", "density", "coverage")]
    # the feature file in place of the directory: the same lines; either side may be such a file
    fd_swav.main(["--path1", out_npz] + tail)
    assert [ln for ln in capfd.readouterr().out.splitlines() if ln.startswith(_PREFIXES)] == lines
    assert abs(fd_swav.calculate_fd_swav_given_paths([out_npz, out_npz])["fd"]) <= margin_dev
    # a feature file of another network is refused, on either side; no parameters and no --synthetic-weights is refused too
    other = str(tmp_path / "dino.npz")
    fid_score.save_stats_npz(other, a1.mean(0), s1, "dinov2-vitl14", r1)
    for args in (["--path1", other, "--path2", gen], ["--path1", ref, "--path2", other]):
        with pytest.raises(RuntimeError, match="dinov2-vitl14"):
            fd_swav.main(args + ["--synthetic-weights"])
    monkeypatch.setenv("TORCH_HOME", str(tmp_path / "no_torch_home"))
    with pytest.raises(RuntimeError, match="no parameters for SwAV ResNet-50"):
        fd_swav.main(["--path1", ref, "--path2", gen])
    # the A/B route: the fp32 module on library kernels gives the same rows up to the towers' difference
    monkeypatch.setenv("TISE_RESNET", "torch")
    lib = resnet_hip.build_tower(None, world.dev, 0)
    assert isinstance(lib, resnet_hip.TorchResNet50)
    ra = lib.features_from_u8(u8[:4].to(world.dev)).cpu()
    assert (rel_rows(ra, want[:4]) <= 1e-4).all()
