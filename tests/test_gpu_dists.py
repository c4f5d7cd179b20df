"""GPU: the whole DISTS route (dists_hip.HipDists: stage-0 sums, input kernel, thirteen split convolutions, four L2 pools, five
head calls) against the fp64 forward of dists_model.DistsVGG16 on the CPU, its exact properties, the range guard and the CLI.

BOUND of the route, per pair: 4 delta.  delta is the largest distance of the module's own fp32 CPU forward from its fp64 forward
over this file's pairs: the device has to be as good as fp32 library arithmetic, with the factor 4 for the split format's 22
significand bits against fp32's 24.  Measured figures: README, DISTS entry."""
import os

import numpy as np
import pytest
import torch

from tests import _jpeg_writer

# the smallest; every pool rounds up (17 -> 9 -> 5 -> 3 -> 2); even sizes; odd at every level; the convolutions' fall-back width
SHAPES = [(16, 16), (17, 19), (32, 48), (35, 67), (16, 256)]
SIGMAS = (8.0, 25.0)
N_PAIRS = len(SHAPES) * len(SIGMAS)


def _smooth(h, w, rng):
    yy, xx = np.mgrid[0:h, 0:w]
    chans = [127.0 + 100.0 * np.sin(xx / (3.0 + c) + rng.uniform(0, 6)) * np.cos(yy / (4.0 + c) + rng.uniform(0, 6)) for c in range(3)]
    return np.stack(chans, -1)


@pytest.fixture(scope="module")
def reference():
    """The seeded module, the 10 pairs (per shape a smooth image against itself plus noise of sigma 8 and 25), the fp64 values,
    delta and the largest activation -- computed once, on the CPU, and left unchanged."""
    from tise_toolbox_amd import dists_model
    model = dists_model.DistsVGG16().init_synthetic(0)
    m64 = dists_model.DistsVGG16().init_synthetic(0).double()
    rng = np.random.default_rng(0)
    xs, ys, v64, v32, amax = [], [], [], [], []
    for h, w in SHAPES:
        a = _smooth(h, w, rng)
        for sigma in SIGMAS:
            xs.append(torch.from_numpy(np.clip(np.rint(a), 0, 255).astype(np.uint8)))
            ys.append(torch.from_numpy(np.clip(np.rint(a + rng.normal(0.0, sigma, a.shape)), 0, 255).astype(np.uint8)))
            v64.append(float(m64(xs[-1][None], ys[-1][None], amax)[0]))
            v32.append(float(model(xs[-1][None], ys[-1][None])[0]))
    v64, v32 = np.array(v64), np.array(v32, dtype=np.float64)
    return {"model": model, "m64": m64, "xs": xs, "ys": ys, "v64": v64, "delta": float(np.abs(v32 - v64).max()), "amax": max(amax)}


@pytest.fixture(scope="module")
def hip(cuda_device, reference):
    from tise_toolbox_amd.dists_hip import HipDists
    return HipDists(reference["model"], cuda_device)


def _stage_breakdown(reference, i, cuda_device):
    """Per stage: the fp64 module's value of pair i and the device's (printed when a pair misses its bound)."""
    from tise_toolbox_amd import dists_model
    from tise_toolbox_amd.dists_hip import HipDists
    m64 = reference["m64"]
    x, y = reference["xs"][i][None], reference["ys"][i][None]
    s1, s2, al, be = m64.similarities(x, y)
    at = 0
    for k, c in enumerate(dists_model.STAGE_CHANNELS):
        only = dists_model.DistsVGG16().init_synthetic(0)
        keep = torch.zeros(dists_model.N_CHANNELS, dtype=torch.bool)
        keep[at:at + c] = True
        scale = float(al.sum() + be.sum()) / float(al[keep].sum() + be[keep].sum())       # undo the renormalisation of the masked model
        only.alpha[0, ~keep, 0, 0], only.beta[0, ~keep, 0, 0] = 0.0, 0.0
        want = float((al[at:at + c] * (1 - s1[0, at:at + c]) + be[at:at + c] * (1 - s2[0, at:at + c])).sum())
        got = float(HipDists(only, cuda_device)([x[0].to(cuda_device)], [y[0].to(cuda_device)])[0]) / scale
        print(f"    pair {i} stage {k} ({c} channels): fp64 module {want:.9e} device {got:.9e} difference {got - want:+.3e}")
        at += c


@pytest.mark.gpu
def test_route_against_the_fp64_module(cuda_device, reference, hip):
    v64, delta = reference["v64"], reference["delta"]
    # from the reference alone, before anything runs on the device
    assert delta > 0.0
    assert reference["amax"] < 65504.0 / 16
    assert (v64 > 5e-4).all(), v64
    xs = [t.to(cuda_device) for t in reference["xs"]]
    ys = [t.to(cuda_device) for t in reference["ys"]]
    got = hip(xs, ys)
    assert got.dtype == np.float64 and got.shape == (N_PAIRS,)
    bound = 4.0 * delta
    err = np.abs(got - v64)
    print(f"dists route: delta {delta:.3e}, largest activation {reference['amax']:.3f}, worst device error {err.max():.3e} "
          f"= {err.max() / bound:.3f} of the bound 4 delta")
    for i, (t, e, v) in enumerate(zip(reference["xs"], err, v64)):
        print(f"dists route pair {i} {t.shape[0]} x {t.shape[1]}: value {v:.6e} device error {e:.3e} bound {bound:.3e}")
    for i in np.nonzero(err > bound)[0]:
        _stage_breakdown(reference, int(i), cuda_device)
    assert (err <= bound).all(), (err, bound)


@pytest.mark.gpu
def test_exact_cases(cuda_device, reference, hip):
    from tise_toolbox_amd import dists
    from tise_toolbox_amd.dists_hip import HipDists
    xs = [t.to(cuda_device) for t in reference["xs"]]
    ys = [t.to(cuda_device) for t in reference["ys"]]
    assert hip(xs, xs).tobytes() == np.zeros(N_PAIRS).tobytes()              # identical pairs: exactly 0.0
    full = hip(xs, ys)
    assert hip(ys, xs).tobytes() == full.tobytes()                           # d(x, y) and d(y, x): the same bits
    assert hip(xs, ys).tobytes() == full.tobytes()                           # a second call
    assert hip(xs[::-1], ys[::-1])[::-1].tobytes() == full.tobytes()         # the reversed list
    for i in range(N_PAIRS):                                                 # every pair alone
        assert hip([xs[i]], [ys[i]]).tobytes() == full[i:i + 1].tobytes(), i
    assert hip(torch.stack(xs[:2]), torch.stack(ys[:2])).tobytes() == full[:2].tobytes()     # the stacked form of one size
    tiny = HipDists(reference["model"], cuda_device, budget=1)               # every pair its own chunk
    assert tiny(xs, ys).tobytes() == full.tobytes()
    assert dists.dists_from_images(xs, ys, hip).tobytes() == full.tobytes()
    assert dists.dists_from_images(xs, ys, reference["model"]).tobytes() == full.tobytes()
    assert hip([], []).shape == (0,)
    with pytest.raises(ValueError, match="both sides >= 16"):
        hip([xs[0][:15]], [ys[0][:15]])
    with pytest.raises(ValueError, match="two sizes"):
        hip([xs[0]], [ys[2]])
    with pytest.raises(TypeError, match="DistsVGG16"):
        from tise_toolbox_amd import lpips_model
        HipDists(lpips_model.LpipsVGG16().init_synthetic(0), cuda_device)


@pytest.mark.gpu
def test_range_guard_raises(cuda_device, reference):
    """One layer scaled so that the reference leaves the fp16 range: the flag is read once per call and raised."""
    from tise_toolbox_amd import device, dists_model
    from tise_toolbox_amd.dists_hip import HipDists
    model = dists_model.DistsVGG16().init_synthetic(0)
    model.convs[4].weight.mul_(2.0 ** 15)
    m64 = dists_model.DistsVGG16().init_synthetic(0).double()
    m64.convs[4].weight.mul_(2.0 ** 15)
    amax = []
    m64(reference["xs"][4][None], reference["ys"][4][None], amax)
    assert max(amax) > 65504.0 and np.isfinite(max(amax))
    device.read_split_overflow()                                             # nothing pending from another test
    hip = HipDists(model, cuda_device)
    with pytest.raises(FloatingPointError, match="fp16 range"):
        hip([reference["xs"][4].to(cuda_device)], [reference["ys"][4].to(cuda_device)])
    assert device.read_split_overflow() is False                             # read and cleared


def _jpeg_bytes(h, w, seed):
    rng = np.random.default_rng(seed)
    blocks = []
    for bh, bw in _jpeg_writer.blocks_shape(w, h, [(1, 1)] * 3):
        b = np.zeros((bh, bw, 64), dtype=np.int64)
        b[:, :, 0] = rng.integers(-60, 61, size=(bh, bw))
        b[:, :, [1, 8, 9]] = rng.integers(-6, 7, size=(bh, bw, 3))
        blocks.append(b)
    return _jpeg_writer.write_jpeg(w, h, blocks, [np.full(64, 8)] * 3)


@pytest.fixture(scope="module")
def directories(tmp_path_factory):
    """ORIG (PNG) and RECON (JPEG, one level deeper for two of them), 7 pairs of two sizes; pair 3 is identical."""
    from PIL import Image
    root = tmp_path_factory.mktemp("dists")
    orig, recon = str(root / "orig"), str(root / "recon")
    stems = ["a/p0", "a/p1", "p2", "p3", "p4", "p5", "p6"]
    sizes = [(32, 48), (35, 40), (32, 48), (35, 40), (32, 48), (32, 48), (35, 40)]
    xs, ys = [], []
    rng = np.random.default_rng(5)
    for k, (stem, (h, w)) in enumerate(zip(stems, sizes)):
        for d in (orig, recon):
            os.makedirs(os.path.dirname(os.path.join(d, stem)), exist_ok=True)
        with open(os.path.join(recon, stem + ".jpg"), "wb") as f:
            f.write(_jpeg_bytes(h, w, k))
        y = np.asarray(Image.open(os.path.join(recon, stem + ".jpg")).convert("RGB")).copy()
        assert y.shape == (h, w, 3)
        x = y.copy() if k == 3 else np.clip(np.rint(y + rng.normal(0.0, 6.0 + 3.0 * k, y.shape)), 0, 255).astype(np.uint8)
        Image.fromarray(x).save(os.path.join(orig, stem + ".png"))
        xs.append(x)
        ys.append(y)
    return orig, recon, xs, ys, stems


@pytest.mark.gpu
def test_cli_on_two_directories(cuda_device, directories, tmp_path, capsys):
    from tise_toolbox_amd import dists, dists_model, weights
    orig, recon, xs, ys, stems = directories
    want = dists.dists_from_images([torch.as_tensor(x, device=cuda_device) for x in xs],
                                   [torch.as_tensor(y, device=cuda_device) for y in ys], dists_model.DistsVGG16().init_synthetic(0))
    assert want[3] == 0.0 and (np.delete(want, 3) > 5e-4).all() and np.std(want) >= 5e-4
    csv, saved = str(tmp_path / "pairs.csv"), str(tmp_path / "out.txt")
    capsys.readouterr()
    res = dists.main(["--path1", orig, "--path2", recon, "--batch-size", "3", "--num-workers", "2", "--synthetic-weights",
                      "--per-pair", csv, "--saved_file", saved])
    lines = capsys.readouterr().out.strip().split("\n")
    assert res["n"] == 7 and res["per_pair"]["dists"].tobytes() == want.tobytes()        # per pair: the bits of the one-list call
    assert len(lines) == 1 and lines[0].startswith("DISTS: ") and lines[0].endswith(weights.SYNTHETIC_TAG)
    assert open(saved).read() == lines[0]
    mean, std = (float(v) for v in lines[0][len("DISTS: "):-len(weights.SYNTHETIC_TAG)].split(" +- "))
    assert mean == res["dists"] and std == res["dists_std"]
    assert abs(mean - np.mean(want)) <= 1e-15 and abs(std - np.std(want)) <= 1e-13, (lines[0], np.mean(want), np.std(want))
    rows = open(csv).read().split("\n")
    assert rows[0] == "pair,file1,file2,h,w,dists" and rows[-1] == "" and len(rows) == 9
    for i, row in enumerate(rows[1:8]):
        f = row.split(",")
        assert f[:5] == [str(i), os.path.join(orig, stems[i] + ".png"), os.path.join(recon, stems[i] + ".jpg"), str(xs[i].shape[0]),
                         str(xs[i].shape[1])]
        assert float(f[5]) == want[i]
    # a stem present on one side only is refused, naming the file
    extra = os.path.join(orig, "zz_extra.png")
    from PIL import Image
    Image.fromarray(xs[0]).save(extra)
    try:
        with pytest.raises(RuntimeError, match="missing image: zz_extra.png"):
            dists.main(["--path1", orig, "--path2", recon, "--synthetic-weights"])
    finally:
        os.remove(extra)
    with pytest.raises(RuntimeError, match="no parameters for DISTS VGG-16"):
        dists.main(["--path1", orig, "--path2", recon, "--weights", "", "--dists-weights", ""])


@pytest.mark.gpu
def test_cli_self_pairs_is_reproducible(cuda_device, directories, tmp_path, capsys):
    import shutil
    from tise_toolbox_amd import dists, paired
    orig, _, xs, _, stems = directories
    one = tmp_path / "one_size"
    one.mkdir()
    keep = [i for i in range(7) if xs[i].shape == (32, 48, 3)]
    for i in keep:
        shutil.copy(os.path.join(orig, stems[i] + ".png"), str(one / f"{i}.png"))
    capsys.readouterr()
    outs = []
    for _ in range(2):
        res = dists.main(["--path1", str(one), "--self-pairs", "5", "--seed", "0", "--num-workers", "2", "--synthetic-weights"])
        outs.append((capsys.readouterr().out, res["per_pair"]["dists"].tobytes(), res["files1"], res["files2"]))
    assert outs[0] == outs[1] and res["n"] == 5
    idx = paired.draw_self_pairs(len(keep), 5, 0)
    files = paired.list_files(str(one))
    assert res["files1"] == [files[i] for i in idx[:, 0]] and res["files2"] == [files[j] for j in idx[:, 1]]
    assert outs[0][0].startswith("DISTS: ")
