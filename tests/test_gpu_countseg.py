"""GPU: the whole CountSeg route (countseg_hip.HipCountSeg: the ResNet-50 trunk as a map, the mix convolution, the head kernel)
against the seeded module's fp64 CPU forward, its invariances, the range guard, and the CA CLI end to end.

The bound of the route: with s = the largest |value| of an image's reference maps, confidence and density mean within 4 delta s,
delta = the module's OWN fp32-against-fp64 distance on those maps relative to s (computed here, asserted > 0 first) -- the margin
the ResNet-50, LPIPS and DISTS routes use.  Every decision of the reference (a local maximum against its neighbours and the median,
a confidence against 0, a density mean against the nearest half-integer) rests on a gap of at least 8 delta s, asserted from the
reference alone before the device is touched; the seeds below were chosen on the CPU so that every image and class qualifies.
Measured figures: README, CA entry."""
import os
import pickle

import numpy as np
import pytest
import torch

from tests import _countseg_ref as R

pytestmark = pytest.mark.gpu

SIZES = ((32, 32, 2), (33, 47, 2), (96, 96, 2), (160, 128, 2), (448, 448, 1))            # (H, W, images): maps 1x1, 2x2, 3x3, 5x4, 14x14
GT = {"person": 2, "dog": 1, "traffic light": 3, "unicorn": 1, "toothbrush": 0}


def seed_of(h, w):
    """Chosen on the CPU: the smallest margin over 8 delta s is 7.6 at 448 x 448 and 12.7 .. 291 at the other sizes."""
    return 4 if (h, w) == (448, 448) else 100 + 31 * h + w


@pytest.fixture(scope="module")
def world(cuda_device):
    """The seeded module, its fp64 twin, the device counter, and per size the images and the fp64 reference: computed once."""
    from tise_toolbox_amd import countseg_hip, countseg_model

    class World:
        pass
    w = World()
    w.dev = cuda_device
    w.model = countseg_model.CountSeg().init_synthetic(0)
    w.model64 = countseg_model.CountSeg().init_synthetic(0).double()
    w.cases = {}
    for h, wd, n in SIZES:
        w.cases[(h, wd)] = reference_case(w.model, w.model64, torch.from_numpy(R.images(n, h, wd, seed_of(h, wd))))
    w.counter = countseg_hip.HipCountSeg(w.model, cuda_device)
    return w


def reference_case(model, model64, img):
    m64, d64 = model64.maps(img)
    m32, d32 = model.maps(img)
    conf, den, cnt = model64(img)
    n = img.shape[0]
    s = np.array([max(float(m64[i].abs().max()), float(d64[i].abs().max())) for i in range(n)])
    delta = np.array([max(float((m32[i].double() - m64[i]).abs().max()), float((d32[i].double() - d64[i]).abs().max())) for i in range(n)]) / s
    return dict(img=img, maps=m64.numpy(), conf=conf.numpy(), den=den.numpy(), peaks=cnt.numpy().astype(np.int32), s=s, delta=delta)


def rmse_rows(rows):
    from tise_toolbox_amd import CA
    return np.array([CA.item_rmse(GT, c) for c in CA.predicted_counts(rows)])


@pytest.mark.parametrize("h,w", [s[:2] for s in SIZES])
def test_route_against_fp64_module(world, h, w):
    from tise_toolbox_amd import CA
    c = world.cases[(h, w)]
    s, delta = c["s"], c["delta"]
    assert (delta > 0).all(), delta
    conf_np, peaks_np = R.peak_stimulation(c["maps"])                       # the module agrees with the neighbour rule on its own maps
    assert np.array_equal(peaks_np, c["peaks"]) and np.abs(conf_np - c["conf"]).max() <= 1e-12 * s.max()
    margin = R.decision_margin(c["maps"], c["conf"], c["den"])
    counts = R.counts(c["conf"], c["den"])
    print(f"countseg route {h}x{w}: s {s}, delta {delta}, margin / (8 delta s) {margin / (8 * delta * s)}")
    assert (margin >= 8 * delta * s).all(), (margin, 8 * delta * s)
    for i in range(len(s)):
        assert (c["conf"][i] > 0).any() and (c["conf"][i] <= 0).any() and len(np.unique(counts[i])) >= 3
    rows = world.counter.rows_from_u8(c["img"].to(world.dev)).cpu().numpy()
    peaks = world.counter.last_peaks.cpu().numpy()
    assert rows.shape == (len(s), 160) and rows.dtype == np.float64
    e_conf = np.abs(rows[:, :80] - c["conf"]).max(1) / (4 * delta * s)
    e_den = np.abs(rows[:, 80:] - c["den"]).max(1) / (4 * delta * s)
    print(f"countseg route {h}x{w}: conf error {e_conf}, den error {e_den} of the bound 4 delta s")
    assert (e_conf <= 1).all() and (e_den <= 1).all()
    assert np.array_equal(peaks, c["peaks"])
    assert np.array_equal(rows[:, :80] > 0, c["conf"] > 0) and np.array_equal(CA.predicted_counts(rows), counts)
    want = np.array([R.item_rmse(GT, counts[i], list(CA.CLASS_NAMES)) for i in range(len(s))])
    assert np.abs(rmse_rows(rows) - want).max() <= 1e-12


def test_row_bits_do_not_depend_on_batch_chunk_or_call(world):
    from tise_toolbox_amd import countseg_hip, resnet_hip
    img = torch.cat([world.cases[(96, 96)]["img"], torch.from_numpy(R.images(3, 96, 96, 7))]).to(world.dev)
    whole = world.counter.rows_from_u8(img)
    peaks = world.counter.last_peaks.clone()
    assert torch.equal(world.counter.rows_from_u8(img), whole) and torch.equal(world.counter.last_peaks, peaks)      # a second call
    for i in (0, 4):
        assert torch.equal(world.counter.rows_from_u8(img[i:i + 1]), whole[i:i + 1])      # alone
    tiny = countseg_hip.HipCountSeg(world.model, world.dev, budget=1)
    assert resnet_hip.images_per_chunk(96, 96, 1) == 1
    assert torch.equal(tiny.rows_from_u8(img), whole) and torch.equal(tiny.last_peaks, peaks)                        # one image per chunk


def test_range_guard_fires(world):
    from tise_toolbox_amd import countseg_hip, countseg_model, device
    big = countseg_model.CountSeg().init_synthetic(0)
    big.trunk.layer1[0].conv1.weight.mul_(2.0 ** 15)
    counter = countseg_hip.HipCountSeg(big, world.dev)
    device.read_split_overflow()
    with pytest.raises(FloatingPointError, match="65504"):
        counter.rows_from_u8(world.cases[(32, 32)]["img"].to(world.dev))
    assert not device.read_split_overflow()                                              # read and cleared by the call
    nan = countseg_model.CountSeg().init_synthetic(0)
    nan.cls.bias[5] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        countseg_hip.HipCountSeg(nan, world.dev)
    with pytest.raises(TypeError, match="CountSeg"):
        countseg_hip.HipCountSeg(world.model.trunk, world.dev)


def _write_pngs(path, shapes, seed):
    from PIL import Image
    os.makedirs(path)
    for k, (h, w) in enumerate(shapes):
        Image.fromarray(R.images(1, h, w, seed + k)[0]).save(os.path.join(path, f"{1000 + k}.png"))
    return str(path)


@pytest.mark.timeout(600)
def test_cli_end_to_end(world, tmp_path, capfd, monkeypatch):
    """CA.main on a ragged directory (two image sizes: the DataLoader, Pillow's resize) and on a one-size directory (the ring, the
    device's resize), --batch-size 3, a repeated caption_id, --synthetic-weights --per-image: the line, the tag and the CSV against
    the functions on the same bytes."""
    from PIL import Image
    from tise_toolbox_amd import CA, countseg_model
    from tise_toolbox_amd.weights import SYNTHETIC_TAG
    monkeypatch.delenv("TISE_COUNTSEG", raising=False)
    infos = [{"person": 2, "dog": 1}, {"traffic light": 3}, {"unicorn": 1, "cat": 2, "toothbrush": 1}, {"pizza": 4}, {"person": 1}, {"bus": 2, "car": 2},
             {"bird": 5}]
    for name, shapes in (("ragged", [(64, 64)] * 4 + [(48, 80)] * 3), ("one_size", [(64, 72)] * 7)):
        root = _write_pngs(tmp_path / name, shapes, 50)
        ids = [1000 + k for k in range(7)]
        items = [{"caption_id": ids[k], "caption": "x", "counting_info": infos[k]} for k in range(7)]
        items.append({"caption_id": ids[2], "caption": "again", "counting_info": {"dog": 3, "person": 1}})          # a repeated image
        pkl, out_txt, out_csv = str(tmp_path / f"{name}.pkl"), str(tmp_path / f"{name}.txt"), str(tmp_path / f"{name}.csv")
        with open(pkl, "wb") as f:
            pickle.dump(items, f)
        capfd.readouterr()
        res = CA.main(["--image_dir", root, "--ct_input_file", pkl, "--result_file", out_txt, "--batch-size", "3", "--num-workers", "2",
                       "--synthetic-weights", "--per-image", out_csv])
        lines = [ln for ln in capfd.readouterr().out.splitlines() if ln.startswith("CA = ")]
        u8 = torch.stack([countseg_model.preprocess_u8(Image.open(os.path.join(root, f"{i}.png"))) for i in ids])
        rows = world.counter.rows_from_u8(u8.to(world.dev)).cpu().numpy()
        counts = CA.predicted_counts(rows)[[0, 1, 2, 3, 4, 5, 6, 2]]
        rmse = np.array([CA.item_rmse(it["counting_info"], counts[k]) for k, it in enumerate(items)])
        assert res["n"] == 8 and res["rmse"].tobytes() == rmse.tobytes() and np.array_equal(res["counts"], counts)
        assert res["ca"] == float(np.mean(rmse))
        assert lines == [f"CA = {res['ca']}{SYNTHETIC_TAG}"] and open(out_txt).read() == lines[0]
        csv = open(out_csv).read().split("\n")
        assert csv[0] == "item,caption_id,rmse,predicted" and csv[-1] == "" and len(csv) == 10
        for k, it in enumerate(items):
            assert csv[1 + k] == f"{k},{it['caption_id']},{float(rmse[k])!r},{CA.predicted_text(counts[k])}"
        assert any(c for c in csv[1:9] if c.split(",")[3])                   # some class is predicted somewhere
    os.remove(os.path.join(root, "1003.png"))
    with pytest.raises(FileNotFoundError, match="1003.png"):
        CA.main(["--image_dir", root, "--ct_input_file", pkl, "--synthetic-weights"])
    with pytest.raises(RuntimeError, match="no parameters for CountSeg"):
        monkeypatch.chdir(tmp_path)
        CA.main(["--image_dir", root, "--ct_input_file", pkl])
