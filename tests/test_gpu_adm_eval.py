"""GPU: the ADM sample-batch suite end to end (tise_toolbox_amd/adm_eval.py) against a CPU route on the same arrays.

Two .npz batches of 20 seeded smooth 40 x 40 images (the reference side shifted), stand-in weights, Inception Score chunks of 8
(8, 8, 4) fed in device batches of 7, which straddle both borders.  The CPU route: the numpy restatement of the TF1 resize
(tests/_tf1_resize_ref.py), the project's fp32 InceptionV3(network="inception-2015") module on the CPU with the same stand-in
weights, a forward hook on Mixed_6d's branch1x1 for the spatial rows, np.mean / np.cov, the oracle's Frechet distance and a
numpy Inception Score in fp64.

sFID's budget is max(1e-3, 4 * delta), delta = |sFID(fp32 CPU route) - sFID(the same route with the module in fp64)|: with
N = 20 < d the covariances are rank deficient and the distance amplifies fp32 rounding of the features by an amount that has
no fixed figure; the device differs from the fp32 CPU route by summation order and the 22-bit activation format, both of
fp32-rounding class, hence the factor 4.  Both figures are printed.
"""
import numpy as np
import pytest
import torch

from oracle import fid_oracle
from tests import _cases
from tests import _tf1_resize_ref as tf1
from tise_toolbox_amd.weights import SYNTHETIC_TAG

pytestmark = pytest.mark.gpu

NET = "inception-2015"
N, SPLIT, BATCH = 20, 8, 7


def _numpy_inception_score(logits, split):
    lg = np.asarray(logits, dtype=np.float64)
    scores = []
    for lo in range(0, len(lg), split):
        z = lg[lo:lo + split]
        z = z - z.max(1, keepdims=True)
        p = np.exp(z)
        p /= p.sum(1, keepdims=True)
        kl = p * (np.log(p) - np.log(p.mean(0, keepdims=True)))
        scores.append(np.exp(kl.sum(1).mean()))
    return float(np.mean(scores)), len(scores)


def _cpu_side(model, u8, dtype):
    """-> (pool3 rows, spatial rows, bias-free logits) of the CPU module in ``dtype`` on the restatement's network input."""
    x = torch.as_tensor(tf1.network_input_tf1(u8, (299, 299))).permute(0, 3, 1, 2).to(dtype)
    got = []
    hook = model.blocks[2][6].branch1x1.register_forward_hook(lambda m, i, o: got.append(o.detach()[:, :7].permute(0, 2, 3, 1).flatten(1).clone()))
    feats = []
    with torch.no_grad():
        for i in range(0, len(x), 10):
            feats.append(model(x[i:i + 10], prenormalized=True)[0].flatten(1))
        feats = torch.cat(feats)
        logits = model.logits(feats, bias=False)
    hook.remove()
    return feats.double().numpy(), torch.cat(got).double().numpy(), logits.double().numpy()


def _cpu_spatial(model, u8, dtype):
    """The spatial rows alone: the same module and hook, the forward stopped after Mixed_6d."""
    x = torch.as_tensor(tf1.network_input_tf1(u8, (299, 299))).permute(0, 3, 1, 2).to(dtype)
    got = []
    hook = model.blocks[2][6].branch1x1.register_forward_hook(lambda m, i, o: got.append(o.detach()[:, :7].permute(0, 2, 3, 1).flatten(1).clone()))
    with torch.no_grad():
        for i in range(0, len(x), 10):
            model.blocks[2][:7](model.blocks[1](model.blocks[0](x[i:i + 10])))
    hook.remove()
    return torch.cat(got).double().numpy()


def _frechet(a, b):
    return float(fid_oracle.calculate_frechet_distance(a.mean(0), np.cov(a, rowvar=False), b.mean(0), np.cov(b, rowvar=False)))


@pytest.fixture(scope="module")
def case(cuda_device, tmp_path_factory):
    from tise_toolbox_amd.inception import InceptionV3
    torch.set_num_threads(min(16, torch.get_num_threads()))
    d = tmp_path_factory.mktemp("adm")
    sample = _cases.smooth_images(N, 40, 40, seed=41)
    ref = _cases.smooth_images(N, 40, 40, seed=42, shift=0.15)
    np.savez(d / "ref.npz", ref)                                       # stored
    np.savez_compressed(d / "sample.npz", sample, np.arange(N))        # deflated, with an arr_1 of labels
    model = InceptionV3([3], seed=0, network=NET).eval()
    assert type(model.blocks[2][6]).__name__ == "InceptionC" and model.blocks[2][6].branch1x1.conv.out_channels == 192
    fr, sr, _ = _cpu_side(model, ref, torch.float32)
    fs, ss, lg = _cpu_side(model, sample, torch.float32)
    assert sr.shape == (N, 2023)
    cpu = dict(fid=_frechet(fr, fs), sfid=_frechet(sr, ss), inception_score=_numpy_inception_score(lg, SPLIT))
    model = model.double()
    cpu["sfid64"] = _frechet(_cpu_spatial(model, ref, torch.float64), _cpu_spatial(model, sample, torch.float64))
    return dict(dir=d, ref=ref, sample=sample, cpu=cpu)


@pytest.fixture(scope="module")
def run(case):
    """The CLI once on (ref, sample), in this process, with --save-stats and --saved_file."""
    import os
    from tise_toolbox_amd import adm_eval
    old = os.environ.get("TISE_CONV")
    os.environ["TISE_CONV"] = "split"
    try:
        d = case["dir"]
        argv = ["--synthetic-weights", "--is-split-size", str(SPLIT), "--batch-size", str(BATCH)]
        result = adm_eval.main([str(d / "ref.npz"), str(d / "sample.npz"), "--save-stats", str(d / "ref_stats.npz"),
                                "--saved_file", str(d / "out.txt")] + argv)
        yield dict(result=result, argv=argv)
    finally:
        if old is None:
            os.environ.pop("TISE_CONV", None)
        else:
            os.environ["TISE_CONV"] = old


def test_five_numbers_vs_cpu_route(case, run):
    got, cpu = run["result"], case["cpu"]
    assert got["n_ref"] == N and got["n_sample"] == N and len(got["is_chunks"]) == 3 and cpu["inception_score"][1] == 3
    delta = abs(cpu["sfid"] - cpu["sfid64"])
    print("FID device", got["fid"], "cpu", cpu["fid"], "diff", abs(got["fid"] - cpu["fid"]))
    print("IS device", got["inception_score"], "cpu", cpu["inception_score"][0], "diff", abs(got["inception_score"] - cpu["inception_score"][0]))
    print("sFID device", got["sfid"], "cpu fp32", cpu["sfid"], "cpu fp64", cpu["sfid64"], "delta", delta, "device diff", abs(got["sfid"] - cpu["sfid"]))
    assert abs(got["fid"] - cpu["fid"]) <= 1e-3
    assert abs(got["inception_score"] - cpu["inception_score"][0]) <= 1e-4
    assert abs(got["sfid"] - cpu["sfid"]) <= max(1e-3, 4 * delta)
    assert got["fid"] > 1.0 and got["sfid"] > 0.0 and got["inception_score"] > 1.0       # two different image sets: not a trivial match


def test_lines_and_statistics_file(case, run):
    from tise_toolbox_amd import adm_eval
    got, d = run["result"], case["dir"]
    lines = (d / "out.txt").read_text().split("\n")
    assert [ln.split(":")[0] for ln in lines] == ["Inception Score", "FID", "sFID", "Precision", "Recall"]
    assert all(ln.endswith(SYNTHETIC_TAG) for ln in lines)
    assert lines == adm_eval.result_lines(got, SYNTHETIC_TAG)
    with np.load(d / "ref_stats.npz") as f:
        assert set(f.files) == {"mu", "sigma", "mu_s", "sigma_s", "features", "network", "mode"}
        assert f["mu"].shape == (2048,) and f["sigma"].shape == (2048, 2048) and f["mu_s"].shape == (2023,)
        assert f["sigma_s"].shape == (2023, 2023) and f["features"].shape == (N, 2048) and f["features"].dtype == np.float32
        assert str(f["mode"]) == "adm" and str(f["network"]) == NET
        rows = f["features"].astype(np.float64)
        assert np.abs(f["mu"] - rows.mean(0)).max() <= 1e-12 * np.abs(rows).max()                  # the rows are the ones FID used


def test_saved_statistics_serve_as_ref_and_prdc_is_wired(case, run):
    from tise_toolbox_amd import adm_eval
    from tise_toolbox_amd.prdc import prdc_from_features
    got, d, argv = run["result"], case["dir"], run["argv"]
    again = adm_eval.main([str(d / "ref_stats.npz"), str(d / "sample.npz")] + argv)
    assert abs(again["fid"] - got["fid"]) <= 1e-6 * abs(got["fid"]) and abs(again["sfid"] - got["sfid"]) <= 1e-6 * abs(got["sfid"])
    assert again["inception_score"] == got["inception_score"]
    assert (again["precision"], again["recall"]) == (got["precision"], got["recall"])
    # the sample side's rows: the same run with the sides exchanged stores them
    swapped = adm_eval.main([str(d / "sample.npz"), str(d / "ref.npz"), "--save-stats", str(d / "sample_stats.npz")] + argv)
    assert abs(swapped["fid"] - got["fid"]) <= 1e-6 * abs(got["fid"])                      # the distance is symmetric
    fr, fs = np.load(d / "ref_stats.npz")["features"], np.load(d / "sample_stats.npz")["features"]
    want = prdc_from_features(fr, fs, nearest_k=3)
    assert (got["precision"], got["recall"]) == (want["precision"], want["recall"])
    assert (swapped["precision"], swapped["recall"]) == (want["recall"], want["precision"])   # the two manifolds exchange roles
    # a statistics file without rows: refused, unless Precision and Recall are switched off
    with np.load(d / "ref_stats.npz") as f:
        np.savez(d / "evaluator.npz", mu=f["mu"], sigma=f["sigma"], mu_s=f["mu_s"], sigma_s=f["sigma_s"])
        np.savez(d / "clean.npz", mu=f["mu"], sigma=f["sigma"], mu_s=f["mu_s"], sigma_s=f["sigma_s"], features=f["features"],
                 network=np.asarray(NET), mode=np.asarray("clean"))
    with pytest.raises(RuntimeError, match="features"):
        adm_eval.main([str(d / "evaluator.npz"), str(d / "sample.npz")] + argv)
    with pytest.raises(RuntimeError, match="clean"):
        adm_eval.main([str(d / "clean.npz"), str(d / "sample.npz")] + argv)
    three = adm_eval.main([str(d / "evaluator.npz"), str(d / "sample.npz"), "--no-prdc"] + argv)
    assert "precision" not in three and abs(three["fid"] - got["fid"]) <= 1e-6 * abs(got["fid"])
    assert abs(three["sfid"] - got["sfid"]) <= 1e-6 * abs(got["sfid"])


def test_the_numbers_are_another_routes(case, run, monkeypatch):
    """The default fid_score --network inception-2015 route (Pillow's 8-bit resize, whole batches) on the same images written
    as PNG files gives another FID."""
    from PIL import Image
    from tise_toolbox_amd import fid_score
    monkeypatch.setenv("TISE_CONV", "split")
    d = case["dir"]
    for name in ("ref", "sample"):
        (d / name).mkdir()
        for i, im in enumerate(case[name]):
            Image.fromarray(im).save(d / name / f"{i:05d}.png")
    other = fid_score.main(["--batch-size", "5", "--path1", str(d / "ref"), "--path2", str(d / "sample"), "--num-workers", "0",
                            "--synthetic-weights", "--network", NET])
    print("fid_score route", other, "adm route", run["result"]["fid"])
    assert abs(other - run["result"]["fid"]) > 1e-3
