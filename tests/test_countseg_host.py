"""CPU: the host side of counting alignment -- the numpy restatement of the head (tests/_countseg_ref.py) against the module's torch
formulation (max_pool2d's indices, torch.median), the parameter loader with every refusal, the stand-ins, the arithmetic of CA
against a hand-computed case, the CLI surface and ``ranking_score --collect --ca``."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

from tests import _countseg_ref as R


# ---- peak stimulation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", ((1, 1), (1, 2), (2, 1), (1, 5), (5, 1), (3, 3), (2, 7), (14, 14), (15, 17)))
def test_restatement_against_the_torch_formulation(h, w):
    from tise_toolbox_amd import countseg_model
    rng = np.random.default_rng(100 * h + w)
    maps = rng.standard_normal((3, 5, h, w))
    conf, cnt = countseg_model.peak_stimulation(torch.from_numpy(maps))
    want_conf, want_cnt = R.peak_stimulation(maps)
    assert np.array_equal(cnt.numpy(), want_cnt) and np.abs(conf.numpy() - want_conf).max() <= 1e-14
    assert (want_cnt >= 1).all()                                            # the first global maximum is always a peak
    den = torch.from_numpy(maps).mean((2, 3)).numpy()
    assert np.abs(R.density_mean(maps) - den).max() <= 1e-15
    # small integers: ties everywhere, every value exact
    ties = rng.integers(-2, 3, (4, 6, h, w)).astype(np.float64)
    conf, cnt = countseg_model.peak_stimulation(torch.from_numpy(ties))
    want_conf, want_cnt = R.peak_stimulation(ties)
    assert np.array_equal(cnt.numpy(), want_cnt) and np.abs(conf.numpy() - want_conf).max() <= 1e-15
    # fp32 maps take the same decisions on the same values
    conf32, cnt32 = countseg_model.peak_stimulation(torch.from_numpy(ties).float())
    assert np.array_equal(cnt32.numpy(), want_cnt) and conf32.dtype == torch.float32


@pytest.mark.parametrize("name", sorted(R.TIE_MAPS))
def test_tie_cases_by_hand(name):
    from tise_toolbox_amd import countseg_model
    m, peak_at, conf0 = R.TIE_MAPS[name]
    med = np.sort(m.reshape(-1))[(m.size - 1) // 2]
    sel = R.local_maxima(m) & (m >= med)
    assert [tuple(int(v) for v in t) for t in np.argwhere(sel)] == peak_at
    for conf, cnt in (R.peak_stimulation(m[None, None]), (t.numpy() for t in countseg_model.peak_stimulation(torch.from_numpy(m)[None, None]))):
        assert conf[0, 0] == conf0 and cnt[0, 0] == len(peak_at)


def test_median_rank_rule():
    """The lower median is the value v with #(x < v) <= k < #(x <= v), k = (hw - 1) // 2: what the kernel counts."""
    rng = np.random.default_rng(3)
    for size in (1, 2, 5, 8, 196, 255):
        x = rng.integers(0, 6, size).astype(np.float64)
        k = (size - 1) // 2
        med = float(torch.median(torch.from_numpy(x)))
        assert med == np.sort(x)[k] and (x < med).sum() <= k < (x <= med).sum()
        assert all(not ((x < v).sum() <= k < (x <= v).sum()) for v in set(x.tolist()) - {med})


def test_a_nan_map_gives_nan_confidence_and_no_peaks():
    from tise_toolbox_amd import countseg_model
    maps = np.random.default_rng(0).standard_normal((2, 3, 4, 4))
    maps[1, 2, 3, 0] = np.nan
    conf, cnt = countseg_model.peak_stimulation(torch.from_numpy(maps))
    want_conf, want_cnt = R.peak_stimulation(maps)
    assert np.argwhere(np.isnan(conf.numpy())).tolist() == [[1, 2]] and np.array_equal(cnt.numpy(), want_cnt) and want_cnt[1, 2] == 0
    keep = ~np.isnan(want_conf)
    assert np.array_equal(np.isnan(want_conf), np.isnan(conf.numpy())) and np.abs(conf.numpy()[keep] - want_conf[keep]).max() <= 1e-14


def test_decision_margin():
    m = np.array([[[[0.0, 1.0, 0.0], [0.0, 0.5, 3.0], [0.25, 0.0, 0.0]]]])
    conf, peaks = R.peak_stimulation(m)
    assert peaks[0, 0] == 1 and conf[0, 0] == 3.0                          # (0, 1) = 1 sits next to 3; (2, 0) = 0.25 next to 0.5
    den = np.array([[1.25]])
    # neighbours: 0.25 against 0.5 is the closest pair; the maximum 3 against the median 0 is 3; conf 3 from 0; den 0.25 from 1.5
    assert R.decision_margin(m, conf, den)[0] == 0.25
    assert R.decision_margin(m, conf, np.array([[1.4375]]))[0] == 0.0625
    assert R.decision_margin(m, np.array([[-0.125]]), den)[0] == 0.125
    flat = np.zeros((1, 1, 2, 2))
    assert R.decision_margin(flat, np.array([[1.0]]), den)[0] == 0.0        # a tie is a decision with no margin


# ---- the module, the loader, the stand-ins -------------------------------------------------------------------------------------------
def _small_model(seed=0):
    from tise_toolbox_amd import countseg_model
    return countseg_model.CountSeg().init_synthetic(seed)


def test_module_forward_and_stand_ins():
    from tise_toolbox_amd import countseg_model, resnet_model
    a, b, c = _small_model(0), _small_model(0), _small_model(1)
    assert a.synthetic and not countseg_model.CountSeg().synthetic
    sa, sb, sc = a.state_dict(), b.state_dict(), c.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa) and not torch.equal(sa["mix.weight"], sc["mix.weight"])
    trunk = resnet_model.ResNet50().init_synthetic(0).state_dict()          # the trunk's stand-ins as they are
    assert all(torch.equal(sa["trunk." + k], v) for k, v in trunk.items())
    assert tuple(sa["mix.weight"].shape) == (240, 2048, 1, 1) and tuple(sa["cls.weight"].shape) == (80, 120, 1, 1) == tuple(sa["den.weight"].shape)
    assert -0.5 <= float(sa["den.bias"].min()) and float(sa["den.bias"].max()) <= 3.5
    img = torch.from_numpy(R.images(2, 64, 40, 5))
    conf, den, cnt = a(img)
    m, d = a.maps(img)
    assert m.shape == (2, 80, 2, 2) == d.shape and conf.shape == (2, 80) == den.shape == cnt.shape and conf.dtype == torch.float32
    assert torch.equal(a.trunk(img), a.trunk.feature_map(img).mean((2, 3)))                # the trunk's own output keeps its bits
    m64, d64 = _small_model(0).double().maps(img)
    want_conf, want_cnt = R.peak_stimulation(m64.numpy())
    conf64, den64, cnt64 = _small_model(0).double()(img)
    assert np.array_equal(cnt64.numpy(), want_cnt) and np.abs(conf64.numpy() - want_conf).max() <= 1e-12
    assert np.abs(den64.numpy() - R.density_mean(d64.numpy())).max() <= 1e-12
    counts = R.counts(conf64.numpy(), den64.numpy())
    for i in range(2):                                                       # what the stand-in biases are drawn for
        assert (conf64[i] > 0).any() and (conf64[i] <= 0).any() and len(np.unique(counts[i])) >= 3


def test_loader_and_its_refusals(tmp_path):
    from tise_toolbox_amd import countseg_model
    src = _small_model(3)
    names = {"conv1": "0", "bn1": "1", "layer1": "4", "layer2": "5", "layer3": "6", "layer4": "7"}
    nest = {}
    for k, v in src.state_dict().items():
        if k.startswith("trunk."):
            parts = k.split(".")[1:]
            nest["module.0.features." + ".".join([names[parts[0]]] + parts[1:])] = v
        else:
            nest["module.0." + k] = v
    assert "module.0.features.0.weight" in nest and "module.0.features.4.0.bn1.num_batches_tracked" in nest and "module.0.mix.bias" in nest
    path = str(tmp_path / "coco14.pt")
    torch.save({"model": nest, "epoch": 3}, path)
    got = countseg_model.CountSeg().load_countseg(path)
    assert not got.synthetic and all(torch.equal(v, got.state_dict()[k]) for k, v in src.state_dict().items())
    plain = {(k[len("trunk."):] if k.startswith("trunk.") else k): v for k, v in src.state_dict().items()}
    got = countseg_model.CountSeg().load_countseg(plain)                     # a bare state dict, the trunk under its own names
    assert all(torch.equal(v, got.state_dict()[k]) for k, v in src.state_dict().items())
    torch.save(plain, path)
    assert torch.equal(countseg_model.build_model(path).mix.weight, src.mix.weight)
    for key in ("fc.weight", "module.0.classifier.weight", "features.2.weight", "mix.running_mean", "head.mix.weight"):
        with pytest.raises(ValueError, match=key.replace(".", r"\.") + " is"):
            countseg_model.CountSeg().load_countseg(dict(plain, **{key: torch.zeros(3, 2)}))
    with pytest.raises(ValueError, match=r"cls\.weight is \(80, 60, 1, 1\), CountSeg has \(80, 120, 1, 1\)"):
        countseg_model.CountSeg().load_countseg(dict(plain, **{"cls.weight": torch.zeros(80, 60, 1, 1)}))
    with pytest.raises(ValueError, match=r"den\.bias is missing, CountSeg has \(80,\)"):
        countseg_model.CountSeg().load_countseg({k: v for k, v in plain.items() if k != "den.bias"})
    with pytest.raises(ValueError, match=r"the trunk: layer2\.0\.conv1\.weight is \(1, 1\), ResNet-50 has \(128, 256, 1, 1\)"):
        countseg_model.CountSeg().load_countseg(dict(plain, **{"layer2.0.conv1.weight": torch.zeros(1, 1)}))
    with pytest.raises(ValueError, match=r"the trunk: bn1\.weight is missing"):
        countseg_model.CountSeg().load_countseg({k: v for k, v in plain.items() if k != "bn1.weight"})
    with pytest.raises(RuntimeError, match="mutually exclusive"):
        countseg_model.build_model(path, synthetic=True)
    with pytest.raises(RuntimeError, match="needs a parameter file"):
        countseg_model.build_model(None)


def test_preprocess_is_pillows_bilinear_resize():
    from PIL import Image
    from tise_toolbox_amd import countseg_model
    img = Image.fromarray(R.images(1, 50, 70, 2)[0])
    got = countseg_model.preprocess_u8(img.convert("L"))
    assert got.shape == (448, 448, 3) and got.dtype == torch.uint8
    want = np.asarray(img.resize((448, 448), Image.BILINEAR))
    assert np.array_equal(countseg_model.preprocess_u8(img).numpy(), want)


# ---- the arithmetic of CA --------------------------------------------------------------------------------------------------------------
def test_ca_arithmetic_by_hand():
    from tise_toolbox_amd import CA
    names = list(CA.CLASS_NAMES)
    assert len(names) == 80 and names[0] == "person" and names[-1] == "toothbrush" and len(set(names)) == 80
    assert all(k in names for k in ("tv", "couch", "potted plant", "dining table", "cell phone", "hair drier"))
    rows = np.zeros((1, 160))
    conf, den = rows[0, :80], rows[0, 80:]
    conf[:] = -1.0
    den[:] = 7.0                                                             # absent classes: their density does not count
    for name, c, d in (("person", 0.5, 2.4), ("dog", 1e-300, 0.5), ("cat", 3.0, 1.5), ("bus", 2.0, 2.5), ("car", 1.0, -0.7), ("bird", 1.0, 0.4),
                       ("kite", 0.0, 3.0)):
        conf[names.index(name)], den[names.index(name)] = c, d
    counts = CA.predicted_counts(rows)[0]
    want = {"person": 2.0, "dog": 0.0, "cat": 2.0, "bus": 2.0, "car": -1.0, "bird": 0.0, "kite": 0.0}                   # half to even at 0.5, 1.5, 2.5
    assert all(counts[names.index(k)] == v for k, v in want.items()) and np.count_nonzero(counts) == 4
    assert np.array_equal(counts, R.counts(conf, den))
    # person 3 vs 2; dog 1 vs 0 (0.5 rounds to 0: not predicted); car 2 vs -1; unicorn 4 vs 0 (no such class); cat is predicted but
    # absent from gt: ignored
    gt = {"person": 3, "dog": 1, "car": 2, "unicorn": 4}
    want_rmse = np.sqrt((1.0 + 1.0 + 9.0 + 16.0) / 4.0)
    assert CA.item_rmse(gt, counts) == want_rmse == R.item_rmse(gt, counts, names)
    assert CA.item_rmse({"cat": 2}, counts) == 0.0 and CA.item_rmse({"kite": 0, "bird": 2}, counts) == np.sqrt(2.0)
    assert CA.predicted_text(counts) == "person:2;car:-1;bus:2;cat:2"                  # in class order


def test_cli_surface(tmp_path, monkeypatch):
    from tise_toolbox_amd import CA, weights
    a = CA.parse_args([])
    assert (a.image_dir, a.ct_input_file, a.result_file, a.gpu_id) == ("", "captions/CA_input_captions.pkl", "", 0)
    assert (a.weights, a.synthetic_weights, a.batch_size, a.num_workers, a.png_feed, a.per_image) == (None, False, 50, 0, "ring", "")
    a = CA.parse_args(["--image_dir", "d", "--ct_input_file", "f.pkl", "--result_file", "r", "--gpu_id", "1", "--png-feed", "dataloader",
                       "--per-image", "o.csv", "--synthetic-weights"])
    assert (a.image_dir, a.gpu_id, a.png_feed, a.per_image, a.synthetic_weights) == ("d", 1, "dataloader", "o.csv", True)
    assert CA.RESOLUTION == 448
    monkeypatch.chdir(tmp_path)
    assert weights._KINDS["countseg"][1]() == [os.path.join("weights", "coco14.pt")]
    with pytest.raises(RuntimeError, match="no parameters for CountSeg"):
        weights.resolve(None, False, "countseg")
    os.makedirs("weights")
    open(os.path.join("weights", "coco14.pt"), "wb").close()
    assert weights.resolve(None, False, "countseg") == (os.path.join("weights", "coco14.pt"), "")
    assert weights.resolve(None, True, "countseg") == (None, weights.SYNTHETIC_TAG)
    # the input file
    good = [{"caption_id": 5, "counting_info": {"dog": 2}}, {"caption_id": 6, "counting_info": {"cat": 1}}]
    for name, items, match in (("empty.pkl", good + [{"caption_id": 77, "counting_info": {}}], "caption_id 77.*empty counting_info"),
                               ("dict.pkl", {"a": good}, "a list of items"), ("bad.pkl", [{"caption": "x"}], "item 0 has no caption_id")):
        with open(name, "wb") as f:
            pickle.dump(items, f)
        with pytest.raises(ValueError, match=match):
            CA.load_items(name)
    with open("good.pkl", "wb") as f:
        pickle.dump(good, f)
    assert CA.load_items("good.pkl") == good
    with pytest.raises(FileNotFoundError, match=r"6\.png"):                  # refused by name before anything is encoded
        os.makedirs("img")
        open(os.path.join("img", "5.png"), "wb").close()
        CA.ca_of_items(None, good, "img", "cpu", 3)


def test_ranking_score_collects_ca(tmp_path):
    from tise_toolbox_amd import ranking_score, weights
    ca = tmp_path / "ca.txt"
    ca.write_text("CA = 1.8125")
    assert ranking_score.parse_result_file("CA", str(ca)) == 1.8125
    others = [f"{m}=1" for m in ranking_score.METRICS if m != "CA"]
    args = ["--methods-dir", str(tmp_path / "methods"), "--collect", "ours"] + [v for kv in others for v in ("--set", kv)]
    ranking_score.main(args + ["--ca", str(ca)])
    assert json.load(open(tmp_path / "methods" / "ours.json"))["CA"] == 1.8125
    ranking_score.main(args + ["--set", "CA=2.5"])                           # the literal keeps working
    assert json.load(open(tmp_path / "methods" / "ours.json"))["CA"] == 2.5
    ca.write_text("CA = 1.8125" + weights.SYNTHETIC_TAG)
    with pytest.raises(ValueError, match="synthetic-weights"):
        ranking_score.main(args + ["--ca", str(ca)])
    ca.write_text("PA = 0.5")
    with pytest.raises(ValueError, match="no CA result line"):
        ranking_score.main(args + ["--ca", str(ca)])
