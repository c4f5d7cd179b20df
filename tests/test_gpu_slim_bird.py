"""GPU: --network slim (the TF-slim InceptionV3 of the reference's IS* for CUB birds) on the MI355X.

Kernels: the exclude-padding average pool at the Mixed_7c instance (8 x 8, 2048-channel input, the fused 1x1's pool segment)
and the 2048 -> 51 classifier (split form; its last cout tile is partial) against fp64.  Trunks: SplitTrunk and FusedTrunk
pool3 features and 51-class logits against the independent fp64 restatement written from the TF-layout tensors
(tests/_slim_ref.py).  End to end: the inception_score_bird CLI on V1 and V2 checkpoints written from the stand-in weights,
against the CPU path on the same selection; calibration on a labelled folder feeding its T to the bird CLI."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import is_oracle, resize_oracle
from tests import _cases
from tests import _slim_ref as ref
from tests._tf_ckpt_writer import slim_checkpoint_tensors, write_v1, write_v2

pytestmark = pytest.mark.gpu

NET = "slim"
T_BIRD = 0.5980541706085205


def _excl_ref(raw64, bias64):
    y = F.avg_pool2d(raw64.permute(0, 3, 1, 2), 3, 1, 1, count_include_pad=False) + bias64.view(1, -1, 1, 1)
    return torch.relu(y).permute(0, 2, 3, 1)


# ------------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("n", [1, 3])
def test_mixed_7c_exclude_padding_pool_fp32_vs_fp64(cuda_device, n):
    """Mixed_7c's fused 1x1 output (1344 couts) keeps its pool segment 1152..1343; the pool runs on it at 8 x 8 and writes
    couts 1856..2047 of the 2048-channel block output."""
    from tise_toolbox_amd.trunk import FusedTrunk
    g = torch.Generator().manual_seed(70 + n)
    raw = torch.randn((n, 8, 8, 1344), generator=g).to(cuda_device)
    bias = torch.randn(192, generator=g).to(cuda_device)
    out = torch.full((n, 8, 8, 2048), -5.0, device=cuda_device)
    FusedTrunk._avgpool_bias_relu(raw, bias, 1152, 192, out, 1856, excl=True)
    want = _excl_ref(raw[..., 1152:].double(), bias.double())
    assert (out[..., 1856:].double() - want).abs().max().item() <= 1e-6 * max(1.0, want.abs().max().item())
    assert bool((out[..., :1856] == -5.0).all())
    for y, x, div in ((0, 0, 4), (0, 3, 6), (7, 7, 4), (4, 4, 9), (7, 2, 6)):    # every divisor class of the 8 x 8 map
        ys, xs = slice(max(0, y - 1), y + 2), slice(max(0, x - 1), x + 2)
        s = raw[0, ys, xs, 1152:].double().sum((0, 1)) / div + bias.double()
        assert torch.allclose(out[0, y, x, 1856:].double(), s.clamp_min(0), atol=1e-6)


@pytest.mark.parametrize("n", [1, 3])
def test_mixed_7c_exclude_padding_pool_split_vs_fp64(cuda_device, n):
    from tise_toolbox_amd.conv_split import merge
    from tise_toolbox_amd.trunk import SplitTrunk
    g = torch.Generator().manual_seed(80 + n)
    raw = torch.randn((n, 8, 8, 192), generator=g).to(cuda_device)
    bias = torch.randn(192, generator=g).to(cuda_device)
    out = torch.zeros((n, 8, 8, 2 * 2048), dtype=torch.float16, device=cuda_device)
    SplitTrunk._avgpool_split(raw, bias, out, 1856, excl=True)
    want = _excl_ref(raw.double(), bias.double())
    got = merge(out).double()
    assert (got[..., 1856:] - want).abs().max().item() <= 2e-6 * max(1.0, want.abs().max().item())
    assert got[..., :1856].abs().max().item() == 0


def test_classifier_2048_to_51_split_vs_fp64(cuda_device):
    """The 1x1 split convolution of the bird head: 51 couts, the last 8-cout chunk (48..55) and the 64-cout tile partial.
    The destination row is padded to 56 (SplitTrunk.fc_logits); a row of 51 is refused by the launcher, not overrun."""
    from tise_toolbox_amd import _lib
    from tise_toolbox_amd.conv_split import SplitConv, split
    g = torch.Generator().manual_seed(51)
    for n in (1, 5, 130):
        w = torch.randn((51, 2048, 1, 1), generator=g) * 0.05
        x = torch.rand((n, 1, 1, 2048), generator=g) * 2.0
        conv = SplitConv(w.to(cuda_device), torch.zeros(51), (1, 1), (0, 0), cuda_device, variant="fast")
        out = torch.full((n, 1, 1, 56), 7.0, device=cuda_device)
        conv(split(x.to(cuda_device)), [(0, 51, out, 0, 1)])
        want = x.double().view(n, 2048) @ w.double().view(51, 2048).T
        got = out.view(n, 56)[:, :51].double().cpu()
        assert (got - want).abs().max().item() <= 4e-6 * want.abs().max().item(), n
        assert bool((out.view(n, 56)[:, 51:] == 0).all())                  # zero-weight couts of the padded chunk
        tight = torch.zeros((n, 1, 1, 52), device=cuda_device)
        with pytest.raises(_lib.TiseStatusError, match="invalid argument"):
            conv(split(x.to(cuda_device)), [(0, 51, tight, 0, 1)])


# ------------------------------------------------------------------------------------------------------- trunks
@pytest.fixture(scope="module")
def netslim(cuda_device):
    from tise_toolbox_amd.inception import build_inception3
    torch.set_num_threads(min(16, torch.get_num_threads()))
    sd = {k: v.float() for k, v in build_inception3(seed=0, network=NET).state_dict().items()}
    assert all(bool((v == 1).all()) for k, v in sd.items() if k.endswith("bn.weight"))
    tf = slim_checkpoint_tensors(sd, extra=False)
    u8 = np.stack([resize_oracle.resize_bilinear_u8(im, 299, 299) for im in _cases.smooth_images(4, 256, 256, seed=5)])
    feats, logits = ref.features_of_u8(tf, u8, torch.float64, chunk=4)
    return dict(sd=sd, tf=tf, u8=u8, feats=feats, logits=logits)


@pytest.mark.parametrize("conv", ["split", "miopen"])
def test_trunk_features_and_logits_vs_fp64(cuda_device, netslim, conv, monkeypatch):
    from tise_toolbox_amd.engine import RealismEngine
    from tise_toolbox_amd.trunk import FusedTrunk, SplitTrunk
    monkeypatch.setenv("TISE_CONV", conv)
    torch.backends.cudnn.benchmark = False
    eng = RealismEngine(dims=2048, seed=0, with_logits=True, network=NET)
    assert type(eng.fused) is (SplitTrunk if conv == "split" else FusedTrunk) and eng.fused.avg_excl
    assert eng.model.fc.out_features == 51
    eng.begin(n_total=4, rule="bird", drop_first_class=True)               # bird: the biased logits
    feats, logits = eng.features_from_u8(torch.as_tensor(netslim["u8"], device=cuda_device))
    f, want = feats.double().cpu().numpy(), netslim["feats"]
    print(conv, "pool3 max abs err", np.abs(f - want).max(), "scale", np.abs(want).max())
    assert np.abs(f - want).max() <= 2e-4 * np.abs(want).max()
    lg, lw = logits.double().cpu().numpy(), netslim["logits"]
    assert lg.shape == (4, 51)
    assert np.abs(lg - lw).max() <= 2e-3 * max(1.0, np.abs(lw).max())


# ----------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def bird_dir(tmp_path_factory):
    from PIL import Image
    d = tmp_path_factory.mktemp("birds") / "imgs"
    d.mkdir()
    for i, im in enumerate(_cases.smooth_images(203, 96, 112, seed=31)):
        Image.fromarray(im).save(d / f"{i:05d}.png")
    return d


@pytest.fixture(scope="module")
def checkpoints(netslim, tmp_path_factory):
    root = tmp_path_factory.mktemp("ckpt")
    tensors = slim_checkpoint_tensors(netslim["sd"])
    v1, v2 = str(root / "v1" / "model.ckpt"), str(root / "v2" / "model.ckpt")
    (root / "v1").mkdir()
    (root / "v2").mkdir()
    write_v1(v1, tensors, compression=1, block_size=1 << 16)
    write_v2(v2, tensors, compression=0)
    return v1, v2


def test_bird_cli_vs_cpu(cuda_device, netslim, bird_dir, checkpoints, tmp_path, capsys, monkeypatch):
    from PIL import Image
    from tise_toolbox_amd import img_data, inception_score as isc, inception_score_bird as bird
    monkeypatch.setenv("TISE_CONV", "split")
    files = img_data.get_filenames(str(bird_dir))
    chosen = bird.bird_selection(files, 64, seed=7)
    assert len(chosen) == 192
    u8 = np.stack([resize_oracle.resize_bilinear_u8(np.asarray(Image.open(f).convert("RGB")), 299, 299) for f in chosen])
    _, lg = ref.features_of_u8(netslim["tf"], u8, torch.float32, chunk=16)
    want = is_oracle.inception_score_from_logits(lg[:, 1:], T_BIRD, 10, "coco", dtype=np.float64)
    try:
        results = []
        for ck in checkpoints:
            out = tmp_path / f"is_{len(results)}.txt"
            mean, std = bird.main(["--image_folder", str(bird_dir), "--saved_file", str(out), "--checkpoint_dir", ck,
                                   "--shuffle-seed", "7"])
            print("IS* slim device", mean, std, "cpu", want)
            assert abs(mean - want[0]) <= 1e-4 and abs(std - want[1]) <= 1e-4
            assert out.read_text() == f"IS = {mean}  +-  {std}"
            assert f"mean: {mean:.2f} std: {std:.2f}" in capsys.readouterr().out
            assert isc._ENGINE.model.network == NET and isc._ENGINE.model.fc.out_features == 51
            results.append((mean, std))
        again = bird.main(["--image_folder", str(bird_dir), "--checkpoint_dir", checkpoints[1], "--shuffle-seed", "7"])
        assert results[0] == results[1] == again                            # same weights, same order: bit-identical
        # the stand-in run is tagged and gives the same numbers (the checkpoint holds the stand-in weights)
        syn = tmp_path / "syn.txt"
        m3 = bird.main(["--image_folder", str(bird_dir), "--saved_file", str(syn), "--synthetic-weights", "--shuffle-seed", "7"])
        from tise_toolbox_amd.weights import SYNTHETIC_TAG
        assert syn.read_text() == f"IS = {m3[0]}  +-  {m3[1]}" + SYNTHETIC_TAG and m3 == again
    finally:
        isc.configure(network="torchvision", rule="coco", drop_first_class=False, temperature=is_oracle.T_COCO, weights=None,
                      num_classes=None, num_workers=0, png_feed="ring")


def test_calibration_slim_bird_feeds_the_bird_cli(cuda_device, netslim, checkpoints, tmp_path, monkeypatch):
    from PIL import Image
    from tise_toolbox_amd import calibration, inception_score as isc, inception_score_bird as bird
    monkeypatch.setenv("TISE_CONV", "split")
    d = tmp_path / "labelled"
    imgs = _cases.smooth_images(24, 80, 80, seed=41)
    for i, im in enumerate(imgs):
        sub = d / f"class_{i % 3:02d}"
        sub.mkdir(parents=True, exist_ok=True)
        Image.fromarray(im).save(sub / f"{i:03d}.png")
    try:
        res = calibration.main(["--network", NET, "--rule", "bird", "--image_dir", str(d), "--weights", checkpoints[1],
                                "--saved_file", str(tmp_path / "t.txt")])
        t = float(res["temperature"])
        assert np.isfinite(t) and t > 0
        # the same fit from the CPU path's logits (class offset 1: label k is logit column k + 1)
        files, labels, _ = calibration.labels_from_subdirs(str(d))
        u8 = np.stack([resize_oracle.resize_bilinear_u8(np.asarray(Image.open(f).convert("RGB")), 299, 299) for f in files])
        _, lg = ref.features_of_u8(netslim["tf"], u8, torch.float32, chunk=12)
        cpu = calibration.set_temperature_from_logits(torch.as_tensor(lg, device=cuda_device).float().contiguous(), labels,
                                                      c0=1, verbose=False)
        assert abs(cpu["temperature"] - t) <= 1e-3 * max(1.0, abs(t))
        out = tmp_path / "is.txt"
        m = bird.main(["--image_folder", str(d), "--saved_file", str(out), "--checkpoint_dir", checkpoints[0],
                       "--shuffle-seed", "3", "--batch_size", "8", "--temperature", repr(t)])
        assert isc._CONFIG["temperature"] == t and out.read_text() == f"IS = {m[0]}  +-  {m[1]}"
    finally:
        isc.configure(network="torchvision", rule="coco", drop_first_class=False, temperature=is_oracle.T_COCO, weights=None,
                      num_classes=None, num_workers=0, png_feed="ring")
