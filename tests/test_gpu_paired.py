"""GPU: tise_toolbox_amd.paired end to end -- psnr_ssim_from_images against tests/_ssim_ref.py, and the CLI on two temporary
directories against the functions on the same decoded arrays.

Bounds (derived; the measured values are printed and quoted in README's paired entry):
  PSNR     1e-12 relative: the SSE is an exact integer on both sides, only log10 differs.
  SSIM     3e-9 absolute, the bound of tests/test_gpu_ssim.py for a map mean (a channel mean of three such means).
  MS-SSIM  1e-7 absolute: d prod m_s^w_s <= sum_s w_s 3e-9 / m_s with every m_s >= 0.05 -- and that condition is asserted FROM THE
           REFERENCE ALONE before anything is compared."""
import os

import numpy as np
import pytest

from tests import _jpeg_writer
from tests import _ssim_ref as ref

SHAPES = [(176, 176), (177, 191), (256, 256)]
SIGMAS = (4, 25)


@pytest.mark.gpu
def test_psnr_ssim_ms_ssim_against_the_reference(cuda_device):
    import torch
    from tise_toolbox_amd import paired
    pairs = [ref.smooth_pair(h, w, s, seed=7 * h + w + s) for (h, w) in SHAPES for s in SIGMAS]
    scale = np.stack([ref.ms_scale_means(x, y) for x, y in pairs])
    assert scale.min() >= 0.05, scale.min()                              # the MS-SSIM bound's condition, from the reference alone
    want_psnr = np.array([ref.psnr(x, y) for x, y in pairs])
    want_ssim = np.array([ref.ssim(x, y) for x, y in pairs])
    want_ms = np.array([ref.ms_from_means(m) for m in scale])
    xs = [torch.as_tensor(x, device=cuda_device) for x, _ in pairs]
    ys = [torch.as_tensor(y, device=cuda_device) for _, y in pairs]
    got = paired.psnr_ssim_from_images(xs, ys, ms_ssim=True)
    assert got["sse"].tolist() == [ref.sse(x, y) for x, y in pairs]
    d_psnr = float(np.max(np.abs(got["psnr"] - want_psnr) / want_psnr))
    d_ssim = float(np.max(np.abs(got["ssim"] - want_ssim)))
    d_scale = float(np.max(np.abs(got["ms_scale_means"] - scale)))
    d_ms = float(np.max(np.abs(got["ms_ssim"] - want_ms)))
    print(f"paired vs reference: PSNR rel {d_psnr:.3e}, SSIM {d_ssim:.3e}, scale means {d_scale:.3e}, MS-SSIM {d_ms:.3e}; "
          f"smallest reference scale mean {scale.min():.3f}")
    assert d_psnr <= 1e-12 and d_ssim <= 3e-9 and d_scale <= 3e-9 and d_ms <= 1e-7
    again = paired.psnr_ssim_from_images(xs[::-1], ys[::-1], ms_ssim=True)          # another order, other neighbours: the same bits
    for k in ("psnr", "ssim", "ms_ssim"):
        assert again[k][::-1].tobytes() == got[k].tobytes(), k
    plain = paired.psnr_ssim_from_images(torch.stack(xs[4:6]), torch.stack(ys[4:6]))
    assert "ms_ssim" not in plain and plain["ssim"].tobytes() == got["ssim"][4:6].tobytes()
    same = paired.psnr_ssim_from_images(xs[:2], [t.clone() for t in xs[:2]], ms_ssim=True)
    assert np.all(np.isposinf(same["psnr"])) and same["ssim"].tolist() == [1.0, 1.0] and same["ms_ssim"].tolist() == [1.0, 1.0]
    with pytest.raises(ValueError, match="176"):
        paired.psnr_ssim_from_images([xs[0][:175]], [ys[0][:175]], ms_ssim=True)
    with pytest.raises(ValueError, match="11"):
        paired.psnr_ssim_from_images([xs[0][:10]], [ys[0][:10]])


def _jpeg_bytes(h, w, seed):
    """A 4:4:4 baseline JPEG of smooth random content: per block a DC term and three low AC terms, quantisation step 8."""
    rng = np.random.default_rng(seed)
    shapes = _jpeg_writer.blocks_shape(w, h, [(1, 1)] * 3)
    blocks = []
    for bh, bw in shapes:
        b = np.zeros((bh, bw, 64), dtype=np.int64)
        b[:, :, 0] = rng.integers(-60, 61, size=(bh, bw))
        b[:, :, [1, 8, 9]] = rng.integers(-6, 7, size=(bh, bw, 3))
        blocks.append(b)
    return _jpeg_writer.write_jpeg(w, h, blocks, [np.full(64, 8)] * 3)


@pytest.fixture(scope="module")
def directories(tmp_path_factory):
    """ORIG (PNG) and RECON (JPEG, one level deeper for two of them), 7 pairs of two sizes; pair 3 is identical.  -> (orig dir,
    recon dir, decoded originals, decoded reconstructions, stems) in the order of the sorted stems."""
    from PIL import Image
    root = tmp_path_factory.mktemp("paired")
    orig, recon = str(root / "orig"), str(root / "recon")
    stems = ["a/p0", "a/p1", "p2", "p3", "p4", "p5", "p6"]
    sizes = [(176, 176), (177, 191), (176, 176), (177, 191), (176, 176), (176, 176), (177, 191)]
    xs, ys = [], []
    rng = np.random.default_rng(5)
    for k, (stem, (h, w)) in enumerate(zip(stems, sizes)):
        for d in (orig, recon):
            os.makedirs(os.path.dirname(os.path.join(d, stem)), exist_ok=True)
        with open(os.path.join(recon, stem + ".jpg"), "wb") as f:
            f.write(_jpeg_bytes(h, w, k))
        y = np.asarray(Image.open(os.path.join(recon, stem + ".jpg")).convert("RGB")).copy()
        assert y.shape == (h, w, 3)
        x = y.copy() if k == 3 else np.clip(np.rint(y + rng.normal(0.0, 6.0, y.shape)), 0, 255).astype(np.uint8)
        Image.fromarray(x).save(os.path.join(orig, stem + ".png"))
        xs.append(x)
        ys.append(y)
    assert sorted(stems) == stems
    return orig, recon, xs, ys, stems


@pytest.mark.gpu
def test_cli_on_two_directories(cuda_device, directories, tmp_path, capsys):
    """7 pairs, two sizes, --batch-size 3 (a ragged directory, a last short batch), PNG against JPEG, one identical pair: the
    result lines, the CSV, the identical-pairs line and mean +- std against the functions on the same decoded arrays."""
    import torch
    from tise_toolbox_amd import paired
    orig, recon, xs, ys, stems = directories
    want = paired.psnr_ssim_from_images([torch.as_tensor(x, device=cuda_device) for x in xs],
                                        [torch.as_tensor(y, device=cuda_device) for y in ys], ms_ssim=True)
    csv, saved = str(tmp_path / "pairs.csv"), str(tmp_path / "out.txt")
    capsys.readouterr()
    res = paired.main(["--path1", orig, "--path2", recon, "--ms-ssim", "--batch-size", "3", "--num-workers", "2",
                       "--per-pair", csv, "--saved_file", saved])
    lines = capsys.readouterr().out.strip().split("\n")
    assert res["n"] == 7 and res["identical"] == 1
    for k in ("psnr", "ssim", "ms_ssim"):                                 # per pair: the bits of the one-batch call
        assert res["per_pair"][k].tobytes() == want[k].tobytes(), k
    assert np.isposinf(want["psnr"][3]) and np.isfinite(np.delete(want["psnr"], 3)).all()
    assert want["ssim"][3] == 1.0 and want["ms_ssim"][3] == 1.0
    assert lines[0] == "PSNR: inf +- nan" and lines[3] == "identical pairs: 1" and len(lines) == 4
    assert open(saved).read() == "\n".join(lines)
    for line, name, key in ((lines[1], "SSIM", "ssim"), (lines[2], "MS-SSIM", "ms_ssim")):
        head, rest = line.split(": ")
        mean, std = (float(v) for v in rest.split(" +- "))
        assert head == name and mean == res[key] and std == res[key + "_std"]
        assert np.std(want[key]) >= 1e-3                                  # the std below is no cancellation artefact
        assert abs(mean - np.mean(want[key])) <= 1e-14 and abs(std - np.std(want[key])) <= 1e-12, (line, np.mean(want[key]), np.std(want[key]))
    rows = open(csv).read().split("\n")
    assert rows[0] == "pair,file1,file2,h,w,psnr,ssim,ms_ssim" and rows[-1] == "" and len(rows) == 9
    for i, row in enumerate(rows[1:8]):
        f = row.split(",")
        ext1 = os.path.join(orig, stems[i] + ".png")
        ext2 = os.path.join(recon, stems[i] + ".jpg")
        assert f[:5] == [str(i), ext1, ext2, str(xs[i].shape[0]), str(xs[i].shape[1])]
        assert [float(v) for v in f[5:]] == [want["psnr"][i], want["ssim"][i], want["ms_ssim"][i]]
    # without --ms-ssim: no MS-SSIM line, an empty last field; the DataLoader road for side one gives the same numbers
    res2 = paired.main(["--path1", orig, "--path2", recon, "--batch-size", "3", "--num-workers", "2", "--png-feed", "dataloader",
                        "--per-pair", csv])
    lines2 = capsys.readouterr().out.strip().split("\n")
    assert lines2 == [lines[0], lines[1], lines[3]] and res2["ssim"] == res["ssim"]
    assert all(r.endswith(",") for r in open(csv).read().split("\n")[1:8])


@pytest.mark.gpu
def test_cli_self_pairs_is_reproducible(cuda_device, directories, tmp_path, capsys):
    import shutil
    from tise_toolbox_amd import paired
    orig, _, xs, _, stems = directories
    one = tmp_path / "one_size"
    one.mkdir()
    keep = [i for i in range(7) if xs[i].shape == (176, 176, 3)]
    for i in keep:
        shutil.copy(os.path.join(orig, stems[i] + ".png"), str(one / f"{i}.png"))
    capsys.readouterr()
    outs = []
    for _ in range(2):
        res = paired.main(["--path1", str(one), "--self-pairs", "5", "--seed", "0", "--ms-ssim", "--num-workers", "2"])
        outs.append((capsys.readouterr().out, res["per_pair"]["ms_ssim"].tobytes(), res["files1"], res["files2"]))
    assert outs[0] == outs[1] and res["n"] == 5 and res["identical"] == 0
    idx = paired.draw_self_pairs(len(keep), 5, 0)
    files = paired.list_files(str(one))
    assert res["files1"] == [files[i] for i in idx[:, 0]] and res["files2"] == [files[j] for j in idx[:, 1]]
    assert outs[0][0].startswith("PSNR: ") and "MS-SSIM: " in outs[0][0]
    with pytest.raises(SystemExit):
        paired.main(["--path1", str(one), "--path2", str(one), "--self-pairs", "5"])
