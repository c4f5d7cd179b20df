"""GPU: clip_score end to end on the tiny open_clip tower (tests/test_openclip_host.py's: heads of 80, exact GELU) with seeded
parameters: 12 PNGs of 64 x 64 with a captions JSON, and again with an RP pickle.  Both result lines equal numpy fp64 on the
--save-features rows within 1e-12, the Python API returns the same values, `--prefix ""` changes the number, and a missing
caption or image is refused with the reason."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TINY = dict(resolution=154, patch=14, width=160, layers=2, heads=2, embed_dim=64, text_width=128, text_layers=2, text_heads=2,
            act="gelu")
TINY_NAME = "tiny-test-H"
WORDS = "a photo of two red green small large dogs cats on the table near water under sky".split()


def _png_dir(path, n, seed):
    from PIL import Image
    from tests import _cases
    os.makedirs(path)
    pool = _cases.smooth_images(12, 64, 64, seed=seed)
    for k in range(n):
        Image.fromarray(np.ascontiguousarray(np.roll(pool[k % 12], 3 * k + seed, axis=1))).save(os.path.join(path, f"{k}.png"))
    return str(path)


def _numpy_lines(npz, tower, tag, w=2.5):
    with np.load(npz) as f:
        a, b = f["image_features"].astype(np.float64), f["text_features"].astype(np.float64)
    cos = (a * b).sum(1) / np.sqrt((a * a).sum(1) * (b * b).sum(1))
    s = w * np.maximum(cos, 0)
    return s.mean(), s.std(), 100 * cos.mean(), cos


def _parse(lines):
    a, b = lines
    head, rest = a.split(": ", 1)
    mean, std = rest.split(" [")[0].split(" +- ")
    return float(mean), float(std), float(b.split(": ", 1)[1].split(" [")[0])


@pytest.mark.timeout(300)
@pytest.mark.parametrize("route", [None, "torch"], ids=["default-route", "library-module"])
def test_cli_on_a_captions_json_and_an_rp_pickle(cuda_device, tmp_path, capfd, monkeypatch, route):
    """``route``: the default (clip_hip.HipTowers: head width 80, the exact GELU and the K-padded GEMMs under the CLI) and
    TISE_CLIP=torch (the fp16 library module, the route a tower wider than 1024 columns takes)."""
    from tise_toolbox_amd import clip_score, openclip_model
    from tise_toolbox_amd.weights import SYNTHETIC_TAG
    monkeypatch.setitem(openclip_model.CONFIGS, TINY_NAME, TINY)
    if route:
        monkeypatch.setenv("TISE_CLIP", route)
    else:
        monkeypatch.delenv("TISE_CLIP", raising=False)
    d = _png_dir(tmp_path / "img", 12, 3)
    rng = np.random.default_rng(0)
    caps = {(f"{k}.png" if k % 2 else str(k)): " ".join(rng.choice(WORDS, 3 + k % 5)) for k in range(12)}
    caps["11.png"] = caps["1.png"]                                                     # a repeated caption: embedded once
    cj, pk, npz, txt = (str(tmp_path / n) for n in ("caps.json", "rp.pkl", "rows.npz", "out.txt"))
    json.dump(caps, open(cj, "w"))
    tail = ["--image_dir", d, "--tower", TINY_NAME, "--synthetic-weights", "--batch-size", "5", "--num-workers", "2"]
    capfd.readouterr()
    res = clip_score.main(tail + ["--captions", cj, "--save-features", npz, "--saved_file", txt])
    lines = [ln for ln in capfd.readouterr().out.splitlines() if ln.startswith(("CLIPScore (", "Cosine x100 ("))]
    assert len(lines) == 2 and lines[0].startswith(f"CLIPScore ({TINY_NAME}): ") and lines[1].startswith(f"Cosine x100 ({TINY_NAME}): ")
    assert all(ln.endswith(SYNTHETIC_TAG) for ln in lines) and open(txt).read() == "\n".join(lines)
    mean, std, c100, cos = _numpy_lines(npz, TINY_NAME, SYNTHETIC_TAG)
    got = _parse(lines)
    print(f"captions JSON: CLIPScore {got[0]} +- {got[1]}, cosine x100 {got[2]}; numpy on the saved rows {mean} +- {std}, {c100}")
    assert abs(got[0] - mean) <= 1e-12 and abs(got[1] - std) <= 1e-12 and abs(got[2] - c100) <= 1e-12
    assert res["n"] == 12 and np.abs(res["cos"] - cos).max() <= 1e-12 and std > 0
    # the Python API: from the rows, and from the paths
    with np.load(npz) as f:
        api = clip_score.clip_score_from_features(f["image_features"], f["text_features"])
        half = clip_score.clip_score_from_features(torch.from_numpy(f["image_features"]).half().to(cuda_device),
                                                   torch.from_numpy(f["text_features"]).half().to(cuda_device), w=2.5)
        assert str(f["tower"]) == TINY_NAME and f["image_features"].shape == (12, 64) and f["text_features"].shape == (12, 64)
    for r in (api, half):                                                                # the saved rows are fp16 values: the same bits
        assert (r["clip_score"], r["clip_score_std"], r["cosine_x100"]) == (res["clip_score"], res["clip_score_std"], res["cosine_x100"])
        assert np.array_equal(r["cos"], res["cos"])
    again = clip_score.calculate_clip_score_given_paths(d, captions_file=cj, tower=TINY_NAME, batch_size=5, num_workers=2)
    assert again["clip_score"] == res["clip_score"] and np.array_equal(again["cos"], res["cos"])
    # another prefix is another number; w scales the first line only
    bare = clip_score.calculate_clip_score_given_paths(d, captions_file=cj, tower=TINY_NAME, batch_size=5, num_workers=2, prefix="")
    assert bare["cosine_x100"] != res["cosine_x100"] and not np.array_equal(bare["cos"], res["cos"])
    w1 = clip_score.calculate_clip_score_given_paths(d, captions_file=cj, tower=TINY_NAME, batch_size=5, num_workers=2, w=1.0)
    assert w1["cosine_x100"] == res["cosine_x100"] and abs(w1["clip_score"] * 2.5 - res["clip_score"]) <= 1e-12
    # the RP pickle: the true caption and <caption_id>.png, in item order
    order = [5, 0, 11, 3, 7, 1, 2, 4, 6, 8, 9, 10]
    cap_of = lambda k: caps[f"{k}.png" if k % 2 else str(k)]
    pickle.dump([{"caption_id": k, "caption": cap_of(k), "mismatched_captions": ["x"] * 2} for k in order], open(pk, "wb"))
    capfd.readouterr()
    rp = clip_score.main(tail + ["--rp_input_file", pk, "--save-features", npz])
    lines_rp = [ln for ln in capfd.readouterr().out.splitlines() if ln.startswith(("CLIPScore (", "Cosine x100 ("))]
    mean, std, c100, cos_rp = _numpy_lines(npz, TINY_NAME, SYNTHETIC_TAG)
    got = _parse(lines_rp)
    assert abs(got[0] - mean) <= 1e-12 and abs(got[1] - std) <= 1e-12 and abs(got[2] - c100) <= 1e-12
    by_name = {os.path.basename(p): c for p, c in zip(sorted(os.listdir(d)), res["cos"])}   # the JSON road sorts by file name
    same = np.array([by_name[f"{k}.png"] for k in order])
    if route is None:
        assert np.array_equal(rp["cos"], same)                                             # the same pairs, the same bits: batch-invariant kernels
    else:                                                                                  # library kernels may differ with the batch: fp16 rows,
        assert np.abs(rp["cos"] - same).max() <= 4 * 2.0 ** -11                            # each element within 2^-11 relative, twice per side
    # refusals, with the reason
    short = dict(caps)
    del short["4"]
    json.dump(short, open(cj, "w"))
    with pytest.raises(RuntimeError, match="missing caption: image '4.png'"):
        clip_score.main(tail + ["--captions", cj])
    json.dump(dict(caps, **{"40": "nothing there"}), open(cj, "w"))
    with pytest.raises(RuntimeError, match="missing image: caption '40'"):
        clip_score.main(tail + ["--captions", cj])
    os.remove(os.path.join(d, "7.png"))
    with pytest.raises(RuntimeError, match="missing image: .*7.png"):
        clip_score.main(tail + ["--rp_input_file", pk])
    with pytest.raises(RuntimeError, match="no default file"):                              # no parameters and no --synthetic-weights
        clip_score.main(["--image_dir", d, "--tower", TINY_NAME, "--rp_input_file", pk])
