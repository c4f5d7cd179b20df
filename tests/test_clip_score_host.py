"""CPU: clip_score's host logic -- caption-file parsing and its refusals, the RP pickle's pairs, the result-line format, and that
{n, sum, sum of squares} is additive over unequal shards, one of them empty."""
import json
import os
import pickle

import numpy as np
import pytest


def _touch(d, names):
    os.makedirs(d, exist_ok=True)
    for n in names:
        open(os.path.join(d, n), "wb").close()
    return str(d)


def test_caption_file_parsing(tmp_path):
    from tise_toolbox_amd import clip_score
    d = _touch(tmp_path / "img", ["b.png", "a.png", "c.jpg", "notes.txt"])
    paths, caps = clip_score.pairs_from_captions(d, {"a": "first", "b.png": "second", "c": "third"})
    assert [os.path.basename(p) for p in paths] == ["a.png", "b.png", "c.jpg"] and caps == ["first", "second", "third"]
    with pytest.raises(RuntimeError, match="missing caption: image 'c.jpg'"):
        clip_score.pairs_from_captions(d, {"a": "first", "b": "second"})
    with pytest.raises(RuntimeError, match="missing image: caption 'z'"):
        clip_score.pairs_from_captions(d, {"a": "1", "b": "2", "c": "3", "z": "4"})
    with pytest.raises(RuntimeError, match="two captions"):
        clip_score.pairs_from_captions(d, {"a": "1", "a.png": "1 again", "b": "2", "c": "3"})
    with pytest.raises(RuntimeError, match="not a string"):
        clip_score.pairs_from_captions(d, {"a": ["1"], "b": "2", "c": "3"})
    with pytest.raises(RuntimeError, match="one JSON object"):
        clip_score.pairs_from_captions(d, ["1", "2", "3"])
    _touch(d, ["a.jpg"])
    with pytest.raises(RuntimeError, match="more than one image"):
        clip_score.pairs_from_captions(d, {"a": "1", "b": "2", "c": "3"})
    # through the files
    os.remove(os.path.join(d, "a.jpg"))
    cj = str(tmp_path / "caps.json")
    json.dump({"a": "first", "b": "second", "c": "third"}, open(cj, "w"))
    assert clip_score.load_pairs(d, captions_file=cj)[1] == ["first", "second", "third"]
    with pytest.raises(RuntimeError, match="exactly one"):
        clip_score.load_pairs(d)
    with pytest.raises(RuntimeError, match="exactly one"):
        clip_score.load_pairs(d, cj, cj)
    with pytest.raises(RuntimeError, match="Invalid path"):
        clip_score.load_pairs(str(tmp_path / "nowhere"), cj)


def test_rp_pickle_pairs(tmp_path):
    from tise_toolbox_amd import clip_score
    d = _touch(tmp_path / "img", ["7.png", "12.png"])
    rp = [{"caption_id": 12, "caption": "twelve", "mismatched_captions": ["x"] * 3},
          {"caption_id": 7, "caption": "seven", "mismatched_captions": ["y"] * 3}]
    pk = str(tmp_path / "rp.pkl")
    pickle.dump(rp, open(pk, "wb"))
    paths, caps = clip_score.load_pairs(d, rp_input_file=pk)
    assert [os.path.basename(p) for p in paths] == ["12.png", "7.png"] and caps == ["twelve", "seven"]   # item order, true captions
    with pytest.raises(RuntimeError, match="missing image: .*9.png"):
        clip_score.pairs_from_rp(d, rp + [{"caption_id": 9, "caption": "nine"}])
    with pytest.raises(RuntimeError, match="missing caption: item 2"):
        clip_score.pairs_from_rp(d, rp + [{"caption_id": 7}])


def test_sums_are_additive_and_give_numpy_s_statistics():
    from tise_toolbox_amd import clip_score
    rng = np.random.default_rng(3)
    cos = rng.uniform(-0.2, 0.6, 37)
    whole = clip_score.score_sums(cos, 2.5)
    parts = clip_score.score_sums(cos[:5], 2.5) + clip_score.score_sums(cos[5:5], 2.5) + clip_score.score_sums(cos[5:], 2.5)
    assert np.array_equal(clip_score.score_sums(cos[5:5]), np.zeros((2, 3)))              # an empty shard adds nothing
    assert np.allclose(parts, whole, rtol=1e-15, atol=0) and parts[0, 0] == 37
    res = clip_score.result_from_sums(parts)
    s = 2.5 * np.maximum(cos, 0)
    assert res["n"] == 37 and (cos < 0).any()
    assert abs(res["clip_score"] - s.mean()) <= 1e-12 and abs(res["clip_score_std"] - s.std()) <= 1e-12
    assert abs(res["cosine_x100"] - 100 * cos.mean()) <= 1e-12
    assert clip_score.result_from_sums(clip_score.score_sums(cos, 1.0))["clip_score"] == pytest.approx(np.maximum(cos, 0).mean(), abs=1e-15)
    with pytest.raises(RuntimeError, match="at least one"):
        clip_score.result_from_sums(np.zeros((2, 3)))
    nan = clip_score.result_from_sums(clip_score.score_sums([0.3, np.nan]))                # a zero row shows
    assert np.isnan(nan["clip_score"]) and np.isnan(nan["clip_score_std"]) and np.isnan(nan["cosine_x100"])
    one = clip_score.result_from_sums(clip_score.score_sums([0.25]))
    assert one["clip_score"] == 0.625 and one["clip_score_std"] == 0.0 and one["cosine_x100"] == 25.0


def test_result_lines_and_cli_surface():
    from tise_toolbox_amd import clip_score, weights
    res = {"clip_score": 0.625, "clip_score_std": 0.125, "cosine_x100": 25.0, "n": 2}
    assert clip_score.result_lines(res, "ViT-H-14") == ["CLIPScore (ViT-H-14): 0.625 +- 0.125", "Cosine x100 (ViT-H-14): 25.0"]
    tagged = clip_score.result_lines(res, "ViT-B/32", weights.SYNTHETIC_TAG)
    assert all(ln.endswith(weights.SYNTHETIC_TAG) for ln in tagged) and len(tagged) == 2
    assert clip_score.towers() == ["ViT-B/32", "ViT-L/14@336", "ViT-H-14"]
    args = clip_score.parse_args(["--image_dir", "d", "--captions", "c.json"])
    assert (args.tower, args.prefix, args.w, args.batch_size, args.gpu_id) == ("ViT-B/32", "A photo depicts ", 2.5, 256, "0")
    assert clip_score.parse_args(["--image_dir", "d", "--rp_input_file", "r.pkl", "--tower", "ViT-H-14", "--prefix", ""]).prefix == ""
    # ViT-H-14 has no default parameter file: --weights or --synthetic-weights it has to be
    assert clip_score.tower_kind("ViT-H-14") is None and clip_score.tower_kind("ViT-B/32") == "clip"
    with pytest.raises(RuntimeError, match="no default file"):
        weights.resolve(None, False, clip_score.tower_kind("ViT-H-14"), "CLIP ViT-H-14")
    with pytest.raises(ValueError):
        clip_score.tower_kind("ViT-g-14")
