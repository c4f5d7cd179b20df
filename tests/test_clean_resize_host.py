"""CPU: the numpy restatement of Pillow's float32 resize (tests/_clean_resize_ref.py) against Pillow itself, bit for bit, and the
plumbing of fid_score --mode clean that needs no device.  Writes nothing: tests/golden/pil_resize_f32.npz is made once by
tests/golden/make_golden_clean_resize.py."""
import os

import numpy as np
import pytest

from tests import _clean_resize_ref as ref

SHAPES = [(256, 256), (480, 640), (37, 53), (299, 400), (300, 298), (299, 299), (1, 1), (2, 3), (1000, 700), (1000, 9), (3000, 17),
          (9, 1000)]


def _same_bits(a, b):
    a, b = ref.bits(a), ref.bits(b)
    assert a.shape == b.shape
    bad = int((a != b).sum())
    assert bad == 0, f"{bad} of {a.size} values differ in their bits"


@pytest.mark.parametrize("kind", ["rand", "bw"])
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_equals_pillow_bicubic(hw, kind):
    x = ref.content(kind, 1000 + hw[0] + hw[1], *hw)
    _same_bits(ref.resize_f32(x, (299, 299), "bicubic"), ref.pil_resize_f32(x, (299, 299), "bicubic"))


@pytest.mark.parametrize("hw", [(480, 640), (37, 53), (1000, 9)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_equals_pillow_bilinear(hw):
    x = ref.content("rand", 7, *hw)
    _same_bits(ref.resize_f32(x, (299, 299), "bilinear"), ref.pil_resize_f32(x, (299, 299), "bilinear"))


def test_zero_and_255_content_drives_both_clips():
    y = ref.resize_f32(ref.content("bw", 3, 256, 256), (299, 299))
    assert y.min() < -60 and y.max() > 315                       # bicubic overshoot: about -70 and about 326
    z = ref.affine(y)
    assert z.min() == -1.0 and z.max() == np.float32((255.0 - 128.0) / 128.0)


def test_tall_rule_is_visible_and_the_restatement_follows_it():
    """(1000, 9) and (3000, 17) -> 299 x 299: horizontal-first differs from Pillow in the last bit of many pixels, vertical-first
    is Pillow; the rule itself is the device's (device.pillow_vertical_first) and the restatement's, which must agree."""
    from tise_toolbox_amd import device
    for h, w in ((1000, 9), (3000, 17)):
        x = ref.content("rand", 5, h, w)
        pil = ref.pil_resize_f32(x, (299, 299))
        assert (ref.bits(ref.resize_f32(x, (299, 299), order=0)) != ref.bits(pil)).mean() > 0.05
        _same_bits(ref.resize_f32(x, (299, 299), order=1), pil)
    for h, w, oh in ((1000, 9, 299), (1000, 10, 299), (901, 9, 299), (900, 9, 299), (200, 1, 299), (299, 2, 299), (300, 2, 299),
                     (3000, 17, 299), (64, 2000, 37), (2000, 64, 37)):
        assert device.pillow_vertical_first(h, w, oh) == ref.vertical_first(h, w, oh) == (h > 100 * w and oh < h)


def test_golden_file_is_what_this_pillow_gives():
    """The committed Pillow outputs the GPU tests compare with (made with the Pillow version the file names) are this
    restatement's bits too, so the file and the restatement pin the same thing."""
    import hashlib
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pil_resize_f32.npz"))
    assert os.path.getsize(g.fid.name) < 700 * 1024
    n = int(g["n_cases"])
    assert n >= 10
    for i in range(n):
        kind, seed, h, w, oh, ow, filt = [str(v) for v in g[f"case_{i}"]]
        y = ref.resize_f32(ref.content(kind, int(seed), int(h), int(w)), (int(oh), int(ow)), filt)
        if f"out_{i}" in g.files:
            _same_bits(y, g[f"out_{i}"])
        else:
            assert hashlib.sha256(np.ascontiguousarray(y).tobytes()).hexdigest() == str(g[f"sha_{i}"])
            _same_bits(y[::int(g["row_step"])], g[f"rows_{i}"])


# ---- mode plumbing -------------------------------------------------------------------------------------------------------
def test_mode_clean_refuses_another_network(capsys):
    from tise_toolbox_amd import fid_score
    assert fid_score.resolve_mode("clean", None) == "inception-2015"
    assert fid_score.resolve_mode("clean", "inception-2015") == "inception-2015"
    assert fid_score.resolve_mode("tise", None) == "torchvision"
    assert fid_score.resolve_mode("tise", "inception-2015") == "inception-2015"
    with pytest.raises(ValueError, match="inception-2015 only"):
        fid_score.resolve_mode("clean", "torchvision")
    with pytest.raises(ValueError, match="unknown mode"):
        fid_score.resolve_mode("legacy_tensorflow", None)
    with pytest.raises(SystemExit) as e:                          # refused by the parser, before a device or a file is touched
        fid_score.main(["--path1", "a", "--path2", "b", "--mode", "clean", "--network", "torchvision", "--synthetic-weights"])
    assert e.value.code == 2 and "inception-2015 only" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        fid_score.main(["--path1", "a", "--path2", "b", "--mode", "clean", "--u8-cache", "--synthetic-weights"])
    a = fid_score._build_parser().parse_args(["--path2", "b"])
    assert a.mode == "tise" and a.network == "torchvision" and a.network_given is False


def test_stats_npz_mode_tag(tmp_path):
    from tise_toolbox_amd import fid_score
    mu, sigma = np.arange(4.0), np.eye(4)
    pc, pt, pu = str(tmp_path / "c.npz"), str(tmp_path / "t.npz"), str(tmp_path / "u.npz")
    fid_score.save_stats_npz(pc, mu, sigma, "inception-2015", mode="clean")
    fid_score.save_stats_npz(pt, mu, sigma, "inception-2015", mode="tise")
    np.savez(pu, mu=mu, sigma=sigma, network=np.asarray("inception-2015"))           # a file from before the tag existed
    with np.load(pc) as f:
        assert sorted(f.files) == ["mode", "mu", "network", "sigma"] and str(f["mode"]) == "clean"
    with np.load(pt) as f:
        assert sorted(f.files) == ["mu", "network", "sigma"]                         # the default mode's files stay what they were

    class Model:                                                                      # what _compute_statistics_of_path reads of a model
        network = "inception-2015"

        def __init__(self, mode):
            self.fid_mode = mode

    def load(path, mode):
        return fid_score._compute_statistics_of_path(path, Model(mode), 50, 4, True)

    m, s = load(pc, "clean")
    assert np.array_equal(m, mu) and np.array_equal(s, sigma)
    for path in (pt, pu):                                                             # untagged reads as tise
        m, s = load(path, "tise")
        assert np.array_equal(m, mu)
        with pytest.raises(RuntimeError, match="statistics of mode 'tise', this run uses --mode clean"):
            load(path, "clean")
    with pytest.raises(RuntimeError, match="statistics of mode 'clean', this run uses --mode tise"):
        load(pc, "tise")


def test_engine_resize_default_is_the_reference():
    import inspect
    from tise_toolbox_amd import engine
    assert engine.RESIZES == ("reference", "clean")
    assert inspect.signature(engine.RealismEngine.__init__).parameters["resize"].default == "reference"
