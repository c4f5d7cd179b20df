"""CPU: the numpy restatement of torch's float32 bilinear interpolation (tests/_torch_resize_ref.py) against the installed torch
itself and against torch's recorded outputs (tests/golden/torch_bilinear_f32.npz, made once by
tests/golden/make_golden_torch_resize.py), bit for bit, and the plumbing of fid_score --mode pytorch-fid / torch-fidelity that
needs no device.  Writes nothing outside tmp_path.

torch's CPU build has TWO bilinear kernels that differ in the last bits, and picks by the call: with more than one thread and
oh + ow > 128 (pytorch-fid's 299 x 299) the one ``ref.interpolate`` restates and csrc/resize_torch.hip implements; on ONE thread
(for 3 channels), and at the small outputs, the one ``ref.interpolate_channels_last_kernel`` restates.  Both are held to torch
here; the tests pin torch's thread count, which is otherwise the machine's."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

from tests import _torch_resize_ref as ref

# sources resized to 299 x 299: the nine of the issue, a scale just above 1, and a 3-pixel-wide column
SOURCES = [(1, 1), (2, 5), (64, 64), (256, 256), (299, 299), (150, 700), (512, 384), (640, 427), (1024, 1024), (300, 299), (700, 3)]
SMALL_SOURCES = [(1, 1), (2, 5), (64, 64), (299, 299), (640, 427), (700, 3), (512, 384)]


@pytest.fixture(autouse=True)
def two_torch_threads():
    """torch chooses its kernel by at::get_num_threads(): more than one here, whatever the machine has; restored afterwards."""
    import torch
    before = torch.get_num_threads()
    torch.set_num_threads(2)
    yield
    torch.set_num_threads(before)


def _same_bits(a, b, what=""):
    a, b = ref.bits(a), ref.bits(b)
    assert a.shape == b.shape
    bad = int((a != b).sum())
    assert bad == 0, f"{what}: {bad} of {a.size} values differ in their bits"


def test_fma_is_libm_fmaf():
    """The float64 round-to-odd construction against the C library's fmaf, on operands of very different magnitudes (where a
    plain float64 multiply-add rounds twice)."""
    libm = ctypes.CDLL("libm.so.6")
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    rng = np.random.RandomState(0)
    n = 4000
    a, b = rng.rand(n).astype(np.float32), rng.rand(n).astype(np.float32)
    c = (rng.rand(n) * rng.choice([1.0, 2.0 ** -24, 2.0 ** -30, 2.0 ** -40, 2.0 ** 12], n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    # a * b = 1 + 2^-11 + 2^-24 is exactly half way between two float32 values, and c lies far below the float64 grid: the
    # float64 sum drops c, and only its sign says which way the single rounding goes
    a[:4], b[:4] = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12)
    c[:4] = np.float32([2.0 ** -80, -2.0 ** -80, 2.0 ** -100, 0.0])
    assert len(set(ref.bits(ref.fma(a[:2], b[:2], c[:2])).tolist())) == 2
    want = np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], dtype=np.float32)
    _same_bits(ref.fma(a, b, c), want, "fma")


@pytest.mark.parametrize("hw", SOURCES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_equals_torch_at_299(hw):
    """F.interpolate(x, (299, 299), mode="bilinear", align_corners=False) on NCHW and on channels_last inputs, and the
    2 x - 1 epilogue against ``2 * t - 1``: equality, not a tolerance."""
    import torch
    u8 = ref.content(1000 + hw[0] + hw[1], 2, *hw)
    x = ref.unit(u8)
    assert np.array_equal(x, (torch.from_numpy(u8).float() / 255).numpy())                 # ToTensor's division
    y = ref.interpolate(x, (299, 299))
    t = ref.torch_interpolate(x, (299, 299))
    _same_bits(y, t, "NCHW")
    _same_bits(y, ref.torch_interpolate(x, (299, 299), channels_last=True), "channels_last")
    _same_bits(ref.network_input_torch(u8, (299, 299)), (2 * torch.from_numpy(t) - 1).numpy(), "2 x - 1")
    if hw == (299, 299):                                                                   # identity: the byte's own value
        _same_bits(y, x, "identity")


@pytest.mark.parametrize("out_hw", [(5, 7), (1, 1)], ids=lambda s: f"to{s[0]}x{s[1]}")
@pytest.mark.parametrize("hw", SMALL_SOURCES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_small_outputs_equal_torch(hw, out_hw):
    """Outputs 5 x 7 and 1 x 1: torch serves them (oh + ow <= 128) with its channels_last kernel, whatever the memory format of
    the input, and ``interpolate_channels_last_kernel`` is that kernel bit for bit.  The kernel the device implements
    (``interpolate``) differs from it there by at most 2 ulp of 1 (measured: 1.2e-7; 29 to 83 of the 210 values of a 5 x 7
    case): the device kernel is pinned to ``interpolate`` at every size (tests/test_gpu_torch_resize.py), which is torch's
    result at pytorch-fid's 299 x 299 and NOT torch's at these small outputs."""
    import torch
    u8 = ref.content(2000 + hw[0] + hw[1], 2, *hw)
    x = ref.unit(u8)
    y = ref.interpolate_channels_last_kernel(x, out_hw)
    t = ref.torch_interpolate(x, out_hw)
    _same_bits(y, t, "NCHW")
    _same_bits(y, ref.torch_interpolate(x, out_hw, channels_last=True), "channels_last")
    _same_bits((y * np.float32(2) - np.float32(1)).astype(np.float32), (2 * torch.from_numpy(t) - 1).numpy(), "2 x - 1")
    assert np.abs(ref.interpolate(x, out_hw) - t).max() <= 2.0 ** -22


def test_one_thread_takes_the_other_kernel():
    """What is NOT pinned, shown: on one thread torch resizes a 3-channel image to 299 x 299 with its channels_last kernel, and
    that differs from the multi-thread result (the device's) in the last bits of about a third of the values."""
    import torch
    u8 = ref.content(77, 1, 64, 80)
    x = ref.unit(u8)
    torch.set_num_threads(1)
    t1 = ref.torch_interpolate(x, (299, 299))
    torch.set_num_threads(2)
    _same_bits(ref.interpolate_channels_last_kernel(x, (299, 299)), t1, "one thread")
    y = ref.interpolate(x, (299, 299))
    frac = float((ref.bits(y) != ref.bits(t1)).mean())
    assert 0.05 < frac < 0.6 and np.abs(y - t1).max() <= 2.0 ** -22, (frac, np.abs(y - t1).max())


def test_golden_file_is_what_the_restatement_gives():
    """The committed torch outputs (made with the torch build the file names) are the restatement's bits: the comparison above
    also holds on a machine whose torch is another build.  Every 299 x 299 case is the kernel the device implements."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "torch_bilinear_f32.npz"))
    assert os.path.getsize(g.fid.name) < 700 * 1024
    n = int(g["n_cases"])
    assert n >= 16
    fns = {"generic": ref.interpolate, "channels_last": ref.interpolate_channels_last_kernel}
    seen = set()
    for i in range(n):
        seed, k, h, w, oh, ow, kernel = [str(v) for v in g[f"case_{i}"]]
        out_hw = (int(oh), int(ow))
        assert out_hw != (299, 299) or kernel == "generic"
        seen.add((out_hw, kernel))
        y = fns[kernel](ref.unit(ref.content(int(seed), int(k), int(h), int(w))), out_hw)
        if f"out_{i}" in g.files:
            _same_bits(y, g[f"out_{i}"], f"case {i}")
        else:
            _same_bits(y[:, ::int(g["row_step"])], g[f"rows_{i}"], f"case {i} rows")
            assert hashlib.sha256(np.ascontiguousarray(y).tobytes()).hexdigest() == str(g[f"sha_{i}"]), f"case {i}"
    assert ((299, 299), "generic") in seen and ((5, 7), "channels_last") in seen


# ---- mode plumbing -------------------------------------------------------------------------------------------------------
NEW_MODES = ("pytorch-fid", "torch-fidelity")


def test_modes_resolve_and_refuse_another_network(capsys):
    from tise_toolbox_amd import fid_score
    assert fid_score.MODES == ("tise", "clean") + NEW_MODES
    assert fid_score.MODE_RESIZE == {"tise": "reference", "clean": "clean", "pytorch-fid": "torch", "torch-fidelity": "tf1"}
    for mode in NEW_MODES:
        assert fid_score.resolve_mode(mode, None) == "inception-2015"
        assert fid_score.resolve_mode(mode, "inception-2015") == "inception-2015"
        with pytest.raises(ValueError, match=f"--mode {mode} .* inception-2015 only"):
            fid_score.resolve_mode(mode, "torchvision")
        with pytest.raises(SystemExit) as e:                      # refused by the parser, before a device or a file is touched
            fid_score.main(["--path1", "a", "--path2", "b", "--mode", mode, "--network", "torchvision", "--synthetic-weights"])
        assert e.value.code == 2 and "inception-2015 only" in capsys.readouterr().err
        with pytest.raises(SystemExit) as e:
            fid_score.main(["--path1", "a", "--path2", "b", "--mode", mode, "--u8-cache", "--synthetic-weights"])
        assert e.value.code == 2 and "--u8-cache is not available" in capsys.readouterr().err
        assert fid_score.mode_tag(mode) == f" [mode {mode}]"
        a = fid_score._build_parser().parse_args(["--path2", "b", "--mode", mode])
        assert a.mode == mode and a.untagged_stats is None
    assert fid_score.mode_tag("tise") == "" and fid_score.mode_tag("clean") == fid_score.CLEAN_TAG
    assert fid_score.resolve_mode("tise", None) == "torchvision"
    with pytest.raises(ValueError, match="unknown mode"):
        fid_score.resolve_mode("legacy_tensorflow", None)
    with pytest.raises(SystemExit):
        fid_score._build_parser().parse_args(["--path2", "b", "--untagged-stats", "legacy_tensorflow"])


class _Model:                                                      # what _compute_statistics_of_path reads of a model
    network = "inception-2015"

    def __init__(self, mode):
        self.fid_mode = mode


def _load(path, mode):
    from tise_toolbox_amd import fid_score
    return fid_score._compute_statistics_of_path(str(path), _Model(mode), 50, 4, True)


def test_stats_npz_tags_and_cross_mode_refusals(tmp_path):
    """Every mode writes its tag (the default one none) and reads only its own files: 4 x 4 combinations."""
    from tise_toolbox_amd import fid_score
    mu, sigma = np.arange(4.0), np.eye(4)
    modes = fid_score.MODES
    for m in modes:
        fid_score.save_stats_npz(str(tmp_path / f"{m}.npz"), mu, sigma, "inception-2015", mode=m)
        with np.load(tmp_path / f"{m}.npz") as f:
            if m == "tise":
                assert sorted(f.files) == ["mu", "network", "sigma"]                 # the default mode's files stay what they were
            else:
                assert sorted(f.files) == ["mode", "mu", "network", "sigma"] and str(f["mode"]) == m
    for made in modes:
        for run in modes:
            if made == run:
                m, s = _load(tmp_path / f"{made}.npz", run)
                assert np.array_equal(m, mu) and np.array_equal(s, sigma)
            else:
                with pytest.raises(RuntimeError, match=f"statistics of mode '{made}', this run uses --mode {run}"):
                    _load(tmp_path / f"{made}.npz", run)


def test_untagged_stats_flag(tmp_path, capsys):
    """An untagged {mu, sigma} file (what pytorch-fid writes) reads as tise; the refusal under the new modes names the flag;
    with the flag it is taken as that mode's and one stderr line says so; a tagged file is never overridden."""
    from tise_toolbox_amd import fid_score
    mu, sigma = np.arange(4.0), np.eye(4)
    pu, pc = tmp_path / "untagged.npz", tmp_path / "clean.npz"
    np.savez(pu, mu=mu, sigma=sigma)
    fid_score.save_stats_npz(str(pc), mu, sigma, "inception-2015", mode="clean")
    try:
        assert fid_score._UNTAGGED_STATS is None
        assert np.array_equal(_load(pu, "tise")[0], mu)
        for mode in NEW_MODES:
            with pytest.raises(RuntimeError, match=f"statistics of mode 'tise', this run uses --mode {mode}.*--untagged-stats {mode}"):
                _load(pu, mode)
        with pytest.raises(RuntimeError, match="this run uses --mode clean$"):       # no package of that name writes untagged files
            _load(pu, "clean")
        capsys.readouterr()
        fid_score.set_untagged_stats("pytorch-fid")
        m, s = _load(pu, "pytorch-fid")
        assert np.array_equal(m, mu) and np.array_equal(s, sigma)
        err = capsys.readouterr().err
        assert err.count("\n") == 1 and "taken as statistics of mode pytorch-fid (--untagged-stats)" in err and str(pu) in err
        with pytest.raises(RuntimeError, match="statistics of mode 'pytorch-fid', this run uses --mode tise"):
            _load(pu, "tise")                                                         # the flag says what the file is, for every mode
        capsys.readouterr()
        with pytest.raises(RuntimeError, match="statistics of mode 'clean', this run uses --mode pytorch-fid"):
            _load(pc, "pytorch-fid")                                                  # a tag is never overridden
        assert np.array_equal(_load(pc, "clean")[0], mu)
        assert capsys.readouterr().err == ""                                          # ... and a tagged file is not announced
        with pytest.raises(ValueError, match="unknown mode"):
            fid_score.set_untagged_stats("legacy_tensorflow")
    finally:
        fid_score.set_untagged_stats(None)
    # the parser takes the flag and main() applies it before anything else
    a = fid_score._build_parser().parse_args(["--path2", "b", "--mode", "pytorch-fid", "--untagged-stats", "pytorch-fid"])
    assert a.untagged_stats == "pytorch-fid"


def test_engine_resizes_keep_their_values():
    import inspect
    from tise_toolbox_amd import engine
    assert engine.RESIZES == ("reference", "clean") and engine.SUITE_RESIZES == ("tf1",)
    assert engine.TORCH_RESIZES == ("torch",)
    assert inspect.signature(engine.RealismEngine.__init__).parameters["resize"].default == "reference"
