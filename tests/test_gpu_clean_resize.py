"""GPU: clean-fid's float32 bicubic resize (csrc/resize_f32.hip) and fid_score --mode clean on the MI355X.

Kernel: tise_resize_f32 and tise_resize_ragged_f32 against the numpy restatement of Pillow's algorithm (tests/_clean_resize_ref.py,
itself pinned to Pillow by tests/test_clean_resize_host.py) and against Pillow's own recorded outputs
(tests/golden/pil_resize_f32.npz), bit for bit, at the smallest shapes that reach each branch.  Engine: the float route feeds the
trunk the restatement's bits.  End to end: the CLI against the CPU route on the same files."""
import ctypes
import functools
import hashlib
import os

import numpy as np
import pytest
import torch

from tests import _cases
from tests import _clean_resize_ref as ref

pytestmark = pytest.mark.gpu

NET = "inception-2015"
INF = float("inf")
STD = dict(clip=(0.0, 255.0), sub=128.0, div=128.0)           # clean-fid's clip and input map
RAW = dict(clip=(-INF, INF), sub=0.0, div=1.0)                # the identity: the resampled value itself


@functools.lru_cache(maxsize=None)
def _want(kind, seed, h, w, oh, ow, filt, order):
    """The restatement's unclipped (oh, ow, 3) float32 result, computed once per case and shared (read-only)."""
    y = ref.resize_f32(ref.content(kind, seed, h, w), (oh, ow), filt, order)
    y.setflags(write=False)
    return y


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _run(dev, x, out_hw, filt="bicubic", nhwc=True, order=0, clip=(0.0, 255.0), sub=128.0, div=128.0):
    """tise_resize_f32 on a (n, h, w, 3) uint8 array -> (n, oh, ow, 3) float32 array, whichever layout the kernel wrote."""
    from tise_toolbox_amd import _lib
    n, h, w, _ = x.shape
    oh, ow = out_hw
    src = torch.as_tensor(x, device=dev)
    dst = torch.full((n, oh, ow, 3) if nhwc else (n, 3, oh, ow), float("nan"), dtype=torch.float32, device=dev)
    _lib.call("tise_resize_f32", ctypes.c_void_p(src.data_ptr()), n, h, w, ctypes.c_void_p(dst.data_ptr()), oh, ow, 1 if nhwc else 0,
              {"bilinear": 0, "bicubic": 1}[filt], clip[0], clip[1], sub, div, order, _stream())
    out = dst if nhwc else dst.permute(0, 2, 3, 1)
    return out.cpu().numpy()


def _same_bits(got, want, what=""):
    g, w = ref.bits(got), ref.bits(want)
    assert g.shape == w.shape, (g.shape, w.shape)
    bad = np.argwhere(g != w)
    assert len(bad) == 0, f"{what}: {len(bad)} of {g.size} values differ in their bits, first at {tuple(bad[0])}: " \
                          f"{np.asarray(got)[tuple(bad[0])]!r} != {np.asarray(want)[tuple(bad[0])]!r}"


# (h, w, oh, ow): the smallest shapes that reach each branch of the kernel
SHAPES = [
    (37, 53, 41, 37),        # up on both axes (<= 5 taps: coefficients in registers); h*w*3 odd: images 2 and 3 of a batch start misaligned
    (64, 2000, 37, 100),     # down with 81 taps per horizontal window; LDS allows a row tile of 4 only
    (2000, 64, 37, 100),     # 219 vertical taps: no float32 row tile fits LDS, one streamed output row per workgroup
    (37, 53, 41, 53),        # identity on x: the horizontal pass is skipped
    (37, 53, 37, 41),        # identity on y
    (37, 53, 37, 53),        # identity on both: the clipped input
    (9, 1, 11, 13), (9, 5, 11, 13), (9, 6, 11, 13), (9, 17, 11, 13),      # w*3 = 3, 15, 18, 51 straddles the 16-byte load
    (8, 16, 11, 13),         # w*3 = 48: the 16-byte loads themselves (image 0; 384 bytes per image keep the others aligned too)
    (20, 24, 17, 19), (20, 24, 15, 19), (40, 24, 33, 7), (40, 24, 31, 7),  # oh one more / one less than a multiple of the row tile (16)
    (1, 1, 1, 1), (1, 1, 37, 41), (2, 3, 5, 4),
    (256, 256, 299, 299),    # the flagship shape (16-byte loads, 19 row tiles)
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_batch_kernel_equals_restatement(cuda_device, shape):
    """n = 3 (random, 0/255-only, random content), both output layouts, clean-fid's clip and affine; n = 1 and the identity
    affine on the first image."""
    h, w, oh, ow = shape
    cases = [("rand", 100), ("bw", 101), ("rand", 102)]
    x = np.stack([ref.content(k, s, h, w) for k, s in cases])
    raw = np.stack([_want(k, s, h, w, oh, ow, "bicubic", 0) for k, s in cases])
    want = ref.affine(raw, **STD)
    for nhwc in (True, False):
        _same_bits(_run(cuda_device, x, (oh, ow), nhwc=nhwc), want, f"n=3 nhwc={nhwc}")
    _same_bits(_run(cuda_device, x[:1], (oh, ow), **RAW), raw[:1], "n=1, identity affine")
    if (h, w) == (oh, ow):
        assert np.array_equal(_run(cuda_device, x, (oh, ow), **RAW), x.astype(np.float32))


@pytest.mark.parametrize("shape", [(37, 53, 41, 37), (64, 2000, 37, 100), (2000, 64, 37, 100), (9, 5, 11, 13), (40, 24, 33, 7)],
                         ids=lambda s: "%dx%d-%dx%d" % s)
def test_batch_kernel_bilinear(cuda_device, shape):
    h, w, oh, ow = shape
    cases = [("rand", 110), ("bw", 111), ("rand", 112)]
    x = np.stack([ref.content(k, s, h, w) for k, s in cases])
    want = ref.affine(np.stack([_want(k, s, h, w, oh, ow, "bilinear", 0) for k, s in cases]), **STD)
    for nhwc in (True, False):
        _same_bits(_run(cuda_device, x, (oh, ow), "bilinear", nhwc=nhwc), want, f"nhwc={nhwc}")


def test_clip_and_affine(cuda_device):
    """0/255 content overshoots to about -70 and 326: both clips act; other bounds and another affine follow the same two
    fp32 operations."""
    h, w, oh, ow = 37, 53, 41, 37
    x = ref.content("bw", 101, h, w)[None]
    raw = _want("bw", 101, h, w, oh, ow, "bicubic", 0)[None]
    assert raw.min() < -40 and raw.max() > 295
    got = _run(cuda_device, x, (oh, ow))
    assert got.min() == -1.0 and got.max() == np.float32(127.0 / 128.0)
    _same_bits(got, ref.affine(raw, **STD))
    for clip, sub, div in (((0.0, 255.0), 0.0, 1.0), ((10.5, 200.25), 3.0, 7.0), ((-INF, INF), 127.5, 127.5), ((0.0, 255.0), 0.0, 255.0)):
        _same_bits(_run(cuda_device, x, (oh, ow), clip=clip, sub=sub, div=div), ref.affine(raw, clip, sub, div), f"{clip} {sub} {div}")


@pytest.mark.parametrize("shape", [(64, 20, 17, 31), (9, 7, 20, 18), (300, 2, 37, 41), (37, 53, 37, 41), (37, 53, 41, 53)],
                         ids=lambda s: "%dx%d-%dx%d" % s)
def test_vertical_first_order(cuda_device, shape):
    """order = 1 at any shape is the restatement's vertical-first result (down, up, a skipped pass on either axis)."""
    h, w, oh, ow = shape
    cases = [("rand", 120), ("bw", 121), ("rand", 122)]
    x = np.stack([ref.content(k, s, h, w) for k, s in cases])
    want = ref.affine(np.stack([_want(k, s, h, w, oh, ow, "bicubic", 1) for k, s in cases]), **STD)
    for nhwc in (True, False):
        _same_bits(_run(cuda_device, x, (oh, ow), nhwc=nhwc, order=1), want, f"nhwc={nhwc}")


# ---- Pillow's recorded outputs -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "pil_resize_f32.npz"))
    out = []
    for i in range(int(g["n_cases"])):
        kind, seed, h, w, oh, ow, filt = [str(v) for v in g[f"case_{i}"]]
        out.append(dict(kind=kind, seed=int(seed), h=int(h), w=int(w), oh=int(oh), ow=int(ow), filt=filt,
                        out=g[f"out_{i}"] if f"out_{i}" in g.files else None,
                        sha=str(g[f"sha_{i}"]) if f"sha_{i}" in g.files else None,
                        rows=g[f"rows_{i}"] if f"rows_{i}" in g.files else None, step=int(g["row_step"])))
    return out


def _check_golden(got, c, what):
    if c["out"] is not None:
        _same_bits(got, c["out"], what)
    else:
        _same_bits(got[::c["step"]], c["rows"], what + " (every %d-th row)" % c["step"])
        assert hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest() == c["sha"], what + ": SHA-256 of the whole output"


def test_device_resize_f32_equals_pillow_golden(cuda_device, golden):
    """device.resize_f32 (which applies Pillow's tall-image rule itself) == Pillow's recorded bits on every case of the golden
    file: up, down, 0/255 content, bilinear, (1, 1), a skipped pass, (256, 256) -> (299, 299) and the tall (1000, 9) sources."""
    from tise_toolbox_amd import device
    assert any(c["h"] > 100 * c["w"] for c in golden) and any((c["h"], c["w"], c["oh"]) == (256, 256, 299) for c in golden)
    for c in golden:
        x = torch.as_tensor(ref.content(c["kind"], c["seed"], c["h"], c["w"])[None], device=cuda_device)
        for cl in (True, False):
            y = device.resize_f32(x, (c["oh"], c["ow"]), c["filt"], channels_last=cl, **RAW)
            assert tuple(y.shape) == (1, 3, c["oh"], c["ow"]) and y.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
            _check_golden(y.permute(0, 2, 3, 1).cpu().numpy()[0], c, "%(kind)s %(h)dx%(w)d -> %(oh)dx%(ow)d %(filt)s" % c)


def test_order_argument_on_the_tall_golden_case(cuda_device, golden):
    """(1000, 9) -> (299, 299) through the C entry point: order = 1 is Pillow's recorded output, order = 0 is not (about a quarter
    of the values differ by one ulp), so the rule cannot be dropped unnoticed."""
    c = next(c for c in golden if (c["h"], c["w"], c["oh"], c["ow"]) == (1000, 9, 299, 299))
    x = ref.content(c["kind"], c["seed"], c["h"], c["w"])[None]
    _check_golden(_run(cuda_device, x, (299, 299), order=1, **RAW)[0], c, "order=1")
    h0 = _run(cuda_device, x, (299, 299), order=0, **RAW)[0]
    _same_bits(h0, _want(c["kind"], c["seed"], 1000, 9, 299, 299, "bicubic", 0), "order=0")
    assert (ref.bits(h0[::c["step"]]) != ref.bits(c["rows"])).mean() > 0.05


# ---- ragged ----------------------------------------------------------------------------------------------------------------
RAGGED = [(37, 53), (64, 2000), (2000, 64), (4000, 9), (37, 71), (9, 100), (37, 100), (1, 1), (9, 5)]   # -> (37, 100): up, many taps,
#   streamed, TALL (vertical first), identity on y, identity on x, identity on both, one pixel, w*3 = 15


@pytest.mark.parametrize("count", [1, 9])
@pytest.mark.parametrize("misaligned", [False, True])
def test_ragged_equals_the_batch_entry_point(cuda_device, count, misaligned):
    from tise_toolbox_amd import device
    oh, ow = 37, 100
    shapes = RAGGED[3:4] if count == 1 else RAGGED
    assert any(device.pillow_vertical_first(h, w, oh) for h, w in shapes)
    imgs = [ref.content("bw" if i % 3 == 1 else "rand", 200 + i, h, w) for i, (h, w) in enumerate(shapes)]
    if misaligned:           # views at odd offsets of one buffer, as crops of a feed's output buffer are
        flat = torch.empty(sum(im.size + 1 for im in imgs), dtype=torch.uint8, device=cuda_device)
        crops, pos = [], 1
        for im in imgs:
            v = flat[pos:pos + im.size].view(im.shape)
            v.copy_(torch.as_tensor(im))
            crops.append(v)
            pos += im.size + 1
        assert any(c.data_ptr() % 16 for c in crops)
    else:
        crops = [torch.as_tensor(im, device=cuda_device) for im in imgs]
    for cl in (True, False):
        got = device.resize_ragged_f32(crops, (oh, ow), channels_last=cl)
        assert tuple(got.shape) == (len(imgs), 3, oh, ow)
        for i, c in enumerate(crops):
            one = device.resize_f32(c.contiguous().unsqueeze(0), (oh, ow), channels_last=cl)
            assert torch.equal(got[i].view(torch.int32), one[0].view(torch.int32)), (i, shapes[i], cl)
        want = np.stack([ref.clean_input(im, (oh, ow)) for im in imgs])           # order: Pillow's rule
        _same_bits(got.permute(0, 2, 3, 1).cpu().numpy(), want, f"channels_last={cl}")


def test_ragged_refuses_before_enqueueing(cuda_device):
    from tise_toolbox_amd import _lib, device
    good = torch.zeros((8, 8, 3), dtype=torch.uint8, device=cuda_device)
    wide = torch.zeros((2, 1 << 17, 3), dtype=torch.uint8, device=cuda_device)      # one source row is 384 KB: no row tile fits LDS
    with pytest.raises(_lib.TiseStatusError, match="image 1 of the batch"):
        device.resize_ragged_f32([good, wide], (4, 4))
    with pytest.raises(_lib.TiseStatusError):
        device.resize_f32(wide.unsqueeze(0), (4, 4))
    with pytest.raises(ValueError):
        device.resize_ragged_f32([], (4, 4))


# ---- engine ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clean_engine(cuda_device):
    from tise_toolbox_amd.engine import RealismEngine
    torch.backends.cudnn.benchmark = False
    return RealismEngine(dims=2048, seed=0, network=NET, resize="clean")


def test_engine_clean_route_feeds_the_trunk_the_restatement(cuda_device, clean_engine):
    """features_from_u8 == the same trunk on the input the restatement builds on the host, to the last bit (the same launches
    on the same input bits); features_from_u8_list on equal-sized images == features_from_u8."""
    imgs = np.stack([ref.content("rand", 300 + i, 64, 80) for i in range(8)])
    x = torch.from_numpy(np.stack([ref.clean_input(im, (299, 299)) for im in imgs])).to(cuda_device).permute(0, 3, 1, 2)
    want, _ = clean_engine._trunk(x, prenormalized=True)
    want = want.clone()
    u8 = torch.as_tensor(imgs, device=cuda_device)
    got, _ = clean_engine.features_from_u8(u8)
    assert got.shape == (8, 2048) and torch.isfinite(got).all()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    lst, _ = clean_engine.features_from_u8_list([u8[i] for i in range(8)])
    assert torch.equal(lst.view(torch.int32), want.view(torch.int32))
    # the float route is not the uint8 route
    from tise_toolbox_amd.engine import RealismEngine
    ref_eng = RealismEngine(dims=2048, seed=0, network=NET, resize="reference")
    base, _ = ref_eng.features_from_u8(u8)
    assert (base - got).abs().max().item() > 1e-4 * base.abs().max().item()
    # ... and resize="reference" is the engine built without the argument, bit for bit
    plain, _ = RealismEngine(dims=2048, seed=0, network=NET).features_from_u8(u8)
    assert torch.equal(plain.view(torch.int32), base.view(torch.int32))
    assert clean_engine.resize == "clean" and ref_eng.resize == "reference"


def test_engine_refuses_clean_on_another_network(cuda_device):
    from tise_toolbox_amd.engine import RealismEngine
    with pytest.raises(ValueError, match="inception-2015"):
        RealismEngine(dims=2048, seed=0, resize="clean")
    with pytest.raises(ValueError, match="unknown resize"):
        RealismEngine(dims=2048, seed=0, network=NET, resize="bicubic")


# ---- end to end ------------------------------------------------------------------------------------------------------------
def _write(d, imgs):
    from PIL import Image
    d.mkdir(parents=True)
    for i, im in enumerate(imgs):
        Image.fromarray(im).save(d / f"{i:05d}.png")


def test_fid_cli_mode_clean_vs_cpu_route(cuda_device, tmp_path, monkeypatch, capsys):
    """fid_score --mode clean on two directories of 60 seeded 48 x 64 PNGs at batch 50 (drop-last would lose 10 images) against
    the CPU route on the same files: Pillow's float resize per channel, clip, (x - 128) / 128, the project's fp32
    InceptionV3(network="inception-2015") on the CPU with the same stand-in weights, np.cov over all 60 rows, the oracle's
    Frechet function.  |dFID| <= 1e-3 absolute (the project's standing budget).  On these images the CPU routes alone give
    30.85 for the clean route against 35.50 for the reference's route (uint8 bilinear resize, the first 50 images; 34.18 on all
    60, so the resize alone moves it too): the modes are told apart."""
    from PIL import Image
    from oracle import fid_oracle
    from tise_toolbox_amd import fid_score, img_data
    from tise_toolbox_amd.inception import InceptionV3
    from tise_toolbox_amd.weights import SYNTHETIC_TAG
    monkeypatch.setenv("TISE_CONV", "split")
    gdir, rdir = tmp_path / "gen", tmp_path / "ref"
    _write(gdir, _cases.smooth_images(60, 48, 64, seed=31))
    _write(rdir, _cases.smooth_images(60, 48, 64, seed=32, shift=0.15))
    stats, out = tmp_path / "gen_clean.npz", tmp_path / "fid.txt"
    argv = ["--batch-size", "50", "--path1", str(rdir), "--path2", str(gdir), "--num-workers", "0", "--synthetic-weights"]
    v = fid_score.main(argv + ["--mode", "clean", "--save-stats", str(stats), "--kid", "--saved_file", str(out)])
    assert out.read_text() == f"FID: {v}{fid_score.CLEAN_TAG}{SYNTHETIC_TAG}"           # result lines name the mode
    assert "KID: " in capsys.readouterr().out

    torch.set_num_threads(min(16, torch.get_num_threads()))
    model = InceptionV3([3], seed=0, network=NET).eval()

    def cpu_stats(root):
        files = img_data.get_filenames(str(root))
        assert len(files) == 60
        x = np.stack([ref.affine(ref.pil_resize_f32(np.asarray(Image.open(f).convert("RGB")), (299, 299))) for f in files])
        x = torch.from_numpy(x).permute(0, 3, 1, 2)
        with torch.no_grad():
            f = torch.cat([model(x[i:i + 20], prenormalized=True)[0].flatten(1) for i in range(0, 60, 20)]).numpy().astype(np.float64)
        return f.mean(axis=0), np.cov(f, rowvar=False), f
    mr, sr, _ = cpu_stats(rdir)
    mg, sg, fg = cpu_stats(gdir)
    want = fid_oracle.calculate_frechet_distance(mr, sr, mg, sg)
    print("FID --mode clean device", v, "cpu route", want, "difference", abs(v - want))
    assert abs(v - want) <= 1e-3
    with np.load(stats) as f:
        assert str(f["mode"]) == "clean" and str(f["network"]) == NET
        assert f["features"].shape == (60, 2048)                                       # every image: n is 60, not 50
        assert np.abs(f["mu"] - mg).max() <= 1e-4 * np.abs(mg).max()
    # the mode is visible: the reference's route on the same files (uint8 bilinear resize, the last 10 files dropped) is another number
    t = fid_score.main(argv + ["--network", NET])
    print("FID --mode tise --network inception-2015", t)
    assert abs(t - v) > 1e-3
    # the tagged statistics serve --mode clean and are refused by --mode tise; an explicit other network is refused
    v2 = fid_score.main(["--batch-size", "50", "--path1", str(stats), "--path2", str(rdir), "--num-workers", "0", "--synthetic-weights",
                         "--mode", "clean"])
    assert abs(v2 - v) <= 1e-6 * max(1.0, abs(v))
    with pytest.raises(RuntimeError, match="statistics of mode 'clean'"):
        fid_score.main(["--batch-size", "50", "--path1", str(stats), "--path2", str(rdir), "--num-workers", "0", "--synthetic-weights",
                        "--network", NET])
    with pytest.raises(SystemExit):
        fid_score.main(argv + ["--mode", "clean", "--network", "torchvision"])

