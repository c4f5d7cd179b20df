"""GPU: pytorch-fid's float32 bilinear resize (csrc/resize_torch.hip) and fid_score --mode pytorch-fid / torch-fidelity on the MI355X.

Kernel: tise_resize_torch_f32 and tise_resize_ragged_torch_f32 against the numpy restatement of torch's CPU kernel
(tests/_torch_resize_ref.py, itself pinned to torch by tests/test_torch_resize_host.py), bit for bit, at the smallest shapes that
reach each branch.  Engine: the route feeds the trunk the restatement's bits.  End to end: the CLIs against a CPU route on the same
files whose resize is torch's own F.interpolate (pytorch-fid) or the TF1 restatement (torch-fidelity)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from tests import _cases
from tests import _tf1_resize_ref as tf1
from tests import _torch_resize_ref as ref

pytestmark = pytest.mark.gpu

NET = "inception-2015"
NAN = float("nan")
CAP_PIXELS = 4096 * 1024             # output pixels of one pass of the capped grid (csrc/resize_torch.hip: kMaxBlocks workgroups, a tile of 1024 pixels each)


@functools.lru_cache(maxsize=None)
def _want(seed, n, h, w, oh, ow):
    """The restatement's (n, oh, ow, 3) network input (2 x - 1), computed once per case and shared (read-only)."""
    y = ref.network_input_torch(ref.content(seed, n, h, w), (oh, ow))
    y.setflags(write=False)
    return y


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _call(src, n, h, w, dst, oh, ow, mul=2.0, sub=1.0):
    from tise_toolbox_amd import _lib
    _lib.call("tise_resize_torch_f32", ctypes.c_void_p(src.data_ptr()), n, h, w, ctypes.c_void_p(dst.data_ptr()), oh, ow, mul, sub, _stream())


def _run(dev, x, out_hw, mul=2.0, sub=1.0):
    """tise_resize_torch_f32 on a (n, h, w, 3) uint8 array -> (n, oh, ow, 3) float32 array; the output starts as NaN."""
    n, h, w, _ = x.shape
    src = torch.as_tensor(x, device=dev)
    dst = torch.full((n,) + tuple(out_hw) + (3,), NAN, dtype=torch.float32, device=dev)
    _call(src, n, h, w, dst, out_hw[0], out_hw[1], mul, sub)
    return dst.cpu().numpy()


def _same_bits(got, want, what=""):
    g, w = ref.bits(got), ref.bits(want)
    assert g.shape == w.shape, (g.shape, w.shape)
    bad = np.argwhere(g != w)
    assert len(bad) == 0, f"{what}: {len(bad)} of {g.size} values differ in their bits, first at {tuple(bad[0])}: " \
                          f"{np.asarray(got)[tuple(bad[0])]!r} != {np.asarray(want)[tuple(bad[0])]!r}"


# 1 x 1 and 2 x 5 (every tap clamped), a 3-pixel-wide column, up, the identity, a scale just above 1, the flagship shape, down and non-square
SOURCES = [(1, 1), (2, 5), (700, 3), (64, 64), (299, 299), (300, 299), (256, 256), (640, 427)]
OUTPUTS = [(299, 299), (5, 7), (1, 1)]


@pytest.mark.parametrize("out_hw", OUTPUTS, ids=lambda s: f"to{s[0]}x{s[1]}")
@pytest.mark.parametrize("hw", SOURCES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_equals_restatement(cuda_device, hw, out_hw):
    """Two images per case (h * w * 3 is odd for several: the second image then starts at an odd address); 2 * 299 * 299 pixels
    are 174 whole tiles of 1024 (16-byte stores out of LDS; tiles cross rows and the image border) and one of 626 pixels (each
    thread stores its own); the small outputs are one short tile."""
    seed = 500 + hw[0] + hw[1]
    x = ref.content(seed, 2, *hw)
    want = _want(seed, 2, hw[0], hw[1], *out_hw)
    _same_bits(_run(cuda_device, x, out_hw), want, f"{hw} -> {out_hw}")
    if hw == out_hw:                                              # the identity: 2 * (b / 255) - 1 of the byte itself, exactly
        b = x.astype(np.float32) / np.float32(255.0)
        _same_bits(want, b * np.float32(2.0) - np.float32(1.0), "identity")


def test_affine_is_a_separate_multiply_and_subtract(cuda_device):
    """mul and sub other than 2 and 1 (where fusing would change bits): v * mul - sub as two float32 operations; mul = 1,
    sub = 0 hands out the interpolated value itself."""
    x = ref.content(7, 2, 37, 53)
    for mul, sub in ((1.0, 0.0), (255.0, 128.0), (0.7, 0.3)):
        _same_bits(_run(cuda_device, x, (41, 37), mul, sub), ref.network_input_torch(x, (41, 37), mul, sub), f"mul {mul} sub {sub}")


@pytest.mark.parametrize("hw,out_hw", [((64, 64), (299, 299)), ((37, 53), (5, 7))], ids=["to299", "to5x7"])
def test_device_front_end_both_layouts(cuda_device, hw, out_hw):
    from tise_toolbox_amd import device
    seed = 500 + hw[0] + hw[1]
    u8 = torch.as_tensor(ref.content(seed, 2, *hw), device=cuda_device)
    want = _want(seed, 2, hw[0], hw[1], *out_hw)
    cl = device.resize_torch_f32(u8, out_hw, channels_last=True)
    assert cl.shape == (2, 3) + out_hw and cl.permute(0, 2, 3, 1).is_contiguous()
    nchw = device.resize_torch_f32(u8, out_hw, channels_last=False)
    assert nchw.shape == (2, 3) + out_hw and nchw.is_contiguous()
    _same_bits(cl.permute(0, 2, 3, 1).cpu().numpy(), want, "channels_last")
    _same_bits(nchw.permute(0, 2, 3, 1).cpu().numpy(), want, "NCHW")
    assert device.resize_torch_f32(u8[:0], out_hw).shape == (0, 3) + out_hw
    with pytest.raises(ValueError, match=r"\(N,H,W,3\) uint8"):
        device.resize_torch_f32(u8.float(), out_hw)
    with pytest.raises(ValueError, match=r"\(N,H,W,3\) uint8"):
        device.resize_torch_f32(u8[..., :2], out_hw)
    with pytest.raises(ValueError, match="must be positive"):
        device.resize_torch_f32(u8, (0, 7))


def test_odd_source_address_unaligned_destination_and_padding(cuda_device):
    """The source is a slice that starts at an odd byte address, with sentinel bytes in front of and behind it: two runs whose
    sentinels differ (0 and 255) give the same bits, the restatement's -- nothing outside the images is read into the result.
    The destination lies between sentinel floats that both runs leave alone; once 16-byte aligned (the 16-byte stores) and
    once 4 bytes past that (dword stores for whole tiles too): the same bits."""
    n, h, w, oh, ow = 3, 9, 7, 37, 41                             # 3 * 37 * 41 = 4551 pixels: four whole tiles and one of 455 pixels
    x = ref.content(11, n, h, w)
    want = ref.network_input_torch(x, (oh, ow))
    count = n * oh * ow * 3
    for pad_byte in (0, 255):
        for shift in (0, 1):
            buf = torch.full((64 + x.size + 64,), pad_byte, dtype=torch.uint8, device=cuda_device)
            src = buf[33:33 + x.size]
            assert src.data_ptr() % 2 == 1
            src.copy_(torch.as_tensor(x.reshape(-1), device=cuda_device))
            out = torch.full((64 + count + 64,), -7.0, dtype=torch.float32, device=cuda_device)
            dst = out[16 + shift:16 + shift + count]
            assert dst.data_ptr() % 16 == 4 * shift
            _call(src, n, h, w, dst, oh, ow)
            _same_bits(dst.cpu().numpy().reshape(n, oh, ow, 3), want, f"pad {pad_byte} shift {shift}")
            assert (out[:16 + shift] == -7.0).all() and (out[16 + shift + count:] == -7.0).all()
            assert (buf[:33] == pad_byte).all() and (buf[33 + x.size:] == pad_byte).all()


def test_every_byte_at_every_tap_position(cuda_device):
    """A 2 x 128 ramp, channel c holding (pixel index + 85 c) mod 256, resized to 5 x 300: all 256 byte values stand at each of
    the four tap positions (upper / lower, left / right) at least once over the three channels -- the whole byte -> float
    table is read through every operand of the three fused multiply-adds."""
    idx = np.arange(256).reshape(2, 128)
    x = np.stack([(idx + 85 * c) % 256 for c in range(3)], axis=-1).astype(np.uint8)[None]
    oh, ow = 5, 300
    y0, y1, _, _ = ref.axis_taps(2, oh)
    x0, x1, _, _ = ref.axis_taps(128, ow)
    for ys, xs in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)):
        assert len(np.unique(x[0][ys][:, xs])) == 256
    _same_bits(_run(cuda_device, x, (oh, ow)), ref.network_input_torch(x, (oh, ow)), "ramp")


def test_grid_stride_loop_takes_a_second_trip(cuda_device):
    """60 images of 8 x 8 to 299 x 299 are 5.36 M output pixels, more than one pass of the capped grid (4.19 M): the loop's
    second trip starts inside image 46.  Every image equals its own one-image launch, and the images at the start, at both
    sides of the trip border and at the end equal the restatement."""
    n = 60
    assert n * 299 * 299 > CAP_PIXELS > 46 * 299 * 299
    x = ref.content(21, n, 8, 8)
    src = torch.as_tensor(x, device=cuda_device)
    dst = torch.full((n, 299, 299, 3), NAN, dtype=torch.float32, device=cuda_device)
    _call(src, n, 8, 8, dst, 299, 299)
    one = torch.full((n, 299, 299, 3), NAN, dtype=torch.float32, device=cuda_device)
    for i in range(n):
        _call(src[i], 1, 8, 8, one[i], 299, 299)
    assert torch.equal(dst.view(torch.int32), one.view(torch.int32))
    pick = [0, 45, 46, 47, 59]
    _same_bits(dst[pick].cpu().numpy(), ref.network_input_torch(x[pick], (299, 299)), "images around the trip border")


def test_float_index_past_2_to_31(cuda_device):
    """8007 images of 1 x 1 to 299 x 299 are 2 147 573 421 floats (8.6 GB): the float index of the last images exceeds 2^31.
    All four taps of an output value are the image's one pixel, so a channel's 299 x 299 plane depends on its byte alone: the
    256 planes come from one small launch over 256 grey images (held to the restatement at bytes 0, 1, 127 and 255) and every
    plane of the large launch must be the plane of its byte, compared on the device."""
    n = 8007
    assert n * 299 * 299 * 3 > 2 ** 31
    free, _ = torch.cuda.mem_get_info(cuda_device)
    assert free > 24 * 2 ** 30, "this test needs 24 GB of free device memory"
    grey = np.arange(256, dtype=np.uint8).reshape(256, 1, 1, 1).repeat(3, axis=3)
    planes = torch.full((256, 299, 299, 3), NAN, dtype=torch.float32, device=cuda_device)
    _call(torch.as_tensor(grey, device=cuda_device), 256, 1, 1, planes, 299, 299)
    pick = [0, 1, 127, 255]
    _same_bits(planes[pick].cpu().numpy(), ref.network_input_torch(grey[pick], (299, 299)), "planes of bytes 0, 1, 127, 255")
    table_dev = planes[..., 0].contiguous()                                                                              # (256, 299, 299)
    x = ref.content(23, n, 1, 1)
    src = torch.as_tensor(x, device=cuda_device)
    dst = torch.full((n, 299, 299, 3), NAN, dtype=torch.float32, device=cuda_device)
    _call(src, n, 1, 1, dst, 299, 299)
    for lo in range(0, n, 1000):                                   # compared on the device, 1000 images at a time
        hi = min(n, lo + 1000)
        want = table_dev[src[lo:hi, 0, 0].long()].permute(0, 2, 3, 1)                                                   # (k, 299, 299, 3)
        assert torch.equal(dst[lo:hi].view(torch.int32), want.contiguous().view(torch.int32)), f"images {lo} .. {hi}"


# ---- ragged launch ---------------------------------------------------------------------------------------------------------
def test_ragged_list_equals_the_per_image_results(cuda_device):
    from tise_toolbox_amd import device
    imgs, want = [], []
    for h, w in SOURCES:
        seed = 500 + h + w
        imgs.append(ref.content(seed, 2, h, w)[1])
        want.append(_want(seed, 2, h, w, 299, 299)[1])
    crops = [torch.as_tensor(im, device=cuda_device) for im in imgs]
    got = device.resize_ragged_torch_f32(crops, (299, 299))
    assert got.shape == (len(crops), 3, 299, 299) and got.permute(0, 2, 3, 1).is_contiguous()
    _same_bits(got.permute(0, 2, 3, 1).cpu().numpy(), np.stack(want), "ragged list")
    nchw = device.resize_ragged_torch_f32(crops, (299, 299), channels_last=False)
    assert nchw.is_contiguous()
    _same_bits(nchw.permute(0, 2, 3, 1).cpu().numpy(), np.stack(want), "ragged list, NCHW")
    # ... and the plain entry point's own bits, image by image (the same kernel body)
    for i, c in enumerate(crops):
        assert torch.equal(device.resize_torch_f32(c[None], (299, 299)).view(torch.int32), got[i:i + 1].view(torch.int32))
    # a list of one image; (1,H,W,3) items are taken as images
    single = device.resize_ragged_torch_f32([crops[3][None]], (299, 299))
    _same_bits(single.permute(0, 2, 3, 1).cpu().numpy(), want[3][None], "list of one")


def test_ragged_refusals_come_before_anything_is_enqueued(cuda_device):
    from tise_toolbox_amd import device
    good = torch.zeros((4, 5, 3), dtype=torch.uint8, device=cuda_device)
    with pytest.raises(ValueError, match="empty batch"):
        device.resize_ragged_torch_f32([], (5, 7))
    for bad in (good.float(), good[..., :2], good[None].expand(2, 4, 5, 3), good[:0]):
        with pytest.raises(ValueError, match=r"crop 1 must be \(H,W,3\) uint8"):
            device.resize_ragged_torch_f32([good, bad], (5, 7))
    with pytest.raises(ValueError, match="must be positive"):
        device.resize_ragged_torch_f32([good], (5, 0))


def test_ragged_list_across_the_grid_cap_and_skipped_entries(cuda_device):
    """120 000 tiny images of six sizes to 5 x 7 are 4.2 M output pixels, one more pass than the capped grid covers (50 MB of
    output): the table is read per pixel, a tile of 1024 pixels covers 29 images.  The table is handed to the C
    entry point directly; three entries are marked unusable (a null pointer, h = 0, w = -1) and must leave their output as it
    was (NaN) without disturbing their neighbours."""
    from tise_toolbox_amd import _lib, device
    sizes = [(1, 1), (2, 3), (3, 2), (4, 4), (1, 5), (5, 1)]
    n, oh, ow = 120_000, 5, 7
    assert n * oh * ow > CAP_PIXELS
    rng = np.random.RandomState(5)
    pool = rng.randint(0, 256, size=4096 + 48, dtype=np.uint8)
    kind = rng.randint(0, len(sizes), size=n)
    off = rng.randint(0, 4096, size=n)
    pool_dev = torch.as_tensor(pool, device=cuda_device)
    table = np.empty(n, dtype=device._TORCH_IMAGE)
    table["src"] = np.uint64(pool_dev.data_ptr()) + off.astype(np.uint64)
    table["h"] = np.asarray([s[0] for s in sizes], dtype=np.int32)[kind]
    table["w"] = np.asarray([s[1] for s in sizes], dtype=np.int32)[kind]
    skipped = [7, 60_001, n - 1]
    table["src"][skipped[0]] = 0
    table["h"][skipped[1]] = 0
    table["w"][skipped[2]] = -1
    want = np.empty((n, oh, ow, 3), dtype=np.float32)
    for k, (h, w) in enumerate(sizes):
        sel = np.nonzero(kind == k)[0]
        batch = pool[off[sel][:, None] + np.arange(h * w * 3)[None, :]].reshape(len(sel), h, w, 3)
        want[sel] = ref.network_input_torch(batch, (oh, ow))
    want[skipped] = np.nan
    table_dev = torch.as_tensor(table.view(np.uint8), device=cuda_device)
    dst = torch.full((n, oh, ow, 3), NAN, dtype=torch.float32, device=cuda_device)
    _lib.call("tise_resize_ragged_torch_f32", ctypes.c_void_p(table_dev.data_ptr()), n, ctypes.c_void_p(dst.data_ptr()), oh, ow, 2.0, 1.0,
              _stream())
    got = dst.cpu().numpy()
    assert np.isnan(got[skipped]).all()
    _same_bits(got, want, "ragged list across the grid cap")


# ---- engine ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def torch_engine(cuda_device):
    from tise_toolbox_amd.engine import RealismEngine
    torch.backends.cudnn.benchmark = False
    return RealismEngine(dims=2048, seed=0, network=NET, resize="torch")


def test_engine_torch_route_feeds_the_trunk_the_restatement(cuda_device, torch_engine):
    """features_from_u8 == the same trunk on the input the restatement builds on the host, to the last bit (the same launches
    on the same input bits); features_from_u8_list on equal-sized images == features_from_u8."""
    imgs = ref.content(300, 8, 64, 80)
    x = torch.from_numpy(ref.network_input_torch(imgs, (299, 299))).to(cuda_device).permute(0, 3, 1, 2)
    want, _ = torch_engine._trunk(x, prenormalized=True)
    want = want.clone()
    u8 = torch.as_tensor(imgs, device=cuda_device)
    got, _ = torch_engine.features_from_u8(u8)
    assert got.shape == (8, 2048) and torch.isfinite(got).all()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    lst, _ = torch_engine.features_from_u8_list([u8[i] for i in range(8)])
    assert torch.equal(lst.view(torch.int32), want.view(torch.int32))
    assert torch_engine.resize == "torch"
    # the route is not the ADM suite's: TensorFlow 1's bilinear resize of the same images gives other features
    from tise_toolbox_amd.engine import RealismEngine
    other, _ = RealismEngine(dims=2048, seed=0, network=NET, resize="tf1").features_from_u8(u8)
    assert (other - got).abs().max().item() > 1e-4 * got.abs().max().item()


def test_engine_refuses_torch_on_another_network(cuda_device):
    from tise_toolbox_amd.engine import RealismEngine
    with pytest.raises(ValueError, match="pytorch-fid's route and runs on network 'inception-2015' only"):
        RealismEngine(dims=2048, seed=0, resize="torch")


# ---- end to end ------------------------------------------------------------------------------------------------------------
def _write(d, imgs):
    from PIL import Image
    d.mkdir(parents=True)
    for i, im in enumerate(imgs):
        Image.fromarray(im).save(d / f"{i:05d}.png")


def _torch_route(u8_hwc):
    """pytorch-fid's input of ONE image through torch itself on the CPU: x / 255, F.interpolate, 2 x - 1."""
    import torch.nn.functional as TF
    t = torch.from_numpy(np.ascontiguousarray(u8_hwc)).permute(2, 0, 1)[None].float() / 255
    return 2 * TF.interpolate(t, size=(299, 299), mode="bilinear", align_corners=False) - 1


def _tf1_route(u8_hwc):
    return torch.from_numpy(tf1.network_input_tf1(u8_hwc[None], (299, 299))).permute(0, 3, 1, 2)


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    """Seeded PNG directories: 23 and 27 images of 64 x 64, and 27 images of three sizes mixed inside every loader batch."""
    d = tmp_path_factory.mktemp("torch_modes")
    _write(d / "one23", _cases.smooth_images(23, 64, 64, seed=51))
    _write(d / "one27", _cases.smooth_images(27, 64, 64, seed=52, shift=0.15))
    sizes = [(64, 64), (48, 80), (75, 50)]
    ragged = [_cases.smooth_images(1, *sizes[i % 3], seed=5300 + i, shift=0.15)[0] for i in range(27)]
    _write(d / "ragged27", ragged)
    return d


@pytest.fixture(scope="module")
def cpu_routes(dirs):
    """(mu, sigma, n) per (route, directory, dims): Pillow convert("RGB"), the route's input on the CPU, the project's fp32
    InceptionV3(network="inception-2015") on the CPU with the stand-in weights of seed 0, np.mean / np.cov over every image.
    One forward per image set serves --dims 64 (block 0, averaged over its positions) and --dims 2048."""
    from PIL import Image
    from tise_toolbox_amd import img_data
    from tise_toolbox_amd.inception import InceptionV3
    before = torch.get_num_threads()
    torch.set_num_threads(max(2, min(16, before)))               # more than one thread: the kernel of torch that pytorch-fid meets
    model = InceptionV3([0, 3], seed=0, network=NET).eval()
    out = {}
    try:
        for route, name in (("torch", "one23"), ("torch", "ragged27"), ("tf1", "one23"), ("tf1", "one27")):
            files = img_data.get_filenames(str(dirs / name))
            fn = _torch_route if route == "torch" else _tf1_route
            x = torch.cat([fn(np.asarray(Image.open(f).convert("RGB"))) for f in files])
            with torch.no_grad():
                blocks = [model(x[i:i + 14], prenormalized=True) for i in range(0, len(x), 14)]
            for dims, k in ((64, 0), (2048, 1)):
                f = torch.cat([b[k].mean(dim=(2, 3)) if b[k].shape[2] > 1 else b[k].flatten(1) for b in blocks]).numpy().astype(np.float64)
                out[route, name, dims] = (f.mean(axis=0), np.cov(f, rowvar=False), len(files))
    finally:
        torch.set_num_threads(before)
    return out


def _cli(argv):
    """fid_score.main in this process.  The model and engine of an earlier call form a reference cycle that holds device
    memory until a collector pass (fid_score._own_model); a ragged directory forks DataLoader workers, and a collector pass
    inside a freshly forked worker that finds such a cycle releases device objects in a process that never opened the device,
    and dies.  One CLI process never holds an earlier call's model; here the cycles are collected before every call."""
    import gc
    from tise_toolbox_amd import fid_score
    gc.collect()
    old = os.environ.get("TISE_CONV")
    os.environ["TISE_CONV"] = "split"
    try:
        return fid_score.main(argv)
    finally:
        if old is None:
            os.environ.pop("TISE_CONV", None)
        else:
            os.environ["TISE_CONV"] = old


def _base(dirs, ref_name, gen_name):
    return ["--batch-size", "10", "--path1", str(dirs / ref_name), "--path2", str(dirs / gen_name), "--num-workers", "0", "--synthetic-weights"]


@pytest.mark.parametrize("dims", [2048, 64])
def test_fid_cli_mode_pytorch_fid_vs_cpu_route(cuda_device, dirs, cpu_routes, tmp_path, dims):
    """fid_score --mode pytorch-fid at --batch-size 10 on 23 images of 64 x 64 against 27 images of three sizes (short last
    batches on both sides; the ragged launch) against the CPU route whose resize is torch's own F.interpolate.  |dFID| <= 1e-3
    absolute, the project's bound for a CLI FID against its CPU route; n is the file count on both sides; the result line
    carries the tag.  Measured on the MI355X: see the README entry of the mode."""
    from oracle import fid_oracle
    from tise_toolbox_amd.weights import SYNTHETIC_TAG
    mr, sr, nr = cpu_routes["torch", "one23", dims]
    mg, sg, ng = cpu_routes["torch", "ragged27", dims]
    assert (nr, ng) == (23, 27)
    want = float(fid_oracle.calculate_frechet_distance(mr, sr, mg, sg))
    stats, out = tmp_path / "gen.npz", tmp_path / "fid.txt"
    v = _cli(_base(dirs, "one23", "ragged27") + ["--mode", "pytorch-fid", "--dims", str(dims), "--save-stats", str(stats),
                                                   "--prdc" if dims == 2048 else "--kid", "--saved_file", str(out)])
    print(f"FID --mode pytorch-fid --dims {dims}: device {v!r} cpu route {want!r} difference {abs(v - want):.3e}")
    assert out.read_text() == f"FID: {v} [mode pytorch-fid]{SYNTHETIC_TAG}"
    with np.load(stats) as f:
        assert str(f["mode"]) == "pytorch-fid" and str(f["network"]) == NET
        assert f["features"].shape == (27, dims)                                       # every image: 27, not 20
        dmu = np.abs(f["mu"] - mg).max()
        print(f"  max |mu - cpu mu| = {dmu:.3e} (scale {np.abs(mg).max():.3e})")
        assert dmu <= 1e-4 * np.abs(mg).max()
    assert abs(v - want) <= 1e-3


def test_fid_cli_pytorch_fid_stats_round_trip_and_refusals(cuda_device, dirs, tmp_path, capsys):
    """--save-stats in statistics-only mode, the .npz fed back as --path1 (n = 23 there: every image), refused under --mode
    tise and --mode clean; an untagged copy of it is refused with the flag named and accepted with --untagged-stats; the
    default route on the same directories prints the line it always printed, with no tag."""
    from tise_toolbox_amd.weights import SYNTHETIC_TAG
    stats = tmp_path / "one23.npz"
    common = ["--batch-size", "10", "--num-workers", "0", "--synthetic-weights"]
    assert _cli(common + ["--path2", str(dirs / "one23"), "--mode", "pytorch-fid", "--save-stats", str(stats)]) is None
    assert f"statistics of {dirs / 'one23'} -> {stats} [mode pytorch-fid]{SYNTHETIC_TAG}" in capsys.readouterr().out
    with np.load(stats) as f:
        assert sorted(f.files) == ["mode", "mu", "network", "sigma"] and str(f["mode"]) == "pytorch-fid"
        mu, sigma = f["mu"], f["sigma"]
    direct = _cli(_base(dirs, "one23", "one27") + ["--mode", "pytorch-fid"])
    fed = _cli(common + ["--path1", str(stats), "--path2", str(dirs / "one27"), "--mode", "pytorch-fid"])
    assert abs(fed - direct) <= 1e-6 * max(1.0, abs(direct))
    for mode, extra in (("tise", ["--network", NET]), ("clean", [])):
        with pytest.raises(RuntimeError, match=f"statistics of mode 'pytorch-fid', this run uses --mode {mode}"):
            _cli(common + ["--path1", str(stats), "--path2", str(dirs / "one27"), "--mode", mode] + extra)
    plain = tmp_path / "plain.npz"
    np.savez(plain, mu=mu, sigma=sigma)                                                  # what pytorch-fid's own --save-stats writes
    argv = common + ["--path1", str(plain), "--path2", str(dirs / "one27"), "--mode", "pytorch-fid"]
    with pytest.raises(RuntimeError, match="--untagged-stats pytorch-fid"):
        _cli(argv)
    capsys.readouterr()
    flagged = _cli(argv + ["--untagged-stats", "pytorch-fid"])
    assert abs(flagged - fed) <= 1e-9 * max(1.0, abs(fed))
    cap = capsys.readouterr()
    assert "taken as statistics of mode pytorch-fid (--untagged-stats)" in cap.err and f"FID: {flagged} [mode pytorch-fid]" in cap.out
    from tise_toolbox_amd import fid_score
    fid_score.set_untagged_stats(None)
    # the default route is what it was: whole batches only (20 of 23 and 20 of 27 images), no tag on the line
    t = _cli(_base(dirs, "one23", "one27"))
    shown = capsys.readouterr().out
    assert f"FID: {t}{SYNTHETIC_TAG}\n" in shown and "[mode" not in shown
    assert abs(t - direct) > 1e-3                                                        # another network, resize and image count: another number


def test_fid_cli_mode_torch_fidelity(cuda_device, dirs, cpu_routes, tmp_path, capsys):
    """fid_score --mode torch-fidelity on the two one-size directories against the CPU route with the TF1 restatement as the
    resize: |dFID| <= 1e-3; a directory of several image sizes is refused with the reason."""
    from oracle import fid_oracle
    from tise_toolbox_amd.weights import SYNTHETIC_TAG
    mr, sr, nr = cpu_routes["tf1", "one23", 2048]
    mg, sg, ng = cpu_routes["tf1", "one27", 2048]
    assert (nr, ng) == (23, 27)
    want = float(fid_oracle.calculate_frechet_distance(mr, sr, mg, sg))
    v = _cli(_base(dirs, "one23", "one27") + ["--mode", "torch-fidelity"])
    assert f"FID: {v} [mode torch-fidelity]{SYNTHETIC_TAG}" in capsys.readouterr().out
    print(f"FID --mode torch-fidelity: device {v!r} cpu route {want!r} difference {abs(v - want):.3e}")
    assert abs(v - want) <= 1e-3
    with pytest.raises(RuntimeError, match="differ in size .* the TF1 resize of this mode has no ragged launch"):
        _cli(_base(dirs, "one23", "ragged27") + ["--mode", "torch-fidelity"])


def test_torch_fidelity_statistics_are_adm_evals(cuda_device, dirs, tmp_path):
    """The statistics fid_score --mode torch-fidelity --save-stats writes for a directory are the mu / sigma of adm_eval's pass
    (adm_eval._pass on its own engine: spatial tap, logits) over the same 27 images packed as an .npz batch in the walk's
    order, bit for bit: the same kernels on the same images in the same order, one device batch on both sides."""
    from PIL import Image
    from tise_toolbox_amd import adm_eval, img_data
    from tise_toolbox_amd.engine import RealismEngine
    stats = tmp_path / "one27.npz"
    _cli(["--batch-size", "10", "--num-workers", "0", "--synthetic-weights", "--path2", str(dirs / "one27"), "--mode", "torch-fidelity",
          "--save-stats", str(stats)])
    np.savez(tmp_path / "batch.npz", np.stack([np.asarray(Image.open(f).convert("RGB")) for f in img_data.get_filenames(str(dirs / "one27"))]))
    old = os.environ.get("TISE_CONV")
    os.environ["TISE_CONV"] = "split"
    try:
        eng = RealismEngine(dims=2048, seed=0, with_logits=True, network=NET, resize="tf1", spatial=True)
        side = adm_eval._pass(eng, str(tmp_path / "batch.npz"), 1000, False, 5000)
    finally:
        if old is None:
            os.environ.pop("TISE_CONV", None)
        else:
            os.environ["TISE_CONV"] = old
    assert side["n"] == 27
    with np.load(stats) as a:
        assert str(a["mode"]) == "torch-fidelity" and str(a["network"]) == NET
        for k in ("mu", "sigma"):
            b = side[k].cpu().numpy()
            d = np.abs(a[k] - b).max()
            print(f"  {k}: max |fid_score - adm_eval| = {d:.3e} (scale {np.abs(b).max():.3e})")
            assert np.array_equal(a[k], b), k
