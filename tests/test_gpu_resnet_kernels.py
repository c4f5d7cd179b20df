"""GPU: the kernels ResNet-50 adds (csrc/resnet.hip, stem7_mfma_u8_kernel of csrc/conv_pipe.hip) at every layout edge, and the
split-precision convolution at ResNet's shapes; the stem also past the first iteration of its persistent tile loop (more tiles than
the device has CUs).

Stem (both routes) and convolutions: ``tests/_trunk_audit.CONV_TOL`` of the output scale against an fp64 convolution of the table
values, the project's figure for every split convolution.  Residual add and pool: no tolerance, bit for bit against
``conv_split.split`` of the torch fp32 expression."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests._trunk_audit import CONV_TOL

pytestmark = pytest.mark.gpu

SENT = -7.25                                                     # exact in fp16 and fp32


@pytest.fixture(scope="module")
def dev(cuda_device):
    return cuda_device


def bits16(t):
    return t.contiguous().view(torch.int16).cpu()


def merged64(t):
    from tise_toolbox_amd import conv_split
    hi, lo = conv_split.halves(t.cpu())
    return hi.double() + lo.double() / 2048.0


def seeded_bytes(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)


# ---------------------------------------------------------------------------------------------------------------- the stem
@pytest.fixture(scope="module")
def stem(dev):
    """The seeded module's folded conv1 on both routes, and the fp64 reference."""
    from tise_toolbox_amd import conv_split, device, resnet_hip, resnet_model

    class Stem:
        pass
    s = Stem()
    s.lut = resnet_model.input_table()
    s.lut_dev = s.lut.to(dev)

    def parts(w, b):
        wsp, sc = resnet_hip.pack_stem7_mfma(w, dev)
        w32 = torch.cat([w, torch.zeros((64, 29, 7, 7))], 1)
        return dict(w=w, b=b, wsp=wsp, sc=sc, b_dev=b.to(dev), padded=conv_split.SplitConv(w32, b, (2, 2), (3, 3), dev, name="conv1"))
    w, b = resnet_model.ResNet50().init_synthetic(0).folded()["conv1"]
    s.seeded = parts(w, b)
    s.positive = parts(w.abs(), b.abs())

    def reference(p, img):
        x = torch.stack([s.lut[c][img[..., c].long()] for c in range(3)], 1).double()
        return torch.relu(F.conv2d(x, p["w"].double(), p["b"].double(), 2, 3)).permute(0, 2, 3, 1)

    def mfma(p, x_dev, out=None):
        assert device.stem_conv7x7s2_supported(x_dev)
        return device.stem_conv7x7s2_split_u8(x_dev, s.lut_dev, p["wsp"], p["sc"], p["b_dev"], out=out)

    def padded(p, x_dev):
        x = device.resnet_input_split(x_dev, s.lut_dev)
        n, h, w_, _ = x.shape
        oh, ow = p["padded"].out_hw(h, w_)
        y = torch.full((n, oh, ow, 128), SENT, dtype=torch.float16, device=dev)
        p["padded"](x, [(0, 64, y, 0, 0)])
        return y
    s.reference, s.mfma, s.padded = reference, mfma, padded
    return s


STEM_SHAPES = [(1, 8, 8), (1, 9, 13), (1, 32, 32), (1, 33, 47), (3, 16, 16), (1, 224, 224)]


@pytest.mark.parametrize("n,h,w", STEM_SHAPES)
def test_stem_mfma_against_fp64(dev, stem, n, h, w):
    img = seeded_bytes(n, h, w, 7000 + 100 * h + w)
    want = stem.reference(stem.seeded, img)
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    assert want.shape == (n, oh, ow, 64)
    big = torch.full((n + 2, oh, ow, 128), SENT, dtype=torch.float16, device=dev)         # canaries: an image before and one after
    got = stem.mfma(stem.seeded, img.to(dev), out=big[1:1 + n])
    torch.cuda.synchronize()
    assert bool((big[0] == SENT).all()) and bool((big[-1] == SENT).all())
    scale = want.abs().max().item()
    err = (merged64(got) - want).abs().max().item()
    print(f"stem mfma {n}x{h}x{w}: error / scale = {err / scale:.3e}")
    assert err <= CONV_TOL * scale, (n, h, w, err, scale)
    again = stem.mfma(stem.seeded, img.to(dev))
    assert torch.equal(bits16(again), bits16(got))                                        # a second call, a fresh destination
    if n > 1:                                                                             # an image's bits do not depend on its place
        alone = stem.mfma(stem.seeded, img[n - 1:].to(dev))
        assert torch.equal(bits16(alone), bits16(got[n - 1:]))


@pytest.mark.parametrize("h,w,tiles_per_image,more", [(33, 47, 3, 2), (9, 13, 1, 3)])
def test_stem_mfma_walks_more_tiles_than_there_are_cus(dev, stem, h, w, tiles_per_image, more):
    """stem7_mfma_u8_kernel launches min(tiles, CU count) workgroups and each walks tiles ``gridDim.x`` apart: a batch with more
    tiles than the device has CUs runs the second iteration of that loop -- the barrier at its top, the patch rewritten while other
    waves finish their tile, ``continue`` for the waves past the last output row (33 x 47: 17 output rows, so the third tile of an
    image has one live wave; 9 x 13: one tile per image with five).  Every other stem test stays under the CU count."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    n = cus // tiles_per_image + more
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    assert ((oh + 7) // 8) * ((ow + 31) // 32) == tiles_per_image and n * tiles_per_image > cus
    img = seeded_bytes(n, h, w, 9000 + 100 * h + w)
    want = stem.reference(stem.seeded, img)
    assert want.shape == (n, oh, ow, 64)
    big = torch.full((n + 2, oh, ow, 128), SENT, dtype=torch.float16, device=dev)         # canaries: an image before and one after
    got = stem.mfma(stem.seeded, img.to(dev), out=big[1:1 + n])
    torch.cuda.synchronize()
    assert bool((big[0] == SENT).all()) and bool((big[-1] == SENT).all())
    scale = want.abs().max().item()
    per_image = (merged64(got) - want).abs().flatten(1).amax(1)
    err = per_image.max().item()
    print(f"stem mfma {n}x{h}x{w}: {n * tiles_per_image} tiles on {cus} CUs, error / scale = {err / scale:.3e} "
          f"(images whose tiles a second iteration computes: {per_image[cus // tiles_per_image:].max().item() / scale:.3e})")
    assert err <= CONV_TOL * scale, (n, h, w, err, scale, int(per_image.argmax()))
    alone = stem.mfma(stem.seeded, img[n - 1:].to(dev))                                   # the last image: a second-iteration tile
    assert torch.equal(bits16(alone), bits16(got[n - 1:]))


@pytest.mark.parametrize("n,h,w", STEM_SHAPES)
def test_stem_padded_route_against_fp64(dev, stem, n, h, w):
    from tise_toolbox_amd import conv_split
    img = seeded_bytes(n, h, w, 7000 + 100 * h + w)
    want = stem.reference(stem.seeded, img)
    x = torch.zeros((n, h, w, 32))
    for c in range(3):
        x[..., c] = stem.lut[c][img[..., c].long()]
    from tise_toolbox_amd import device
    assert torch.equal(bits16(device.resnet_input_split(img.to(dev), stem.lut_dev)), bits16(conv_split.split(x)))
    got = stem.padded(stem.seeded, img.to(dev))
    torch.cuda.synchronize()
    scale = want.abs().max().item()
    err = (merged64(got) - want).abs().max().item()
    print(f"stem padded {n}x{h}x{w}: error / scale = {err / scale:.3e}")
    assert err <= CONV_TOL * scale, (n, h, w, err, scale)


def test_stem_odd_address_is_served(dev, stem):
    from tise_toolbox_amd import device
    h, w = 33, 47
    img = seeded_bytes(1, h, w, 11)
    odd = torch.zeros(h * w * 3 + 1, dtype=torch.uint8, device=dev)
    odd[1:] = img.to(dev).reshape(-1)
    x = odd[1:].view(1, h, w, 3)
    assert x.data_ptr() % 2 == 1 and x.is_contiguous()
    assert device.stem_conv7x7s2_supported(x)                                             # the route: the matrix-core stem takes it
    got = stem.mfma(stem.seeded, x)
    assert torch.equal(bits16(got), bits16(stem.mfma(stem.seeded, img.to(dev))))
    got_p = stem.padded(stem.seeded, x)
    assert torch.equal(bits16(got_p), bits16(stem.padded(stem.seeded, img.to(dev))))


@pytest.mark.parametrize("h,w", [(8, 8), (9, 13), (33, 47)])
def test_stem_padding_is_zero_not_the_table(dev, stem, h, w):
    """All-255 bytes and all-positive weights: a padding tap read as table[c][0] (negative) or as table[c][255] would change every
    border pixel by far more than the tolerance."""
    img = torch.full((1, h, w, 3), 255, dtype=torch.uint8)
    want = stem.reference(stem.positive, img)
    inner, corner = want[0, want.shape[1] // 2, want.shape[2] // 2], want[0, 0, 0]
    assert bool((corner < 0.5 * inner).all())                                            # the border sees 16 of 49 taps
    scale = want.abs().max().item()
    for route in (stem.mfma, stem.padded):
        got = route(stem.positive, img.to(dev))
        torch.cuda.synchronize()
        err = (merged64(got) - want).abs().max().item()
        assert err <= CONV_TOL * scale, (route.__name__, err, scale)


def test_stem_entry_minimum(dev, stem):
    """The entry's own minimum is one pixel: 1 x 1 is served (one output pixel: the centre tap), h = 0 is refused before a launch."""
    from tise_toolbox_amd import _lib
    img = seeded_bytes(2, 1, 1, 3)
    want = stem.reference(stem.seeded, img)
    got = stem.mfma(stem.seeded, img.to(dev))
    assert got.shape == (2, 1, 1, 128)
    assert (merged64(got) - want).abs().max().item() <= CONV_TOL * max(want.abs().max().item(), 1e-3)
    p = stem.seeded
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    with pytest.raises(_lib.TiseStatusError) as e:
        _lib.call("tise_stem_conv7x7s2_split_u8_mfma", P(img.to(dev)), P(stem.lut_dev), 1, 0, 1, P(p["wsp"]), P(p["sc"]), P(p["b_dev"]),
                  P(got), None)
    assert e.value.status == _lib.TISE_ERR_INVALID_ARG


# --------------------------------------------------------------------------------------------- convolutions at ResNet's shapes
#              cin, cout, k, stride, pad, mode
CONV_LAYERS = [(256, 512, 1, 2, 0, 1), (128, 128, 3, 2, 1, 0), (512, 512, 3, 2, 1, 0), (64, 256, 1, 1, 0, 1), (512, 2048, 1, 1, 0, 1),
               (32, 64, 7, 2, 3, 0), (64, 64, 3, 1, 1, 0), (128, 128, 3, 1, 1, 0), (256, 1024, 1, 2, 0, 1)]


@pytest.fixture(scope="module")
def conv_layers(dev):
    from tise_toolbox_amd import conv_split
    out = {}
    for L in CONV_LAYERS:
        cin, cout, k, s, p, mode = L
        g = torch.Generator().manual_seed(cin * 7 + cout + k)
        w = torch.randn((cout, cin, k, k), generator=g) * (2.0 / (cin * k * k)) ** 0.5
        b = torch.randn(cout, generator=g) * 0.1
        out[L] = (conv_split.SplitConv(w, b, (s, s), (p, p), dev), w.double(), b.double())      # the kernel left to "auto"
    return out


@pytest.mark.parametrize("h,w", [(8, 8), (7, 7), (15, 9)])
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("L", CONV_LAYERS, ids=lambda L: "x".join(str(v) for v in L))
def test_conv_at_resnet_shapes(dev, conv_layers, L, n, h, w):
    from tise_toolbox_amd import conv_split
    cin, cout, k, s, p, mode = L
    conv, w64, b64 = conv_layers[L]
    g = torch.Generator().manual_seed(h * 100 + w * 10 + n)
    x32 = torch.randn((n, h, w, cin), generator=g)
    if cin == 32:
        x32[..., 3:] = 0.0
    x = conv_split.split(x32)
    ref_in = merged64(x).permute(0, 3, 1, 2)
    oh, ow = conv.out_hw(h, w)
    if mode == 0:
        want = torch.relu(F.conv2d(ref_in, w64, b64, s, p)).permute(0, 2, 3, 1)
        y = torch.full((n, oh, ow, 2 * cout), SENT, dtype=torch.float16, device=dev)
    else:
        want = F.conv2d(ref_in, w64, None, s, p).permute(0, 2, 3, 1)                      # mode 1: scale * conv, no bias, no ReLU
        y = torch.full((n, oh, ow, cout), SENT, dtype=torch.float32, device=dev)
    assert tuple(want.shape) == (n, oh, ow, cout)
    assert conv(x.to(dev), [(0, cout, y, 0, mode)]) == (oh, ow)
    torch.cuda.synchronize()
    got = merged64(y) if mode == 0 else y.cpu().double()
    scale = want.abs().max().item()
    err = (got - want).abs().max().item()
    print(f"conv {L} n={n} {h}x{w} ({conv.variant}): error / scale = {err / scale:.3e}")
    assert err <= CONV_TOL * scale, (L, n, h, w, conv.variant, err, scale)


# ------------------------------------------------------------------------------------------------------- residual add + ReLU
def residual_reference(raw, bias, identity, id_bias=None):
    from tise_toolbox_amd import conv_split
    t = raw + bias
    u = conv_split.merge(identity) if id_bias is None else identity + id_bias
    return conv_split.split(torch.relu(t + u))


def residual_inputs(C, pixels, seed):
    from tise_toolbox_amd import conv_split
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn((pixels, C), generator=g) * 3.0
    bias = torch.randn(C, generator=g)
    ids = conv_split.split(torch.randn((pixels, C), generator=g).abs() * 2.0)
    idr = torch.randn((pixels, C), generator=g) * 2.0
    idb = torch.randn(C, generator=g)
    return raw, bias, ids, idr, idb


@pytest.mark.parametrize("pixels", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("C", [64, 256, 48])
def test_residual_relu_bit_for_bit(dev, C, pixels):
    from tise_toolbox_amd import conv_split, device
    raw, bias, ids, idr, idb = residual_inputs(C, pixels, C * 1000 + pixels)
    d = lambda t: t.to(dev)
    device.read_split_overflow()
    want_s, want_r = residual_reference(raw, bias, ids), residual_reference(raw, bias, idr, idb)
    got_s = device.residual_relu_split(d(raw), d(bias), d(ids))
    got_r = device.residual_relu_split(d(raw), d(bias), d(idr), d(idb))
    assert torch.equal(bits16(got_s), bits16(want_s)) and torch.equal(bits16(got_r), bits16(want_r))
    assert torch.equal(bits16(device.residual_relu_split(d(raw), d(bias), d(ids))), bits16(got_s))      # a second call
    # slices at an offset into wider tensors (the split ones reach into a 16-wide tail when C = 48), canary pixels around out
    raw_w = torch.full((pixels, C + 32), 99.0)
    raw_w[:, 32:] = raw
    idr_w = torch.full((pixels, C + 36), 99.0)
    idr_w[:, 36:] = idr
    ids_w = conv_split.split(torch.cat([torch.full((pixels, 32), 5.0), conv_split.merge(ids)], 1))
    assert torch.equal(conv_split.merge(ids_w)[:, 32:], conv_split.merge(ids))           # split(merge(.)) keeps the 22-bit value
    for identity, kw, want in ((ids_w, dict(id_off=32), want_s), (idr_w, dict(id_off=36, id_bias=d(idb)), want_r)):
        big = torch.full((pixels + 2, 2 * (C + 64)), SENT, dtype=torch.float16, device=dev)
        device.residual_relu_split(d(raw_w), d(bias), d(identity), out=big[1:-1], raw_off=32, out_off=64, channels=C, **kw)
        torch.cuda.synchronize()
        assert bool((big[0] == SENT).all()) and bool((big[-1] == SENT).all())
        hi, lo = conv_split.halves(big[1:-1].cpu())
        whi, wlo = conv_split.halves(want)
        assert torch.equal(bits16(hi[:, 64:]), bits16(whi)) and torch.equal(bits16(lo[:, 64:]), bits16(wlo))
        assert bool((hi[:, :64] == SENT).all()) and bool((lo[:, :64] == SENT).all())
    assert not device.read_split_overflow()


@pytest.mark.parametrize("where", ["raw", "id_split", "id_raw"])
@pytest.mark.parametrize("value", [float("nan"), float("inf")])
def test_residual_guard_sees_non_finite_inputs(dev, where, value):
    from tise_toolbox_amd import conv_split, device
    C, pixels, px, ch = 64, 65, 37, 21
    raw, bias, ids, idr, idb = residual_inputs(C, pixels, 5)
    d = lambda t: t.to(dev)
    if where == "raw":
        raw[px, ch] = value
    elif where == "id_raw":
        idr[px, ch] = value
    else:
        m = conv_split.merge(ids)
        m[px, ch] = value
        ids = conv_split.split(m)                                                        # hi = inf or NaN
    device.read_split_overflow()
    if where == "id_raw":
        got, want = device.residual_relu_split(d(raw), d(bias), d(idr), d(idb)), residual_reference(raw, bias, idr, idb)
    else:
        got, want = device.residual_relu_split(d(raw), d(bias), d(ids)), residual_reference(raw, bias, ids)
    assert device.read_split_overflow()                                                  # raised, although max(v, 0) may be a clean 0
    assert not device.read_split_overflow()                                              # read-and-clear
    keep = torch.ones(pixels, dtype=torch.bool)
    keep[px] = False
    assert torch.equal(bits16(got[keep]), bits16(want[keep]))                            # no other pixel is touched
    hi, lo = conv_split.halves(got.cpu())
    whi, wlo = conv_split.halves(want)
    rest = torch.ones(C, dtype=torch.bool)
    rest[ch] = False
    assert torch.equal(bits16(hi[px][rest]), bits16(whi[px][rest])) and torch.equal(bits16(lo[px][rest]), bits16(wlo[px][rest]))


def test_residual_guard_at_the_edge_of_the_range(dev):
    from tise_toolbox_amd import device
    C = 16
    above = float(torch.nextafter(torch.tensor(65504.0), torch.tensor(float("inf"))))
    zeros = torch.zeros((1, C), device=dev)
    for v, fires in ((65504.0, False), (above, True), (-65504.0, False), (-above, True), (65503.996, False)):
        raw = torch.zeros((1, C))
        raw[0, 3] = v
        device.read_split_overflow()
        got = device.residual_relu_split(raw.to(dev), torch.zeros(C, device=dev), zeros, torch.zeros(C, device=dev))
        assert device.read_split_overflow() == fires, v
        want = residual_reference(raw, torch.zeros(C), torch.zeros((1, C)), torch.zeros(C))
        assert torch.equal(bits16(got), bits16(want)), v


# ---------------------------------------------------------------------------------------------------------------- the pool
@pytest.mark.parametrize("h,w", [(1, 1), (2, 2), (3, 5), (16, 16), (17, 31)])
@pytest.mark.parametrize("C", [64, 48])
def test_maxpool3s2p1_split_bit_for_bit(dev, h, w, C):
    from tise_toolbox_amd import conv_split, device
    g = torch.Generator().manual_seed(h * 1000 + w * 10 + C)
    n = 2
    x32 = torch.randn((n, h, w, C), generator=g) * 3.0
    x32[1] = -x32[1].abs() - 0.5                                                         # an all-negative image: the padding must not win
    x = conv_split.split(x32)
    merged = conv_split.merge(x)
    want = conv_split.split(F.max_pool2d(merged.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous())
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    assert want.shape == (n, oh, ow, 2 * C) and bool((conv_split.merge(want)[1] < 0).all())
    got = device.maxpool3s2p1_split(x.to(dev))
    assert torch.equal(bits16(got), bits16(want))
    # a channel slice of the source into a destination slice at an offset of a wider tensor; the rest of it survives
    Cd, off, x_off, c = 96, 48, 16, 32
    dst = torch.full((n, oh, ow, 2 * Cd), SENT, dtype=torch.float16, device=dev)
    device.maxpool3s2p1_split(x.to(dev), out=dst, out_off=off, x_off=x_off, channels=c)
    torch.cuda.synchronize()
    hi, lo = conv_split.halves(dst.cpu())
    whi, wlo = conv_split.halves(want)
    assert torch.equal(bits16(hi[..., off:off + c]), bits16(whi[..., x_off:x_off + c]))
    assert torch.equal(bits16(lo[..., off:off + c]), bits16(wlo[..., x_off:x_off + c]))
    keep = torch.ones(Cd, dtype=torch.bool)
    keep[off:off + c] = False
    assert bool((hi[..., keep] == SENT).all()) and bool((lo[..., keep] == SENT).all())
