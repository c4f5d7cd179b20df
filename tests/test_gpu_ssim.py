"""GPU: the paired-image kernels of csrc/ssim.hip (tise_ssim_pairs, tise_pair_sse_u8, tise_pool2x2_pairs) through
tise_toolbox_amd.device, against the numpy fp64 restatement tests/_ssim_ref.py.

Inputs are SMOOTH seeded images (_ssim_ref.smooth_pair: blurred noise rescaled to 0..255) and the same plus N(0, sigma) noise,
sigma in {4, 25}, clipped.  Shapes: the single valid position (11 x 11), one extra row / column, an odd byte stride (37 x 53),
64 x 64, and one below, at and one above the output tile's side (64 rows, 64 pixels: images of 73, 74, 75) on both axes, and a
3 x 4-tile image (139 x 203).

TOL = 3e-9 absolute for the two map means, derived, not measured: a moment is a weighted sum of 121 non-negative terms <= 255^2,
so any summation order errs by <= 121 2^-53 65025 ~ 8.7e-10; mu^2 errs by <= 1.7e-9, the sigma terms by <= 2.6e-9; cs has a
denominator >= C2 = 58.5 (<= 1.8e-10), l one >= C1 = 6.5 (<= 1.1e-9), l cs errs by <= 1.3e-9; device and reference may each use
that, so the two together stay under 3e-9.  Measured worst over all cases of this file on MI355X: 1.6e-14 (11 x 12, sigma 4);
the sums, the 2 x 2 means and the identical-pair results carry no tolerance at all."""
import functools

import numpy as np
import pytest

from tests import _ssim_ref as ref

TOL = 3e-9
TILE = 64
SHAPES = [(11, 11), (11, 12), (12, 11), (37, 53), (64, 64),
          (TILE + 9, TILE + 11), (TILE + 10, TILE + 10), (TILE + 11, TILE + 9),       # 63, 64, 65 output rows / pixels
          (2 * TILE + 11, 3 * TILE + 11)]                                              # 139 x 203: 3 x 4 tiles
SMALLEST, LARGEST = SHAPES[0], SHAPES[-1]
SIGMAS = (4, 25)


@functools.lru_cache(maxsize=None)
def case(h, w, sigma):
    x, y = ref.smooth_pair(h, w, sigma, seed=1000 * h + w + sigma)
    means = ref.ssim_means(x, y)
    for a in (x, y, means):
        a.setflags(write=False)
    return x, y, means


def _dev(a, dev):
    import torch
    return torch.as_tensor(np.array(a), device=dev)          # (a copy: the cached cases are read-only)


def _bits(t):
    return t.cpu().numpy().tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_ssim_means_match_the_reference(cuda_device, shape, sigma):
    from tise_toolbox_amd import device
    x, y, want = case(*shape, sigma)
    got = device.ssim_pairs([_dev(x, cuda_device)], [_dev(y, cuda_device)]).cpu().numpy()
    assert got.shape == (1, 3, 2) and got.dtype == np.float64
    worst = float(np.max(np.abs(got[0] - want)))
    print(f"ssim_pairs {shape} sigma {sigma}: worst |device - reference| = {worst:.3e}")
    assert worst <= TOL, (shape, sigma, worst)


@pytest.mark.gpu
def test_identical_pair_is_exactly_one(cuda_device):
    """x == y: numerator and denominator of l and of cs are the same bits at every position, so both means are exactly 1.0 --
    for bytes and for fp32 levels, through distinct tensors of equal content and through one tensor twice."""
    import torch
    from tise_toolbox_amd import device
    xs = [_dev(case(*s, 4)[0], cuda_device) for s in SHAPES]
    for ys in (xs, [t.clone() for t in xs]):
        out = device.ssim_pairs(xs, ys).cpu().numpy()
        assert np.array_equal(out, np.ones((len(SHAPES), 3, 2))), out
    lx, ly = device.pool2x2_pairs([xs[-1]], [xs[-1].clone()])
    assert np.array_equal(device.ssim_pairs(lx, ly).cpu().numpy(), np.ones((1, 3, 2)))
    flat = torch.full((1, 40, 50, 3), 255, dtype=torch.uint8, device=cuda_device)        # zero variance, the largest mean
    assert np.array_equal(device.ssim_pairs(flat, flat.clone()).cpu().numpy(), np.ones((1, 3, 2)))


@pytest.mark.gpu
def test_uint8_and_fp32_input_give_the_same_bits(cuda_device):
    from tise_toolbox_amd import device
    xs = [_dev(case(*s, 25)[0], cuda_device) for s in SHAPES]
    ys = [_dev(case(*s, 25)[1], cuda_device) for s in SHAPES]
    a = device.ssim_pairs(xs, ys)
    b = device.ssim_pairs([t.float() for t in xs], [t.float() for t in ys])
    assert _bits(a) == _bits(b)


@pytest.mark.gpu
def test_ragged_launch_equals_single_launches_bit_for_bit(cuda_device):
    """The smallest and the largest shape (and the ones between) in ONE launch, in two orders: per pair the bits of launching
    the pair alone, and of a second call; a uniform (N,H,W,3) batch gives them too."""
    import torch
    from tise_toolbox_amd import device
    shapes = [SMALLEST, LARGEST, (37, 53), SMALLEST, (TILE + 11, TILE + 9), LARGEST]
    xs = [_dev(case(*s, 25)[0], cuda_device) for s in shapes]
    ys = [_dev(case(*s, 25)[1], cuda_device) for s in shapes]
    alone = torch.cat([device.ssim_pairs([a], [b]) for a, b in zip(xs, ys)])
    together = device.ssim_pairs(xs, ys)
    assert _bits(together) == _bits(alone)
    assert _bits(device.ssim_pairs(xs, ys)) == _bits(together)
    back = device.ssim_pairs(xs[::-1], ys[::-1])
    assert _bits(back.flip(0).contiguous()) == _bits(together)
    big = device.ssim_pairs(torch.stack([xs[1], xs[5], xs[1]]), torch.stack([ys[1], ys[5], ys[1]]))
    assert _bits(big) == _bits(torch.stack([alone[1], alone[5], alone[1]]))
    want = np.stack([case(*s, 25)[2] for s in shapes])
    assert float(np.max(np.abs(together.cpu().numpy() - want))) <= TOL


@pytest.mark.gpu
def test_source_at_an_odd_byte_address(cuda_device):
    import torch
    from tise_toolbox_amd import device
    x, y, want = case(37, 53, 4)
    n = x.size
    buf = torch.zeros(2 * n + 8, dtype=torch.uint8, device=cuda_device)
    bx, by = buf[1:1 + n].view(x.shape), buf[n + 4:2 * n + 4].view(y.shape)      # 37 * 53 * 3 is odd: both addresses are
    bx.copy_(_dev(x, cuda_device))
    by.copy_(_dev(y, cuda_device))
    assert bx.data_ptr() % 2 == 1 and bx.is_contiguous()
    got = device.ssim_pairs([bx], [by])
    assert _bits(got) == _bits(device.ssim_pairs([_dev(x, cuda_device)], [_dev(y, cuda_device)]))
    assert float(np.max(np.abs(got.cpu().numpy()[0] - want))) <= TOL
    assert int(device.pair_sse_u8([bx], [by]).cpu()[0]) == ref.sse(x, y)
    px, py = device.pool2x2_pairs([bx], [by])
    assert np.array_equal(px[0].cpu().numpy().astype(np.float64), ref.pool2x2(x))
    assert np.array_equal(py[0].cpu().numpy().astype(np.float64), ref.pool2x2(y))


@pytest.mark.gpu
def test_canaries_around_every_output_and_the_workspace(cuda_device):
    import torch
    from tise_toolbox_amd import device
    shapes = [SMALLEST, LARGEST, (37, 53)]
    xs = [_dev(case(*s, 4)[0], cuda_device) for s in shapes]
    ys = [_dev(case(*s, 4)[1], cuda_device) for s in shapes]
    n, guard = len(shapes), 64
    need = device.ssim_workspace_bytes(n, LARGEST[0], LARGEST[1])
    assert need == 48 * n * 3 * 4
    ws = torch.full((need + 2 * guard,), 0xA5, dtype=torch.uint8, device=cuda_device)
    out = torch.full((n * 6 + 2 * guard,), -7.0, dtype=torch.float64, device=cuda_device)
    got = device.ssim_pairs(xs, ys, out=out[guard:guard + n * 6].view(n, 3, 2), workspace=ws[guard:guard + need])
    assert _bits(got) == _bits(device.ssim_pairs(xs, ys))
    assert bool((ws[:guard] == 0xA5).all()) and bool((ws[guard + need:] == 0xA5).all())
    assert bool((out[:guard] == -7.0).all()) and bool((out[guard + n * 6:] == -7.0).all())
    sse = torch.full((n + 2 * guard,), -7, dtype=torch.int64, device=cuda_device)
    device.pair_sse_u8(xs, ys, out=sse[guard:guard + n])
    assert sse[guard:guard + n].cpu().tolist() == [ref.sse(*case(*s, 4)[:2]) for s in shapes]
    assert bool((sse[:guard] == -7).all()) and bool((sse[guard + n:] == -7).all())
    total = sum(device.pool2x2_sizes(xs))
    store = torch.full((2 * total + 2 * guard,), -7.0, dtype=torch.float32, device=cuda_device)
    px, py = device.pool2x2_pairs(xs, ys, out=store[guard:guard + 2 * total])
    assert bool((store[:guard] == -7.0).all()) and bool((store[guard + 2 * total:] == -7.0).all())
    for s, a, b in zip(shapes, px, py):
        assert np.array_equal(a.cpu().numpy().astype(np.float64), ref.pool2x2(case(*s, 4)[0]))
        assert np.array_equal(b.cpu().numpy().astype(np.float64), ref.pool2x2(case(*s, 4)[1]))


@pytest.mark.gpu
def test_pair_sse_is_exact(cuda_device):
    """Against numpy int64 on every shape in one ragged launch, and all-0 against all-255 at the largest shape (the largest
    sum a pair of that size can have)."""
    import torch
    from tise_toolbox_amd import device
    xs = [_dev(case(*s, 25)[0], cuda_device) for s in SHAPES]
    ys = [_dev(case(*s, 25)[1], cuda_device) for s in SHAPES]
    got = device.pair_sse_u8(xs, ys)
    assert got.dtype == torch.int64
    assert got.cpu().tolist() == [ref.sse(*case(*s, 25)[:2]) for s in SHAPES]
    assert _bits(device.pair_sse_u8(xs, ys)) == _bits(got)
    h, w = LARGEST
    zero = torch.zeros((2, h, w, 3), dtype=torch.uint8, device=cuda_device)
    full = torch.full((2, h, w, 3), 255, dtype=torch.uint8, device=cuda_device)
    assert device.pair_sse_u8(zero, full).cpu().tolist() == [255 * 255 * 3 * h * w] * 2
    assert device.pair_sse_u8(full, full.clone()).cpu().tolist() == [0, 0]
    one = full.clone()
    one[1, h - 1, w - 1, 2] = 254                                     # the last byte of the last pair
    assert device.pair_sse_u8(full, one).cpu().tolist() == [0, 1]


@pytest.mark.gpu
def test_pool2x2_is_bit_exact_on_odd_sizes_and_down_the_pyramid(cuda_device):
    """Four levels from bytes (uint8 in, then fp32 in): every level equals the fp64 restatement exactly -- the values are
    multiples of 4^-s -- with the last odd row and column dropped."""
    from tise_toolbox_amd import device
    shapes = [(2, 2), (3, 5), (37, 53), LARGEST, (177, 191)]
    pairs = [ref.smooth_pair(h, w, 25, seed=h + w) for h, w in shapes]
    lx = [_dev(p[0], cuda_device) for p in pairs]
    ly = [_dev(p[1], cuda_device) for p in pairs]
    rx, ry = [p[0] for p in pairs], [p[1] for p in pairs]
    for level in range(4):
        keep = [i for i in range(len(lx)) if min(lx[i].shape[0], lx[i].shape[1]) >= 2]
        lx, ly, rx, ry = [lx[i] for i in keep], [ly[i] for i in keep], [rx[i] for i in keep], [ry[i] for i in keep]
        lx, ly = device.pool2x2_pairs(lx, ly)
        rx, ry = [ref.pool2x2(a) for a in rx], [ref.pool2x2(a) for a in ry]
        for a, b, ra, rb in zip(lx, ly, rx, ry):
            assert tuple(a.shape) == ra.shape and a.dtype.is_floating_point and a.element_size() == 4
            assert np.array_equal(a.cpu().numpy().astype(np.float64), ra), level
            assert np.array_equal(b.cpu().numpy().astype(np.float64), rb), level
    assert len(lx) == 3 and tuple(lx[-1].shape) == (11, 11, 3)


@pytest.mark.gpu
def test_refusals(cuda_device):
    import torch
    from tise_toolbox_amd import device
    x = torch.zeros((10, 40, 3), dtype=torch.uint8, device=cuda_device)
    with pytest.raises(ValueError, match="at least 11"):
        device.ssim_pairs([x], [x])
    with pytest.raises(ValueError, match="two sizes"):
        device.ssim_pairs([torch.zeros((12, 12, 3), dtype=torch.uint8, device=cuda_device)],
                          [torch.zeros((12, 13, 3), dtype=torch.uint8, device=cuda_device)])
    with pytest.raises(ValueError, match="uint8"):
        device.pair_sse_u8([x.float()], [x.float()])
    with pytest.raises(ValueError, match="empty batch"):
        device.ssim_pairs([], [])
