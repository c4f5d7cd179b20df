"""GPU: the range guard of the split-fp16 format at every writer, every lane and every launch of the trunk.

A split tensor cannot hold a value above 65504: hi becomes +inf, lo -inf, the pair merges to NaN, and the next layer's
ReLU (fmaxf) turns that into a clean, finite, WRONG activation (tests/test_gpu_nonfinite.py records it).  The only evidence
is the per-device flag every writer raises through ``tise_flag_split_overflow(vmax)`` (csrc/common.h), with ``vmax`` a
per-thread running maximum over whatever the thread happens to convert -- a register quad, a staging pass or a branch that
does not feed it changes no output bit, so no bit-identity or fp64 test can see it.

The contract, asserted by every test here (every number is exact: 65504 = 2047 * 32 = TISE_F16_MAX, 65536 = 2048 * 32
converts to +inf, a one-term split convolution is exact, the weights are pre-scaled by powers of two -- no tolerance):
  1. NO MISSED OVERFLOW.  If any value a launch STORES into a split tensor is >= 65536 before conversion, the flag is set
     after that launch.
  2. NO FALSE ALARM ON LEGAL DATA.  If every value the launch computes is <= 65504 the flag stays clear and 65504 is stored
     as (hi 65504, lo 0) -- the discarded lanes included: M-tail rows, couts beyond Cout, raw fp32 (mode 1) segments.
  3. THE FLAG IS READ-AND-CLEAR.
  4. A LAUNCH THAT WRITES ONLY fp32 NEVER TOUCHES THE FLAG: raw segments, tise_split_mean_nhwc, the classifier's logits.

Part 1 (tests/_guard_cases.py ``CASES``, the stems, split_mean): stand-alone launches with identity-like weights and a
one-hot input, so that exactly one conv output (pixel, cout) is 65536; the one-hot moves over every row of a tile, every
cout of the widest n-tile, the M tail, the second m-tile and the second destination segment -- one launch and one flag
read per position -- then the same with 2047 folded into ONE launch whose outputs are all 65504, and one launch on zeros.
Part 2 (``TrunkSweep``): every launch the trunk itself makes -- its own tile width, variant, K order, segment list and
``out_pad`` -- is run with one bias entry at 7e4, for the first and last cout of each of its segments.
Part 3: the library entry points that hand out trunk features all end in ``check_numerics``.

Recorded, not contracted (``test_record_...``, as tests/test_gpu_nonfinite.py names its records): the kernels take ``vmax``
BEFORE the store mask, so a value that is computed but never stored -- a grid pixel of configuration 34 whose window wraps
into the next image row, a conv column no 3-wide stride-2 window covers -- raises the flag although every stored value is
legal.  That is conservative (the job reruns on the exact path, no wrong number leaves) and masking it would cost
instructions in the hottest epilogues; the tests assert what the kernels do today.

Found by these tests: ``RealismEngine.statistics()`` / ``inception_score()`` read AND CLEAR the flag, while the accumulators
keep the poisoned rows: after one of the two had raised, the other returned a wrong number silently.  The engine now
remembers the hit until the next ``begin()``.  No kernel was found dropping a lane: the epilogues are unchanged.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import _cases
from tests import _guard_cases as G
from tests import _trunk_audit as A
from tests.test_gpu_trunk_launches import CONFIGS, EXPECTED_INSTANCES, _engine

pytestmark = pytest.mark.gpu

TRUNK_CONFIGS = ["torchvision", "torchvision-fma-stem", "inception-2015", "slim", "torchvision-separate-pools",
                 "torchvision-plain-2b-pools-in-consumers"]


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def call(name, *args):
    from tise_toolbox_amd import _lib
    return _lib.call(name, *args)


def flag():
    from tise_toolbox_amd import device
    return device.read_split_overflow()


# ================================================================================================ Part 1: convolutions
def test_the_guard_cases_cover_every_instance_of_the_product_and_of_the_audits_outside_list():
    """The module's instance list is EXPECTED_INSTANCES of tests/test_gpu_trunk_launches.py plus the instances that file lists
    as outside the Inception trunk (two of them ResNet-50's): a new instance there without a guard case here fails.  (Cases marked ``extra`` --
    another Cin % 32 or destination of a template instance already on the list, the POOLH form at six window pieces -- come
    on top and are not on either list.)"""
    required = {c.key for c in G.CASES.values() if not c.extra}
    union = EXPECTED_INSTANCES | G.OUTSIDE
    assert required == union, ("no guard case", union - required, "not an instance of either list", required - union)
    assert not ({c.key for c in G.CASES.values() if c.extra} & union)


@pytest.mark.parametrize("name", list(G.CASES))
def test_one_hot_overflow_reaches_the_flag_from_every_row_and_cout(cuda_device, name):
    """Contract 1-4 for one kernel instance (tests/_guard_cases.py): the dispatch is the instance's, zeros and the all-65504
    launch leave the flag clear and store (65504, 0) exactly, and a single 65536 raises it from every row of a tile, every
    cout, the M tail, the second tile and the second destination segment -- a raw fp32 segment never."""
    case = G.CASES[name]
    bad, launches = G.run_case(case, cuda_device)
    print(f"{name} {case.key}: {launches} one-hot launches, {len(bad)} failures")
    assert not bad, f"{name}: {len(bad)} failures:\n" + "\n".join(bad[:40])


# ---------------------------------------------------------------------------------------------------------- the stems
STEM_SHAPE = (2, 19, 19)          # -> 2 x 9 x 9 = 162 pixels x 4 threads: two full 256-thread workgroups and a partly dead third
STEM_W, STEM_BYTE_LEGAL, STEM_BYTE_OVER, STEM_BIAS_LEGAL = 512.0, 127, 128, 480.0     # 127 * 512 + 480 = 65504, 128 * 512 = 65536


def _stem_tap(c):
    t = c % 27                                                    # (kh, kw, cin): a tap that varies with the cout
    return t // 9, (t % 9) // 3, t % 3


def _stem_weight(couts):
    w = torch.zeros((32, 3, 3, 3))
    for c in couts:
        kh, kw, ci = _stem_tap(c)
        w[c, ci, kh, kw] = STEM_W
    return w


def _stem_runner(entry, dev):
    """-> run(weight key, bias, input) for one of the three entry points; weights packed once per key."""
    from tise_toolbox_amd.trunk import pack_stem_mfma
    n, h, w = STEM_SHAPE
    lut = torch.arange(256, dtype=torch.float32).repeat(3).to(dev)            # lut[b] = b: a background of exactly 0
    packed = {}
    for key in ["all"] + list(range(32)):
        wt = _stem_weight(range(32) if key == "all" else [key])
        packed[key] = pack_stem_mfma(wt, dev) if entry == "mfma" else (wt.permute(2, 3, 1, 0).contiguous().to(dev),)
    out = torch.zeros((n, 9, 9, 64), dtype=torch.float16, device=dev)

    def run(key, bias, x):
        if entry == "fp32":
            call("tise_stem_conv3x3s2_split", P(x), n, h, w, P(packed[key][0]), P(bias), P(out), st())
        elif entry == "u8":
            call("tise_stem_conv3x3s2_split_u8", P(x), P(lut), n, h, w, P(packed[key][0]), P(bias), P(out), st())
        else:
            call("tise_stem_conv3x3s2_split_u8_mfma", P(x), P(lut), n, h, w, P(packed[key][0]), P(packed[key][1]), P(bias), P(out), st())
        return out
    return run


@pytest.mark.parametrize("entry", ["fp32", "u8", "mfma"])
def test_stem_one_hot_overflow_reaches_the_flag_from_every_pixel_and_cout(cuda_device, entry):
    """The three stem entry points: one weight of 512 per cout on a tap that varies with the cout, a table lut[b] = b.  Byte
    127 everywhere with a bias of 480 stores 65504 exactly in all 162 x 32 outputs without a flag; ONE byte of 128 under the
    weights of ONE cout stores one 65536 and must raise it -- for every cout, and for every pixel of the first, the second
    and the partly dead last workgroup."""
    dev = cuda_device
    n, h, w = STEM_SHAPE
    run = _stem_runner(entry, dev)
    dt = torch.float32 if entry == "fp32" else torch.uint8
    zero_bias = torch.zeros(32, device=dev)
    x = torch.zeros((n, h, w, 3), dtype=dt, device=dev)
    flag()
    out = run("all", zero_bias, x)
    assert not flag() and not bool(out.any())
    out = run("all", torch.full((32,), STEM_BIAS_LEGAL, device=dev), torch.full((n, h, w, 3), STEM_BYTE_LEGAL, dtype=dt, device=dev))
    assert not flag(), "FALSE ALARM: every output is 65504"
    assert bool((out[..., :32] == G.F16_MAX).all()) and not bool(out[..., 32:].any()), "65504 is stored as (hi 65504, lo 0)"
    pixels = n * 9 * 9
    positions = [(p, (7 * p + 3) % 32) for p in range(pixels)] + [((11 * c + 5) % pixels, c) for c in range(32)]
    bad = []
    for p, c in positions:
        img, rem = divmod(p, 81)
        oy, ox = divmod(rem, 9)
        kh, kw, ci = _stem_tap(c)
        x[img, 2 * oy + kh, 2 * ox + kw, ci] = STEM_BYTE_OVER
        out = run(c, zero_bias, x)
        f = flag()
        x[img, 2 * oy + kh, 2 * ox + kw, ci] = 0
        infs = int(torch.isinf(out).sum())
        if infs != 2 or not f:
            bad.append(f"pixel {p} cout {c}: {infs} infinite halves stored (2 expected), flag {f}")
    assert not flag()
    assert not bad, f"stem {entry}: {len(bad)} of {len(positions)} positions:\n" + "\n".join(bad[:40])


# --------------------------------------------------------------------------------------------------------- split_mean
def test_split_mean_one_channel_above_range_reaches_the_flag_from_every_channel_of_a_thread(cuda_device):
    """split_mean_kernel<true> (thread = image x 8 channels, 256 threads per workgroup) at C = 2112: 264 threads, the last
    workgroup has eight.  A channel whose HW positions all hold (hi 65504, lo 65504) has the mean 65535.98: the flag must rise
    for each of the eight channels of the first thread, of the first and of the last thread of the partial workgroup; with
    (65504, 0) everywhere the mean is 65504 exactly, stored as (65504, 0), no flag.  The fp32 kernel never touches the flag."""
    dev = cuda_device
    n, hw, C = 2, 4, 2112
    x = torch.zeros((n, hw, 2 * C), dtype=torch.float16, device=dev)
    feat = torch.zeros((n, C), dtype=torch.float32, device=dev)
    row = torch.zeros((n, 2 * C), dtype=torch.float16, device=dev)

    def both():
        call("tise_split_mean_both_nhwc", P(x), n, hw, C, P(feat), P(row), st())
    flag()
    both()
    assert not flag() and not bool(row.any())
    ih, il = A.split_index(C, dev)
    x[:, :, ih] = G.F16_MAX
    both()
    assert not flag(), "FALSE ALARM: every mean is 65504"
    assert bool((feat == G.F16_MAX).all()) and bool((row[:, ih] == G.F16_MAX).all()) and not bool(row[:, il].any())
    x.zero_()
    bad = []
    for c in list(range(8)) + list(range(2048, 2056)) + list(range(C - 8, C)):
        img = c % n
        x[img, :, [G.hi_pos(c, C), G.lo_pos(c, C)]] = G.F16_MAX
        both()
        f = flag()
        call("tise_split_mean_nhwc", P(x), n, hw, C, P(feat), st())
        f32 = flag()
        x[img, :, [G.hi_pos(c, C), G.lo_pos(c, C)]] = 0.0
        if not f or int(torch.isinf(row).sum()) != 2:
            bad.append(f"channel {c}: flag {f}, {int(torch.isinf(row).sum())} infinite halves (2 expected)")
        if f32 or float(feat[img, c]) != G.F16_MAX + G.F16_MAX / 2048.0:
            bad.append(f"channel {c}: the fp32 kernel raised the flag ({f32}) or stored {float(feat[img, c])!r}")
    assert not flag()
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------- recorded, not contracted
def _record(case, dev, plant, weight=None):
    """One launch of ``case`` on zeros with ``plant`` = [(n, y, x, channel, value)] -> (destination tensors, flag)."""
    from tise_toolbox_amd.conv_split import SplitConv
    if weight is None:
        conv = case.build(dev)
    else:
        conv = SplitConv(weight.to(dev), torch.zeros(case.cout, device=dev), (1, 1), case.pad, dev, **case.ctor)
    segs, tens, kw = case.destinations(dev)
    n, h, w = case.shape
    x = torch.zeros((n, h, w, 2 * case.cin), dtype=torch.float16, device=dev)
    for pn, y, xx, ch, v in plant:
        x[pn, y, xx, G.hi_pos(ch, case.cin)] = v
    flag()
    with G.conv_spy() as seen:
        conv(x, segs, **kw)
    assert A.instance_of(seen[0]) == case.key and conv._fallback is None
    return tens, flag()


def _all_ones(case):
    w = torch.zeros((case.cout, case.cin, 3, 3))
    for c in range(case.cout):
        w[c, c % case.cin] = 1.0
    return w


@pytest.mark.parametrize("name", ["pipe34-32-unpadded-plain", "pipe34-64-pooled"])
def test_record_grid_kernel_flags_a_window_that_wraps_into_the_next_image_row(cuda_device, name):
    """NOT a contract: configuration 34 computes one result per pixel of the INPUT grid; at a grid pixel with x >= OW the 3 x 3
    window runs over the row end into the next image row, and the result is masked at the store -- after ``vmax``.  Two
    values of 40000, the last pixel of a row and the first of the next, under all-ones taps: no output window holds both (every
    stored value is at most 40000), the wrapped window sums them to 80000, and the flag rises."""
    case = G.CASES[name]
    n, h, w = case.shape
    tens, f = _record(case, cuda_device, [(0, 1, w - 1, 5, 40000.0), (0, 2, 0, 5, 40000.0)], _all_ones(case))
    got = A.merge64(tens[0])
    assert bool(torch.isfinite(got).all()) and got.max().item() == 40000.0
    print(f"{name}: largest stored value {got.max().item()}, flag {f}")
    assert f is True, "the kernel takes vmax before the store mask (conservative); a change here is a decision, not an accident"
    assert not flag()


@pytest.mark.parametrize("name", ["rowwin3-np6-cin96-poolh", "pipe34-64-pooled"])
def test_record_pooled_epilogue_flags_a_column_no_window_covers(cuda_device, name):
    """NOT a contract: with an even OW the last conv column belongs to no 3-wide stride-2 window, so the pooled epilogues compute
    it and never store it -- ``vmax`` is taken over all conv results.  A one-hot 65536 in that column: every stored value is
    zero, and the flag rises."""
    case = G.CASES[name]
    oh, ow = case.conv_hw()
    assert ow % 2 == 0 and G.windows(ow - 1, ow) == 0
    tens, f = _record(case, cuda_device, [(*case.source(0, 0, ow - 1, 3), G.X_OVER)])
    assert not bool(tens[0].any()), "nothing of the uncovered column is stored"
    print(f"{name}: conv column {ow - 1} of {ow}: flag {f}")
    assert f is True, "the kernel takes vmax over every conv result (conservative); a change here is a decision, not an accident"
    assert not flag()


# ==================================================================================================== Part 2: the trunk
def _forward_of(eng, dev):
    from tise_toolbox_amd import device
    x = device.resize_u8_only(torch.as_tensor(_cases.smooth_images(1, 256, 256, seed=0), device=dev), (299, 299))
    trunk = eng.fused

    def forward():
        f = trunk.forward_u8(x, eng.lut_dev).flatten(1).clone()
        return f, trunk.fc_logits(1).clone()
    return forward


@pytest.mark.parametrize("cfg", TRUNK_CONFIGS)
def test_every_split_writer_the_trunk_launches_raises_the_flag_at_its_own_launch(cuda_device, cfg):
    """A 1-image forward with ``_lib.call`` interposed (tests/_guard_cases.py TrunkSweep): every launch that writes a split
    tensor -- convolutions with a mode-0 segment, the stem, the average-pool tails, the pool3 mean -- is run with ONE bias
    entry at 7e4 (the mean: one channel at 65535.98), the flag clear before and set after exactly that launch, for the first
    and last cout of each split segment; raw segments, the classifier layer and tise_split_mean_nhwc leave it clear; the
    untouched launch leaves it clear; the forward gives the bits it gave before the sweep."""
    network, dims, env, entry = CONFIGS[cfg]
    assert entry == "u8" and dims == 2048
    eng = _engine(network, dims, env)
    forward = _forward_of(eng, cuda_device)
    flag()
    before = forward()
    assert not flag()
    with G.TrunkSweep() as sw:
        swept = forward()
    after = forward()
    assert not flag(), "the flag after the sweep's untouched forward"
    for a, b in zip(before, swept):
        assert torch.equal(a, b), "the swept forward ends with the untouched launches: the same bits"
    for a, b in zip(before, after):
        assert torch.equal(a, b), "the forward after the sweep gives the bits it gave before"
    convs = sw.names.count("tise_conv_split_f16")
    print(f"{cfg}: {len(sw.names)} launches ({convs} convolutions), {sw.targets} targeted launches had to raise the flag, "
          f"{sw.silent} had to leave it clear, {len(sw.failures)} failures")
    assert not sw.failures, f"{cfg}: {len(sw.failures)} failures:\n" + "\n".join(sw.failures[:40])
    assert sum(sw.names.count(s) for s in G.STEM_BIAS) == 1 and sw.names.count("tise_split_mean_both_nhwc") == 1
    avgs = sum(sw.names.count(s) for s in G.AVG_BIAS)
    assert avgs in (8, 9)                                              # the pool branch of Mixed_5b .. 7c (the 2015 graph's 7c takes a max-pool)
    assert convs >= 60 and sw.targets >= 2 * (convs - 1) + 2 * avgs + 4 and sw.silent >= 2 + 2 * avgs + 2
    del eng
    torch.cuda.empty_cache()


def test_a_launch_the_sweep_does_not_know_is_an_error(cuda_device):
    """A future writer cannot slip past: as in the launch recorder, an unknown entry point reached under the interposer fails."""
    from tise_toolbox_amd import _lib
    with G.TrunkSweep():
        with pytest.raises(AssertionError, match="does not know"):
            _lib.call("tise_some_future_split_writer")
    assert _lib.call.__module__ == _lib.__name__                      # the interposer is gone


@pytest.mark.parametrize("network", ["torchvision", "inception-2015", "slim"])
def test_engine_raises_from_both_accessors_and_recovers_after_begin(cuda_device, network):
    """Engine level: a bias of the last block's fused 1x1 launch at 7e4 during one step_u8 -- statistics() AND inception_score()
    of that image set raise FloatingPointError (the flag is read-and-clear, the accumulators are not: the engine remembers the
    hit until begin()); the next begin() / step_u8 on the same engine with the bias restored gives the bits of a fresh engine."""
    from tise_toolbox_amd.conv_split import SplitConv
    imgs = torch.as_tensor(_cases.smooth_images(20, 64, 64, seed=5), device=cuda_device)

    def run(eng):
        eng.begin(n_total=20)
        f = eng.step_u8(imgs, 0).clone()
        mu, sigma = eng.statistics()
        return f, mu.clone(), sigma.clone(), np.asarray(eng.inception_score(), dtype=np.float64)
    want = run(_engine(network, 2048, {}))
    eng = _engine(network, 2048, {})
    late = eng.fused.sblocks[-1][1]["f"]
    assert isinstance(late, SplitConv)
    flag()
    eng.begin(n_total=20)
    with G.blown_bias(late, late.cout // 2):
        eng.step_u8(imgs, 0)
    with pytest.raises(FloatingPointError, match="fp16 range"):
        eng.statistics()
    with pytest.raises(FloatingPointError, match="fp16 range"):
        eng.inception_score()
    with pytest.raises(FloatingPointError, match="fp16 range"):
        eng.statistics()
    got = run(eng)
    for a, b in zip(want[:3], got[:3]):
        assert torch.equal(a, b)
    assert np.array_equal(want[3], got[3], equal_nan=True)
    assert not flag()


# ======================================================================================== Part 3: library entry points
BLOWN_LAYERS = {"early": ("Conv2d_2b_3x3.bn.weight", 3.0e4), "Mixed_7c": ("Mixed_7c.branch1x1.bn.weight", 1.0e7)}


@pytest.fixture(scope="module")
def blown(tmp_path_factory):
    """Stand-in checkpoints (1000 and 80 classes) with ONE BatchNorm scale blown up, and 8 PNG files of 64 x 64."""
    from PIL import Image
    from tise_toolbox_amd.inception import build_inception3
    root = tmp_path_factory.mktemp("range_guard")
    ck = {}
    for classes, kw in ((1000, {}), (80, dict(num_classes=80, calibration="pm1"))):
        sd = {k: v.clone() for k, v in build_inception3(seed=0, **kw).state_dict().items()}
        for layer, (key, factor) in BLOWN_LAYERS.items():
            sd2 = dict(sd)
            sd2[key] = sd[key] * factor
            ck[layer, classes] = str(root / f"blown_{layer}_{classes}.pth")
            torch.save(sd2, ck[layer, classes])
    imgs = _cases.smooth_images(8, 64, 64, seed=11)
    d = root / "imgs"
    d.mkdir()
    for i, im in enumerate(imgs):
        Image.fromarray(im).save(d / f"img{i:03d}_person_{i}.png")
    return dict(ck=ck, imgs=imgs, dir=str(d), files=sorted(str(p) for p in d.iterdir()))


def _reset_is_engine():
    from tise_toolbox_amd import inception_score as isc
    isc.configure(weights=None, num_classes=None, seed=0, rule="coco", drop_first_class=False, fc_bias="auto", batch_size=50,
                  network="torchvision")


@pytest.mark.parametrize("layer", list(BLOWN_LAYERS))
@pytest.mark.parametrize("entry", ["get_activations", "calculate_activation_statistics", "get_inception_score", "ois_inception_score",
                                   "collect_logits"])
def test_library_entry_points_raise_instead_of_returning_features(cuda_device, blown, monkeypatch, entry, layer):
    """The library functions (not the CLIs: nothing reruns on the exact path) on a checkpoint whose activations leave the
    fp16 range in an early layer / in Mixed_7c: each raises FloatingPointError, none returns a value."""
    from tise_toolbox_amd import calibration, fid_score, inception_score as isc, object_centric_inception_score as ois
    from tise_toolbox_amd.inception import InceptionV3
    monkeypatch.setenv("TISE_CONV", "split")
    ck = blown["ck"]
    flag()
    result = None
    try:
        with pytest.raises(FloatingPointError, match="fp16 range"):
            if entry in ("get_activations", "calculate_activation_statistics"):
                model = InceptionV3([3], weights=ck[layer, 1000]).cuda()
                batches = [torch.from_numpy(blown["imgs"][i:i + 4]) for i in (0, 4)]
                result = getattr(fid_score, entry)(batches, model, batch_size=4, dims=2048, cuda=True, verbose=False)
            elif entry == "get_inception_score":
                isc.configure(weights=ck[layer, 1000], batch_size=4)
                result = isc.get_inception_score(blown["files"], splits=2)
            elif entry == "collect_logits":
                result = calibration.collect_logits(blown["files"], weights=ck[layer, 1000], batch_size=4)
            else:
                result = ois.inception_score(ois.IgnoreLabelDataset(blown["dir"]), cuda=True, batch_size=4, splits=1,
                                             weights=ck[layer, 80])
    finally:
        _reset_is_engine()
        for key in [k for k in ois._ENGINES if k[0] in ck.values()]:
            del ois._ENGINES[key]
    assert result is None
    assert not flag(), "check_numerics read and cleared the flag"
