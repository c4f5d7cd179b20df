"""GPU: every launch of the split trunk against fp64, and the trunk at the batch size the product uses.

Part 1 -- the launch audit.  tests/test_gpu_kernels.py checks the convolution and pool kernels one at a time with the
test's own tile width, variant and segment layout; what the TRUNK launches is decided by ``conv_split.pick_tn``, the "auto"
variant, ``korder``, ``rowwin_fits`` / ``pipe_fits`` / ``pool_output_fits`` and the segment lists written out in trunk.py, and
was only checked end to end at 2e-4 of the pool3 scale.  Here a recorder (tests/_trunk_audit.py) keeps the operands of
every launch of a 3-image forward as that launch saw them, and each launch is compared with the same operation in fp64
computed from ITS OWN recorded input, so that no error is carried from one layer into the next.  The per-kernel bounds of
the project, in one place (all taken from the kernel tests, none from what the trunk gives):

  split convolution, any variant      relu(conv2d(x, w, b)) for split (mode 0) segments, conv2d(x, w) for raw fp32 (mode 1)
                                      segments; 4e-6 x max|relu(conv2d + b)| of the launch
    pooled_input=True / "v"           max_pool2d(x, 3, 2) / three vertical taps at stride 2, then the convolution; same
    pool_output / pool_h              max_pool2d(relu(conv), 3, 2) / horizontal 3-tap max at stride 2 of relu(conv); same
    out_pad                           interior as above; the border is exactly zero
  stem kernels (fp32, u8, u8 MFMA)    relu(conv2d) of the fp32 input or of lut[u8]; 4e-6 x max|ref|
  split max pools (s2, s1p1)          max_pool2d of merge(x), -inf padding for s1p1; bit-equal after merge
  split average pools (incl. / excl.) relu(avg_pool2d(raw, 3, 1, 1, count_include_pad=...) + bias); 2e-6 x max(1, max|ref|)
  split_mean (both instances)         fp32 sequential emulation: <= 1 ulp; fp64 mean: HW x 2^-24 x mean per channel
  classifier layer (fc_logits)        pool3.double() @ W.T; 2e-6 of the logit scale

and for every launch, bit for bit: everything in every destination tensor outside the launch's own channel slice (and
outside the interior, for out_pad) is what it was before the call.
Across launches (_trunk_audit.check_assembly): every element of every tensor a launch reads was written by exactly one
earlier launch, which is what a segment offset of trunk.py that is a few channels off breaks.

The mean kernel's bound is derived, not measured: the kernel adds the HW merged values of a channel in position order into
one fp32 accumulator (v = hi + lo x 2^-11 is exact in fp32, so a fused multiply-add there changes nothing) and divides by
(float)HW once.  Against a Python loop of exactly that the result may differ by the division's rounding alone (1 ulp; bit
equality if the library divides in IEEE fashion); against the fp64 mean the textbook bound for recursive summation of
non-negative terms applies (every trunk activation is post-ReLU).

Part 2 -- batch 5000.  ``engine.DEVICE_BATCH_DEFAULT`` images per pass put nearly every activation tensor beyond 2^31
elements; the features of every image must be the bits a 250-image pass gives.
"""
import collections
import ctypes
import time

import pytest
import torch

from tests import _cases
from tests import _trunk_audit as A

pytestmark = pytest.mark.gpu

# id -> (network, --dims, environment at construction, entry point)
CONFIGS = {
    "torchvision": ("torchvision", 2048, {}, "u8"),
    "torchvision-fma-stem": ("torchvision", 2048, {"TISE_STEM": "fma"}, "u8"),
    "torchvision-fp32-input": ("torchvision", 2048, {}, "fp32"),
    "inception-2015": ("inception-2015", 2048, {}, "u8"),
    "slim": ("slim", 2048, {}, "u8"),
    "torchvision-768": ("torchvision", 768, {}, "u8"),
    "torchvision-192": ("torchvision", 192, {}, "u8"),
    "torchvision-64": ("torchvision", 64, {}, "u8"),
    "torchvision-separate-pools": ("torchvision", 2048, {"TISE_POOL_FUSE": "0"}, "u8"),
    # the documented A/B switches that reach the remaining product instances: Conv2d_2b's padded
    # kernel on the plain tensor, and both stem pools taken whole inside their consumers' operand loads
    "torchvision-plain-2b-pools-in-consumers": ("torchvision", 2048, {"TISE_CONV_PADBUF": "0", "TISE_POOL2_SPLIT": "0"}, "u8"),
    # the float route of the ADM suite: TensorFlow 1's resize on the device, the fp32 stem on the Inception-2015 weights and
    # the spatial tap behind Mixed_6d (ENGINE_KW below)
    "inception-2015-tf1-spatial": ("inception-2015", 2048, {}, "fp32"),
}
# id -> further RealismEngine arguments; the fp32 input of these is device.resize_tf1_f32 of the audit images
ENGINE_KW = {"inception-2015-tf1-spatial": dict(resize="tf1", spatial=True)}
SPATIAL_CFG = "inception-2015-tf1-spatial"
# the tap's launch, stated here and not read from the trunk: channels [0, 7) of Mixed_6d's 17 x 17 x 768 output (sblocks[6];
# Mixed_6e is sblocks[7]) into rows of 2048
TAP_SCALARS = dict(hw=289, C=768, c0=0, nc=7, ld=2048)
TAP_BLOCK = 6
CLASSES = {"torchvision": 1000, "inception-2015": 1008, "slim": 51}

# Every kernel instance the dispatchers can launch for the Inception trunk, read off csrc/conv_split.hip (tise_conv_split_f16,
# launch_rowwin_any, launch_poolin) and csrc/conv_pipe.hip (launch_regw32, launch_regw32_pool) with the tile widths
# conv_split.pick_tn returns for the trunk's Couts (tests/_trunk_audit.py instance_of names them the same way):
#   ("fast", tn, Cin % 32, K order) / ("rowwin", tn, Cin % 32, window pieces NP, POOLH) / ("poolin", TNW, taps) /
#   ("pipe34", Cout, padding, destination)
# Outside THIS trunk -- no layer of the Inception trunk on a 299 x 299 input selects them (two of them, conv_split_rowwin_kernel
# <2, 6> and <4, 5>, are product instances all the same: ResNet-50 reaches them, and tests/test_gpu_resnet_launches.py audits them
# there): conv_split_fast_kernel<1> (pick_tn gives 1 to Cout = 32 only: Conv2d_2a, which is configuration 34), its block-major
# form at tn 2, its paired-16-channel-tail steps (the 48- and 80-channel inputs feed 5x5 / 3x3 stride-1 layers: row-window kernel), conv_split_rowwin_kernel<2, 6> and
# <4, 5> (tn 2 rows are 35 wide: 5 pieces; tn 4 rows are 17 or 8 wide: 6 pieces), conv_poolin_kernel<2, VT> (the vertical-tap
# consumer is Mixed_5b: 208+ couts), conv_regw32_kernel<32, padded>; and the tools' instances: every conv_split_glds_kernel
# (the tests' reference kernel), the DBG / instrumented forms (nseg bits 0x700 / 0x800 / 0x1000).
EXPECTED_INSTANCES = {
    ("fast", 2, 0, "tap"), ("fast", 3, 0, "tap"), ("fast", 4, 0, "tap"), ("fast", 5, 0, "tap"),
    ("fast", 3, 0, "block"), ("fast", 4, 0, "block"), ("fast", 5, 0, "block"),
    ("rowwin", 2, 16, 5, ""), ("rowwin", 3, 0, 5, ""), ("rowwin", 3, 0, 6, ""), ("rowwin", 3, 16, 5, ""), ("rowwin", 4, 0, 6, ""),
    ("rowwin", 3, 16, 5, "POOLH"),
    ("poolin", 2, "9tap"), ("poolin", 4, "9tap"), ("poolin", 4, "VT"),
    ("pipe34", 32, "unpadded", "border"), ("pipe34", 32, "unpadded", "plain"), ("pipe34", 64, "padded", "plain"),
    ("pipe34", 64, "unpadded", "plain"), ("pipe34", 64, "unpadded", "pooled"),
}


class Audit:
    """What is kept of one audited forward once its tensors are gone."""

    def __init__(self):
        self.failures, self.rows, self.members, self.instances, self.sizes, self.means = [], [], [], {}, {}, []
        self.names = collections.Counter()


def _engine(network, dims, env, **kw):
    from tise_toolbox_amd.engine import RealismEngine
    from tise_toolbox_amd.trunk import SplitTrunk
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("TISE_CONV", "split")
        for k, v in env.items():
            mp.setenv(k, v)
        with A.keep_weights():
            eng = RealismEngine(dims=dims, seed=0, with_logits=dims == 2048, network=network, **kw)
    assert type(eng.fused) is SplitTrunk
    return eng


def _run_audit(cfg, dev):
    from tise_toolbox_amd import device
    network, dims, env, entry = CONFIGS[cfg]
    eng = _engine(network, dims, env, **ENGINE_KW.get(cfg, {}))
    trunk = eng.fused
    imgs = torch.as_tensor(_cases.smooth_images(3, 256, 256, seed=0), device=dev)

    # resized by the product's own kernel, outside the recording (the recorder admits the trunk's entry points only)
    if cfg in ENGINE_KW:
        x = device.resize_tf1_f32(imgs, (299, 299), 128, 2.0 ** -7, channels_last=True)
    else:
        x = device.resize_u8_only(imgs, (299, 299)) if entry == "u8" else device.resize_bilinear_u8(imgs, (299, 299), eng.lut, channels_last=True)

    def forward():
        f = trunk.forward_u8(x, eng.lut_dev) if entry == "u8" else trunk(x)
        rows = trunk._spatial_rows.clone() if trunk.spatial else None
        return f.flatten(1).clone(), (trunk.fc_logits(3).clone() if trunk.sfc is not None else None), rows
    with A.Recorder() as rec:
        feats, logits, rows = forward()
    plain = forward()
    assert tuple(feats.shape) == (3, dims) and (logits is None or tuple(logits.shape) == (3, CLASSES[network]))
    assert (rows is not None) == (cfg == SPATIAL_CFG) and (rows is None or tuple(rows.shape) == (3, TAP_SCALARS["ld"]))
    au = Audit()
    au.failures += A.check_assembly(rec.launches)
    if not (torch.equal(feats, plain[0]) and (logits is None or torch.equal(logits, plain[1])) and
            (rows is None or torch.equal(A.bits(rows), A.bits(plain[2])))):
        au.failures.append("the recorded forward and a plain one differ: recording must change nothing")
    for k, L in enumerate(rec.launches):
        au.names[L.name] += 1
        try:
            kind, fig = A.check_launch(L, trunk)
        except AssertionError as e:
            au.failures.append(f"launch {k}: {e}")
            continue
        au.rows.append((k, kind, repr(L), fig))
        if kind == "mean":
            au.means.append((L.name, L.ints[2], fig))
        if L.conv is not None:
            au.instances.setdefault(A.instance_of(L), []).append(repr(L))
    au.members = A.conv_members(rec.launches)
    au.sequence = [(L.name, repr(L)) for L in rec.launches]
    # where the launches of Mixed_6d and Mixed_6e are: the convolutions of sblocks[6] and sblocks[7] by identity
    from tise_toolbox_amd.conv_split import SplitConv
    au.block_launches = [[k for k, L in enumerate(rec.launches) if any(L.conv is c for c in trunk.sblocks[b][1].values() if isinstance(c, SplitConv))]
                         for b in (TAP_BLOCK, TAP_BLOCK + 1)] if dims == 2048 else None
    au.taps = [(k, dict(L.ints), L.in_ptr, [d[1] for d in L.dsts], rows) for k, L in enumerate(rec.launches) if L.name == A.TAP]
    au.readers = {k: L.in_ptr for k, L in enumerate(rec.launches)}
    au.writers = {k: list(L.dst_ptrs) for k, L in enumerate(rec.launches)}
    au.stems = [(3, 32, 3, 3, 2, 2, 0, 0, *L.dsts[0][1].shape[1:3]) for L in rec.launches if L.name in A.STEMS]
    au.sizes = A.tensor_sizes(rec.launches)
    au.flags = (trunk.stem_mfma, trunk.fuse_pool, trunk.pool_in_2b, trunk.pool2_split, trunk.pad2b)
    del rec, eng, trunk
    torch.cuda.empty_cache()
    return au


@pytest.fixture(scope="module")
def audits(cuda_device):
    cache = {}

    def get(cfg):
        if cfg not in cache:
            cache[cfg] = _run_audit(cfg, cuda_device)
        return cache[cfg]
    return get


# ------------------------------------------------------------------------------------------------ the launch audit
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_every_launch_matches_fp64_from_its_own_input(audits, cfg):
    """Part B of the audit for one forward: every recorded launch within its kernel's own bound of the fp64 operation on
    the launch's recorded input, nothing outside its slice of any destination touched, and the launches' slices tiling
    every tensor exactly once.  Observed on MI355X (largest error over the ten forwards, as a fraction of the bound's scale):
    convolutions 1.17e-6 (bound 4e-6), stems 5.7e-7 (4e-6), classifier layer 7.2e-7 (2e-6); average pools 1.5e-6 absolute
    (2e-6 x max(1, scale)); max pools bit-equal."""
    au = audits(cfg)
    worst = collections.defaultdict(float)
    for k, kind, name, fig in au.rows:
        if kind != "mean":
            worst[kind] = max(worst[kind], fig)
        print(f"{cfg} launch {k:3d} {kind:5s} {name}  {fig}")
    print(f"{cfg}: {sum(au.names.values())} launches {dict(au.names)}; worst per kind {dict(worst)}")
    assert not au.failures, f"{cfg}: {len(au.failures)} launches are wrong:\n" + "\n".join(au.failures)
    network, dims, env, entry = CONFIGS[cfg]
    stem_mfma, fuse_pool, pool_in_2b, pool2_split, pad2b = au.flags
    assert stem_mfma == (env.get("TISE_STEM") != "fma") and fuse_pool == (env.get("TISE_POOL_FUSE") != "0")
    stem = {"fp32": "tise_stem_conv3x3s2_split", "u8": "tise_stem_conv3x3s2_split_u8_mfma" if stem_mfma else "tise_stem_conv3x3s2_split_u8"}
    assert au.names[stem[entry]] == 1 and sum(au.names[s] for s in A.STEMS) == 1
    if env.get("TISE_POOL_FUSE") == "0" and dims == 2048:       # the stand-alone stem pools + Mixed_6a / 7a's pool branches
        assert au.names["tise_maxpool3s2_split_nhwc"] == 4
    assert au.names[A.TAP] == (1 if cfg == SPATIAL_CFG else 0)


def test_the_spatial_float_route_launches_the_u8_routes_trunk_and_one_tap(audits):
    """The engine adm_eval builds (Inception-2015, TensorFlow 1's resize, spatial) against the audited ``inception-2015``
    forward: one fp32 stem in place of the u8 one, exactly one tap, every other launch the same launch in the same order.
    The tap's scalars are the ones stated at the top of this file (not read from the trunk), its source is the buffer
    Mixed_6d's last launch wrote and Mixed_6e's first launch reads, and it sits between exactly those two: after every
    launch of sblocks[6]'s convolutions and before every launch of sblocks[7]'s, with nothing but that block boundary's
    pools beside it.  Its rows are the rows the engine hands out.  (Each launch's values: the test above.)"""
    au, base = audits(SPATIAL_CFG), audits("inception-2015")
    assert not au.failures, au.failures
    assert len(au.taps) == 1, f"{len(au.taps)} taps launched"
    k, ints, src, dsts, rows = au.taps[0]
    what = f"the tap (launch {k}: {au.sequence[k][1]})"
    rest = [s for s in au.sequence if s[0] != A.TAP]
    assert [s[0] for s in rest if s[0] in A.STEMS] == ["tise_stem_conv3x3s2_split"]
    assert [s[0] for s in base.sequence if s[0] in A.STEMS] == ["tise_stem_conv3x3s2_split_u8_mfma"]
    assert [s for s in rest if s[0] not in A.STEMS] == [s for s in base.sequence if s[0] not in A.STEMS], "the float route launches another trunk"
    assert (ints[1], ints[2], ints[3], ints[4], ints[5], ints[7]) == (3, *(TAP_SCALARS[f] for f in ("hw", "C", "c0", "nc", "ld"))), (what, ints)
    b6, b7 = au.block_launches
    assert b6 and b7 and max(b6) < k < min(b7), f"{what} is not between Mixed_6d's launches {b6} and Mixed_6e's {b7}"
    between = [au.sequence[j][0] for j in range(max(b6) + 1, min(b7)) if j != k]
    assert all("pool" in name for name in between), (what, between)
    last_writer = max(j for j in range(k) if src in au.writers[j])
    first_reader = min(j for j in range(k + 1, len(au.sequence)) if au.readers[j] == src)
    assert min(b6) <= last_writer < k, f"{what} reads a buffer Mixed_6d did not write (last written by launch {last_writer})"
    assert k < first_reader <= min(b7), f"{what} reads a buffer Mixed_6e does not read (next read by launch {first_reader})"
    assert not any(au.readers[j] == src for j in range(min(b6), k)), f"{what}: its source was read inside Mixed_6d"
    assert torch.equal(A.bits(dsts[0]), A.bits(rows)), f"{what}: the engine's rows are not what the launch wrote"


def test_every_convolution_of_the_graph_is_launched_once(audits):
    """Completeness 1: the (Cin, Cout, kernel, stride, padding, output grid) of the default network's launches -- a fused
    1x1 launch once per segment -- are exactly the 94 convolutions among pool3's ancestors in the reference listing
    (tests/golden/inception_v3_topology.json), plus the classifier layer."""
    from tests.test_topology import reference_pool3_graph
    ref = collections.Counter(op[1][:8] + op[1][10:] for op in reference_pool3_graph() if op[0] == "conv")
    assert sum(ref.values()) == 94
    want = ref + collections.Counter([(2048, 1000, 1, 1, 1, 1, 0, 0, 1, 1)])
    for cfg in ("torchvision", "torchvision-fp32-input", "torchvision-separate-pools", "torchvision-plain-2b-pools-in-consumers"):
        au = audits(cfg)
        got = collections.Counter(au.members) + collections.Counter(au.stems)
        print(f"{cfg}: {sum(got.values()) - 1} + 1 convolutions launched, {sum((got & want).values()) - 1} + 1 matched")
        assert got == want, (cfg, "missing", want - got, "unexpected", got - want)


def test_every_product_kernel_instance_is_hit(audits):
    """Completeness 2: the audited forwards together reach every convolution kernel instance the product can launch."""
    table = collections.defaultdict(set)
    for cfg in CONFIGS:
        for inst, layers in audits(cfg).instances.items():
            table[inst].update((cfg, layer) for layer in layers)
    for inst in sorted(table, key=str):
        layers = sorted({layer for _, layer in table[inst]})
        print(f"{inst}: {len(layers)} layer shapes in {sorted({c for c, _ in table[inst]})}")
        for layer in layers:
            print(f"    {layer}")
    assert set(table) == EXPECTED_INSTANCES, ("missing", EXPECTED_INSTANCES - set(table), "unexpected", set(table) - EXPECTED_INSTANCES)


def test_audit_layout_restatement_is_the_products(cuda_device):
    """The helper's own statement of the split layout against conv_split.split / merge (32-channel blocks and a 16-channel tail)."""
    from tise_toolbox_amd.conv_split import merge, split
    for C in (16, 32, 48, 80, 288):
        x = torch.randn((2, 3, C), device=cuda_device) * 3
        s = split(x)
        assert torch.equal(A.merge64(s), merge(s).double())
        m = A.raw_mask(C, 8, 24, True, cuda_device)
        probe = torch.zeros((1, C), device=cuda_device)
        probe[:, 8:24] = 1.5 + 2.0 ** -14
        assert torch.equal(split(probe)[0] != 0, m)


# ------------------------------------------------------------------------------------------------- the mean kernel
MEAN_CASES = [(64, 2048), (289, 768), (1225, 192), (1225, 288), (5329, 64)]


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("hw,C", MEAN_CASES)
def test_split_mean_is_the_sequential_fp32_sum(cuda_device, hw, C, both):
    """split_mean_kernel at the HW of the four --dims (8^2, 17^2, 35^2, 73^2) on post-ReLU-like data (a third zeros, heavy
    tail): <= 1 ulp from the fp32 emulation of its summation, within HW x 2^-24 x mean of the fp64 mean.  Observed on MI355X:
    bit-equal to the emulation (0 ulp: IEEE division) in all ten cases; fp64 error 4.7e-6 / 4.0e-6 / 6.7e-6 / 6.0e-6 / 7.7e-6
    at HW 64 / 289 / 1225 / 1225 / 5329 = 0.14 / 0.044 / 0.017 / 0.016 / 0.008 of the bound."""
    from tise_toolbox_amd import _lib
    from tise_toolbox_amd.conv_split import split
    g = torch.Generator().manual_seed(hw + C)
    x = torch.relu(torch.randn((3, hw, C), generator=g) + 0.4) ** 3 * torch.exp2(torch.randint(-6, 3, (1, 1, C), generator=g).float())
    xs = split(x.to(cuda_device)).reshape(3, hw, 1, 2 * C)
    feat = torch.full((3, C), -1.0, device=cuda_device)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr())                # noqa: E731
    if both:
        row = torch.zeros((3, 2 * C), dtype=torch.float16, device=cuda_device)
        _lib.call("tise_split_mean_both_nhwc", P(xs), 3, hw, C, P(feat), P(row), st)
        ih, il = A.split_index(C, cuda_device)
        hi = feat.half()
        assert torch.equal(row[:, ih], hi) and torch.equal(row[:, il], ((feat - hi.float()) * 2048.0).half())
    else:
        _lib.call("tise_split_mean_nhwc", P(xs), 3, hw, C, P(feat), st)
    ulps, err, ratio = A.check_mean_values(xs, hw, feat)
    print(f"split_mean{'_both' if both else ''} HW {hw} C {C}: {ulps} ulp from the fp32 emulation; fp64 error {err:.3e} = {ratio:.4f} of HW * 2^-24 * mean")


def test_split_mean_launches_of_the_trunk(audits):
    """The same two checks on the trunk's own mean launches (real activations): HW 64 (both instances: with and without the
    classifier row), 289, 1225 and 5329.  Observed on MI355X: 0 ulp from the emulation at all four; fp64 error 2.8e-7 / 6.9e-7 /
    2.8e-6 / 5.5e-6 = 0.10 / 0.038 / 0.033 / 0.013 of the bound."""
    seen = set()
    for cfg in ("torchvision", "torchvision-768", "torchvision-192", "torchvision-64"):
        au = audits(cfg)
        assert not [f for f in au.failures if "split_mean" in f], au.failures
        for name, hw, (ulps, err, ratio) in au.means:
            seen.add((name, hw))
            print(f"{cfg}: {name} HW {hw}: {ulps} ulp from the fp32 emulation; fp64 error {err:.3e} = {ratio:.4f} of the bound")
    assert seen == {("tise_split_mean_both_nhwc", 64), ("tise_split_mean_nhwc", 289), ("tise_split_mean_nhwc", 1225),
                    ("tise_split_mean_nhwc", 5329)}


# ------------------------------------------------------------------------------------------------------ batch 5000
BATCH_CASES = {"torchvision": ("torchvision", {}), "torchvision-separate-pools": ("torchvision", {"TISE_POOL_FUSE": "0"}),
               "inception-2015": ("inception-2015", {}), SPATIAL_CFG: ("inception-2015", {})}
# the tensors whose 2^31-element (fp16 split maps) or 2^32-byte (fp32 network input) mark a full device batch must pass:
# Conv2d_1a's output and Conv2d_2a's zero-bordered one, Conv2d_4a's half-pooled map, the 35 x 35 x 288 and 17 x 17 x 768 maps
EDGE_TENSORS = ["149x149x64 float16", "71x35x384 float16", "35x35x576 float16", "17x17x1536 float16"]


def _crossings(sizes):
    """{tensor: (images at which it holds more than 2^31 elements, images at which it holds more than 2^32 bytes)}"""
    return {k: (2 ** 31 // el + 1, 2 ** 32 // by + 1) for k, (el, by) in sizes.items()}


def test_a_full_device_batch_is_beyond_the_32_bit_marks(audits):
    """The batch-5000 cases below cover the edge they are there for: from the recorded launch shapes, the number of images
    at which each activation tensor passes 2^31 elements and 2^32 bytes; ``engine.DEVICE_BATCH_DEFAULT`` lies beyond every
    one of EDGE_TENSORS' marks (the last: the 17 x 17 x 768 maps at 4838 images) and beyond the fp32 network input's 4 GiB
    (4004 images).  The u8 cases never hold that input; ``inception-2015-tf1-spatial`` does: its input is ONE
    tise_resize_tf1_f32 launch of 5000 images (5.4 GB) that the fp32 stem reads whole, and its tap reads the 17 x 17 x 1536
    map past 2^31 elements.  Fails when the default batch is lowered or a layout change moves a tensor off the list."""
    from tise_toolbox_amd.engine import DEVICE_BATCH_DEFAULT as B
    sizes = dict(audits("torchvision-fp32-input").sizes)
    for cfg in BATCH_CASES:
        sizes.update(audits(cfg).sizes)
    marks = _crossings(sizes)
    for k, (e, b) in sorted(marks.items(), key=lambda kv: kv[1]):
        if min(e, b) <= 4 * B:
            print(f"{k:28s} 2^31 elements after {e:6d} images{' <= ' + str(B) if e <= B else ''}; 2^32 bytes after {b:6d}{' <= ' + str(B) if b <= B else ''}")
    for k in EDGE_TENSORS:
        assert marks[k][0] <= B, (k, marks[k], B)
    assert marks["299x299x3 float32"][1] <= B
    below = sorted(m for pair in marks.values() for m in pair if m <= B)
    above = sorted(m for pair in marks.values() for m in pair if m > B)
    print(f"largest mark within a batch of {B}: {below[-1]}; first beyond: {above[0]}")
    assert below[-1] == marks["17x17x1536 float16"][0] == 4838


def _first_last(a, b):
    rows = (a != b).flatten(1).any(1).nonzero().flatten()
    return None if rows.numel() == 0 else (int(rows[0]), int(rows[-1]), int(rows.numel()))


def _float_input(B, dev):
    """The fp32 network input of the spatial case: ONE device.resize_tf1_f32 call on B distinct 32 x 32 images (5.4 GB at
    5000: past 4 GiB, about 107 rounds of the kernel's grid-stride loop).  Every value is pinned: bit-equal to the same
    call on 250-image slices (launches of 6 rounds each, the kind tests/test_gpu_tf1_resize.py holds to the restatement
    past the grid cap), and the first and last 4 images to the restatement itself."""
    import numpy as np
    from tests import _tf1_resize_ref as tf1
    from tise_toolbox_amd import device
    src = torch.as_tensor(np.random.default_rng(5).integers(0, 256, (B, 32, 32, 3), dtype=np.uint8), device=dev)   # distinct images
    x = device.resize_tf1_f32(src, (299, 299), 128, 2.0 ** -7, channels_last=True)
    assert tuple(x.shape) == (B, 3, 299, 299) and x.numel() * 4 > 2 ** 32
    for i in range(0, B, 250):
        part = device.resize_tf1_f32(src[i:i + 250], (299, 299), 128, 2.0 ** -7, channels_last=True)
        assert torch.equal(A.bits(x[i:i + 250].permute(0, 2, 3, 1)), A.bits(part.permute(0, 2, 3, 1))), \
            f"the {B}-image resize differs from the 250-image call at images {i}..{i + 249}: first / last / count {_first_last(x[i:i + 250], part)}"
    for sl in (slice(0, 4), slice(B - 4, B)):
        want = tf1.network_input_tf1(src[sl].cpu().numpy(), (299, 299))
        got = x[sl].permute(0, 2, 3, 1).contiguous().cpu().numpy()
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), f"images {sl} of the {B}-image resize differ from the restatement"
    return x


@pytest.mark.parametrize("case", list(BATCH_CASES))
def test_batch_5000_every_image_bit_for_bit(cuda_device, case):
    """pool3 and the logits of every image of one ``engine.DEVICE_BATCH_DEFAULT``-image pass are the bits a 250-image pass
    gives (a first / last differing image names the tensor whose 32-bit mark was crossed), and at the fed paths' 1000 images
    the bits single-image passes give for the first and last 8 images.  The spatial case runs the float route: the fp32 input
    of ``_float_input`` through the fp32 stem, and the spatial rows of every pass are compared like pool3 and the logits --
    the stem reads past 2^32 bytes, and the tap strides (5000 x 2048 values) over a source past 2^31 elements."""
    import bench
    from tise_toolbox_amd import device
    from tise_toolbox_amd.engine import DEVICE_BATCH_DEFAULT as B, FEED_DEVICE_BATCH_DEFAULT as FB
    network, env = BATCH_CASES[case]
    eng = _engine(network, 2048, env, **ENGINE_KW.get(case, {}))
    trunk, lut = eng.fused, eng.lut_dev
    t0 = time.time()
    if case in ENGINE_KW:
        u8 = _float_input(B, cuda_device)                        # (B, 3, 299, 299) fp32 in channels_last storage

        def run(x):
            f = trunk(x).flatten(1).clone()
            return f, trunk.fc_logits(x.shape[0]).clone(), A.bits(trunk._spatial_rows).clone()
    else:
        u8 = torch.empty((B, 299, 299, 3), dtype=torch.uint8, device=cuda_device)
        for i in range(0, B, 500):                                   # distinct images, resized by the product's own kernel
            device.resize_u8_only(bench.synth_images_device(i, min(i + 500, B), cuda_device, seed=0), (299, 299), out=u8[i:i + 500])

        def run(x):
            f = trunk.forward_u8(x, lut).flatten(1).clone()
            return f, trunk.fc_logits(x.shape[0]).clone(), torch.empty((x.shape[0], 0), dtype=torch.int32, device=x.device)   # no rows
    try:
        full_f, full_l, full_r = run(u8)
        assert tuple(full_f.shape) == (B, 2048) and tuple(full_l.shape) == (B, CLASSES[network])
        assert tuple(full_r.shape) == (B, TAP_SCALARS["ld"] if case in ENGINE_KW else 0)
        if case in ENGINE_KW:                                    # the rows are values, not zeros, and their padding is +0
            used = TAP_SCALARS["hw"] * TAP_SCALARS["nc"]
            assert bool((full_r[:, :used] != 0).any(1).all()) and not bool(full_r[:, used:].any())
        assert bool(torch.isfinite(full_f).all()) and full_f.std(0).mean().item() > 0
        # a slice of 299 x 299 x 3 byte images starts on an odd address; the engine hands the trunk a fresh tensor per batch
        parts = [run(u8[i:i + 250].clone()) for i in range(0, B, 250)]
        part_f, part_l, part_r = (torch.cat([p[j] for p in parts]) for j in range(3))
        del parts
        assert torch.equal(full_f, part_f), f"{case}: pool3 of a {B}-image pass differs from 250-image passes: first / last / count {_first_last(full_f, part_f)}"
        assert torch.equal(full_l, part_l), f"{case}: logits differ: first / last / count {_first_last(full_l, part_l)}"
        assert torch.equal(full_r, part_r), f"{case}: the spatial rows differ: first / last / count {_first_last(full_r, part_r)}"
        fed_f, fed_l, fed_r = run(u8[:FB].clone())
        assert torch.equal(fed_f, full_f[:FB]) and torch.equal(fed_l, full_l[:FB]), _first_last(fed_f, full_f[:FB])
        assert torch.equal(fed_r, full_r[:FB]), f"{case}: the spatial rows: first / last / count {_first_last(fed_r, full_r[:FB])}"
        for i in list(range(8)) + list(range(FB - 8, FB)):
            one_f, one_l, one_r = run(u8[i:i + 1].clone())
            assert torch.equal(one_f, fed_f[i:i + 1]) and torch.equal(one_l, fed_l[i:i + 1]) and torch.equal(one_r, fed_r[i:i + 1]), (case, i)
        torch.cuda.synchronize()
        print(f"{case}: {B} images bit-identical to 20 passes of 250; {FB} to single images; {time.time() - t0:.1f} s")
    finally:
        del u8, eng, trunk
        full_f = full_l = part_f = part_l = fed_f = fed_l = full_r = part_r = fed_r = None
        torch.cuda.empty_cache()
