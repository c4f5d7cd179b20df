"""GPU: every launch of the ResNet-50 trunk (resnet_hip.py) and of CountSeg on it (countseg_hip.py) against fp64.

tests/test_gpu_resnet.py and tests/test_gpu_countseg.py hold the routes end to end, at four times the fp32 module's own distance
from fp64 per feature row; tests/test_gpu_resnet_kernels.py checks the kernels one at a time with the test's own shapes.  What the
ROUTE launches -- the tile width from ``conv_split.pick_tn``, the "auto" variant, the row-window kernel's fall-back on short rows,
the segment lists and leading dimensions written out in resnet_hip.py -- is checked here as the Inception trunk's launches are in
tests/test_gpu_trunk_launches.py: the recorder of tests/_trunk_audit.py keeps the operands of every launch of one forward as that
launch saw them, and each launch is compared with the same operation computed from ITS OWN recorded input and the module's
ORIGINAL parameters (``resnet_model.ResNet50.folded()``, the CountSeg module's head), so that no error is carried from one layer
into the next.  The bounds are the project's own, none new:

  7 x 7 stem (matrix cores)            relu(conv2d(table[u8], w, b, 2, 3)) in fp64; 4e-6 x max|ref|
  resnet_input_split (route "padded")  the split of the table values in channels 0..2, +0 elsewhere; bit for bit
  SplitConv, split segments            relu(conv2d(x, w, b)); 4e-6 x max|ref| of the launch
  SplitConv, fp32 segments             conv2d(x, w), no bias (conv3, the downsample convolution, CountSeg's mix); 4e-6 x max|ref|
  3 x 3 / s2 / p1 max pool             max_pool2d(merge(x), 3, 2, 1); equal after merge
  residual add + ReLU                  split(relu((raw + bias) + u)) in fp32 torch operations, u = merge(identity) or id_raw + id_bias;
                                       bit for bit, and the range guard is clear after the launch
  mean                                 fp32 sequential emulation: <= 1 ulp; fp64 mean: HW x 2^-24 x mean per channel
  CountSeg head                        tests/_countseg_ref.head on the recorded fp32 map: confidences, density means and peak
                                       counts bit for bit

and for every launch, bit for bit: everything in every destination outside the launch's own slice is what it was before the
call.  Across launches (_trunk_audit.check_assembly): every element of every tensor a launch reads -- the residual launch reads
two -- was written by exactly one earlier launch.  Each forward is also run unrecorded and gives the same bits.

Observed on MI355X (largest figure over the seven forwards, as a fraction of the bound's scale): convolutions into split
segments 1.22e-6 (layer4.0's 3 x 3 / stride 2 at 224 x 224; bound 4e-6), convolutions into fp32 segments 7.4e-7 (CountSeg's
mix at 14 x 14; 4e-6), the
matrix-core stem 2.7e-7 (4e-6); input split, pool, the 112 residual launches and both heads bit-equal, every guard clear; the mean
0 ulp from the fp32 emulation at HW 1, 4, 9 and 49, fp64 error 7.2e-7 / 2.2e-6 / 4.5e-6 at HW 4 / 9 / 49 = 0.50 / 0.37 / 0.13 of
HW x 2^-24 x mean.  71 launches per ResNet-50 forward (72 on the padded-stem route and for CountSeg): 53 convolutions with the
stem, 54 for CountSeg.  No launch was found wrong.
"""
import collections

import pytest
import torch

from tests import _countseg_ref as R
from tests import _trunk_audit as A

pytestmark = pytest.mark.gpu

# id -> (route, H, W, images, stem).  The sizes are the smallest that reach each kernel instance and fall-back width (SIZE_TABLE);
# 33 x 47 is odd at every halving.
CONFIGS = {
    "32x32x2": ("resnet", 32, 32, 2, "mfma"),
    "33x47x3": ("resnet", 33, 47, 3, "mfma"),
    "96x96x2": ("resnet", 96, 96, 2, "mfma"),
    "224x224x2": ("resnet", 224, 224, 2, "mfma"),
    "33x47x2-padded-stem": ("resnet", 33, 47, 2, "padded"),
    "countseg-160x128x2": ("countseg", 160, 128, 2, "mfma"),          # map 5 x 4
    "countseg-448x448x1": ("countseg", 448, 448, 1, "mfma"),          # map 14 x 14: the size CA runs at
}

# Every convolution kernel instance the two routes launch, in _trunk_audit.instance_of's form: pick_tn gives tile width 2 to
# Cout 64 and 4 to every other Cout of the network (128, 240, 256, 512, 1024, 2048); the 1 x 1 and the stride-2 layers, the
# padded-stem route's 7 x 7 layer and the row-window kernel's fall-backs take the default kernel in tap-major K order, the
# 3 x 3 / stride 1 layers the row-window kernel with five or six window pieces by their row width.
EXPECTED_INSTANCES = {
    ("fast", 2, 0, "tap"), ("fast", 4, 0, "tap"),
    ("rowwin", 2, 0, 5, ""), ("rowwin", 2, 0, 6, ""), ("rowwin", 4, 0, 5, ""), ("rowwin", 4, 0, 6, ""),
}

# (H, W) -> ({(tile width, window pieces): row-window launches}, {row width: 3 x 3 / s1 launches on the default kernel through
# ``_fallback``}) of the 16 3 x 3 layers with stride 1 (the three with stride 2 always take the default kernel).  Written out
# here, held against conv_split.py's own functions on the CPU (test_the_dispatch_per_size) and against what each audited
# forward launched: a change of dispatch shows up in both.
SIZE_TABLE = {
    (32, 32): ({(2, 6): 3}, {4: 3, 2: 5, 1: 2}),
    (33, 47): ({(2, 5): 3, (4, 6): 3}, {3: 5, 2: 2}),
    (96, 96): ({(2, 5): 3, (4, 5): 3, (4, 6): 5}, {3: 2}),
    (160, 128): ({(2, 5): 3, (4, 5): 3, (4, 6): 5}, {4: 2}),
    (224, 224): ({(2, 5): 3, (4, 5): 8, (4, 6): 2}, {}),
    (448, 448): ({(2, 5): 3, (4, 5): 10}, {}),
}


class Audit:
    """What is kept of one audited forward once its tensors are gone."""

    def __init__(self):
        self.failures, self.rows, self.members, self.instances = [], [], [], {}       # failures: (launch or None, message)
        self.names = collections.Counter()
        self.rowwin, self.fallback = collections.Counter(), collections.Counter()
        self.fallback_launches = []
        self.layer_launch, self.residual_launch, self.sequence = {}, [], []


def _run_audit(cfg, dev, mutate=None):
    from tise_toolbox_amd import countseg_hip, countseg_model, resnet_hip, resnet_model
    route, h, w, n, stem = CONFIGS[cfg]
    with pytest.MonkeyPatch.context() as mp:
        for k in ("TISE_RESNET_STEM", "TISE_CONV_VARIANT", "TISE_CONV_KORDER"):
            mp.delenv(k, raising=False)
        counter = head = None
        if route == "resnet":
            model = resnet_model.ResNet50().init_synthetic(0)
            tower = resnet_hip.HipResNet50(model, dev, stem=stem)
        else:
            head = countseg_model.CountSeg().init_synthetic(0)
            counter = countseg_hip.HipCountSeg(head, dev)
            tower, model = counter.trunk, head.trunk
    assert tower.stem == stem
    if mutate is not None:
        mutate(tower)
    img = torch.as_tensor(R.images(n, h, w, seed=1000 * h + w)).to(dev)

    def forward():
        if counter is None:
            return (tower.features_from_u8(img).clone(),)
        return counter.rows_from_u8(img).clone(), counter.last_peaks.clone()
    with A.Recorder() as rec:
        out = forward()
    plain = forward()
    assert tower.last_stem == stem
    assert tuple(out[0].shape) == ((n, 2048) if counter is None else (n, 160))
    au = Audit()
    au.failures += [(None, f) for f in A.check_assembly(rec.launches)]
    if not all(torch.equal(A.bits(a), A.bits(b)) for a, b in zip(out, plain)):
        au.failures.append((None, "the recorded forward and a plain one differ: recording must change nothing"))
    au.guard_reads = rec.guard_reads
    refs = A.ResNetRefs(model, tower, dev, counter, head)
    for k, L in enumerate(rec.launches):
        au.names[L.name] += 1
        au.sequence.append(L.name)
        if L.name == A.RESIDUAL:
            au.residual_launch.append(k)
        if L.conv is not None:
            layer, fell_back = refs.layer_of(L.conv)
            inst = A.instance_of(L)
            au.layer_launch[layer] = k
            au.instances.setdefault(inst, []).append(f"{layer}: {L!r}")
            c = L.conv
            if inst[0] == "rowwin":
                au.rowwin[(inst[1], inst[3])] += 1
            if fell_back:
                au.fallback[L.args["OW"]] += 1
                au.fallback_launches.append((layer, L.args["OW"], inst, (c.kh, c.kw, c.stride, c.padding)))
        try:
            kind, fig = A.check_resnet_launch(L, refs, block=len(au.residual_launch) - 1)
        except AssertionError as e:
            au.failures.append((k, f"launch {k}: {e}"))
            continue
        au.rows.append((k, kind, repr(L), fig))
    au.members = A.conv_members(rec.launches)
    au.stems = [(3, 64, 7, 7, 2, 2, 3, 3, *L.dsts[0][1].shape[1:3]) for L in rec.launches if L.name == A.STEM7]
    au.module = A.module_convs(model, h, w)
    del rec, refs, tower, counter
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
def test_every_launch_matches_its_reference_from_its_own_input(audits, cfg):
    """Every recorded launch of one forward within its kernel's own bound of the reference on the launch's recorded input, nothing
    outside its slice of any destination touched, every tensor read written exactly once, the recorded forward bit-equal to a
    plain one; and the row-window launches and fall-backs are SIZE_TABLE's for this size.  The figures: this file's docstring."""
    au = audits(cfg)
    route, h, w, n, stem = CONFIGS[cfg]
    worst = collections.defaultdict(float)
    for k, kind, name, fig in au.rows:
        worst[kind] = max(worst[kind], fig[2] if kind == "mean" else fig)
        print(f"{cfg} launch {k:3d} {kind:8s} {name}  {fig}")
    print(f"{cfg}: {sum(au.names.values())} launches {dict(au.names)}; worst per kind {dict(worst)} (mean: of its bound)")
    assert not au.failures, f"{cfg}: {len(au.failures)} launches are wrong:\n" + "\n".join(m for _, m in au.failures)
    assert len(au.rows) == sum(au.names.values())
    assert au.guard_reads == (1 if route == "resnet" else 2)             # the route's own reads of the range guard, once per call
    assert (dict(au.rowwin), dict(au.fallback)) == SIZE_TABLE[(h, w)], (cfg, dict(au.rowwin), dict(au.fallback))


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_the_launches_are_the_modules_graph(audits, cfg):
    """The convolutions launched, as (Cin, Cout, kernel, stride, padding, output grid), plus the stem, are exactly the 53
    ``nn.Conv2d`` of the torch module with the size arithmetic (_trunk_audit.module_convs) -- CountSeg adds its one mix
    convolution -- in the module's order: per block conv1, conv2, conv3, the downsample convolution where there is one, one
    residual launch.  16 residual launches, one pool; one mean (ResNet-50) or one head and no mean (CountSeg); the stem is one
    matrix-core launch, or resnet_input_split and a 32-channel convolution on the padded-stem route."""
    au = audits(cfg)
    route, h, w, n, stem = CONFIGS[cfg]
    assert not au.failures, au.failures
    oh, ow = au.module[-1][8:]
    want = collections.Counter(au.module)
    assert sum(want.values()) == 53
    if route == "countseg":
        want[(2048, 240, 1, 1, 1, 1, 0, 0, oh, ow)] += 1
    launched = list(au.members)
    if stem == "padded":                                                 # conv1 as a 32-channel layer: 29 zero input channels
        at = [j for j, m in enumerate(launched) if m[:4] == (32, 64, 7, 7)]
        assert at == [0], at
        launched[0] = (3,) + launched[0][1:]
    got = collections.Counter(launched) + collections.Counter(au.stems)
    print(f"{cfg}: {sum(got.values())} convolutions launched, {sum((got & want).values())} of the module's {sum(want.values())} matched")
    assert got == want, (cfg, "missing", want - got, "unexpected", got - want)
    conv, res = "tise_conv_split_f16", A.RESIDUAL
    first = [A.STEM7] if stem == "mfma" else [A.INPUT_SPLIT, conv]
    blocks = []
    for j in range(16):
        blocks += [conv] * (4 if j in (0, 3, 7, 13) else 3) + [res]      # the first block of a layer has the downsample convolution
    last = ["tise_split_mean_nhwc"] if route == "resnet" else [conv, A.HEAD]
    assert au.sequence == first + ["tise_maxpool3s2p1_split_nhwc"] + blocks + last, au.sequence
    assert au.names[res] == 16 and au.names["tise_maxpool3s2p1_split_nhwc"] == 1
    assert au.names[conv] == (52 if stem == "mfma" else 53) + (1 if route == "countseg" else 0)


def test_every_kernel_instance_of_the_routes_is_hit(audits):
    """The audited forwards together reach exactly EXPECTED_INSTANCES."""
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


def test_short_rows_fall_back_to_the_default_kernel(audits):
    """The 3 x 3 / stride 1 layers whose output rows are 1 to 4 pixels wide -- the row-window kernel's window would need seven
    pieces per wave -- run on the default kernel through ``SplitConv._fallback``, with the layer's tile width, in tap-major K
    order; no other layer falls back.  (Their values: the audit above, which checks a fall-back launch like any other.)"""
    widths = set()
    for cfg in CONFIGS:
        for layer, ow, inst, (kh, kw, stride, padding) in audits(cfg).fallback_launches:
            print(f"{cfg}: {layer} at row width {ow}: {inst}")
            assert (kh, kw, stride, padding) == (3, 3, (1, 1), (1, 1)) and layer.endswith(".conv2"), (cfg, layer)
            assert inst in {("fast", 2, 0, "tap"), ("fast", 4, 0, "tap")} and inst[1] == (2 if layer.startswith("layer1.") else 4), (cfg, layer, inst)
            assert ow <= 4, (cfg, layer, ow)
            widths.add(ow)
    assert widths == {1, 2, 3, 4}


def test_the_dispatch_per_size():
    """SIZE_TABLE against conv_split.pick_tn, rowwin_applies, rowwin_fits and rowwin_divides on the torch module's 52 block
    convolutions (no device): which row-window instances a size launches and which row widths fall back."""
    for (h, w), want in SIZE_TABLE.items():
        got = A.resnet_dispatch(h, w)
        print(f"{h}x{w}: row-window {got[0]}, fall-backs at row widths {got[1]}")
        assert got == want, ((h, w), got, want)
        assert sum(got[0].values()) + sum(got[1].values()) == 13          # the sixteen 3 x 3 layers less the three with stride 2
    assert {(CONFIGS[c][1], CONFIGS[c][2]) for c in CONFIGS} == set(SIZE_TABLE)


# ------------------------------------------------------------------------------------ a wrong trunk fails where it is wrong
def _scale_one_packed_weight(tower):
    """layer1.1.conv2 (row-window kernel <2, 5> at 33 x 47): the largest hi half of cout 5's packed weights times 1 + 2^-9."""
    wf = tower.blocks[1].conv2.w_fast                                       # (cout_pad, K / 32, [hi, lo], 32) fp16
    row = wf[5, :, 0, :]
    kb, j = divmod(int(row.abs().argmax()), 32)
    old = row[kb, j].clone()
    wf[5, kb, 0, j] = (old.float() * (1.0 + 2.0 ** -9)).half()
    assert wf[5, kb, 0, j] != old and wf.shape[2] == 2


def _swap_in_another_blocks_bias(tower):
    a, b = tower.blocks[1].conv3.bias, tower.blocks[2].conv3.bias
    assert a.shape == b.shape and not torch.equal(a, b)
    a.copy_(b)


def _double_one_stem_scale(tower):
    tower.stem_scale[17] *= 2.0


MUTATIONS = {
    "one packed weight": (_scale_one_packed_weight, lambda au: au.layer_launch["layer1.1.conv2"]),
    "another block's residual bias": (_swap_in_another_blocks_bias, lambda au: au.residual_launch[1]),
    "one stem un-scaling entry doubled": (_double_one_stem_scale, lambda au: au.sequence.index(A.STEM7)),
}


@pytest.mark.parametrize("what", list(MUTATIONS))
def test_a_wrong_trunk_fails_the_audit_at_that_launch(cuda_device, what):
    """Three mistakes made on a built HipResNet50 INSTANCE (never in product code), values only, sizes and pointers as they were:
    one element of layer1.1.conv2's packed ``w_fast`` scaled by 1 + 2^-9; layer1.1's residual bias replaced by layer1.2's; one
    entry of the stem's un-scaling vector doubled.  Each is reported at exactly its own launch and at no other: every later
    launch reads that launch's (wrong) recorded output as its own input and passes.  The unmutated tower passes ([33x47x3])."""
    mutate, where = MUTATIONS[what]
    au = _run_audit("33x47x3", cuda_device, mutate=mutate)
    for _, m in au.failures:
        print(m)
    assert [k for k, _ in au.failures] == [where(au)], (what, au.failures)
    assert len(au.rows) == sum(au.names.values()) - 1
