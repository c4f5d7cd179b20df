"""One-hot overflow cases and the trunk interposer of tests/test_gpu_range_guard.py (helper, no tests).

Part 1 -- ``ConvCase``: one stand-alone launch configuration per kernel instance.  The weights are identity-like -- one
non-zero weight per cout, ``w[c, c mod Cin, tap(c)] = 32`` -- so a convolution output is ONE product and every number of
the contract is exact: an input of 2047 gives 65504 = TISE_F16_MAX, an input of 2048 gives 65536, which converts to +inf.
A case knows which input element feeds the conv output (pixel, cout) alone (``source``), how many STORED outputs hold that
conv output (``stored``: 1, or the number of pooling windows that cover it for the pooled epilogues) and the positions to
sweep (``positions``); ``run_case`` does the launches and returns what went wrong as a list of lines.

Part 2 -- ``TrunkSweep``: while a ``SplitTrunk`` forward runs, every launch that writes a split tensor is run once per
target with ONE entry of the bias it reads set to 7e4 (the mean kernel: one input channel raised), the flag read before and
after, then once more untouched.  A ``tise_*`` name it does not know is an error, as in tests/_trunk_audit.Recorder.

Nothing here touches a device at import time.
"""
import contextlib
import ctypes
import types

import torch
import torch.nn.functional as F

from tests import _trunk_audit as A

F16_MAX = 65504.0          # TISE_F16_MAX = 2047 * 32
OVER = 65536.0             # 2048 * 32: fp16(65536) = +inf
W_ON, W_OFF = 32.0, 16.0   # the weight of the cout under test / of the other half of a 64-on-32 layer (-> 32768)
X_LEGAL, X_OVER = 2047.0, 2048.0
BLOWN = 7.0e4

ARG_FIELDS = ("N", "H", "W", "Cin", "KH", "KW", "SH", "SW", "PH", "PW", "OH", "OW", "Cout", "K", "Kpad", "M", "nseg",
              "out_hp", "out_wp", "out_y0", "out_x0")


def hi_pos(c, C):
    """Position of channel c's hi half inside a pixel's 2C-element split row (csrc/common.h tise_ilv_off)."""
    full = C & ~31
    return (c >> 5) * 64 + (c & 31) if c < full else 2 * full + (c - full)


def lo_pos(c, C):
    return hi_pos(c, C) + (32 if c < (C & ~31) else 16)


def windows(x, ow):
    """Number of 3-wide stride-2 windows of a row of ``ow`` columns that cover column x."""
    owp = (ow - 3) // 2 + 1
    return sum(1 for o in range(owp) if 2 * o <= x <= 2 * o + 2)


@contextlib.contextmanager
def conv_spy():
    """Records (code, ConvArgs fields) of every tise_conv_split_f16 launch as objects ``_trunk_audit.instance_of`` reads."""
    from tise_toolbox_amd import _lib
    seen, orig = [], _lib.call

    def call(name, *args):
        if name == "tise_conv_split_f16":
            s = args[0]._obj
            seen.append(types.SimpleNamespace(code=int(args[1]), args={f: getattr(s, f) for f in ARG_FIELDS}))
        return orig(name, *args)
    _lib.call = call
    try:
        yield seen
    finally:
        _lib.call = orig


class ConvCase:
    """``key``: the instance in the form of ``_trunk_audit.instance_of``.  ``extra``: an instance beyond the product's and
    the audit's "deliberately outside" list (another Cin % 32, another destination of the same template instance).
    ``tap`` / ``other_tap``: the tap of the couts under test / of the other half of the 64-on-32 layers of configuration 34,
    ``upper``: the half under test.  ``layout``: "one" destination, or "three" = split | raw fp32 | split as
    test_conv_split_matches_fp64_conv lays them out.  ``grid``: tile rows are pixels of the INPUT grid (configuration 34)."""

    def __init__(self, name, key, cin, cout, k, stride, pad, shape, ctor, call=None, layout="one", tile=128, tap=(0, 0),
                 other_tap=None, upper=False, grid=False, extra=False, np_=None):
        self.name, self.key, self.cin, self.cout = name, key, cin, cout
        self.kh, self.kw = k
        self.stride, self.pad, self.shape = stride, pad, shape
        self.ctor, self.call, self.layout, self.tile = ctor, dict(call or {}), layout, tile
        self.tap, self.other_tap, self.upper, self.grid, self.extra, self.np_ = tap, other_tap, upper, grid, extra, np_
        assert cout <= cin or (other_tap is not None and cout == 2 * cin), "one input channel per cout, or two halves on two taps"

    def __repr__(self):
        return self.name

    # ---- the layer -------------------------------------------------------------------------------------------
    def tested(self, c):
        return self.other_tap is None or (c >= self.cin) == self.upper

    def weight(self):
        w = torch.zeros((self.cout, self.cin, self.kh, self.kw))
        for c in range(self.cout):
            a, b = self.tap if self.tested(c) else self.other_tap
            w[c, c % self.cin, a, b] = W_ON if self.tested(c) else W_OFF
        return w

    def build(self, dev):
        from tise_toolbox_amd.conv_split import SplitConv
        return SplitConv(self.weight().to(dev), torch.zeros(self.cout, device=dev), (self.stride, self.stride), self.pad, dev, **self.ctor)

    @property
    def pin(self):
        return self.call.get("pooled_input", False)

    def conv_in_hw(self):
        n, h, w = self.shape
        if self.pin == "v":
            return (h - 3) // 2 + 1, w
        if self.pin:
            return (h - 3) // 2 + 1, (w - 3) // 2 + 1
        return h, w

    def conv_hw(self):
        h, w = self.conv_in_hw()
        return ((h + 2 * self.pad[0] - self.kh) // self.stride + 1, (w + 2 * self.pad[1] - self.kw) // self.stride + 1)

    def out_hw(self):
        oh, ow = self.conv_hw()
        if self.call.get("pool_output"):
            return (oh - 3) // 2 + 1, (ow - 3) // 2 + 1
        if self.call.get("pool_h"):
            return oh, (ow - 3) // 2 + 1
        return oh, ow

    def source(self, n, y, x, c):
        """The raw-input element (n, yi, xi, channel) that alone feeds conv output (n, y, x, c) of a tested cout."""
        a, b = self.tap
        yi, xi = y * self.stride + a - self.pad[0], x * self.stride + b - self.pad[1]
        if self.pin == "v":
            yi = 2 * yi + 1                                       # the middle tap of one vertical window
        elif self.pin:
            yi, xi = 2 * yi + 1, 2 * xi + 1                       # odd coordinates: inside one 3 x 3 stride-2 window
        h, w = self.shape[1:]
        assert 0 <= yi < h and 0 <= xi < w, (self.name, y, x, c)
        return n, yi, xi, c % self.cin

    def stored(self, y, x):
        oh, ow = self.conv_hw()
        if self.call.get("pool_output"):
            return windows(y, oh) * windows(x, ow)
        if self.call.get("pool_h"):
            return windows(x, ow)
        return 1

    # ---- destinations ----------------------------------------------------------------------------------------
    def segments(self):
        """[(c0, c1, destination index, offset, mode)], [(channels, dtype is split)] per destination."""
        if self.layout == "three":
            assert self.cout > 32
            return [(0, 16, 0, 16, 0), (16, 32, 1, 0, 1), (32, self.cout, 0, 64, 0)], [(self.cout + 32, True), (16, False)]
        return [(0, self.cout, 0, 0, 0)], [(-(-self.cout // 16) * 16, True)]     # a split tensor holds a multiple of 16 channels

    def destinations(self, dev):
        n = self.shape[0]
        oh, ow = self.out_hw()
        kw = dict(self.call)
        if kw.pop("border", False):
            kw["out_pad"] = (oh + 2, ow + 2, 1, 1)
            oh, ow = oh + 2, ow + 2
        segs, dsts = self.segments()
        tens = [torch.zeros((n, oh, ow, 2 * c if sp else c), dtype=torch.float16 if sp else torch.float32, device=dev) for c, sp in dsts]
        return [(c0, c1, tens[di], off, mode) for c0, c1, di, off, mode in segs], tens, kw

    def mode_of(self, c):
        return next(mode for c0, c1, _, _, mode in self.segments()[0] if c0 <= c < c1)

    # ---- positions -------------------------------------------------------------------------------------------
    def rows_total(self):
        n, h, w = self.shape
        oh, ow = self.conv_hw()
        return n * h * w if self.grid else n * oh * ow

    def pixel(self, r):
        """Tile-row ordinal r -> conv output (n, y, x), or None where the row stores nothing (a grid pixel outside the
        output, a column no window covers)."""
        oh, ow = self.conv_hw()
        gh, gw = self.shape[1:] if self.grid else (oh, ow)
        n, rem = divmod(r, gh * gw)
        y, x = divmod(rem, gw)
        if y >= oh or x >= ow or self.stored(y, x) == 0:
            return None
        return n, y, x

    def positions(self):
        """(tile-row ordinal, cout) pairs: every row of the first tile at a cout that varies with the row, every tested cout
        at a row that varies with the cout, the last pixel of the M tail, the first pixel of the second tile, the first and
        last cout of each further destination segment, the seam rows of the overlapping POOLH tiles."""
        total, T = self.rows_total(), self.tile
        couts = [c for c in range(self.cout) if self.tested(c)]
        out = []

        def add(r, c):
            r %= total
            for _ in range(total):                               # the next row that stores something
                if self.pixel(r) is not None:
                    out.append((r, c))
                    return
                r = (r + 1) % total
            raise AssertionError(f"{self.name}: no row stores anything")
        for r in range(min(T, total)):
            if self.pixel(r) is not None:
                out.append((r, couts[(7 * r + 3) % len(couts)]))
        for i, c in enumerate(couts):
            add((11 * i + 5) % min(T, total), c)
        last = next(r for r in range(total - 1, -1, -1) if self.pixel(r) is not None)
        out.append((last, couts[-1]))
        if total > T:
            add(T, couts[0])
            add(T + 1, couts[-1])
        for c0, c1, _, _, _ in self.segments()[0][1:]:
            add(3, c0)
            add(total - 2, c1 - 1)
        if self.call.get("pool_h"):
            for r in range(124, 131):
                if self.pixel(r) is not None:
                    out.append((r, couts[(5 * r) % len(couts)]))
        return list(dict.fromkeys(out))

    # ---- the exact reference of the legal launch -----------------------------------------------------------------
    def reference(self, value):
        """fp64 NHWC (linear, activated on the destination grid) for an input of ``value`` everywhere."""
        n, h, w = self.shape
        x = torch.full((n, self.cin, h, w), value, dtype=torch.float64)
        if self.pin == "v":
            x = F.max_pool2d(x, (3, 1), (2, 1))
        elif self.pin:
            x = F.max_pool2d(x, 3, 2)
        lin = F.conv2d(x, self.weight().double(), None, self.stride, self.pad)
        act = torch.relu(lin)
        if self.call.get("pool_output"):
            act = F.max_pool2d(act, 3, 2)
        elif self.call.get("pool_h"):
            act = F.max_pool2d(act, (1, 3), (1, 2))
        return lin.permute(0, 2, 3, 1).contiguous(), act.permute(0, 2, 3, 1).contiguous()


def check_dispatch(case, conv, seen, ow):
    """The instance under test is the one dispatched: no fall-back, the key ``_trunk_audit.instance_of`` gives the launch."""
    from tise_toolbox_amd.conv_split import rowwin_fits
    bad = []
    if conv._fallback is not None:
        bad.append("the construction fell back to another kernel")
    if len(seen) != 1:
        return bad + [f"{len(seen)} launches from one call"]
    got = A.instance_of(seen[0])
    if got != case.key:
        bad.append(f"dispatched {got}, the case is for {case.key}")
    for k, v in case.ctor.items():
        if k in ("tn", "variant", "korder") and getattr(conv, k) != v:
            bad.append(f"SplitConv.{k} is {getattr(conv, k)!r}, asked for {v!r}")
    if conv.variant == "rowwin":
        if not rowwin_fits(ow, conv.kw) or A.rowwin_np(ow, conv.kw) != case.np_:
            bad.append(f"row-window pieces {A.rowwin_np(ow, conv.kw)} at OW {ow}, the case is for {case.np_}")
        steps = (conv.cin // 32) * conv.kw + ((conv.kw + 1) // 2 if conv.cin % 32 else 0)
        if conv.kpad != conv.kh * steps * 32:
            bad.append(f"kpad {conv.kpad}")
    return bad


def run_case(case, dev):
    """All launches of one case -> (failures, number of one-hot launches)."""
    from tise_toolbox_amd import device
    from tise_toolbox_amd.conv_split import split
    conv = case.build(dev)
    segs, tens, kw = case.destinations(dev)
    n, h, w = case.shape
    cin = case.cin
    bad = []
    x = torch.zeros((n, h, w, 2 * cin), dtype=torch.float16, device=dev)
    device.read_split_overflow()
    # zeros: the dispatch, no flag, zeros out
    with conv_spy() as seen:
        conv(x, segs, **kw)
    bad += check_dispatch(case, conv, seen, case.conv_hw()[1])
    if device.read_split_overflow():
        bad.append("flag raised on an input of zeros")
    if any(bool(t.any()) for t in tens):
        bad.append("non-zero output on an input of zeros")
    # the legal launch: every tested output is 65504 = (hi 65504, lo 0) exactly, the flag stays clear
    conv(split(torch.full((n, h, w, cin), X_LEGAL, device=dev)), segs, **kw)
    if device.read_split_overflow():
        bad.append("FALSE ALARM: flag raised although every value the launch computes is <= 65504")
    lin, act = case.reference(X_LEGAL)
    assert act.max().item() == F16_MAX and lin.max().item() == F16_MAX
    border = "out_pad" in kw
    for c0, c1, dst, off, mode in segs:
        got = dst.cpu()
        if border:
            inner = got[:, 1:-1, 1:-1]
            if bool(got[:, 0].any()) or bool(got[:, -1].any()) or bool(got[:, :, 0].any()) or bool(got[:, :, -1].any()):
                bad.append("the border of the destination is not zero")
            got = inner
        if mode == 0:
            ih, il = A.split_index(got.shape[-1] // 2, "cpu")
            hi, lo = got[..., ih][..., off:off + c1 - c0], got[..., il][..., off:off + c1 - c0]
            if not (torch.equal(hi.double(), act[..., c0:c1]) and not bool(lo.any())):
                bad.append(f"legal launch, segment [{c0}, {c1}): not (hi, lo) = (reference, 0) exactly")
        elif not torch.equal(got[..., off:off + c1 - c0].double(), lin[..., c0:c1]):
            bad.append(f"legal launch, raw segment [{c0}, {c1}): not the reference exactly")
    # the one-hot sweep
    pos = case.positions()
    for r, c in pos:
        pn, py, px = case.pixel(r)
        sn, sy, sx, sc = case.source(pn, py, px, c)
        x[sn, sy, sx, hi_pos(sc, cin)] = X_OVER
        conv(x, segs, **kw)
        flag = device.read_split_overflow()
        x[sn, sy, sx, hi_pos(sc, cin)] = 0.0
        # a stored 65536 is (hi +inf, lo -inf); the pooled epilogues re-split merge(hi, lo) = NaN: two non-finite halves either way
        infs = sum(int((~torch.isfinite(t)).sum()) for t in tens if t.dtype == torch.float16)
        where = f"tile row {r} = pixel {(pn, py, px)}, cout {c}"
        if case.mode_of(c) == 0:
            want = 2 * case.stored(py, px)                        # both halves of every stored output that holds it
            if infs != want:
                bad.append(f"{where}: {infs} non-finite halves stored, the case expects {want}")
            if not flag:
                bad.append(f"MISSED OVERFLOW: {where}: 65536 stored into a split tensor, flag clear")
        else:
            hits = sum(int((t == OVER).sum()) for t in tens if t.dtype == torch.float32)
            if flag or infs or hits != 1:
                bad.append(f"{where} (raw fp32 segment): flag {flag}, {infs} non-finite halves, {hits} elements of 65536")
    if device.read_split_overflow():
        bad.append("the flag is not read-and-clear")
    return bad, len(pos)


# --------------------------------------------------------------------------------------------------- the cases
def _cases():
    out = []

    def add(*a, **k):
        out.append(ConvCase(*a, **k))
    # default kernel and its generic twin, 1x1, M = 144: full width, an invalid last 8-cout chunk, three segments
    for variant in ("fast", "glds"):
        for tn in (1, 2, 3, 4, 5):
            key = ("fast", tn, 0, "tap") if variant == "fast" else ("glds", tn, 0)
            ctor = dict(tn=tn, variant=variant)
            c = 32 * tn
            add(f"{variant}{tn}", key, c, c, (1, 1), 1, (0, 0), (1, 12, 12), ctor)
            add(f"{variant}{tn}-cout-tail", key, c, c - 8, (1, 1), 1, (0, 0), (1, 12, 12), ctor)
            if tn == 1:                                           # three segments need more than 32 couts: two n-tiles
                add(f"{variant}{tn}-three-segments", key, 64, 48, (1, 1), 1, (0, 0), (1, 12, 12), ctor, layout="three")
            else:
                add(f"{variant}{tn}-three-segments", key, c, c, (1, 1), 1, (0, 0), (1, 12, 12), ctor, layout="three")
    # the paired 16-channel-tail steps: couts 0..31 read the full block, 32..47 the tail
    add("fast2-paired-tails", ("fast", 2, 16, "tap"), 48, 48, (3, 3), 1, (1, 1), (1, 12, 12), dict(tn=2, variant="fast"), tap=(1, 1))
    # block-major K order
    for tn in (2, 3, 4, 5):
        add(f"fast{tn}-block-major", ("fast", tn, 0, "block"), 32 * tn, 32 * tn, (3, 3), 2, (0, 0), (9, 9, 9),
            dict(tn=tn, variant="fast", korder="block"))
    # row-window kernel
    shapes = {5: (1, 4, 35), 6: (3, 6, 8)}
    expected = {(2, 16, 5), (3, 0, 5), (3, 0, 6), (3, 16, 5), (4, 0, 6), (2, 0, 6), (4, 0, 5)}
    for np_ in (5, 6):
        for tn, cin in ((2, 64), (3, 96), (4, 128), (2, 48), (3, 112)):
            if (tn, cin % 32, np_) == (3, 16, 6):
                continue
            add(f"rowwin{tn}-np{np_}-cin{cin}", ("rowwin", tn, cin % 32, np_, ""), cin, min(cin, 32 * tn), (1, 3), 1, (0, 1), shapes[np_],
                dict(tn=tn, variant="rowwin"), tap=(0, 1), np_=np_, extra=(tn, cin % 32, np_) not in expected)
    for np_, cin, extra in ((5, 112, False), (5, 96, True), (6, 96, True)):
        add(f"rowwin3-np{np_}-cin{cin}-poolh", ("rowwin", 3, cin % 32, np_, "POOLH"), cin, 96, (1, 3), 1, (0, 1), shapes[np_],
            dict(tn=3, variant="rowwin"), call=dict(pool_h=True), tap=(0, 1), np_=np_, extra=extra)
    # pooled-input kernel: 64-pixel tiles, M = 80 (nine taps) / 180 (vertical taps)
    for c, tnw in ((128, 2), (256, 4)):
        add(f"poolin{tnw}", ("poolin", tnw, "9tap"), c, c, (1, 1), 1, (0, 0), (5, 9, 9), dict(variant="fast"), call=dict(pooled_input=True), tile=64)
        add(f"poolin{tnw}-vt", ("poolin", tnw, "VT"), c, c, (1, 1), 1, (0, 0), (5, 9, 9), dict(variant="fast"), call=dict(pooled_input="v"), tile=64)
    # configuration 34: tile rows are grid pixels, 144 of them
    product = {(32, "unpadded", "border"), (32, "unpadded", "plain"), (32, "padded", "plain"), (64, "padded", "plain"), (64, "unpadded", "plain")}
    ctor = dict(variant="pipe", pipe_cfg=34)
    for cout in (32, 64):
        for padded in (False, True):
            for dest in ("plain", "border"):
                pad, tap, other = ((1, 1), (1, 1), (0, 0)) if padded else ((0, 0), (0, 0), (1, 1))
                key = ("pipe34", cout, "padded" if padded else "unpadded", dest)
                for upper in ((False, True) if cout == 64 else (False,)):
                    add(f"pipe34-{cout}-{key[2]}-{dest}" + ("-upper" if upper else ""), key, 32, cout, (3, 3), 1, pad, (1, 12, 12), ctor,
                        call=dict(border=True) if dest == "border" else None, tap=tap, other_tap=other if cout == 64 else None, upper=upper,
                        grid=True, extra=key[1:] not in product)
    for upper in (False, True):
        add("pipe34-64-pooled" + ("-upper" if upper else ""), ("pipe34", 64, "unpadded", "pooled"), 32, 64, (3, 3), 1, (0, 0), (1, 5, 128), ctor,
            call=dict(pool_output=True), tap=(0, 0), other_tap=(1, 1), upper=upper, grid=True)
    return out


CASES = {c.name: c for c in _cases()}
assert len(CASES) == len(_cases())

# the instances tests/test_gpu_trunk_launches.py lists as outside the Inception trunk, in instance_of's form.  The set describes that
# trunk and stays as it is; it is not "outside the product": ("rowwin", 2, 0, 6, "") and ("rowwin", 4, 0, 5, "") are reached by
# ResNet-50 (32 x 32 images; 96 x 96 and up) and audited in tests/test_gpu_resnet_launches.py
OUTSIDE = {("fast", 1, 0, "tap"), ("fast", 2, 0, "block"), ("fast", 2, 16, "tap"), ("rowwin", 2, 0, 6, ""), ("rowwin", 4, 0, 5, ""),
           ("poolin", 2, "VT"), ("pipe34", 32, "padded", "plain")} | {("glds", tn, 0) for tn in (1, 2, 3, 4, 5)}


# ------------------------------------------------------------------------------------------------ Part 2: the trunk
STEM_BIAS = {"tise_stem_conv3x3s2_split": 5, "tise_stem_conv3x3s2_split_u8": 6, "tise_stem_conv3x3s2_split_u8_mfma": 7}
AVG_BIAS = {"tise_avgpool3_bias_relu_split_nhwc": 7, "tise_avgpool3_excl_bias_relu_split_nhwc": 7}
# split tensors in, the maximum of EXISTING values out: nothing new is converted, the guard is not involved
MOVERS = ("tise_maxpool3s2_split_nhwc", "tise_maxpool3s1p1_split_nhwc")


class TrunkSweep:
    """``with TrunkSweep() as sw: forward()`` -> ``sw.failures`` (lines), ``sw.targets`` (launches run with a blown entry that
    had to raise the flag), ``sw.silent`` (those that had to leave it clear), ``sw.names`` (launch names seen)."""

    def __init__(self):
        self.failures, self.targets, self.silent, self.names = [], 0, 0, []
        self._stack, self._tensors = [], {}

    def _poke(self, what, tensor, index, run, expect):
        """One launch with ``tensor[index]`` = 7e4: the flag clear before it, ``expect`` after it, the entry restored."""
        from tise_toolbox_amd import device
        if device.read_split_overflow():
            self.failures.append(f"{what}: the flag was set BEFORE the targeted launch")
        old = tensor[index].clone()
        tensor[index] = BLOWN
        try:
            run()
        finally:
            tensor[index] = old
        flag = device.read_split_overflow()
        if expect:
            self.targets += 1
        else:
            self.silent += 1
        if flag != expect:
            self.failures.append(f"{what}: " + ("MISSED OVERFLOW: flag clear after a 7e4 bias" if expect else "flag raised by a launch that writes no split value from it"))

    def _clean(self, what, run):
        from tise_toolbox_amd import device
        r = run()
        if device.read_split_overflow():
            self.failures.append(f"{what}: flag raised by the untouched launch")
        return r

    def __enter__(self):
        from tise_toolbox_amd import _lib, trunk
        from tise_toolbox_amd.conv_split import SplitConv
        sw = self
        self._orig = (SplitConv.__call__, _lib.call, trunk._p)
        orig_call, orig_lib, orig_p = self._orig

        def p(t):
            sw._tensors[t.data_ptr()] = t
            return orig_p(t)

        def conv_call(self, xs, segs, pooled_input=False, **kw):
            sw._stack.append((self, list(segs)))
            try:
                return orig_call(self, xs, segs, pooled_input=pooled_input, **kw)
            finally:
                sw._stack.pop()

        def tensor(name, args, i):
            t = sw._tensors.get(args[i].value)
            assert t is not None, (name, i)
            return t

        def lib_call(name, *args):
            run = lambda: orig_lib(name, *args)                   # noqa: E731
            if name == "tise_split_overflow_check":               # the sweep's own flag reads
                return run()
            sw.names.append(name)
            if name == "tise_conv_split_f16":
                assert sw._stack, "tise_conv_split_f16 outside SplitConv.__call__"
                conv, segs = sw._stack[-1]                        # the innermost frame launches (an outer one handed on to its _fallback)
                what = f"conv {conv.cin}->{conv.cout} k{conv.kh}x{conv.kw} code {int(args[1]):#x}"
                for c0, c1, _, _, mode in segs:
                    for c in sorted({c0, c1 - 1}):
                        sw._poke(f"{what} cout {c} of segment [{c0}, {c1}) mode {mode}", conv.bias, c, run, mode == 0)
                return sw._clean(what, run)
            if name in STEM_BIAS or name in AVG_BIAS:
                bias = tensor(name, args, STEM_BIAS.get(name, 7))
                for c in sorted({0, bias.numel() - 1}):
                    sw._poke(f"{name} channel {c} of {bias.numel()}", bias, c, run, True)
                return sw._clean(name, run)
            if name == "tise_split_mean_both_nhwc":
                a, (n, hw, C) = tensor(name, args, 0), args[1:4]
                rows = a.view(n, hw, 2 * C)
                feat = torch.empty((n, C), dtype=torch.float32, device=a.device)
                for c in sorted({0, C - 1}):                      # every position of the channel (65504, 65504): a mean of 65535.98
                    cols = [hi_pos(c, C), lo_pos(c, C)]
                    old = rows[n - 1, :, cols].clone()
                    rows[n - 1, :, cols] = F16_MAX
                    try:
                        sw._poke(f"{name} channel {c} of {C}", feat, (0, 0), run, True)     # (the poked scratch entry is not read)
                        sw._poke(f"tise_split_mean_nhwc channel {c} of {C}", feat, (0, 0),
                                 lambda: orig_lib("tise_split_mean_nhwc", args[0], n, hw, C, ctypes.c_void_p(feat.data_ptr()), args[-1]), False)
                    finally:
                        rows[n - 1, :, cols] = old
                return sw._clean(name, run)
            if name in MOVERS or name == "tise_split_mean_nhwc":
                return sw._clean(name, run)
            raise AssertionError(f"the trunk reached {name}, which the range-guard sweep does not know")

        SplitConv.__call__, _lib.call, trunk._p = conv_call, lib_call, p
        return self

    def __exit__(self, *exc):
        from tise_toolbox_amd import _lib, trunk
        from tise_toolbox_amd.conv_split import SplitConv
        SplitConv.__call__, _lib.call, trunk._p = self._orig
        self._tensors.clear()


@contextlib.contextmanager
def blown_bias(conv, cout):
    """One bias entry of a SplitConv at 7e4 while the block runs."""
    old = conv.bias[cout].clone()
    conv.bias[cout] = BLOWN
    try:
        yield
    finally:
        conv.bias[cout] = old
