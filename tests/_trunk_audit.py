"""Launch recorder and fp64 references for tests/test_gpu_trunk_launches.py (the Inception trunk) and
tests/test_gpu_resnet_launches.py (the ResNet-50 and CountSeg routes: ``ResNetRefs``, ``check_resnet_launch``); helper, no tests.

While a ``SplitTrunk`` forward runs, ``Recorder`` intercepts ``SplitConv.__call__`` with the integer ``code`` it hands to
``tise_conv_split_f16`` and every other ``tise_*`` entry point the trunk reaches through ``_lib.call``, and keeps the
operands AS THAT LAUNCH SAW THEM: a clone of the input, a clone of every destination before and after the call, the
segment list and the integer arguments.  ``check_launch`` then computes the same operation in fp64 from the recorded
input of that launch alone, so no error is carried from one layer into the next, and compares at the tolerance the
project uses for that kernel on its own.

The fp64 references need each convolution's ORIGINAL weights: ``keep_weights`` wraps ``SplitConv.__init__`` and keeps
``(weight.double(), bias.double())`` beside each instance -- never unpacked from ``SplitConv.w`` / ``w_fast``, which
would test the packing with itself.  The split layout (csrc/common.h) is restated here (``split_index``) instead of
imported from conv_split.py for the same reason.

Nothing here touches a device at import time.
"""
import contextlib
import ctypes

import torch
import torch.nn.functional as F

CONV_TOL = 4e-6        # of the launch's output scale: test_gpu_kernels.py, every convolution test against fp64
AVG_TOL = 2e-6         # of max(1, output scale): test_gpu_inception2015.py::test_exclude_padding_avgpool_split_vs_fp64
FC_TOL = 2e-6          # of the logit scale
U24 = 2.0 ** -24       # unit roundoff of fp32

# name -> (input pointer positions, destination pointer positions) among the arguments of _lib.call(name, *args)
KNOWN = {
    "tise_stem_conv3x3s2_split": ((0,), (6,)),
    "tise_stem_conv3x3s2_split_u8": ((0, 1), (7,)),
    "tise_stem_conv3x3s2_split_u8_mfma": ((0, 1), (8,)),
    "tise_maxpool3s2_split_nhwc": ((0,), (7,)),
    "tise_maxpool3s1p1_split_nhwc": ((0,), (7,)),
    "tise_avgpool3_bias_relu_split_nhwc": ((0, 7), (8,)),
    "tise_avgpool3_excl_bias_relu_split_nhwc": ((0, 7), (8,)),
    "tise_split_mean_nhwc": ((0,), (4,)),
    "tise_split_mean_both_nhwc": ((0,), (4, 5)),
    "tise_split_tap_rows": ((0,), (6,)),
    # the ResNet-50 and CountSeg routes (resnet_hip.py, countseg_hip.py through device.py); positions as in include/tise_hip.h
    "tise_stem_conv7x7s2_split_u8_mfma": ((0, 1), (8,)),
    "tise_resnet_input_split": ((0, 1), (5,)),
    "tise_maxpool3s2p1_split_nhwc": ((0,), (7,)),
    "tise_residual_relu_split_nhwc": ((0, 4, 7), (13,)),         # raw, then the one identity that is not NULL: split or fp32
    "tise_countseg_head": ((0,), (13, 14, 15)),
}
TAP = "tise_split_tap_rows"      # the one launch that comes from device.py (device._ptr), not from trunk.py (trunk._p)
STEMS = ("tise_stem_conv3x3s2_split", "tise_stem_conv3x3s2_split_u8", "tise_stem_conv3x3s2_split_u8_mfma")
STEM7 = "tise_stem_conv7x7s2_split_u8_mfma"
INPUT_SPLIT = "tise_resnet_input_split"
RESIDUAL = "tise_residual_relu_split_nhwc"
HEAD = "tise_countseg_head"
GUARD_READ = "tise_split_overflow_check"   # no launch: the read-and-clear of the range guard (device.read_split_overflow); counted, passed on


# ---------------------------------------------------------------------------------------------------- split layout
def split_index(C, device):
    """Positions of the hi and the lo half of channel c inside a (..., 2C) split row: blocks of 32 channels as
    [hi x32 | lo x32], then a last block [hi x16 | lo x16] when C % 32 == 16."""
    assert C % 16 == 0
    c = torch.arange(C, device=device)
    full = C & ~31
    hi = torch.where(c < full, (c // 32) * 64 + c % 32, 2 * full + (c - full))
    lo = torch.where(c < full, hi + 32, hi + 16)
    return hi, lo


def merge64(t):
    """split tensor (..., 2C) fp16 -> fp64 (..., C), hi + lo * 2**-11 (exact)."""
    hi, lo = split_index(t.shape[-1] // 2, t.device)
    return t[..., hi].double() + t[..., lo].double() * (2.0 ** -11)


def raw_mask(C, c0, c1, split, device):
    """Boolean mask over the raw last dimension of a destination row: the elements that hold channels [c0, c1)."""
    if not split:
        m = torch.zeros(C, dtype=torch.bool, device=device)
        m[c0:c1] = True
        return m
    hi, lo = split_index(C, device)
    m = torch.zeros(2 * C, dtype=torch.bool, device=device)
    m[hi[c0:c1]] = True
    m[lo[c0:c1]] = True
    return m


def bits(t):
    """The tensor's bit patterns (uninitialised memory may hold NaNs, which never compare equal as numbers)."""
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 1: torch.uint8, 8: torch.int64}[t.element_size()])


# ------------------------------------------------------------------------------------------------------- recording
class Launch:
    """One kernel launch: ``name``, the cloned ``inputs``, ``dsts`` = [(before, after)] per distinct destination tensor,
    and for a convolution ``conv`` (the SplitConv), ``segs`` = [(c0, c1, destination index, off, mode)], ``kw``, ``code``
    and ``args`` (the ConvArgs fields as passed); for the others ``ints`` = the call's integer arguments by position
    (``ctypes.c_int64`` ones too), ``ptrs`` = its pointer arguments by position (None = NULL; an input that is NULL is None in
    ``inputs``) and ``read_ptrs`` = every input pointer that is not NULL.  The tap also keeps ``inputs_after``: its input as
    the launch left it; the residual launch keeps ``flag``: the range guard read (and cleared) right after it."""

    def __init__(self, name):
        self.name = name
        self.inputs, self.dsts = [], []
        self.conv = self.segs = self.kw = self.code = self.args = None
        self.ints, self.ptrs = {}, {}
        self.in_ptr = None
        self.read_ptrs = None
        self.dst_ptrs = []
        self.inputs_after = None
        self.flag = None

    def __repr__(self):
        if self.conv is not None:
            c = self.conv
            return (f"{self.args['H']}x{self.args['W']}x{c.cin}->{c.cout} k{c.kh}x{c.kw} s{c.stride[0]} p{c.padding} "
                    f"code {self.code:#x} {self.kw or ''}")
        return f"{self.name} {[v for _, v in sorted(self.ints.items())]}"


@contextlib.contextmanager
def keep_weights():
    """While active every new SplitConv keeps ``_audit_wb`` = (weight.double(), bias.double()) on its own device."""
    from tise_toolbox_amd.conv_split import SplitConv
    orig = SplitConv.__init__

    def init(self, weight, bias, *a, **k):
        orig(self, weight, bias, *a, **k)
        self._audit_wb = (weight.detach().double().to(self.scale.device), bias.detach().double().to(self.scale.device))
    SplitConv.__init__ = init
    try:
        yield
    finally:
        SplitConv.__init__ = orig


class Recorder:
    """``with Recorder() as rec: trunk.forward_u8(...)`` -> ``rec.launches``.  A ``tise_*`` name the recorder does not know
    is an error: a future kernel cannot slip past the audit."""

    def __init__(self, sync=None):
        self.launches = []
        self.guard_reads = 0
        self._stack, self._tensors = [], {}
        self._sync = sync or torch.cuda.synchronize

    def _clone(self, t):
        self._sync()
        return t.detach().clone()

    def __enter__(self):
        from tise_toolbox_amd import _lib, device, trunk
        from tise_toolbox_amd.conv_split import SplitConv
        rec = self
        self._orig = (SplitConv.__call__, _lib.call, trunk._p, device._ptr)
        orig_call, orig_lib, orig_p, orig_ptr = self._orig
        self._kw = keep_weights()
        self._kw.__enter__()

        def p(t):                                                # trunk._p: remember which tensor a raw pointer is
            rec._tensors[t.data_ptr()] = t
            return orig_p(t)

        def ptr(t):                                              # device._ptr: the same for the tap's wrapper
            rec._tensors[t.data_ptr()] = t
            return orig_ptr(t)

        def conv_call(self, xs, segs, pooled_input=False, **kw):   # signature handling as tools/split_layer_probe.py
            fr = dict(conv=self, segs=list(segs), kw=dict(kw, pooled_input=pooled_input), launch=None)
            uniq = []
            for sg in segs:
                if all(sg[2] is not u for u in uniq):
                    uniq.append(sg[2])
            fr["uniq"] = uniq
            x0 = rec._clone(xs)
            before = [rec._clone(u) for u in uniq]
            rec._stack.append(fr)
            try:
                r = orig_call(self, xs, segs, pooled_input=pooled_input, **kw)
            finally:
                rec._stack.pop()
            L = fr["launch"]
            if L is not None:                                     # this frame launched (not the one that handed on to a _fallback)
                L.inputs = [x0]
                L.dsts = [(b, rec._clone(u)) for b, u in zip(before, uniq)]
                L.in_ptr, L.dst_ptrs = xs.data_ptr(), [u.data_ptr() for u in uniq]
            return r

        def lib_call(name, *args):
            if name == "tise_conv_split_f16":
                assert rec._stack, "tise_conv_split_f16 outside SplitConv.__call__"
                fr = rec._stack[-1]
                assert fr["launch"] is None, "two launches from one SplitConv.__call__"
                a = args[0]._obj
                L = Launch(name)
                L.conv, L.kw, L.code = fr["conv"], {k: v for k, v in fr["kw"].items() if v}, int(args[1])
                L.segs = [(c0, c1, next(i for i, u in enumerate(fr["uniq"]) if u is d), off, mode) for c0, c1, d, off, mode in fr["segs"]]
                L.args = {f: getattr(a, f) for f in ("N", "H", "W", "Cin", "KH", "KW", "SH", "SW", "PH", "PW", "OH", "OW", "Cout", "K",
                                                     "Kpad", "M", "nseg", "out_hp", "out_wp", "out_y0", "out_x0")}
                fr["launch"] = L
                rec.launches.append(L)
                return orig_lib(name, *args)
            if name == GUARD_READ:
                rec.guard_reads += 1
                return orig_lib(name, *args)
            if name not in KNOWN:
                raise AssertionError(f"the trunk reached {name}, which the launch recorder does not know")
            ins, outs = KNOWN[name]
            L = Launch(name)

            def tensor(i):
                t = rec._tensors.get(args[i].value)
                assert t is not None, (name, i)
                return t
            L.ptrs = {i: v.value for i, v in enumerate(args) if isinstance(v, ctypes.c_void_p)}
            L.inputs = [rec._clone(tensor(i)) if L.ptrs[i] is not None else None for i in ins]
            dst = [tensor(i) for i in outs]
            before = [rec._clone(t) for t in dst]
            L.ints = {i: (v.value if isinstance(v, ctypes.c_int64) else v) for i, v in enumerate(args) if isinstance(v, (int, ctypes.c_int64))}
            L.in_ptr, L.dst_ptrs = args[ins[0]].value, [t.data_ptr() for t in dst]
            L.read_ptrs = [L.ptrs[i] for i in ins if L.ptrs[i] is not None]
            r = orig_lib(name, *args)
            L.dsts = [(b, rec._clone(t)) for b, t in zip(before, dst)]
            if name == RESIDUAL:                                  # its guard, by itself: the flag is clear, so reading it changes nothing
                flag = ctypes.c_int(0)
                orig_lib(GUARD_READ, ctypes.byref(flag), args[-1])
                L.flag = bool(flag.value)
            if name == TAP:
                L.inputs_after = [rec._clone(tensor(i)) for i in ins]
            rec.launches.append(L)
            return r

        SplitConv.__call__, _lib.call, trunk._p, device._ptr = conv_call, lib_call, p, ptr
        return self

    def __exit__(self, *exc):
        from tise_toolbox_amd import _lib, device, trunk
        from tise_toolbox_amd.conv_split import SplitConv
        SplitConv.__call__, _lib.call, trunk._p, device._ptr = self._orig
        self._kw.__exit__(*exc)
        self._tensors.clear()


# ------------------------------------------------------------------------------------------------------ references
def _nchw(x):
    return x.permute(0, 3, 1, 2)


def _nhwc(x):
    return x.permute(0, 2, 3, 1)


def _untouched(L, di, own):
    """Everything of destination ``di`` outside ``own`` (a bool tensor broadcastable to it: True = the launch's own
    elements) must hold the bits it held before the call."""
    before, after = L.dsts[di]
    same = bits(before) == bits(after)
    assert bool((same | own).all()), f"{L!r}: destination {di} changed outside the launch's own slice"


def conv_reference(L, wb=None):
    """fp64 NHWC (linear, relu(linear + bias), output scale) of a recorded convolution launch from the launch's own input;
    the activated result is on the grid of the destinations (pooled for pool_output / pool_h).  ``wb``: the layer's original
    fp64 (weight, bias) where the caller has them from the module itself (default: what keep_weights kept)."""
    c, kw = L.conv, L.kw
    w, b = wb if wb is not None else c._audit_wb
    x = _nchw(merge64(L.inputs[0]))
    pin = kw.get("pooled_input")
    if pin == "v":
        x = F.max_pool2d(x, (3, 1), (2, 1))                       # three vertical taps at stride 2
    elif pin:
        x = F.max_pool2d(x, 3, 2)
    lin = F.conv2d(x, w, None, c.stride, c.padding)
    act = torch.relu(lin + b.view(1, -1, 1, 1))
    scale = act.abs().max().item()
    assert (L.args["OH"], L.args["OW"]) == tuple(lin.shape[2:]), (L, lin.shape)
    if kw.get("pool_output"):
        act = F.max_pool2d(act, 3, 2)
    elif kw.get("pool_h"):
        act = F.max_pool2d(act, (1, 3), (1, 2))                   # horizontal 3-tap max at stride 2
    return _nhwc(lin), _nhwc(act), scale


def check_conv(L, fc=False, raw=False, wb=None):
    """Returns the launch's largest error as a fraction of its output scale (asserted <= the tolerance).  ``raw``: a launch
    whose every segment is mode 1 and whose bias is its consumer's (a bottleneck's conv3 and downsample, CountSeg's mix):
    conv2d(x, w) at CONV_TOL of max|conv2d(x, w)|, as tests/test_gpu_resnet_kernels.py compares it."""
    kw = L.kw
    lin, act, scale = conv_reference(L, wb)
    tol = CONV_TOL
    if fc:                                                        # raw logits: of the logit scale
        tol, scale = FC_TOL, lin.abs().max().item()
    if raw:
        assert all(sg[4] == 1 for sg in L.segs), f"{L!r}: a split segment in a launch checked as raw"
        scale = lin.abs().max().item()
    pooled = bool(kw.get("pool_output") or kw.get("pool_h"))
    out_pad = kw.get("out_pad")
    n, gh, gw = act.shape[:3]
    worst = 0.0
    masks = [None] * len(L.dsts)
    for c0, c1, di, off, mode in L.segs:
        before, after = L.dsts[di]
        split = mode == 0
        assert not (pooled and not split)
        C = after.shape[3] // 2 if split else after.shape[3]
        got = merge64(after) if split else after.double()
        want = (act if split else lin)[..., c0:c1]
        if out_pad is not None:
            hp, wp, y0, x0 = out_pad
            assert tuple(after.shape[:3]) == (n, hp, wp)
            inner = torch.zeros((hp, wp), dtype=torch.bool, device=after.device)
            inner[y0:y0 + gh, x0:x0 + gw] = True
            assert not bool(got[:, ~inner][..., off:off + c1 - c0].any()), f"{L!r}: the border of the destination is not zero"
            got = got[:, y0:y0 + gh, x0:x0 + gw]
            rows = inner.view(1, hp, wp, 1)
        else:
            assert tuple(after.shape[:3]) == (n, gh, gw), (L, after.shape, act.shape)
            rows = torch.ones((1, 1, 1, 1), dtype=torch.bool, device=after.device)
        err = (got[..., off:off + c1 - c0] - want).abs().max().item()
        worst = max(worst, err / scale)
        assert err <= tol * scale, f"{L!r}: segment [{c0}, {c1}) at offset {off}: error {err:.3e} > {tol:g} x scale {scale:.3e}"
        # an fp32 segment receives whole 8-cout chunks (51 bird logits -> 56: the destination row is padded for them)
        width = c1 - c0 if split else -(-(c1 - c0) // 8) * 8
        m = raw_mask(C, off, off + width, split, after.device).view(1, 1, 1, -1) & rows
        masks[di] = m if masks[di] is None else (masks[di] | m)
    for di, m in enumerate(masks):
        _untouched(L, di, m)
    return worst


def check_stem(L, trunk):
    i = L.ints
    w, b = trunk.c1a.w.double(), trunk.c1a.b.double()             # the folded fp32 parameters, not the kernels' packed forms
    if L.name == "tise_stem_conv3x3s2_split":
        x = L.inputs[0]
        n, h, wd = i[1], i[2], i[3]
        assert x.numel() == n * h * wd * 3 and x.dtype == torch.float32
        x = x.reshape(n, h, wd, 3).double()
    else:
        u8, lut = L.inputs
        n, h, wd = i[2], i[3], i[4]
        assert u8.dtype == torch.uint8 and tuple(u8.shape) == (n, h, wd, 3) and lut.numel() == 768
        x = torch.stack([lut.view(3, 256)[ch][u8[..., ch].long()] for ch in range(3)], -1).double()
    want = _nhwc(torch.relu(F.conv2d(_nchw(x), w, b, 2)))
    before, after = L.dsts[0]
    assert tuple(after.shape) == (*want.shape[:3], 64)
    scale = want.abs().max().item()
    err = (merge64(after) - want).abs().max().item()
    assert err <= CONV_TOL * scale, f"{L!r}: error {err:.3e} > {CONV_TOL:g} x scale {scale:.3e}"
    return err / scale


def check_pool(L):
    """The two split max pools (bit-equal after merge) and the two split average pools (AVG_TOL); returns the error."""
    i = L.ints
    ld, x_off, n, h, w, C = i[1], i[2], i[3], i[4], i[5], i[6]
    avg = "avgpool" in L.name
    out_ld, out_off = (i[9], i[10]) if avg else (i[8], i[9])
    x = L.inputs[0]
    before, after = L.dsts[0]
    assert tuple(x.shape) == (n, h, w, ld if avg else 2 * ld) and after.shape[3] == 2 * out_ld and after.shape[0] == n
    if avg:
        assert x.dtype == torch.float32 and L.inputs[1].numel() == C
        raw = _nchw(x.double()[..., x_off:x_off + C])
        want = torch.relu(F.avg_pool2d(raw, 3, 1, 1, count_include_pad="excl" not in L.name) + L.inputs[1].double().view(1, -1, 1, 1))
    else:
        xin = _nchw(merge64(x)[..., x_off:x_off + C])
        if "3s2p1" in L.name:
            want = F.max_pool2d(xin, 3, 2, 1)
        else:
            want = F.max_pool2d(xin, 3, 2) if "3s2" in L.name else F.max_pool2d(xin, 3, 1, 1)  # max_pool2d pads with -inf
    want = _nhwc(want)
    assert tuple(after.shape[:3]) == tuple(want.shape[:3])
    got = merge64(after)[..., out_off:out_off + C]
    err = (got - want).abs().max().item()
    if avg:
        bound = AVG_TOL * max(1.0, want.abs().max().item())
        assert err <= bound, f"{L!r}: error {err:.3e} > {bound:.3e}"
    else:
        assert torch.equal(got, want), f"{L!r}: not bit-equal to max_pool2d of the merged input (max difference {err:.3e})"
    _untouched(L, 0, raw_mask(out_ld, out_off, out_off + C, True, after.device).view(1, 1, 1, -1))
    return err


def mean_emulation(v):
    """fp32 (N, HW, C) -> (N, C): the HW values of a channel added in position order into one fp32 accumulator, then one
    fp32 division by (float)HW -- a plain loop of HW tensor additions, vectorised over images and channels."""
    acc = torch.zeros((v.shape[0], v.shape[2]), dtype=torch.float32, device=v.device)
    for s in range(v.shape[1]):
        acc = acc + v[:, s, :]
    return acc / torch.tensor(float(v.shape[1]), dtype=torch.float32, device=v.device)


def check_mean_values(x_split, hw, got):
    """split_mean's fp32 output ``got`` (N, C) of the split tensor (N, HW, 2C) against the fp32 sequential emulation
    (<= 1 ulp: the division) and the fp64 mean (recursive summation of non-negative terms: HW * 2**-24 * mean per channel).
    Returns (largest ulp distance to the emulation, largest fp64 error, largest fp64 error / bound)."""
    n = x_split.shape[0]
    v64 = merge64(x_split.reshape(n, hw, -1))
    v32 = v64.float()
    assert torch.equal(v32.double(), v64)                         # hi + lo * 2**-11 is exact in fp32
    assert bool((v64 >= 0).all()), "the bound is for non-negative terms (post-ReLU activations)"
    emu = mean_emulation(v32)
    ulps = (bits(got).long() - bits(emu).long()).abs().max().item()
    assert ulps <= 1, f"split_mean at HW {hw}: {ulps} ulp from the fp32 sequential emulation"
    mean = v64.mean(1)
    bound = hw * U24 * mean
    err = (got.double() - mean).abs()
    assert bool((err <= bound).all()), f"split_mean at HW {hw}: fp64 error {err.max().item():.3e} beyond HW * 2^-24 * mean"
    assert bool(((emu.double() - mean).abs() <= bound).all())     # ... which guards the emulation itself
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    return ulps, err.max().item(), ratio


def check_mean(L):
    i = L.ints
    n, hw, C = i[1], i[2], i[3]
    x = L.inputs[0]
    assert x.shape[0] == n and x.shape[1] * x.shape[2] == hw and x.shape[3] == 2 * C
    feat = L.dsts[0][1]
    assert tuple(feat.shape) == (n, C) and feat.dtype == torch.float32
    res = check_mean_values(x, hw, feat)
    if L.name == "tise_split_mean_both_nhwc":                     # the split row is the exact split of the fp32 row
        row = L.dsts[1][1].reshape(n, 2 * C)
        hi = feat.half()
        lo = ((feat - hi.float()) * 2048.0).half()
        ih, il = split_index(C, feat.device)
        assert torch.equal(row[:, ih], hi) and torch.equal(row[:, il], lo)
    return res


def check_tap(L, trunk):
    """tise_split_tap_rows: the scalars are the trunk's SPATIAL_*; row i of the destination is, bit for bit,
    merge(input)[i, :, :, c0:c0+nc] flattened in h, w, c order (hi + lo * 2**-11 is exact in fp64, so its fp32 rounding is
    the kernel's one fp32 addition) and exactly +0 from column hw * nc on; the input's bits are what they were.  Returns the
    number of values compared."""
    i = L.ints
    n, hw, C, c0, nc, ld = i[1], i[2], i[3], i[4], i[5], i[7]
    x = L.inputs[0]
    what = f"tap {L!r}"
    assert (c0, nc, ld) == (trunk.SPATIAL_C0, trunk.SPATIAL_NC, trunk.SPATIAL_LD), \
        f"{what}: channels [{c0}, {c0 + nc}) into rows of {ld}, the trunk states [{trunk.SPATIAL_C0}, {trunk.SPATIAL_C0 + trunk.SPATIAL_NC}) and {trunk.SPATIAL_LD}"
    assert x.dtype == torch.float16 and x.dim() == 4 and x.shape[0] == n and x.shape[1] * x.shape[2] == hw and x.shape[3] == 2 * C, \
        f"{what}: input {tuple(x.shape)} is not the (n, h, w, 2C) the scalars state"
    assert 0 <= c0 and c0 + nc <= C and hw * nc <= ld, what
    before, after = L.dsts[0]
    assert tuple(after.shape) == (n, ld) and after.dtype == torch.float32, f"{what}: destination {tuple(after.shape)}"
    used = hw * nc
    want = merge64(x)[..., c0:c0 + nc].float().reshape(n, used)
    bad = bits(after[:, :used]) != bits(want)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} values are not merge(input)[..., {c0}:{c0 + nc}] in h, w, c order " \
                                f"(first at row, column {tuple(int(v) for v in bad.nonzero()[0])})"
    pad = bits(after[:, used:])
    assert not bool((pad != 0).any()), f"{what}: {int((pad != 0).sum())} padding columns from {used} on are not +0"
    assert L.inputs_after is not None and torch.equal(bits(L.inputs_after[0]), bits(x)), f"{what}: the launch changed its input"
    return bad.numel()


def check_launch(L, trunk):
    """Dispatch on the launch's kind; returns (kind, figure) for the printed table."""
    if L.conv is not None:
        fc = L.conv is getattr(trunk, "sfc", None)
        return ("fc" if fc else "conv"), check_conv(L, fc)
    if L.name in STEMS:
        return "stem", check_stem(L, trunk)
    if L.name == TAP:
        return "tap", check_tap(L, trunk)
    if "pool" in L.name:
        return "pool", check_pool(L)
    return "mean", check_mean(L)


# ------------------------------------------------------------------------- the ResNet-50 and CountSeg routes
def split_halves(x):
    """fp32 (..., C) -> (hi, lo) fp16 of the split format: hi = fp16(x), lo = fp16((x - hi) * 2**11), both round-to-nearest-even."""
    hi = x.half()
    return hi, ((x - hi.float()) * 2048.0).half()


def _bits_equal(got, want, what):
    bad = bits(got) != bits(want)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} values differ (first at {tuple(int(v) for v in bad.nonzero()[0])})"


class ResNetRefs:
    """Where the ResNet-50 / CountSeg references take their parameters from: ``model.folded()`` (a resnet_model.ResNet50) and
    the head's own module (a countseg_model.CountSeg) -- never the kernels' packed forms.  ``tower`` (the HipResNet50 under
    audit) and ``counter`` (the HipCountSeg, or None) only say which SplitConv instance is which layer."""

    def __init__(self, model, tower, dev, counter=None, head=None):
        self.dev, self.tower, self.counter, self.head = dev, tower, counter, head
        self.folded = {k: (w.to(dev), b.to(dev)) for k, (w, b) in model.folded().items()}      # fp32, as resnet_hip.py receives them
        self.table = model.table.detach().float().to(dev)
        self.blocks = [name for name, _ in model.blocks()]

    def owners(self):
        """[(layer name, SplitConv)] of the tower as it stands (the padded stem exists once that route has run)."""
        t = self.tower
        out = [("conv1", t._stem_padded)] if t._stem_padded is not None else []
        for name, blk in zip(self.blocks, t.blocks):
            out += [(f"{name}.conv1", blk.conv1), (f"{name}.conv2", blk.conv2), (f"{name}.conv3", blk.conv3)]
            if blk.down is not None:
                out.append((f"{name}.downsample.0", blk.down))
        if self.counter is not None:
            out.append(("mix", self.counter.mix))
        return out

    def layer_of(self, conv):
        """(layer name, whether ``conv`` is that layer's ``_fallback``) of the SplitConv a launch came from."""
        for name, c in self.owners():
            if conv is c or conv is c._fallback:
                return name, conv is not c
        raise AssertionError("a convolution launch from a SplitConv that is no layer of the tower")

    def wb(self, layer):
        """fp64 (weight, bias) of the layer as its SplitConv received them: conv1 with 29 zero input channels, mix with a zero bias."""
        if layer == "mix":
            w = self.head.mix.weight.detach().double().to(self.dev)
            return w, torch.zeros(w.shape[0], dtype=torch.float64, device=self.dev)
        w, b = (t.double() for t in self.folded[layer])
        if layer == "conv1":
            w = torch.cat([w, torch.zeros((64, 29, 7, 7), dtype=torch.float64, device=self.dev)], 1)
        return w, b


def _table_values(u8, lut):
    """(n, h, w, 3) uint8 and the (3, 256) table -> fp32 (n, h, w, 3)."""
    return torch.stack([lut.view(3, 256)[ch][u8[..., ch].long()] for ch in range(3)], -1)


def check_stem7(L, refs):
    i = L.ints
    n, h, wd = i[2], i[3], i[4]
    u8, lut = L.inputs
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (n, h, wd, 3) and lut.numel() == 768
    _bits_equal(lut.reshape(-1), refs.table.reshape(-1), f"{L!r}: the table")
    w, b = (t.double() for t in refs.folded["conv1"])
    want = _nhwc(torch.relu(F.conv2d(_nchw(_table_values(u8, lut).double()), w, b, 2, 3)))
    before, after = L.dsts[0]
    assert tuple(after.shape) == (*want.shape[:3], 128), (L, after.shape, want.shape)
    scale = want.abs().max().item()
    err = (merge64(after) - want).abs().max().item()
    assert err <= CONV_TOL * scale, f"{L!r}: error {err:.3e} > {CONV_TOL:g} x scale {scale:.3e}"
    return err / scale


def check_input_split(L, refs):
    """tise_resnet_input_split: channels 0..2 the split of the table values, channels 3..31 +0 in both halves; bit for bit."""
    i = L.ints
    n, h, wd = i[2], i[3], i[4]
    u8, lut = L.inputs
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (n, h, wd, 3) and lut.numel() == 768
    _bits_equal(lut.reshape(-1), refs.table.reshape(-1), f"{L!r}: the table")
    x = torch.zeros((n, h, wd, 32), dtype=torch.float32, device=u8.device)
    x[..., :3] = _table_values(u8, lut)
    hi, lo = split_halves(x)
    after = L.dsts[0][1]
    assert tuple(after.shape) == (n, h, wd, 64) and after.dtype == torch.float16
    ih, il = split_index(32, after.device)
    _bits_equal(after[..., ih], hi, f"{L!r}: hi halves")
    _bits_equal(after[..., il], lo, f"{L!r}: lo halves")
    return 0.0


def check_residual(L, refs, block):
    """tise_residual_relu_split_nhwc of block number ``block``: fp32 torch operations in the kernel's order, (raw + bias) + u,
    relu, split; u = the merged identity or id_raw + id_bias.  Bit for bit; the range guard is clear after the launch."""
    i, p = L.ints, L.ptrs
    raw_ld, raw_off, pixels, C, out_ld, out_off = i[1], i[2], i[11], i[12], i[14], i[15]
    name = refs.blocks[block]
    assert (p[4] is None) != (p[7] is None), f"{L!r}: exactly one identity"
    assert (p[7] is not None) == (f"{name}.downsample.0" in refs.folded) == (p[10] is not None), f"{L!r}: the identity of {name}"
    raw = L.inputs[0]
    assert raw.dtype == torch.float32 and raw.numel() == pixels * raw_ld
    t = raw.reshape(pixels, raw_ld)[:, raw_off:raw_off + C] + refs.folded[f"{name}.conv3"][1]
    if p[4] is not None:
        ids, id_ld, id_off = L.inputs[1], i[5], i[6]
        assert ids.dtype == torch.float16 and ids.numel() == pixels * 2 * id_ld
        u = merge64(ids.reshape(pixels, 2 * id_ld))[:, id_off:id_off + C].float()          # hi + lo 2^-11 is exact in fp32
    else:
        idr, id_ld, id_off = L.inputs[2], i[8], i[9]
        assert idr.dtype == torch.float32 and idr.numel() == pixels * id_ld
        u = idr.reshape(pixels, id_ld)[:, id_off:id_off + C] + refs.folded[f"{name}.downsample.0"][1]
    hi, lo = split_halves(torch.relu(t + u))
    before, after = L.dsts[0]
    assert after.dtype == torch.float16 and after.numel() == pixels * 2 * out_ld and tuple(after.shape[:-1]) == tuple(raw.shape[:-1])
    got = after.reshape(pixels, 2 * out_ld)
    ih, il = split_index(out_ld, after.device)
    _bits_equal(got[:, ih[out_off:out_off + C]], hi, f"{L!r} ({name}): hi halves")
    _bits_equal(got[:, il[out_off:out_off + C]], lo, f"{L!r} ({name}): lo halves")
    assert L.flag is False, f"{L!r} ({name}): the range guard is raised after the launch"
    _untouched(L, 0, raw_mask(out_ld, out_off, out_off + C, True, after.device).view(*([1] * (after.dim() - 1)), -1))
    return 0.0


def check_head(L, refs):
    """tise_countseg_head against tests/_countseg_ref.head on the launch's recorded fp32 map and the module's own parameters:
    the confidences, the density means and the peak counts, bit for bit."""
    import numpy as np
    from tests import _countseg_ref as R
    i = L.ints
    ld, off, n, h, w, P, C = i[1], i[2], i[8], i[9], i[10], i[11], i[12]
    assert L.ptrs[16] is None, f"{L!r}: the route asks for no maps"
    mix = L.inputs[0]
    assert mix.dtype == torch.float32 and tuple(mix.shape) == (n, h, w, ld) and off + 2 * P <= ld
    m = refs.head
    f32 = lambda t: t.detach().float().cpu().numpy()                                       # noqa: E731
    assert (m.n_classes, m.width) == (C, P)
    T = (mix.cpu().numpy()[..., off:off + 2 * P] + f32(m.mix.bias)).astype(np.float32)
    conf, den, peaks, _ = R.head(T, f32(m.cls.weight).reshape(C, P), f32(m.cls.bias), f32(m.den.weight).reshape(C, P), f32(m.den.bias))
    got = [d[1].cpu().numpy() for d in L.dsts]
    assert got[0].shape == (n, C) and got[0].dtype == np.float64 and got[2].dtype == np.int32
    assert np.array_equal(got[2], peaks), f"{L!r}: {int((got[2] != peaks).sum())} peak counts differ"
    for g, r, what in ((got[0], conf, "confidences"), (got[1], den, "density means")):
        bad = g.view(np.int64) != np.ascontiguousarray(r).view(np.int64)
        assert not bad.any(), f"{L!r}: {int(bad.sum())} of {bad.size} {what} are not the restatement's bits (largest difference {np.abs(g - r).max():.3e})"
    return 0.0


def check_resnet_launch(L, refs, block=None):
    """Dispatch on the launch's kind; returns (kind, figure).  ``block``: which bottleneck a residual launch ends."""
    if L.conv is not None:
        layer, _ = refs.layer_of(L.conv)
        raw = layer == "mix" or layer.endswith((".conv3", ".downsample.0"))
        assert raw == all(sg[4] == 1 for sg in L.segs), f"{L!r}: {layer} writes {'split' if raw else 'fp32'} segments"
        return ("raw" if raw else "conv"), check_conv(L, raw=raw, wb=refs.wb(layer))
    if L.name == STEM7:
        return "stem", check_stem7(L, refs)
    if L.name == INPUT_SPLIT:
        return "input", check_input_split(L, refs)
    if L.name == RESIDUAL:
        return "residual", check_residual(L, refs, block)
    if L.name == HEAD:
        return "head", check_head(L, refs)
    if "pool" in L.name:
        return "pool", check_pool(L)
    assert L.name == "tise_split_mean_nhwc", L.name
    return "mean", check_mean(L)


def module_convs(model, h, w):
    """(Cin, Cout, kh, kw, sh, sw, ph, pw, OH, OW) of the 53 ``nn.Conv2d`` of a resnet_model.ResNet50 on an h x w image, in
    launch order, by the size arithmetic alone: conv1, MaxPool2d(3, 2, 1), then per block conv1, conv2, conv3 and, where there
    is one, the downsample convolution on the block's input."""
    def member(c, h, w):
        oh = (h + 2 * c.padding[0] - c.kernel_size[0]) // c.stride[0] + 1
        ow = (w + 2 * c.padding[1] - c.kernel_size[1]) // c.stride[1] + 1
        return (c.in_channels, c.out_channels, *c.kernel_size, *c.stride, *c.padding, oh, ow)
    out = [member(model.conv1, h, w)]
    h, w = out[-1][8:]
    h, w = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
    for _, blk in model.blocks():
        out.append(member(blk.conv1, h, w))
        out.append(member(blk.conv2, *out[-1][8:]))
        out.append(member(blk.conv3, *out[-1][8:]))
        if blk.downsample is not None:
            out.append(member(blk.downsample[0], h, w))
            assert out[-1][8:] == out[-2][8:]
        h, w = out[-1][8:]
    assert len(out) == sum(isinstance(m, torch.nn.Conv2d) for m in model.modules()) == 53
    return out


def resnet_dispatch(h, w):
    """What conv_split.py's dispatch gives the 52 block convolutions of an h x w image, from pick_tn, rowwin_applies, rowwin_fits
    and rowwin_divides alone (no device): ({(tn, window pieces): row-window launches}, {row width: launches that fall back to
    the default kernel})."""
    import collections
    from tise_toolbox_amd import conv_split, resnet_model
    rowwin, fallback = collections.Counter(), collections.Counter()
    for cin, cout, kh, kw, sh, sw, ph, pw, oh, ow in module_convs(resnet_model.ResNet50(), h, w)[1:]:
        tn = conv_split.pick_tn(cout)
        if conv_split.rowwin_applies(cin, cout, kh, kw, (sh, sw), (ph, pw), tn):
            if conv_split.rowwin_fits(ow, kw) and conv_split.rowwin_divides(ow, kw):
                rowwin[(tn, rowwin_np(ow, kw))] += 1
            else:
                fallback[ow] += 1
    return dict(rowwin), dict(fallback)


# ------------------------------------------------------------------------------------- how the launches fit together
def own_rows(L):
    """[(destination index, 1-D bool mask over the destination's raw row)]: the elements of a pixel's row the launch writes."""
    dev = L.dsts[0][1].device
    if L.conv is not None:
        out = {}
        for c0, c1, di, off, mode in L.segs:
            after = L.dsts[di][1]
            split = mode == 0
            C = after.shape[3] // 2 if split else after.shape[3]
            m = raw_mask(C, off, off + (c1 - c0 if split else -(-(c1 - c0) // 8) * 8), split, dev)
            out[di] = m if di not in out else (out[di] | m)
        return sorted(out.items())
    if "pool" in L.name:
        i = L.ints
        out_ld, out_off = (i[9], i[10]) if "avgpool" in L.name else (i[8], i[9])
        return [(0, raw_mask(out_ld, out_off, out_off + i[6], True, dev))]
    if L.name == RESIDUAL:
        i = L.ints
        return [(0, raw_mask(i[14], i[15], i[15] + i[12], True, dev))]
    return [(di, torch.ones(d[1].shape[-1], dtype=torch.bool, device=dev)) for di, d in enumerate(L.dsts)]


def check_assembly(launches):
    """The segment lists of trunk.py as a whole: every element of every tensor a launch reads was written by exactly one
    earlier launch -- a segment that lands 8 channels off inside a concat buffer overlaps its neighbour's slice (reported at
    that launch) and leaves a gap (reported at the first launch that reads the buffer).  The tap reads channels
    [c0, c0 + nc) of its source only: those must have been written (once: an overlap is reported at its writer) by earlier
    launches -- a tap in front of the block that fills them, or on a buffer no launch wrote, is reported at the tap; it does
    not close the buffer to further writers.  Returns the list of failures.
    (Two whole branches of equal width written to each other's slices would pass here: every later layer then sees its
    input channels permuted, which the end-to-end tests catch at any tolerance.)"""
    state, fails = {}, []                                         # data pointer -> [written mask, sealed by a reader]
    for k, L in enumerate(launches):
        st = state.get(L.in_ptr)
        if L.name == TAP:
            i = L.ints
            need = raw_mask(i[3], i[4], i[4] + i[5], True, L.inputs[0].device)
            if st is None or st[0].numel() != need.numel():
                fails.append(f"launch {k}: tap {L!r} reads a tensor no earlier launch has written")
            elif not bool(st[0][need].all()):
                fails.append(f"launch {k}: tap {L!r} reads {int((~st[0][need]).sum())} raw row elements of channels "
                             f"[{i[4]}, {i[4] + i[5]}) that no earlier launch has written")
        else:                                                     # every tensor it reads (the residual launch: two)
            for ptr in (L.read_ptrs or [L.in_ptr]):
                st = state.get(ptr)
                if st is not None:
                    if not bool(st[0].all()) and not st[1]:
                        fails.append(f"launch {k}: {L!r} reads a tensor with {int((~st[0]).sum())} raw row elements no launch has written")
                    st[1] = True
        for di, own in own_rows(L):
            ptr = L.dst_ptrs[di]
            st = state.get(ptr)
            if st is None or st[1] or st[0].numel() != own.numel():
                st = state[ptr] = [torch.zeros_like(own), False]   # a new tensor (the allocator hands addresses out again)
            if bool((st[0] & own).any()):
                fails.append(f"launch {k}: {L!r} writes {int((st[0] & own).sum())} raw row elements of destination {di} that an earlier launch wrote")
            st[0] |= own
    for ptr, st in state.items():
        if not st[1] and not bool(st[0].all()):
            fails.append(f"a tensor no launch read (an output of the forward) has {int((~st[0]).sum())} raw row elements unwritten")
    return fails


# ------------------------------------------------------------------------------------------------- what was launched
def rowwin_np(ow, kw):
    """Window pieces per wave of the row-window kernel (csrc/conv_split.hip rowwin_np)."""
    j = (ow + 126) // ow + 1
    return -(-(128 + j * (kw - 1) + 1) // 32)


def instance_of(L):
    """The kernel template instance a recorded convolution launch selects, as the dispatchers in csrc/conv_split.hip
    (tise_conv_split_f16, launch_rowwin_any, launch_poolin) and csrc/conv_pipe.hip (launch_regw32, launch_regw32_pool) do."""
    code, a = L.code, L.args
    if code & 512:
        assert code & 255 == 34
        return ("pipe34", a["Cout"], "padded" if (a["PH"] | a["PW"]) else "unpadded",
                "pooled" if code & 1024 else ("border" if a["out_hp"] else "plain"))
    if code & 256:
        return ("poolin", 2 if a["Cout"] <= 128 else 4, "VT" if code & 2048 else "9tap")
    if code & 64:
        return ("rowwin", code & 15, a["Cin"] % 32, rowwin_np(a["OW"], a["KW"]), "POOLH" if code & 2048 else "")
    if code & 128:
        return ("fast", code & 15, a["Cin"] % 32, "block" if code & 4096 else "tap")
    return ("glds", code & 15, a["Cin"] % 32)


def conv_members(launches):
    """(Cin, Cout, kh, kw, sh, sw, ph, pw, OH, OW) of every convolution the launches compute: a fused 1x1 launch counts once
    per segment; a launch that reads a zero-bordered buffer another launch filled (out_pad) carries that border as its padding."""
    borders, out = {}, []
    for L in launches:
        if L.conv is None:
            continue
        c, a = L.conv, L.args
        ph, pw = c.padding
        if L.in_ptr in borders:
            y0, x0 = borders[L.in_ptr]
            ph, pw = ph + y0, pw + x0
        if L.kw.get("out_pad"):
            for p in L.dst_ptrs:
                borders[p] = tuple(L.kw["out_pad"][2:])
        for c0, c1, _, _, _ in L.segs:
            out.append((c.cin, c1 - c0, c.kh, c.kw, *c.stride, ph, pw, a["OH"], a["OW"]))
    return out


def tensor_sizes(launches):
    """{description: (elements per image, bytes per image)} of every activation tensor the launches read or wrote."""
    out = {}
    for L in launches:
        for t in list(L.inputs[:1]) + [d[1] for d in L.dsts]:
            n = t.shape[0]
            key = f"{'x'.join(str(s) for s in t.shape[1:])} {str(t.dtype).replace('torch.', '')}"
            out[key] = (t.numel() // n, t.numel() // n * t.element_size())
    return out
