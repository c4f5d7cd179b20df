"""GPU: csrc/calibrate.hip pinned at every kernel instance, lane slot and input edge.

tests/test_gpu_calibration.py compares sums over seeded rows; here single rows are looked at.  The kernel returns sums only, so
a PROBE row sits in a field of NEUTRAL rows: logit 0 at the label, -1e4 elsewhere, T <= 10.  exp(-1e4 / T) is exactly 0, so a
neutral row has s = 1, nll = +0, g = +0, confidence 1 and a correct prediction: it adds exact zeros to the two sums and a 1 to
the top bin.  The sums that come back are then the probe's own nll and g, compared with the fp64 oracle's PER-ROW bound
(tests/_calib_ref.py: twice the bound, the oracle's own error being checked against mpmath in tests/test_calibration_host.py;
no fold term, nothing was folded).  Bin, count and correct are compared exactly: every probe's 1 / s is asserted, from mpmath
alone, to be further than 1e-10 (relative) from an fp32 rounding boundary, and its fl32 confidence to be a multiple of the
top bin's fp64 spacing, so conf_sum is exact as well.

Instances (calib_shape): <4,16> C <= 64, <8,16> <= 128, <16,16> <= 256, <64,16> <= 1024, <64,32> <= 2048, <64,0> (streaming)
above.  PIN_C has both sides of every dispatch edge; 2047 and 2111 are the odd widths of the last two (the -FLT_MAX padding
of <64,32>, a partial last pass of the streaming form).  R = 64 / G rows share a wave, rpb = 4 R rows a block step.

Memory hygiene as in test_gpu_calibration.py: every matrix lives in a NaN-filled allocation, the workspace and the output of the
direct C ABI calls have exactly the documented size between guard bytes.  Every launch is a legal input."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from tests import _calib_ref as R
from tests.test_gpu_calibration import TEMPS, check_case
from tise_toolbox_amd import _lib, device

pytestmark = pytest.mark.gpu

PIN_C = [64, 65, 128, 129, 256, 257, 1024, 1025, 2047, 2048, 2049, 2111]
INSTANCE_C = [64, 128, 256, 1024, 2048, 2049]                        # one width per kernel instance
T_PROBE = 0.598
FLT_MAX = float(np.finfo(np.float32).max)
NAN, INF = float("nan"), float("inf")
SENTINEL = -7.25                                                     # what the guard doubles around `out` hold
GUARD_BYTES = 256
WORST = {}                                                           # instance -> [nll error / bound, g error / bound]


@pytest.fixture(scope="module")
def dev(cuda_device):
    torch.cuda.set_device(cuda_device)
    yield cuda_device
    for inst in sorted(WORST):
        print(f"\ncalibrate.hip {inst}: worst error / bound  nll {WORST[inst][0]:.3f}  g {WORST[inst][1]:.3f}", end="")
    print()


def record(C, e_nll, b_nll, e_g, b_g):
    w = WORST.setdefault(R.instance_of(C), [0.0, 0.0])
    w[0] = max(w[0], e_nll / b_nll if e_nll else 0.0)
    w[1] = max(w[1], e_g / b_g if e_g else 0.0)


def default_edges(n_bins):
    return torch.linspace(0, 1, n_bins + 1).numpy()


# ---- the C ABI, called directly between guards -------------------------------------------------------------------------------
def guarded_eval(buf, labels_dev, c0, C, T, edges, rows=None, expect=_lib.TISE_OK):
    """tise_calib_eval with a workspace of exactly tise_calib_workspace_bytes bytes and an output of exactly 4 + 3 n_bins
    doubles, both inside guarded buffers; -> the output (numpy), or None for a refused call, whose output must be untouched."""
    dev = buf.device
    rows = int(buf.shape[0]) if rows is None else rows
    nb = len(edges) - 1
    P = 4 + 3 * nb
    edges_dev = torch.as_tensor(np.asarray(edges, np.float32)).to(dev)
    need = ctypes.c_size_t()
    _lib.call("tise_calib_workspace_bytes", rows, C, nb, ctypes.byref(need))
    assert need.value % 8 == 0
    ws = torch.full((need.value + 2 * GUARD_BYTES,), 0xA5, dtype=torch.uint8, device=dev)
    out = torch.full((P + 16,), SENTINEL, dtype=torch.float64, device=dev)
    status = _lib.load().tise_calib_eval(
        ctypes.c_void_p(buf.data_ptr()), rows, buf.stride(0), c0, C, ctypes.c_void_p(labels_dev.data_ptr()), float(T),
        ctypes.c_void_p(edges_dev.data_ptr()), nb, ctypes.c_void_p(out.data_ptr() + 64),
        ctypes.c_void_p(ws.data_ptr() + GUARD_BYTES), need.value, device._stream())
    torch.cuda.current_stream().synchronize()
    assert status == expect, (status, expect, T)
    o, w = out.cpu().numpy(), ws.cpu().numpy()
    assert np.all(o[:8] == SENTINEL) and np.all(o[8 + P:] == SENTINEL), "write outside the 4 + 3 n_bins output doubles"
    assert np.all(w[:GUARD_BYTES] == 0xA5) and np.all(w[GUARD_BYTES + need.value:] == 0xA5), "write outside the workspace"
    if status != _lib.TISE_OK:
        assert np.all(o == SENTINEL), "a refused call wrote its output"
        return None
    return o[8:8 + P].copy()


def check_raw(raw, z, y, T, edges, what, exact_nll_g=None):
    """check_case's comparison (test_gpu_calibration.py) for a raw output and any ascending edges."""
    nb, rows = len(edges) - 1, z.shape[0]
    with np.errstate(all="ignore"):
        o = R.oracle(z, y, T, nb, edges=np.asarray(edges, np.float32))
    assert raw[2] == 0 and raw[3] == 0, (what, raw[:4])
    if exact_nll_g is None:
        e_nll, e_g = abs(raw[0] - o["nll"]), abs(raw[1] - o["g"])
        assert e_nll <= o["b_nll"], (what, raw[0], o["nll"], o["b_nll"])
        assert e_g <= o["b_g"], (what, raw[1], o["g"], o["b_g"])
        record(z.shape[1], e_nll, o["b_nll"], e_g, o["b_g"])
    assert np.array_equal(raw[4:4 + nb], o["count"]), (what, raw[4:4 + nb], o["count"])
    assert np.array_equal(raw[4 + 2 * nb:], o["correct"]), what
    assert np.all(np.abs(raw[4 + nb:4 + 2 * nb] - o["conf"]) <= 2 * R.gamma(rows) * o["conf"] + 2 * 2.0 ** -24), what
    assert raw[4:4 + nb].sum() == rows
    return o


# ---- 1. both sides of every dispatch edge against the oracle ---------------------------------------------------------------------
def _recorded_case(dev, rows, C, T, seed, **kw):
    r = check_case(dev, rows, C, T, seed, **kw)
    z, y = R.make_logits(rows, C, T, seed)
    o = R.oracle(z, y, T, kw.get("n_bins", 15))
    record(C, abs(r["nll_sum"] - o["nll"]), o["b_nll"], abs(r["grad_sum"] - o["g"]), o["b_g"])


@pytest.mark.parametrize("C", [c for c in PIN_C if c not in (64, 65, 2048)])     # those three: test_kernel_against_fp64_oracle
def test_dispatch_edges_against_fp64_oracle(dev, C):
    rpb = R.rows_per_block(C)
    for i, rows in enumerate([1, 3, 64, 65, 5 * rpb - 1, 5 * rpb + 1]):
        _recorded_case(dev, rows, C, TEMPS[i % len(TEMPS)], seed=1000 * C + rows)
    for i, T in enumerate(TEMPS):                                      # every temperature, strided rows off column 1
        _recorded_case(dev, 257, C, T, seed=7 * C + i, c0=1, extra_cols=3)


@pytest.mark.parametrize("C,rows,n_bins", [(1000, 1500, 64), (2049, 600, 64), (257, 400, 1)])
def test_bin_lanes_on_the_wide_instances(dev, C, rows, n_bins):
    """n_bins = 64 where a row takes the whole wave (G = 64): the lanes that own the bins are the lanes that hold the row."""
    _recorded_case(dev, rows, C, 0.598, seed=31 * C, n_bins=n_bins)
    _recorded_case(dev, rows, C, 10.0, seed=37 * C, n_bins=n_bins, c0=1, extra_cols=3)


# ---- probe rows ------------------------------------------------------------------------------------------------------------------
class Field:
    """N neutral rows at column 1 of a NaN-filled (N + 1, C + 2) device buffer, and the evaluator over them; put() turns
    one row into a probe with device writes, restore() makes it neutral again."""

    def __init__(self, dev, C, N, n_bins=15):
        self.C, self.N, self.nb = C, N, n_bins
        self.y0 = (np.arange(N) * 7 + 3) % C
        self.buf = torch.full((N + 1, C + 2), NAN, dtype=torch.float32, device=dev)
        self.body = self.buf[:N, 1:1 + C]
        self.body.fill_(-1e4)
        self.body[torch.arange(N, device=dev), torch.from_numpy(self.y0).to(dev)] = 0.0
        self.ev = device.CalibrationEvaluator(self.buf[:N], torch.from_numpy(self.y0), c0=1, num_classes=C, n_bins=n_bins)
        self.edges = default_edges(n_bins)

    def put(self, p, row_dev, label):
        self.body[p] = row_dev
        self.ev.labels[p] = int(label)

    def restore(self, p):
        self.body[p] = -1e4
        self.body[p, int(self.y0[p])] = 0.0
        self.ev.labels[p] = int(self.y0[p])

    def raw(self):
        return self.ev.raw(T_PROBE)

    def neutral(self, n):
        cnt = np.zeros(self.nb)
        cnt[-1] = n
        return cnt

    def check_probe(self, raw, ref, what):
        """raw is the field with ONE probe row whose per-row reference is ref (probe_ref)."""
        e_nll, e_g = abs(raw[0] - ref["nll"]), abs(raw[1] - ref["g"])
        assert e_nll <= 2 * ref["b_nll"], (what, raw[0], ref["nll"], ref["b_nll"])
        assert e_g <= 2 * ref["b_g"], (what, raw[1], ref["g"], ref["b_g"])
        record(self.C, e_nll, 2 * ref["b_nll"], e_g, 2 * ref["b_g"])
        assert raw[2] == 0 and raw[3] == 0, (what, raw[:4])
        # N - 1 + conf and every partial sum of it are exact in fp64 when conf is a multiple of ulp(N) = 2^(bits - 52)
        bits = math.ceil(math.log2(self.N + 1))
        assert math.ldexp(float(ref["conf"]), 52 - bits) % 1.0 == 0.0, "probe confidence too small for an exact bin sum"
        cnt, csum, cor = R.bin_rows(np.array([ref["conf"]]), np.array([ref["correct"]]), self.edges)
        nb, base = self.nb, self.neutral(self.N - 1)
        assert np.array_equal(raw[4:4 + nb], base + cnt), (what, raw[4:4 + nb])
        assert np.array_equal(raw[4 + nb:4 + 2 * nb], base + csum), (what, raw[4 + nb:4 + 2 * nb], csum)
        assert np.array_equal(raw[4 + 2 * nb:], base + cor), (what, raw[4 + 2 * nb:], cor)

    def check_dropped(self, raw, n_nonfinite, n_badlabel, what):
        """raw is the field with ONE row the kernel must leave out: exact zeros, the counters, N - 1 neutral rows."""
        assert raw[2] == n_nonfinite and raw[3] == n_badlabel, (what, raw[:4])
        assert raw[0] == 0.0 and raw[1] == 0.0, (what, raw[:2])
        base = self.neutral(self.N - 1)
        for k in range(3):
            assert np.array_equal(raw[4 + k * self.nb:4 + (k + 1) * self.nb], base), (what, k, raw[4:])


def probe_ref(z_row, label, T=T_PROBE):
    """Per-row reference of one probe: the fp64 oracle's row, and -- from mpmath alone -- the proof that fl32(1 / s) is not a
    close call."""
    o = R.oracle_rows(z_row[None, :], np.array([label]), T)
    _, _, inv_s = R.mp_row(z_row, label, T)
    assert R.fp32_midpoint_distance(inv_s) > 1e-10, "probe row's 1 / s sits on an fp32 rounding boundary: choose another"
    assert o["conf"][0] == np.float32(float(inv_s))
    return {"nll": o["nll"][0], "g": o["g"][0], "b_nll": o["b_nll"][0], "b_g": o["b_g"][0], "conf": o["conf"][0],
            "correct": int(o["pred"][0] == label)}


def clear_row(C, seed, shape_it):
    """The first of the seeded rows seed, seed + 10^6, ... (shaped by shape_it) whose 1 / s is clear of every fp32 rounding
    boundary by 1e-9: about one seeded row in 30 is not, and which ones is decided here from mpmath, before any launch."""
    for k in range(16):
        z = np.random.default_rng(seed + 10 ** 6 * k).standard_normal(C).astype(np.float32)
        shape_it(z)
        if R.fp32_midpoint_distance(R.mp_row(z, 0, T_PROBE)[2]) > 1e-9:
            return z
    raise AssertionError("no seeded probe row clear of an fp32 rounding boundary")


@functools.lru_cache(maxsize=None)
def probe_variants(C):
    """[(name, row, [(label, reference)])] -- (a) unique maximum at column 0, label C - 1; (b) maximum at column C - 1, the
    label swept over the lane / k corners; (c) two tied maxima in one lane (columns G - 1 and 2 G - 1), in adjacent lanes
    (1 and 2) and at the two ends; the label is the second, so the first must win and the row is not correct."""
    G, _ = R.calib_shape(C)

    def peak(j1, j2):
        def shape_it(z):
            keep = np.ones(C, bool)
            keep[[j1, j2]] = False
            z[j1] = z[j2] = z[keep].max() + np.float32(2.0)
        return shape_it
    out = [("max@0", clear_row(C, 11 * C, peak(0, 0)), [C - 1]),
           ("max@C-1", clear_row(C, 11 * C + 1, peak(C - 1, C - 1)), sorted({0, 1, G - 1, G, (C - 1) // 2, C - 2, C - 1}))]
    for i, (name, j1, j2) in enumerate((("tie same lane", G - 1, 2 * G - 1), ("tie adjacent lanes", 1, 2),
                                        ("tie ends", 0, C - 1))):
        out.append((name, clear_row(C, 11 * C + 2 + i, peak(j1, j2)), [j2]))
    res = []
    for name, z, labels in out:
        refs = [(y, probe_ref(z, y)) for y in labels]
        if name.startswith("tie"):
            assert refs[0][1]["correct"] == 0
        res.append((name, z, refs))
    return res


def slots(C, N):
    r = 64 // R.calib_shape(C)[0]
    rpb = R.rows_per_block(C)
    return sorted({0, 1, r - 1, r, rpb - 1, rpb, 2 * rpb - 1, N - 1})


@pytest.mark.parametrize("C", PIN_C)
def test_probe_at_every_slot(dev, C):
    """One probe among 2 rpb + 2 neutral rows, at the first / last lane group of a wave, of a block step and of the matrix."""
    N = 2 * R.rows_per_block(C) + 3
    f = Field(dev, C, N)
    raw = f.raw()
    assert raw[0] == 0.0 and raw[1] == 0.0 and np.array_equal(raw[4:19], f.neutral(N)), "the neutral field is not neutral"
    for name, z, refs in probe_variants(C):
        row = torch.from_numpy(z).to(dev)
        for p in slots(C, N):
            for y, ref in refs:
                f.put(p, row, y)
                f.check_probe(f.raw(), ref, (C, name, "slot", p, "label", y))
            f.restore(p)
    raw = f.raw()
    assert raw[0] == 0.0 and raw[1] == 0.0 and np.array_equal(raw[4:19], f.neutral(N))


@pytest.mark.parametrize("C", INSTANCE_C)
def test_probe_past_the_grid_cap(dev, C):
    """2048 blocks x rpb rows is one grid step; the probe is the first row of the second step, then the last row of a
    partial wave group behind it."""
    G, _ = R.calib_shape(C)
    rpb = R.rows_per_block(C)
    N = 2048 * rpb + 64 // G + 1
    f = Field(dev, C, N)
    for name, z, refs in probe_variants(C):
        if name not in ("max@0", "tie adjacent lanes"):
            continue
        row = torch.from_numpy(z).to(dev)
        for p in (2048 * rpb, N - 1):
            y, ref = refs[0]
            f.put(p, row, y)
            f.check_probe(f.raw(), ref, (C, name, "slot", p))
            f.restore(p)
    bad = torch.from_numpy(probe_variants(C)[0][1]).to(dev).clone()
    bad[C - 1] = NAN
    for p in (2048 * rpb, N - 1):
        f.put(p, bad, C)
        f.check_dropped(f.raw(), 1, 1, (C, "bad row at", p))
        f.restore(p)


# ---- 4. bad rows at every instance -----------------------------------------------------------------------------------------------
def bad_kinds(C):
    """[(name, {column: value}, label or None, rows with a non-finite logit, rows with a bad label)]"""
    G, K = R.calib_shape(C)
    last_k = G * ((C - 1) // G)                      # lane 0's last live column: G (K - 1) when C fills the registers
    kinds = [("nan@0", {0: NAN}, None, 1, 0), ("+inf@0", {0: INF}, None, 1, 0), ("-inf@0", {0: -INF}, None, 1, 0),
             ("nan@C-1", {C - 1: NAN}, None, 1, 0), ("nan@last k of lane 0", {last_k: NAN}, None, 1, 0),
             ("-inf@last lane, first k", {G - 1: -INF}, None, 1, 0), ("nan@C/2", {C // 2: NAN}, None, 1, 0),
             ("label C", {}, C, 0, 1), ("label -1", {}, -1, 0, 1), ("label int32 min", {}, -2 ** 31, 0, 1),
             ("nan@0 + label C", {0: NAN}, C, 1, 1), ("-inf@C-1 + label -1", {C - 1: -INF}, -1, 1, 1)]
    if K == 0:                                       # the streaming form's later passes over the row
        kinds += [("nan@69 (second pass)", {69: NAN}, None, 1, 0), ("+inf@2048 (last pass)", {2048: INF}, None, 1, 0)]
    return kinds


@pytest.mark.parametrize("C", PIN_C)
def test_bad_row_is_counted_and_its_neighbours_are_not_touched(dev, C):
    N = 2 * R.rows_per_block(C) + 3
    f = Field(dev, C, N)
    base = probe_variants(C)[0][1]
    for name, cells, label, nf, bl in bad_kinds(C):
        z = base.copy()
        for col, v in cells.items():
            z[col] = v
        row = torch.from_numpy(z).to(dev)
        for p in slots(C, N):
            f.put(p, row, C - 1 if label is None else label)
            f.check_dropped(f.raw(), nf, bl, (C, name, "slot", p))
            f.restore(p)
    # two bad rows side by side in one wave, a good probe between bad rows
    name, z, refs = probe_variants(C)[0]
    good, bad = torch.from_numpy(z).to(dev), torch.from_numpy(z).to(dev).clone()
    bad[C - 1] = NAN
    f.put(0, bad, C - 1)
    f.put(2, bad, C)
    raw = f.raw()
    assert raw[2] == 2 and raw[3] == 1 and raw[0] == 0.0 and raw[1] == 0.0 and raw[4 + 14] == N - 2, (C, raw[:4])
    f.put(1, good, refs[0][0])
    raw = f.raw()
    assert raw[2] == 2 and raw[3] == 1 and raw[4:19].sum() == N - 2
    assert abs(raw[0] - refs[0][1]["nll"]) <= 2 * refs[0][1]["b_nll"] and abs(raw[1] - refs[0][1]["g"]) <= 2 * refs[0][1]["b_g"]
    with pytest.raises(ValueError, match="2 row.s. with a non-finite logit, 1 row.s. with a label outside"):
        f.ev(T_PROBE)


@pytest.mark.parametrize("C", PIN_C)
def test_flt_max_logits_are_finite_and_accepted(dev, C):
    """+-FLT_MAX are finite logits: the row is evaluated, and -FLT_MAX as a REAL column is what the padding holds."""
    N = 2 * R.rows_per_block(C) + 3
    f = Field(dev, C, N)
    z = probe_variants(C)[0][1].copy()
    z[0], z[1], z[C - 1] = FLT_MAX, -FLT_MAX, -FLT_MAX
    row = torch.from_numpy(z).to(dev)
    with np.errstate(over="ignore"):
        refs = [(y, probe_ref(z, y)) for y in (0, 1, C - 1)]
    assert refs[0][1]["nll"] == 0.0 and refs[0][1]["g"] == 0.0 and refs[0][1]["conf"] == 1.0
    for p in slots(C, N):
        for y, ref in refs:
            f.put(p, row, y)
            f.check_probe(f.raw(), ref, (C, "FLT_MAX row", "slot", p, "label", y))
        f.restore(p)


# ---- 5. the bits depend on (rows, C) only ------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", PIN_C)
def test_bits_do_not_depend_on_the_embedding_or_the_stream(dev, C):
    rows, T, nb = 5 * R.rows_per_block(C) + 1, 0.598, 15
    z, y = R.make_logits(rows, C, T, seed=13 * C)
    y_dev = torch.from_numpy(y).to(dev, torch.int32)
    edges = default_edges(nb)
    outs = []
    for c0, extra in ((0, 0), (1, 0), (3, 5)):
        buf, _ = R.embed(z, c0, extra, dev)
        outs.append(guarded_eval(buf, y_dev, c0, C, T, edges))
    buf, _ = R.embed(z, 0, 0, dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        outs.append(guarded_eval(buf, y_dev, 0, C, T, edges))
    torch.cuda.current_stream().wait_stream(side)
    check_raw(outs[0], z, y, T, edges, (C, "contiguous"))
    for o, name in zip(outs[1:], ("c0 = 1", "c0 = 3, five extra columns", "side stream")):
        assert np.array_equal(o, outs[0]), (C, name)


# ---- 6. C ABI edges --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", INSTANCE_C)
def test_zero_rows(dev, C):
    buf = torch.full((1, C), NAN, dtype=torch.float32, device=dev)
    y = torch.full((1,), -1, dtype=torch.int32, device=dev)
    for nb in (1, 15, 64):
        out = guarded_eval(buf, y, 0, C, 1.0, default_edges(nb), rows=0)
        assert out.shape == (4 + 3 * nb,) and np.all(out == 0.0), (C, nb, out)


@pytest.mark.parametrize("C", PIN_C)
def test_non_uniform_edges(dev, C):
    """The ABI takes any ascending edges.  0.50000006 is the fp32 after 0.5: rows with confidence exactly 0.5 (two tied
    maxima) belong to (0.1, 0.5], a row at 0.5 + 2^-24 to the one-value bin (0.5, 0.50000006], one at 0.5 + 2^-23 above."""
    edges = np.array([0.0, 0.1, 0.5, 0.50000006, 1.0], np.float32)
    assert edges[3] == np.nextafter(np.float32(0.5), np.float32(1))
    T = 1.0
    z, y = R.make_logits(5 * R.rows_per_block(C) + 1, C, T, seed=17 * C)
    extra = np.full((4, C), -1e4, np.float32)
    extra[:, 0] = 0.0
    extra[0, C - 1] = 0.0                                              # 1/2
    extra[1, C - 1] = -2.0 ** -22                                      # 1 / (2 - 2^-22) = 1/2 + 2^-24 (+ 2^-47)
    extra[2, C - 1] = -2.0 ** -21                                      # 1/2 + 2^-23
    extra[3, 1:4] = 0.0                                                # 1/4
    z = np.concatenate([z, extra])
    y = np.concatenate([y, [C - 1, 0, C - 1, 3]])
    for i in range(len(extra)):                                        # none of them a close call for fl32
        assert R.fp32_midpoint_distance(R.mp_row(z[len(z) - 4 + i], 0, T)[2]) > 1e-10
    buf, _ = R.embed(z, 1, 2, dev)
    raw = guarded_eval(buf, torch.from_numpy(y).to(dev, torch.int32), 1, C, T, edges)
    o = check_raw(raw, z, y, T, edges, (C, "non-uniform edges"))
    assert o["count"][2] >= 1 and o["count"][1] >= 2 and o["count"][3] >= 1       # the built rows landed where they were aimed


# ---- 7. the temperature domain ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [50, 200, 1025, 2049])
def test_temperature_domain_upper_end(dev, C):
    """T = 2^100, the largest accepted: the padded columns of the register forms still contribute exactly 0."""
    T = 2.0 ** 100
    z, y = R.make_logits(5 * R.rows_per_block(C) + 1, C, 1.0, seed=19 * C)
    buf, _ = R.embed(z, 1, 3, dev)
    raw = guarded_eval(buf, torch.from_numpy(y).to(dev, torch.int32), 1, C, T, default_edges(15))
    check_raw(raw, z, y, T, default_edges(15), (C, "T = 2^100"))


@pytest.mark.parametrize("C", [50, 200, 1025, 2049])
def test_temperature_domain_lower_end(dev, C):
    """T = 2^-1000 (1 / T = 2^1000 is finite): every logit below the maximum underflows, so with the label on the first
    of k tied maxima nll = log k and g = 0 exactly; the kernel's nll may differ by log's ulp and the fold."""
    T = 2.0 ** -1000
    rows = 5 * R.rows_per_block(C) + 1
    rng = np.random.default_rng(23 * C)
    z = (rng.standard_normal((rows, C)) * 3.0).astype(np.float32)
    y = np.zeros(rows, np.int64)
    ks = 1 + np.arange(rows) % 5
    for i in range(rows):
        cols = np.sort(rng.choice(C, size=ks[i], replace=False))
        z[i, cols] = z[i].max() + np.float32(1.0)
        y[i] = cols[0]
    want = np.log(ks.astype(np.float64)).sum()
    buf, _ = R.embed(z, 1, 3, dev)
    raw = guarded_eval(buf, torch.from_numpy(y).to(dev, torch.int32), 1, C, T, default_edges(15))
    o = check_raw(raw, z, y, T, default_edges(15), (C, "T = 2^-1000"), exact_nll_g=True)
    assert o["g"] == 0.0 and abs(o["nll"] - want) <= (2 * R.U + R.gamma(rows)) * want
    assert raw[1] == 0.0, (C, raw[1])
    e = abs(raw[0] - want)
    assert e <= 2 * (2 * R.U + R.gamma(rows)) * want, (C, raw[0], want)
    record(C, e, 2 * (2 * R.U + R.gamma(rows)) * want, 0.0, 1.0)
    assert raw[4 + 2 * 15:].sum() == rows                              # the first tied column is the prediction


@pytest.mark.parametrize("C", [50, 2049])
def test_temperature_outside_the_domain_is_refused_before_any_launch(dev, C):
    z, _ = R.make_logits(9, C, 1.0, seed=29 * C)
    y = np.argmax(z, axis=1)                                           # label on the maximum: dy / T stays 0
    buf, _ = R.embed(z, 0, 0, dev)
    y_dev = torch.from_numpy(y).to(dev, torch.int32)
    for T in (5e-324, 1e-310, 2.0 ** -1024, float(np.nextafter(2.0 ** 100, np.inf)), 2.0 ** 101, 1e38, 1e300):
        assert guarded_eval(buf, y_dev, 0, C, T, default_edges(15), expect=_lib.TISE_ERR_INVALID_ARG) is None
    ev = device.CalibrationEvaluator(buf, torch.from_numpy(y))
    with pytest.raises(_lib.TiseStatusError):
        ev(1e-310)
    assert np.isfinite(ev(float(np.nextafter(2.0 ** -1024, 1.0)))["nll_sum"])     # the smallest T with a finite 1 / T


# ---- 8. a row offset past 2^31 elements ------------------------------------------------------------------------------------------
def test_row_offset_past_2_to_the_31_elements(dev):
    """5 rows of 50 classes with ld = 2^29 + 3: row 4 starts 2^31 + 12 floats into an allocation of 10.7 GB that is never
    filled -- only the rows' own columns and their NaN neighbours are written."""
    free, _ = torch.cuda.mem_get_info(dev)
    if free < 16 * 2 ** 30:
        pytest.skip(f"needs a 10.7 GB allocation; the device reports {free / 2 ** 30:.1f} GB free (< 16 GB)")
    ld, C, T = 2 ** 29 + 3, 50, 0.598
    z, y = R.make_logits(5, C, T, seed=41, ties=False)
    flat = torch.empty(5 * ld, dtype=torch.float32, device=dev)
    try:
        m = flat.view(5, ld)
        assert m[4].data_ptr() - m.data_ptr() == 4 * (2 ** 31 + 12)
        m[:, 0] = NAN
        m[:, 1:1 + C] = torch.from_numpy(z).to(dev)
        m[:, 1 + C] = NAN
        raw = device.CalibrationEvaluator(m, torch.from_numpy(y), c0=1, num_classes=C).raw(T)
        check_raw(raw, z, y, T, default_edges(15), ("ld = 2^29 + 3",))
    finally:
        del flat, m
        torch.cuda.empty_cache()


# ---- 9. labels -------------------------------------------------------------------------------------------------------------------
def test_labels_are_validated_before_the_int32_conversion(dev):
    C = 50
    z, y = R.make_logits(20, C, 1.0, seed=43, ties=False)
    buf, _ = R.embed(z, 0, 0, dev)
    for v in (2 ** 32 + 3, -2 ** 32 + 1, 2 ** 31, -2 ** 31 - 1):
        bad = y.copy()
        bad[7] = v
        with pytest.raises(ValueError, match=f"label {v} "):
            device.CalibrationEvaluator(buf, torch.from_numpy(bad))
        with pytest.raises(ValueError, match=f"label {v} "):
            device.CalibrationEvaluator(buf, torch.from_numpy(bad).to(dev))
    for t in (torch.from_numpy(y.astype(np.float32)), torch.from_numpy(y.astype(np.float64) + 0.7), torch.from_numpy(y % 2 == 0),
              torch.from_numpy(y.astype(np.float16))):
        with pytest.raises(ValueError, match="label"):
            device.CalibrationEvaluator(buf, t)
    # inside int32 but outside [0, C): still the device's count, as before
    edge = y.copy()
    edge[[2, 9, 11, 15]] = [2 ** 31 - 1, -2 ** 31, C, -1]
    ev = device.CalibrationEvaluator(buf, torch.from_numpy(edge))
    raw = ev.raw(1.0)
    assert raw[2] == 0 and raw[3] == 4 and raw[4:19].sum() == 16
    with pytest.raises(ValueError, match="4 row.s. with a label outside"):
        ev(1.0)
    for dt in (np.int8, np.int16, np.int32, np.uint8):                  # every integer dtype keeps working
        r = device.CalibrationEvaluator(buf, torch.from_numpy(y.astype(dt)))(1.0)
        assert r["count"].sum() == 20
