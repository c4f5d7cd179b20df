"""Plain numpy fp32 emulations of the pool / bias / stem kernels of csrc/trunk_ops.hip, one per kernel, each in the
kernel's documented operation order, and the split-tensor layout of csrc/common.h in numpy.  No torch, no GPU: the
emulations are checked against torch's fp64 ops in tests/test_pool_ref_host.py, so no expected value of
tests/test_gpu_pool_kernels.py comes from the kernels themselves.

Every array op below is on float32 arrays, so numpy rounds each add / divide once to fp32 (IEEE, round to nearest
even) -- what the device does: the library is built with ``-O3`` and nothing that relaxes fp32 arithmetic
(tise_toolbox_amd/build.py: no -ffast-math, no -fno-hip-fp32-correctly-rounded-divide-sqrt, denormals kept), and
the kernels' divisions compile to the v_div_scale / v_div_fmas / v_div_fixup sequence, i.e. correctly rounded.  The
only fused operations are the explicit fmaf chains of the stem kernels, emulated in float64 (the product of two fp32
values is exact there) with one rounding to fp32 per step.

Layouts: fp32 tensors are NHWC; a split tensor of C channels is (..., 2C) fp16 -- per 32-channel block
[hi x32 | lo x32], then [hi x16 | lo x16] when C % 32 == 16.
"""
import numpy as np

F32 = np.float32
LO_SCALE = F32(2048.0)
INV_LO = F32(1.0 / 2048.0)


# ------------------------------------------------------------------------------------------------- split layout
def ilv_index(C):
    """(hi_idx, lo_idx): position of channel c's hi / lo half inside a pixel of 2C fp16 (tise_ilv_off / tise_ilv_second)."""
    assert C % 16 == 0
    c = np.arange(C)
    full = C & ~31
    hi = np.where(c < full, (c >> 5) * 64 + (c & 31), 2 * full + (c - full))
    lo = hi + np.where(c < full, 32, 16)
    return hi, lo


def split_value(v):
    """fp32 -> (hi, lo) fp16: hi = fp16(v), lo = fp16((v - hi) * 2048)."""
    v = np.asarray(v, dtype=F32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = v.astype(np.float16)
        lo = ((v - hi.astype(F32)) * LO_SCALE).astype(np.float16)
    return hi, lo


def merge_value(hi, lo):
    """(hi, lo) fp16 -> the fp32 value hi + lo / 2048 (exact: two 11-bit significands)."""
    with np.errstate(invalid="ignore"):
        return hi.astype(F32) + lo.astype(F32) * INV_LO


def pack_split(dst, v, off):
    """Write split(v) (..., C) into channels [off, off + C) of the split tensor ``dst`` (..., 2 * C_total), in place."""
    hi_idx, lo_idx = ilv_index(dst.shape[-1] // 2)
    hi, lo = split_value(v)
    C = v.shape[-1]
    dst[..., hi_idx[off:off + C]] = hi
    dst[..., lo_idx[off:off + C]] = lo
    return dst


def unpack_split(t, off=0, C=None):
    """(hi, lo) fp16 (..., C) of channels [off, off + C) of the split tensor ``t``."""
    hi_idx, lo_idx = ilv_index(t.shape[-1] // 2)
    C = t.shape[-1] // 2 - off if C is None else C
    return t[..., hi_idx[off:off + C]], t[..., lo_idx[off:off + C]]


def slice_mask(C_total, off, C):
    """Boolean mask over the 2 * C_total fp16 positions of a pixel: True where channels [off, off + C) live."""
    hi_idx, lo_idx = ilv_index(C_total)
    m = np.zeros(2 * C_total, dtype=bool)
    m[hi_idx[off:off + C]] = True
    m[lo_idx[off:off + C]] = True
    return m


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def ulp_distance(a, b):
    """Distance in fp32 units in the last place between same-sign finite fp32 arrays."""
    return np.abs(bits(np.asarray(a, F32)).astype(np.int64) - bits(np.asarray(b, F32)).astype(np.int64))


# ------------------------------------------------------------------------------------------------- emulations
def relu(v):
    """max(v, 0) as v_max_f32 gives it for finite v: +0 for every v <= 0."""
    return np.where(v > 0, v, F32(0.0)).astype(F32)


def bias_relu(x, bias):
    """bias_relu_nhwc: max(x + b, 0); one fp32 add."""
    return relu(np.asarray(x, F32) + np.asarray(bias, F32))


def _divisor(h, w, excl):
    if not excl:
        return np.full((h, w), 9.0, dtype=F32)
    rows = 1 + (np.arange(h) > 0) + (np.arange(h) + 1 < h)
    cols = 1 + (np.arange(w) > 0) + (np.arange(w) + 1 < w)
    return (rows[:, None] * cols[None, :]).astype(F32)


def _zero_padded(x):
    n, h, w, c = x.shape
    p = np.zeros((n, h + 2, w + 2, c), dtype=F32)
    p[:, 1:h + 1, 1:w + 1] = x
    return p


def avgpool_per_output(x, bias, excl=False):
    """avgpool3_bias_relu_nhwc_kernel / avgpool3_bias_relu_split_kernel (pre-split): sequential fp32 sum from 0 over the
    taps inside the map in (dh, dw) row-major order (a tap outside the map adds +0, which changes no bit), / 9 or / the
    count of taps inside the map, + bias, max(., 0)."""
    x = np.asarray(x, F32)
    n, h, w, c = x.shape
    p = _zero_padded(x)
    s = np.zeros_like(x)
    for dh in range(3):
        for dw in range(3):
            s = s + p[:, dh:dh + h, dw:dw + w]
    s = s / _divisor(h, w, excl)[None, :, :, None]
    return relu(s + np.asarray(bias, F32))


def avgpool_colwalk(x, bias, excl=False):
    """avgpool3_bias_relu_split_colwalk_kernel (pre-split): per row (left + centre) + right with zeros outside the map,
    then (above + this) + below with zero rows outside, / 9 or / the count of taps inside the map, + bias, max(., 0)."""
    x = np.asarray(x, F32)
    n, h, w, c = x.shape
    p = _zero_padded(x)
    hs = (p[:, :, 0:w] + p[:, :, 1:w + 1]) + p[:, :, 2:w + 2]            # (n, h + 2, w, c); rows 0 and h + 1 are zero
    s = (hs[:, 0:h] + hs[:, 1:h + 1]) + hs[:, 2:h + 2]
    s = s / _divisor(h, w, excl)[None, :, :, None]
    return relu(s + np.asarray(bias, F32))


def maxpool3s2(x, bias=None):
    """maxpool3s2_nhwc_kernel: exact maximum of the 3 x 3 / stride 2 window, then (with a bias) max(m + b, 0)."""
    x = np.asarray(x, F32)
    n, h, w, c = x.shape
    oh, ow = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    m = np.full((n, oh, ow, c), -np.inf, dtype=F32)
    for dh in range(3):
        for dw in range(3):
            m = np.maximum(m, x[:, dh:dh + 2 * oh - 1:2, dw:dw + 2 * ow - 1:2])
    return m if bias is None else bias_relu(m, bias)


def maxpool3s1p1(x):
    """maxpool3s1p1_nhwc_kernel: exact maximum of the taps inside the map (padding acts as -inf)."""
    x = np.asarray(x, F32)
    n, h, w, c = x.shape
    p = np.full((n, h + 2, w + 2, c), -np.inf, dtype=F32)
    p[:, 1:h + 1, 1:w + 1] = x
    m = np.full_like(x, -np.inf)
    for dh in range(3):
        for dw in range(3):
            m = np.maximum(m, p[:, dh:dh + h, dw:dw + w])
    return m


def maxpool_split(hi, lo, pool):
    """The split max-pools: ``pool`` of the merged values hi + lo / 2048, split again -> (hi, lo)."""
    return split_value(pool(merge_value(hi, lo)))


def stem_fma(x, wt, bias):
    """stem_conv3x3s2_split[_u8]_kernel (pre-split): x (n, h, w, 3) fp32 network input, wt (3, 3, 3, 32) [kh][kw][cin][cout],
    bias (32,).  acc = fma(x, w, acc) from 0 in (kh, kw, cin) order -- in float64, where x * w is exact, rounded once per step
    to fp32 -- then max(acc + bias, 0)."""
    x = np.asarray(x, F32)
    wt = np.asarray(wt, F32)
    n, h, w, _ = x.shape
    oh, ow = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    acc = np.zeros((n, oh, ow, 32), dtype=F32)
    for kh in range(3):
        for kw in range(3):
            for ci in range(3):
                v = x[:, kh:kh + 2 * oh - 1:2, kw:kw + 2 * ow - 1:2, ci].astype(np.float64)[..., None]
                acc = (v * wt[kh, kw, ci].astype(np.float64) + acc.astype(np.float64)).astype(F32)
    return relu(acc + np.asarray(bias, F32))


# ------------------------------------------------------------------------------------------------- cases
MAPS_S1 = [(1, 1), (1, 6), (7, 1), (2, 2), (3, 3), (8, 8), (9, 11)]          # stride-1 pools, bias_relu
MAPS_S2 = [(3, 3), (4, 4), (5, 7), (13, 9)]          # stride-2 pools, stems: (4, 4), (13, 9) and the 7 of (5, 7) leave a row / column uncovered
BATCHES = [1, 3]
# fp32 forms: (C, x_ld, x_off, out_ld, out_off); offsets non-zero and no multiples of 16, and the trunk's Mixed_5b pool slice
SLICES_F32 = [(4, 20, 12, 24, 4), (8, 36, 20, 12, 4), (32, 208, 176, 256, 224)]
# split forms: tensors of 80 (input) and 112 (output) channels -- both C % 32 == 16, so both end in a 16-channel tail block
# (input: blocks [0, 32) [32, 64), tail [64, 80); output: three blocks, tail [96, 112)) -- as (x_off, C, out_off):
SPLIT_X_C, SPLIT_OUT_C = 80, 112
SLICES_SPLIT = [(8, 48, 16),         # wholly in full blocks (crossing a block boundary on both sides)
                (64, 16, 96),        # the whole tail block -> the whole tail block
                (72, 8, 104),        # the second half of the tail block
                (32, 32, 64),        # ends exactly at the tail boundary on both sides
                (24, 8, 56),         # 8 channels at the second half of a 32-block (off % 32 == 24)
                (40, 40, 72),        # from a full block into the tail, to the end of the tensor
                (0, 16, 80)]         # output slice straddling nothing: last half of a full block
# split average pools (fp32 input slice -> split output slice): (C, x_ld, x_off, out_off) into a 112-channel output
SLICES_AVG_SPLIT = [(48, 60, 12, 16), (16, 16, 0, 96), (8, 24, 4, 104), (32, 40, 8, 64), (8, 8, 0, 56), (40, 44, 4, 72)]


def avg_split_cases():
    """The cases of the two split average-pool kernels, identical for the in-process (column-walking) run and the child
    process (per-output): list of dicts with the poisoned fp32 input, bias and geometry."""
    cases = []
    i = 0
    for (h, w) in MAPS_S1:
        for n in BATCHES:
            for (C, x_ld, x_off, out_off) in SLICES_AVG_SPLIT:
                for excl in (False, True):
                    g = np.random.default_rng(1000 + i)
                    i += 1
                    x = np.full((n, h, w, x_ld), np.nan, dtype=F32)
                    x[..., x_off:x_off + C] = g.standard_normal((n, h, w, C)).astype(F32)
                    bias = g.standard_normal(C).astype(F32)
                    cases.append(dict(x=x, bias=bias, n=n, h=h, w=w, C=C, x_ld=x_ld, x_off=x_off, out_C=SPLIT_OUT_C, out_off=out_off,
                                      excl=excl))
    return cases


def avg_split_cross_cases():
    """Cases on which the two summation orders may be compared with each other: non-negative inputs in [0, 1) and a bias in
    [8, 15), so v = avg + bias lies in the binade [8, 16).  With u = 2^-24: the sequential order makes 8 roundings of at most
    u S each (S = the tap sum, every partial sum <= S), the column-walking order 2 per row sum (<= u R_i, R_1 + R_2 + R_3 = S)
    and 2 more (<= u S): the sums differ by at most 12 u S, the averages a = S / d <= 1 by at most 12 u a + 2 u a (their own
    roundings), and v by at most 14 u a + 2 (half an ulp of v) < (14 a / v + 1) ulp(v) <= (14 / 9 + 1) ulp(v) since ulp(v) > u v
    and v >= 8 + a: less than 3, so at most 2 whole ulps between two fp32 numbers of one binade."""
    cases = []
    for i, (h, w) in enumerate(MAPS_S1):
        for excl in (False, True):
            g = np.random.default_rng(5000 + 2 * i + excl)
            C, x_ld, x_off, out_off = SLICES_AVG_SPLIT[i % len(SLICES_AVG_SPLIT)]
            x = np.full((3, h, w, x_ld), np.nan, dtype=F32)
            x[..., x_off:x_off + C] = g.random((3, h, w, C)).astype(F32)
            bias = (8.0 + 7.0 * g.random(C)).astype(F32)
            cases.append(dict(x=x, bias=bias, n=3, h=h, w=w, C=C, x_ld=x_ld, x_off=x_off, out_C=SPLIT_OUT_C, out_off=out_off, excl=excl))
    return cases
