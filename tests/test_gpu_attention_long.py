"""GPU: tise_attention_long_f16 (csrc/clip_ops.hip: streamed key tiles, online softmax with the exact running maximum) pinned
per element to fp64 softmax(Q K^T / 8) V of the same fp16 inputs, at every edge of its key tile and of its 128-query block,
on inputs BUILT so that the online branch does something: scores that rise at every tile, fall at every tile, a last key and a
first key that beat all others by about 30.  A census over the fp64 scores asserts that the constructions did what they are
for (conditions, not measurements).  The reference is PyTorch in float64, computed once per case and shared by every check.

THE BOUND starts from tests/test_gpu_clip_kernels.py::_attention_ref's expression and changes what the new arithmetic changes
(KT = clip_hip.ATTN_LONG_KEY_TILE, T = ceil(seq / KT) tiles; u = 2^-11, eta = 2^-25; every constant is a line of the kernel):

    |o^ - o| <= (1 + 2^-8)[u|o| + eta + (1 + u)(u S_p + eta sum_j|v_j| + (2 KT T + T) 2^-24 S_p + theta |o|
                                                  + (exp(2 D) - 1) sum_j p_j |v_j - o|)]

  * S_p = sum_j p_j |v_j|.  u S_p: p^ = exp(s^_j - m_t) <= 1 is rounded to fp16 as it is (the old kernel rounds p / l), one
    relative u per key; eta sum_j |v_j|: a p^ below the fp16 normal range errs by at most eta, and the final division by
    l >= 1 (the key of the maximum contributes exp(0) = 1 exactly, later alphas are exp(0) = 1) only shrinks it.
  * 2 KT T 2^-24 S_p: the fp32 accumulation of V^T P^T in the matrix cores over the KT T padded keys (c = 2 per add, as there).
  * + T 2^-24 S_p: `oc *= alpha`, one fp32 multiply of the partial sum (at most S_p in magnitude) per tile.
  * theta = (seq + 2 T + 3) 2^-24, common to the row: at most seq inexact fp32 adds on the way of any p into l (adding the 0
    of a padded key is exact), per tile `l * alpha` and `+ psum` (2 T), the add of the two lane halves, the reciprocal and
    the product `oc * inv` (3).  The old kernel has seq + 4 here.
  * D = 2 max_j |s^_j - s_j| + T 2^-20 + 2^-21 (spread + 2 max_j |s^_j - s_j|), spread = max - min score.  A key's weight is
    p^_j prod_{t' > t(j)} alpha_t' = exp(s^_j - m_t) prod exp(m_{t'-1} - m_t'): in exact arithmetic exp(s^_j - M) with M the
    maximum of the COMPUTED scores (the running maximum is exact: fmaxf does not round), so the argument carries the error of
    s^_j and of M (64 exact products summed in fp32, c = 2, as there) and at most T calls of __expf (one for p, one per later
    rescale), each within 2^-20 + 2^-21 |x| of exp(x) as there; their arguments have one sign and sum to M - s^_j <= spread +
    2 max|s^ - s|.  The factor 2 of exp(2 D): a perturbation moves p_j and the normalisation.

CHECK 2 is the project's flat tolerance (tests/test_gpu_clip.py::test_attention_f16): |got - ref| <= 3e-3 max(1, max|ref|); it
guards against a bound that was derived loose.  For seq <= 96 the old kernel must agree within the sum of the two bounds."""
import math

import pytest
import torch

from tests.test_gpu_clip_kernels import C_ACC, ETA16, U16, _attention_ref, _qkv

pytestmark = pytest.mark.gpu

SEQS = (1, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128, 129, 191, 193, 257, 577)
HEADS = (1, 3, 16)
BATCHES = (1, 2, 3)
KINDS = ("randn", "peaked", "uniform", "offset", "ascending", "descending", "spike-last", "spike-first")
SLOPE = 0.05           # score per key of the ramps: 3.2 per tile of 64 keys (1.6 per tile of 32), 29 over 577 keys
SPIKE = 30.0           # the lead of the spike key
FLAT_TOL = 3e-3


def _case_shape(kind, seq):
    i = KINDS.index(kind) * len(SEQS) + SEQS.index(seq)
    return HEADS[i % 3], BATCHES[(i // 3) % 3]


def make_qkv(batch, seq, heads, kind, g, dev):
    """_qkv's four kinds, and four that steer the running maximum: with a unit direction u per (sequence, head),
    q_i = 4 u + 0.05 noise and k_j = b_j u + 0.05 noise, so that score(i, j) = 4 b_j / 8 + small: b_j = 2 * profile_j."""
    if kind in ("randn", "peaked", "uniform", "offset"):
        return _qkv(batch, seq, heads, kind, g, dev)
    j = torch.arange(seq, device=dev, dtype=torch.float32)
    if kind == "ascending":
        prof = SLOPE * j
    elif kind == "descending":
        prof = SLOPE * (seq - 1 - j)
    else:
        prof = torch.zeros(seq, device=dev)
        prof[seq - 1 if kind == "spike-last" else 0] = SPIKE
    u = torch.randn((batch, 1, heads, 64), generator=g, device=dev)
    u = u / u.norm(dim=-1, keepdim=True)
    x = torch.randn((batch, seq, 3, heads, 64), generator=g, device=dev)
    x[:, :, 0] = 4.0 * u + 0.05 * x[:, :, 0]
    x[:, :, 1] = (2.0 * prof).view(1, seq, 1, 1) * u + 0.05 * x[:, :, 1]
    return x.reshape(batch * seq, 3 * heads * 64).half()


def attention_long_ref(qkv, batch, seq, heads, kt):
    """-> (fp64 output, per-element bound (module docstring), census) in the kernel's [batch*seq][heads*64] layout.  Worked
    through in chunks of (sequence, head) pairs: the sum_j p_j |v_j - o| term is S x S x 64 doubles per pair."""
    T = (seq + kt - 1) // kt
    q, k, v = qkv.double().view(batch, seq, 3, heads, 64).permute(2, 0, 3, 1, 4).reshape(3, batch * heads, seq, 64)
    outs, bounds = [], []
    rises = falls = 0
    chunk = max(1, (1 << 26) // (seq * seq * 64))
    for c0 in range(0, batch * heads, chunk):
        qc, kc, vc = q[c0:c0 + chunk], k[c0:c0 + chunk], v[c0:c0 + chunk]
        s = qc @ kc.transpose(-1, -2) / 8
        sabs = qc.abs() @ kc.abs().transpose(-1, -2) / 8
        p = torch.softmax(s, -1)
        o = p @ vc
        err_s = (C_ACC * 65 * 2.0 ** -24 * sabs).amax(-1, keepdim=True)
        spread = s.amax(-1, keepdim=True) - s.amin(-1, keepdim=True)
        delta = 2 * err_s + T * 2.0 ** -20 + 2.0 ** -21 * (spread + 2 * err_s)
        pv_abs = p @ vc.abs()
        pv_dev = (p.unsqueeze(-1) * (vc.unsqueeze(-3) - o.unsqueeze(-2)).abs()).sum(-2)
        vsum = vc.abs().sum(-2, keepdim=True).expand_as(o)
        theta = (seq + 2 * T + 3) * 2.0 ** -24
        inner = (U16 * pv_abs + ETA16 * vsum + (C_ACC * kt * T + T) * 2.0 ** -24 * pv_abs + theta * o.abs()
                 + torch.expm1(2 * delta) * pv_dev)
        outs.append(o)
        bounds.append((1 + 2.0 ** -8) * (U16 * o.abs() + ETA16 + (1 + U16) * inner))
        # census: per (query, tile >= 1), the tile's maximum against the running maximum of the tiles before it
        pad = T * kt - seq
        tmax = torch.nn.functional.pad(s, (0, pad), value=-math.inf).view(s.shape[0], seq, T, kt).amax(-1)
        run = torch.cummax(tmax, -1).values
        if T > 1:
            d = tmax[..., 1:] - run[..., :-1]
            rises += int((d > 1.0).sum().item())
            falls += int((d < -20.0).sum().item())
    o, bound = torch.cat(outs), torch.cat(bounds)
    lay = lambda t: t.view(batch, heads, seq, 64).transpose(1, 2).reshape(batch * seq, heads * 64)
    return lay(o), lay(bound), {"rises": rises, "falls": falls}


_CENSUS = {}           # (kind, seq) -> census of the case, filled by whoever computes the case first


def _run_case(kind, seq, dev):
    """One case: inputs, the fp64 reference (once), every check that shares it.  Returns the printed record."""
    from tise_toolbox_amd import clip_hip
    kt = clip_hip.ATTN_LONG_KEY_TILE
    heads, batch = _case_shape(kind, seq)
    g = torch.Generator(device=dev).manual_seed(1000 * KINDS.index(kind) + seq)
    qkv = make_qkv(batch, seq, heads, kind, g, dev)
    got = clip_hip.attention_long(qkv, batch, seq, heads)
    ref, bound, census = attention_long_ref(qkv, batch, seq, heads, kt)
    _CENSUS[(kind, seq)] = census
    err = (got.double() - ref).abs()
    ratio = (err / bound).max().item()
    flat = (err.max() / max(1.0, ref.abs().max().item())).item()
    rec = {"kind": kind, "seq": seq, "heads": heads, "batch": batch, "ratio": ratio, "flat": flat}
    print(f"{kind} seq {seq} heads {heads} batch {batch}: ratio {ratio:.3f} flat {flat:.2e} census {census}")
    assert torch.isfinite(got).all(), rec
    assert ratio <= 1.0, rec                                             # check 1: the derived bound
    assert flat <= FLAT_TOL, rec                                         # check 2: the project's flat tolerance
    e = heads * 64
    if seq <= 96:                                                        # the old kernel on the same input
        old = clip_hip.attention(qkv, batch, seq, heads, False)
        _, bound_old, _ = _attention_ref(qkv, batch, seq, heads, False)
        cross = ((got.double() - old.double()).abs() / (bound + bound_old)).max().item()
        assert cross <= 1.0, (rec, cross)
    if seq == 1:                                                         # one key: the V row, bit for bit
        assert torch.equal(got, qkv[:, 2 * e:]), rec
    if kind == "uniform":                                                # identical keys: every query gets the same row
        rows = got.view(batch, seq, e)
        assert torch.equal(rows, rows[:, :1].expand_as(rows)), rec
    return rec


@pytest.mark.timeout(300)
@pytest.mark.parametrize("kind", KINDS)
def test_attention_long_matches_fp64_per_element(cuda_device, kind):
    """Every seq of SEQS (each edge of a 32- or 64-key tile and of the 128-query block; 97, the first length the old kernel
    refuses; 129 and 193, a last block with one live query and three idle waves; 257; the real 577), heads 1 / 3 / 16 and
    batch 1 / 2 / 3 rotated: check 1 (ratio = max |got - ref| / bound <= 1, the module docstring's bound), check 2 (the flat
    3e-3), the old kernel within bound_long + bound_old for seq <= 96, seq = 1 exact, `uniform` rows identical."""
    for seq in SEQS:
        _run_case(kind, seq, cuda_device)


@pytest.mark.timeout(300)
def test_constructions_move_the_running_maximum(cuda_device):
    """Census over the fp64 scores, with the kernel's own tile size: over `ascending` and `spike-last` at least 1 000
    (query, tile >= 1) pairs whose tile maximum lies more than 1.0 ABOVE the running maximum of the tiles before (a rescale
    that changes O and l), over `spike-first` and `descending` at least 1 000 whose tile maximum lies more than 20 BELOW it
    (the tile's p underflow against it and alpha = 1)."""
    from tise_toolbox_amd import clip_hip
    for kind in ("ascending", "spike-last", "spike-first", "descending"):
        for seq in SEQS:
            if (kind, seq) not in _CENSUS:
                heads, batch = _case_shape(kind, seq)
                g = torch.Generator(device=cuda_device).manual_seed(1000 * KINDS.index(kind) + seq)
                qkv = make_qkv(batch, seq, heads, kind, g, cuda_device)
                _CENSUS[(kind, seq)] = attention_long_ref(qkv, batch, seq, heads, clip_hip.ATTN_LONG_KEY_TILE)[2]
    rises = sum(_CENSUS[(k, s)]["rises"] for k in ("ascending", "spike-last") for s in SEQS)
    falls = sum(_CENSUS[(k, s)]["falls"] for k in ("spike-first", "descending") for s in SEQS)
    print(f"census: {rises} rises > 1.0, {falls} falls > 20")
    assert rises >= 1000 and falls >= 1000, (rises, falls)


def test_key_tile_constant_is_the_library_s(cuda_device):
    from tise_toolbox_amd import _lib, clip_hip
    assert clip_hip.ATTN_LONG_KEY_TILE == _lib.load().tise_attention_long_key_tile() and clip_hip.ATTN_LONG_KEY_TILE in (32, 64)


def test_attention_long_is_repeatable_and_batch_invariant(cuda_device):
    """Two launches give the same bits; rows [seq : 2 seq] of a batch-3 launch equal, bit for bit, the batch-1 launch on that
    sequence alone (seq 193: two blocks, the second with one live wave; seq 577)."""
    from tise_toolbox_amd import clip_hip
    g = torch.Generator(device=cuda_device).manual_seed(77)
    for seq, heads in ((193, 3), (577, 16)):
        qkv = make_qkv(3, seq, heads, "ascending", g, cuda_device)
        a = clip_hip.attention_long(qkv, 3, seq, heads)
        b = clip_hip.attention_long(qkv, 3, seq, heads)
        assert torch.equal(a, b), seq
        one = clip_hip.attention_long(qkv[seq:2 * seq].contiguous(), 1, seq, heads)
        assert torch.equal(a[seq:2 * seq], one), seq


def test_attention_long_refusals_on_the_device(cuda_device):
    """seq = 0, head_dim 32 and 128, qkv 8 bytes off a 16-byte boundary: TISE_ERR_INVALID_ARG, nothing launched; a causal
    request beyond the old kernel's 96 tokens is a ValueError of the dispatcher."""
    from tise_toolbox_amd import _lib, clip_hip
    lib = _lib.load()
    bad = _lib.TISE_ERR_INVALID_ARG
    qkv = torch.zeros((2 * 97 + 1, 3 * 128), dtype=torch.float16, device=cuda_device)
    out = torch.full((2 * 97, 128), 7.0, dtype=torch.float16, device=cuda_device)
    st = clip_hip._stream()
    assert lib.tise_attention_long_f16(qkv.data_ptr(), 2, 0, 2, 64, out.data_ptr(), st) == bad
    assert lib.tise_attention_long_f16(qkv.data_ptr(), 2, 97, 4, 32, out.data_ptr(), st) == bad
    assert lib.tise_attention_long_f16(qkv.data_ptr(), 2, 97, 1, 128, out.data_ptr(), st) == bad
    assert lib.tise_attention_long_f16(qkv.data_ptr() + 8, 2, 97, 2, 64, out.data_ptr(), st) == bad
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    with pytest.raises(ValueError):
        clip_hip.attention(qkv[:2 * 97], 2, 97, 2, True)
    assert lib.tise_attention_long_f16(qkv.data_ptr(), 2, 97, 2, 64, out.data_ptr(), st) == _lib.TISE_OK   # and the good call runs
    torch.cuda.synchronize()
    assert (out == 0.0).all()                                               # V = 0
