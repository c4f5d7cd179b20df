"""GPU: tise_attention_long_f16 at head width 80 (open_clip ViT-H/14: width 1280 over 16 heads), pinned per element to fp64
softmax(Q K^T / sqrt(80)) V of the same fp16 inputs.  The cases, the constructions that steer the running maximum and the two
checks are those of tests/test_gpu_attention_long.py, at width 80 and on smaller shapes.

THE BOUND is that file's (its docstring derives every term), restated for what width 80 changes:

  * 80 products per score instead of 64: the fp32 sum of the matrix cores errs by C_ACC * 81 * 2^-24 * sum_d |q_d k_d| (was 65);
  * two further relative 2^-24 on every score: the fp32 constant nearest 1 / sqrt(80) (1/8 was exact) and the multiply by it
    (by 1/8 it was exact), so  err_s = (C_ACC * 81 + 2) 2^-24 sum_d |q_d k_d| / sqrt(80);
  * KT = clip_hip.ATTN_LONG_KEY_TILE as the library reports it, T = ceil(seq / KT); every other term unchanged.  The padding
    rows 80 .. 95 of V^T are zeros: they add nothing to any sum.

CHECK 2 is the flat |got - ref| <= 3e-3 max(1, max|ref|).

A store beyond column 79 of a head (the third 32-row output tile is 16 rows wider than the head) would land in the first 16
columns of the next head or, with one head, of the next row: every real element is inside the bound, and a canary row behind
the last output row stays bit-identical.

Measured on an MI355X over the 48 cases: worst error / bound 0.489 (peaked, seq 64, 3 heads), worst flat figure 4.3e-4 (peaked,
seq 129, 16 heads); census 33 943 rises above 1.0 and 24 031 falls below -20."""
import math

import pytest
import torch

from tests.test_gpu_attention_long import attention_long_ref as attention_long_ref64, make_qkv as make_qkv64
from tests.test_gpu_clip_kernels import C_ACC, ETA16, U16, _attention_ref

pytestmark = pytest.mark.gpu

D = 80
SEQS = (1, 63, 64, 65, 127, 128, 129, 257)
HEADS = (1, 3, 16)
BATCHES = (1, 2, 3)
KINDS = ("randn", "peaked", "ascending", "descending", "spike-last", "spike-first")
SLOPE = 0.05           # score per key of the ramps: 3.2 per tile of 64 keys
SPIKE = 30.0           # the lead of the spike key
FLAT_TOL = 3e-3


def _case_shape(kind, seq):
    i = KINDS.index(kind) * len(SEQS) + SEQS.index(seq)
    return HEADS[i % 3], BATCHES[(i // 3) % 3]


def make_qkv(batch, seq, heads, kind, g, dev):
    """tests/test_gpu_attention_long.py::make_qkv at width 80: randn, peaked (q and k times 3.6), and the four kinds that steer
    the running maximum -- with a unit direction u per (sequence, head), q_i = (4 sqrt(80) / 8) u + 0.05 noise and
    k_j = 2 profile_j u + 0.05 noise, so that score(i, j) = profile_j + small, as there."""
    x = torch.randn((batch, seq, 3, heads, D), generator=g, device=dev)
    if kind == "peaked":
        x[:, :, :2] *= 3.6
    elif kind != "randn":
        j = torch.arange(seq, device=dev, dtype=torch.float32)
        if kind == "ascending":
            prof = SLOPE * j
        elif kind == "descending":
            prof = SLOPE * (seq - 1 - j)
        else:
            prof = torch.zeros(seq, device=dev)
            prof[seq - 1 if kind == "spike-last" else 0] = SPIKE
        u = torch.randn((batch, 1, heads, D), generator=g, device=dev)
        u = u / u.norm(dim=-1, keepdim=True)
        x[:, :, 0] = (4.0 * math.sqrt(D) / 8.0) * u + 0.05 * x[:, :, 0]
        x[:, :, 1] = (2.0 * prof).view(1, seq, 1, 1) * u + 0.05 * x[:, :, 1]
    return x.reshape(batch * seq, 3 * heads * D).half()


def attention_d80_ref(qkv, batch, seq, heads, kt):
    """-> (fp64 output, per-element bound (module docstring), census) in the kernel's [batch*seq][heads*80] layout."""
    T = (seq + kt - 1) // kt
    q, k, v = qkv.double().view(batch, seq, 3, heads, D).permute(2, 0, 3, 1, 4).reshape(3, batch * heads, seq, D)
    outs, bounds = [], []
    rises = falls = 0
    chunk = max(1, (1 << 26) // (seq * seq * D))
    for c0 in range(0, batch * heads, chunk):
        qc, kc, vc = q[c0:c0 + chunk], k[c0:c0 + chunk], v[c0:c0 + chunk]
        s = qc @ kc.transpose(-1, -2) / math.sqrt(D)
        sabs = qc.abs() @ kc.abs().transpose(-1, -2) / math.sqrt(D)
        p = torch.softmax(s, -1)
        o = p @ vc
        err_s = ((C_ACC * (D + 1) + 2) * 2.0 ** -24 * sabs).amax(-1, keepdim=True)
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
        pad = T * kt - seq
        tmax = torch.nn.functional.pad(s, (0, pad), value=-math.inf).view(s.shape[0], seq, T, kt).amax(-1)
        run = torch.cummax(tmax, -1).values
        if T > 1:
            d = tmax[..., 1:] - run[..., :-1]
            rises += int((d > 1.0).sum().item())
            falls += int((d < -20.0).sum().item())
    o, bound = torch.cat(outs), torch.cat(bounds)
    lay = lambda t: t.view(batch, heads, seq, D).transpose(1, 2).reshape(batch * seq, heads * D)
    return lay(o), lay(bound), {"rises": rises, "falls": falls}


_CASES = {}            # (kind, seq) -> (qkv, fp64 reference, bound, census): computed once, shared, never written to


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    """The shared cases live on the device for this module only: the files after it find the allocator as they would without it."""
    yield
    _CASES.clear()
    torch.cuda.empty_cache()


def _case(kind, seq, dev):
    from tise_toolbox_amd import clip_hip
    if (kind, seq) not in _CASES:
        heads, batch = _case_shape(kind, seq)
        g = torch.Generator(device=dev).manual_seed(1000 * KINDS.index(kind) + seq)
        qkv = make_qkv(batch, seq, heads, kind, g, dev)
        _CASES[(kind, seq)] = (qkv,) + attention_d80_ref(qkv, batch, seq, heads, clip_hip.ATTN_LONG_KEY_TILE)
    return _CASES[(kind, seq)]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("kind", KINDS)
def test_attention_d80_matches_fp64_per_element(cuda_device, kind):
    """Every seq of SEQS (each edge of the 64-key tile and of the 128-query block; 129: a last block with one live query and three
    idle waves; 257: ViT-H/14's own length), heads 1 / 3 / 16 and batch 1 / 2 / 3 rotated: check 1 (max |got - ref| / bound <= 1),
    check 2 (the flat 3e-3); seq = 1 is the V row bit for bit."""
    from tise_toolbox_amd import clip_hip
    for seq in SEQS:
        heads, batch = _case_shape(kind, seq)
        qkv, ref, bound, census = _case(kind, seq, cuda_device)
        got = clip_hip.attention_long(qkv, batch, seq, heads, D)
        err = (got.double() - ref).abs()
        ratio = (err / bound).max().item()
        flat = (err.max() / max(1.0, ref.abs().max().item())).item()
        rec = {"kind": kind, "seq": seq, "heads": heads, "batch": batch, "ratio": ratio, "flat": flat}
        print(f"{kind} seq {seq} heads {heads} batch {batch}: ratio {ratio:.3f} flat {flat:.2e} census {census}")
        assert got.shape == (batch * seq, heads * D) and torch.isfinite(got).all(), rec
        assert ratio <= 1.0, rec
        assert flat <= FLAT_TOL, rec
        if seq == 1:
            assert torch.equal(got, qkv[:, 2 * heads * D:]), rec
        if seq > clip_hip.ATTN_SHORT_MAX_SEQ:                              # the dispatcher takes the same road
            assert torch.equal(got, clip_hip.attention(qkv, batch, seq, heads, False, D)), rec


@pytest.mark.timeout(300)
def test_constructions_move_the_running_maximum(cuda_device):
    """Census over the fp64 scores with the kernel's own tile size: over `ascending` and `spike-last` at least 1 000 (query,
    tile >= 1) pairs whose tile maximum lies more than 1.0 ABOVE the running maximum of the tiles before, over `spike-first` at
    least 1 000 more than 20 BELOW it (257 keys are too few for `descending` to fall that far: it is there for the small steps)."""
    rises = sum(_case(k, s, cuda_device)[3]["rises"] for k in ("ascending", "spike-last") for s in SEQS)
    falls = sum(_case(k, s, cuda_device)[3]["falls"] for k in ("spike-first", "descending") for s in SEQS)
    print(f"census: {rises} rises > 1.0, {falls} falls > 20")
    assert rises >= 1000 and falls >= 1000, (rises, falls)


def test_nothing_is_stored_beyond_column_79(cuda_device):
    """One head, so that the columns 80 .. 95 of the padded third output tile would be the first 16 columns of the NEXT ROW: a
    canary row behind the last output row stays bit-identical (seq 1, 65, 129, 257: the last row is in wave 0 of the last block),
    and the rows themselves are inside the bound (a row's first columns overwritten by its predecessor's padding would not be)."""
    from tise_toolbox_amd import _lib, clip_hip
    lib = _lib.load()
    g = torch.Generator(device=cuda_device).manual_seed(80)
    for seq in (1, 65, 129, 257):
        for batch in (1, 2):
            qkv = make_qkv(batch, seq, 1, "randn", g, cuda_device)
            buf = torch.empty((batch * seq + 1, D), dtype=torch.float16, device=cuda_device)
            canary = torch.randn(D, generator=g, device=cuda_device).half()
            buf[-1] = canary
            assert lib.tise_attention_long_f16(qkv.data_ptr(), batch, seq, 1, D, buf.data_ptr(), clip_hip._stream()) == _lib.TISE_OK
            torch.cuda.synchronize()
            assert torch.equal(buf[-1], canary), (seq, batch)
            ref, bound, _ = attention_d80_ref(qkv, batch, seq, 1, clip_hip.ATTN_LONG_KEY_TILE)
            assert ((buf[:-1].double() - ref).abs() <= bound).all(), (seq, batch)


def test_d80_is_repeatable_and_batch_invariant(cuda_device):
    """Two launches give the same bits; rows [seq : 2 seq] of a batch-3 launch equal the batch-1 launch on that sequence alone."""
    from tise_toolbox_amd import clip_hip
    g = torch.Generator(device=cuda_device).manual_seed(77)
    for seq, heads in ((129, 3), (257, 16)):
        qkv = make_qkv(3, seq, heads, "ascending", g, cuda_device)
        a = clip_hip.attention_long(qkv, 3, seq, heads, D)
        b = clip_hip.attention_long(qkv, 3, seq, heads, D)
        assert torch.equal(a, b), seq
        one = clip_hip.attention_long(qkv[seq:2 * seq].contiguous(), 1, seq, heads, D)
        assert torch.equal(a[seq:2 * seq], one), seq


def test_other_head_widths_are_refused(cuda_device):
    """head_dim 72 and 96 (multiples of 8 on either side of 80): TISE_ERR_INVALID_ARG, nothing launched; so is a misaligned qkv at
    80.  The dispatcher refuses them as ValueError, and head width 80 on the short / causal road."""
    from tise_toolbox_amd import _lib, clip_hip
    lib = _lib.load()
    bad = _lib.TISE_ERR_INVALID_ARG
    qkv = torch.zeros((2 * 97 + 1, 3 * 2 * 96), dtype=torch.float16, device=cuda_device)
    out = torch.full((2 * 97, 2 * 96), 7.0, dtype=torch.float16, device=cuda_device)
    st = clip_hip._stream()
    assert lib.tise_attention_long_f16(qkv.data_ptr(), 2, 97, 2, 72, out.data_ptr(), st) == bad
    assert lib.tise_attention_long_f16(qkv.data_ptr(), 2, 97, 2, 96, out.data_ptr(), st) == bad
    assert lib.tise_attention_long_f16(qkv.data_ptr() + 8, 2, 97, 2, 80, out.data_ptr(), st) == bad
    assert lib.tise_attention_f16(qkv.data_ptr(), 2, 96, 2, 80, 0, out.data_ptr(), st) == bad
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    q80 = torch.zeros((2 * 50, 3 * 2 * 80), dtype=torch.float16, device=cuda_device)
    with pytest.raises(ValueError):
        clip_hip.attention_long(q80, 2, 50, 2, 72)
    with pytest.raises(ValueError):
        clip_hip.attention(q80, 2, 50, 2, False, 80)                        # 50 tokens: the short kernel, width 64 only
    with pytest.raises(ValueError):
        clip_hip.attention(q80, 2, 50, 2, True, 80)


def test_d64_instance_still_agrees_with_the_short_kernel(cuda_device):
    """The D = 64 instance of the template on tests/test_gpu_attention_long.py's inputs: inside that file's bound, and within the
    sum of the two bounds of tise_attention_f16 (seq <= 96)."""
    from tise_toolbox_amd import clip_hip
    g = torch.Generator(device=cuda_device).manual_seed(64)
    for seq, heads, batch, kind in ((1, 1, 2, "randn"), (63, 3, 1, "peaked"), (64, 16, 2, "ascending"), (65, 3, 3, "spike-last"),
                                    (96, 1, 2, "descending")):
        qkv = make_qkv64(batch, seq, heads, kind, g, cuda_device)
        got = clip_hip.attention_long(qkv, batch, seq, heads)
        ref, bound, _ = attention_long_ref64(qkv, batch, seq, heads, clip_hip.ATTN_LONG_KEY_TILE)
        assert ((got.double() - ref).abs() <= bound).all(), (seq, kind)
        old = clip_hip.attention(qkv, batch, seq, heads, False)
        _, bound_old, _ = _attention_ref(qkv, batch, seq, heads, False)
        assert ((got.double() - old.double()).abs() <= bound + bound_old).all(), (seq, kind)
