"""csrc/retrieval.hip (cosine_top1_kernel<T, KMAX>) against CLIP.forward's rounding, bit for bit.

The reference is oracle/rp_oracle.clip_forward_probs_batched, which also says where its own fp64 arithmetic could
have decided a rounding (`settled`; guard bands derived in its docstring).  At a settled item the kernel has no
freedom: top1 == np.argmax(probs) and p0 == probs[0] in every bit.  At an unsettled one p0 may be one unit in the last
place away, and top1 may differ only between candidates whose probabilities are that close.  How many items may be
unsettled is a condition on the data, asserted on the CPU (tests/test_rp_oracle_batched.py) and again here before a
case is launched.  The shapes sit around one lane stride (64), the KMAX 8 / 16 switch (d = 512 / 513), the limits
(d = 1024, c = RT_MAXC = 1024) and a partly filled last workgroup (4 items, one per wave).

Every input lives inside a NaN-filled allocation and every output is a view into a sentinel-filled one: a read or a
write past an edge shows.  Every launch is a legal input; what must be refused is refused before anything is enqueued."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import rp_oracle
from tests import _retrieval_cases as rc

pytestmark = pytest.mark.gpu

SENT_I, SENT_P, PAD = -77, 1234.5, 5
TORCH = {"float16": torch.float16, "float32": torch.float32}


def _embed(rows, dev):
    """rows (r, d) -> a contiguous view with a NaN row before and after it."""
    buf = torch.full((rows.shape[0] + 2, rows.shape[1]), float("nan"), dtype=TORCH[rows.dtype.name], device=dev)
    buf[1:-1] = torch.from_numpy(rows).to(dev)
    return buf[1:-1]


def _table(cand, indexed, seed):
    """(n, c, d) candidates -> (table rows, index or None).  Indexed: the rows are scattered over a larger table whose
    other rows, which no index names, are NaN."""
    n, c, d = cand.shape
    if not indexed:
        return cand.reshape(n * c, d), None
    rows = n * c + n + 3
    where = np.random.default_rng(seed).permutation(rows)[:n * c]
    table = np.full((rows, d), np.nan, cand.dtype)
    table[where] = cand.reshape(n * c, d)
    return table, where.reshape(n, c).astype(np.int32)


def _raw(dev, img, txt, index, n, c, d, dtype_code, normalize, scale=rc.SCALE, want_p0=True, expect=0):
    """tise_cosine_top1 through the C ABI into sentinel-framed outputs; asserts the status and the frames."""
    from tise_toolbox_amd import _lib
    lib = _lib.load()
    top = torch.full((max(n, 0) + 2 * PAD,), SENT_I, dtype=torch.int32, device=dev)
    p0 = torch.full((max(n, 0) + 2 * PAD,), SENT_P, dtype=torch.float32, device=dev)
    ptr = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off) if t is not None else None
    status = lib.tise_cosine_top1(ptr(img), ptr(txt), ptr(index), ctypes.c_int64(n), c, d, dtype_code, int(normalize),
                                  ctypes.c_float(scale), ptr(top, 4 * PAD), ptr(p0, 4 * PAD) if want_p0 else None,
                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert status == expect, status
    top, p0 = top.cpu().numpy(), p0.cpu().numpy()
    m = max(n, 0) if expect == 0 else 0
    assert (top[:PAD] == SENT_I).all() and (top[PAD + m:] == SENT_I).all(), "top1 written outside its n entries"
    assert (p0[:PAD] == SENT_P).all() and (p0[PAD + (m if want_p0 else 0):] == SENT_P).all(), "p0 written outside its n entries"
    return top[PAD:PAD + m], p0[PAD:PAD + m]


def _run_all_ways(dev, img, cand, indexed, normalize, seed=0, scale=rc.SCALE):
    """The raw entry (with and without p0) and device.cosine_top1 on the same framed inputs: all must agree in every bit."""
    from tise_toolbox_amd import device
    n, c, d = cand.shape
    table, index = _table(cand, indexed, seed)
    ti, tt = _embed(img, dev), _embed(table, dev)
    tidx = torch.from_numpy(index).to(dev) if index is not None else None
    code = 0 if img.dtype == np.float32 else 1
    top, p0 = _raw(dev, ti, tt, tidx, n, c, d, code, normalize, scale)
    top_b, _ = _raw(dev, ti, tt, tidx, n, c, d, code, normalize, scale, want_p0=False)
    assert np.array_equal(top, top_b), "top1 depends on whether p0 is asked for"
    t2, p2 = device.cosine_top1(ti, tt, tidx, normalize=normalize, logit_scale=scale)
    assert np.array_equal(t2.cpu().numpy(), top) and np.array_equal(p2.cpu().numpy().view(np.int32), p0.view(np.int32))
    t3, none = device.cosine_top1(ti, tt, tidx, normalize=normalize, logit_scale=scale, want_p0=False)
    assert none is None and np.array_equal(t3.cpu().numpy(), top)
    return top, p0


@pytest.mark.parametrize("position", range(len(rc.CASES)), ids=[rc.case_id(c) for c in rc.CASES])
def test_kernel_matches_clip_forward_rounding(cuda_device, position):
    case = rc.CASES[position]
    img, cand = rc.make_data(case, position)
    probs, settled, flags = rp_oracle.clip_forward_probs_batched(img, cand, rc.SCALE, case.normalize, case.dtype, detail=True)
    assert not (flags["norm"] | flags["dot"]).any()                      # the caps, before anything goes to the device
    assert settled.all() if case.dtype == "float16" else (~settled).sum() <= 0.10 * case.n
    top, p0 = _run_all_ways(cuda_device, img, cand, case.indexed, case.normalize, seed=position)
    print(f"{rc.case_id(case)}: unsettled {int((~settled).sum())} of {case.n}; top1 == 0 at {int((top == 0).sum())}")
    assert rc.judge(top, p0, probs, settled, np.dtype(case.dtype)) == []


@pytest.mark.parametrize("dtype", ["float16", "float32"])
@pytest.mark.parametrize("d", [64, 768])
def test_result_does_not_depend_on_the_wave(cuda_device, dtype, d):
    """The same 9 items behind 0, 1, 2 and 3 other items: each sits in every wave of a workgroup once."""
    case = rc.Case(d, 65, 12, dtype, True, False, 0)
    img, cand = rc.make_data(case, 902 + d)                               # a seed whose 9 items are all settled
    probs, settled = rp_oracle.clip_forward_probs_batched(img[3:], cand[3:], rc.SCALE, True, dtype)
    want = None
    for lead in (0, 1, 2, 3):
        for indexed in (False, True):
            top, p0 = _run_all_ways(cuda_device, img[3 - lead:], cand[3 - lead:], indexed, True, seed=lead)
            got = (top[lead:].tolist(), p0[lead:].view(np.int32).tolist())
            want = want or got
            assert got == want, lead
    assert settled.all() and rc.judge(np.array(want[0], np.int32), np.array(want[1], np.int32).view(np.float32), probs, settled,
                                      np.dtype(dtype)) == []


@pytest.mark.parametrize("dtype", ["float16", "float32"])
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("d", [64, 768])
def test_duplicate_rows_first_maximum_wins(cuda_device, dtype, normalize, d):
    """Candidates that name the same table row have bit-identical logits, whatever the rounding: the first one must win,
    across lanes (j mod 64) and across strides (j div 64) of the softmax pass."""
    from tise_toolbox_amd import device
    rng = np.random.default_rng(d)
    for c, sets in ((131, [((3, 67, 130), 3), ((67, 130), 67), ((64, 1), 1)]), (1024, [((0, 1023), 0)])):
        n = len(sets)
        img = rng.standard_normal((n, d))
        table = rng.standard_normal((n + 40, d))
        table[:n] = img                                                    # row i: the image itself, cosine 1
        if not normalize:
            img /= np.linalg.norm(img, axis=1, keepdims=True)
            table /= np.linalg.norm(table, axis=1, keepdims=True)
        index = rng.integers(n, n + 40, size=(n, c)).astype(np.int32)
        for i, (js, _) in enumerate(sets):
            index[i, list(js)] = i
        img, table = img.astype(dtype), table.astype(dtype)
        probs, settled = rp_oracle.clip_forward_probs_batched(img, table[index], rc.SCALE, normalize, dtype)
        assert np.argmax(probs, 1).tolist() == [w for _, w in sets]
        ti, tt, tidx = _embed(img, cuda_device), _embed(table, cuda_device), torch.from_numpy(index).to(cuda_device)
        top, p0 = _raw(cuda_device, ti, tt, tidx, n, c, d, 0 if dtype == "float32" else 1, normalize)
        assert top.tolist() == [w for _, w in sets]
        t2, _ = device.cosine_top1(ti, tt, tidx, normalize=normalize)
        assert t2.cpu().tolist() == top.tolist()
        assert (rp_oracle.ulp_distance(p0.astype(dtype), probs[:, 0])[settled] == 0).all()   # top1 above needs no rounding argument


@pytest.mark.parametrize("dtype", ["float16", "float32"])
@pytest.mark.parametrize("normalize", [True, False])
def test_non_finite_items_follow_the_reference(cuda_device, dtype, normalize):
    """A NaN in the image row, a NaN in candidate 5, and (fp16, raw) a logit that overflows: np.argmax of the reference's
    all-NaN probabilities is 0 and p0 is NaN.  The items around them, in the same workgroup, keep their bits."""
    case = rc.Case(64, 8, 11, dtype, normalize, False, 0)
    img, cand = rc.make_data(case, 700)
    clean_top, clean_p0 = _run_all_ways(cuda_device, img, cand, False, normalize)
    img, cand = img.copy(), cand.copy()
    img[1, 7] = np.nan
    cand[6, 5, 3] = np.nan
    bad = [1, 6]
    if dtype == "float16" and not normalize:
        img[9, :2] = 60000
        cand[9, 2, :2] = 60000
        bad.append(9)
    probs, _ = rp_oracle.clip_forward_probs_batched(img, cand, rc.SCALE, normalize, dtype)
    for indexed in (False, True):
        top, p0 = _run_all_ways(cuda_device, img, cand, indexed, normalize)
        print(f"{dtype} normalize={normalize} indexed={indexed}: top1 {top[bad].tolist()} p0 {p0[bad].tolist()}")
        assert ((top >= 0) & (top < case.c)).all(), top.tolist()
        assert np.isnan(probs[bad]).all() and top[bad].tolist() == np.argmax(probs[bad], 1).tolist() == [0] * len(bad)
        assert np.isnan(p0[bad]).all()
        good = np.setdiff1d(np.arange(case.n), bad)
        assert np.array_equal(top[good], clean_top[good]) and np.array_equal(p0[good].view(np.int32), clean_p0[good].view(np.int32))


def test_nan_item_is_a_success_for_rp_and_a_failure_for_pa(cuda_device):
    """RP_coco.py:78 counts np.argmax(probs) == 0, which an all-NaN item satisfies; PA.py:41 asks probs[0] > 0.6, which NaN
    does not."""
    from tise_toolbox_amd import PA, RP_coco
    n, c, d = 20, 4, 64
    img = torch.zeros((n, d), device=cuda_device)
    img[:, 0] = 1.0
    txt = torch.zeros((n * c, d), device=cuda_device)
    txt[:, 0] = -torch.arange(n * c, device=cuda_device).remainder(c).float()          # candidate 0 wins everywhere
    txt[3 * c, 0] = -5.0                                                                # ... but not at item 3
    index = torch.arange(n * c, dtype=torch.int32, device=cuda_device).view(n, c)
    perm = RP_coco.shuffled_ids(n, 2)
    base = RP_coco.r_precision(img, txt, index, perm, normalize=False, logit_scale=1.0)
    assert base[0] == pytest.approx((n - 1) / n)
    txt[3 * c + 2, 5] = float("nan")
    with_nan = RP_coco.r_precision(img, txt, index, perm, normalize=False, logit_scale=1.0)
    assert with_nan[0] == pytest.approx(1.0) and sorted(with_nan[2]) == [1.0] * 10
    pair = torch.arange(2 * n, dtype=torch.int32, device=cuda_device).view(n, 2)
    ptxt = torch.zeros((2 * n, d), device=cuda_device)
    ptxt[0::2, 0] = 3.0                                                                 # softmax([3, 0])[0] = 0.95
    assert PA.pa_successes(img, ptxt, pair, 1.0).cpu().tolist() == [1.0] * n
    ptxt[2 * 7, 9] = float("nan")
    assert PA.pa_successes(img, ptxt, pair, 1.0).cpu().tolist() == [1.0] * 7 + [0.0] + [1.0] * (n - 8)


def test_c_abi_refuses_before_anything_is_enqueued(cuda_device):
    from tise_toolbox_amd import _lib
    n, d = 6, 64
    img = torch.ones((n, d), device=cuda_device)
    txt = torch.ones((n * 1025, d), device=cuda_device)
    big = torch.ones((n, 1025), device=cuda_device)
    bigt = torch.ones((n, 1025), device=cuda_device)
    inv, uns = _lib.TISE_ERR_INVALID_ARG, _lib.TISE_ERR_UNSUPPORTED
    _raw(cuda_device, img, txt, None, n, 1025, d, 0, True, expect=uns)
    _raw(cuda_device, big, bigt, None, n, 1, 1025, 0, True, expect=inv)
    _raw(cuda_device, img, txt, None, n, 2, 0, 0, True, expect=inv)
    _raw(cuda_device, img, txt, None, n, 0, d, 0, True, expect=inv)
    _raw(cuda_device, img, txt, None, n, 2, d, 2, True, expect=inv)
    _raw(cuda_device, img, txt, None, n, 2, d, -1, True, expect=inv)
    _raw(cuda_device, None, txt, None, n, 2, d, 0, True, expect=inv)
    _raw(cuda_device, img, None, None, n, 2, d, 0, True, expect=inv)
    _raw(cuda_device, img, txt, None, -1, 2, d, 0, True, expect=inv)
    lib = _lib.load()
    p0 = torch.full((n,), SENT_P, device=cuda_device)
    st = lib.tise_cosine_top1(ctypes.c_void_p(img.data_ptr()), ctypes.c_void_p(txt.data_ptr()), None, ctypes.c_int64(n), 2, d, 0, 1,
                              ctypes.c_float(1.0), None, ctypes.c_void_p(p0.data_ptr()), None)
    torch.cuda.synchronize()
    assert st == inv and (p0 == SENT_P).all()
    _raw(cuda_device, img, txt, None, 0, 2, d, 0, True, expect=_lib.TISE_OK)           # n = 0: nothing to do, nothing written
    top, _ = _raw(cuda_device, img, txt, None, n, 1024, d, 0, True)                    # one inside the limit runs
    assert top.tolist() == [0] * n


def test_device_wrapper_refuses_bad_indices_and_ragged_tables(cuda_device, monkeypatch):
    """A bad index would be an out-of-bounds read: it must never reach the kernel."""
    from tise_toolbox_amd import _lib, device
    called = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: called.append(name) or real(name, *a))
    n, c, d, rows = 5, 3, 64, 11
    img = torch.ones((n, d), device=cuda_device)
    txt = torch.ones((rows, d), device=cuda_device)
    for where, value in (((0, 0), rows), ((4, 2), rows + 1000), ((2, 1), -1), ((3, 0), -2 ** 31)):
        index = torch.zeros((n, c), dtype=torch.int32, device=cuda_device)
        index[where] = value
        with pytest.raises(ValueError, match="txt_index"):
            device.cosine_top1(img, txt, index)
    for bad_rows in (n * c + 1, n * c - 1, n - 1):
        with pytest.raises(ValueError, match="n \\* c"):
            device.cosine_top1(img, torch.ones((bad_rows, d), device=cuda_device), None)
    assert called == []
    index = torch.full((n, c), rows - 1, dtype=torch.int32, device=cuda_device)          # the last row is a row
    index[:, 0] = 0
    top1, _ = device.cosine_top1(img, txt, index)
    assert called == ["tise_cosine_top1"] and top1.cpu().tolist() == [0] * n
