"""The batched CLIP.forward oracle (oracle/rp_oracle.clip_forward_probs_batched) against the per-item one, its guard
bands, and the conditions the kernel's cases (tests/_retrieval_cases.py) must meet before they go to a device."""
import numpy as np
import pytest

from oracle import rp_oracle
from tests import _retrieval_cases as rc


@pytest.fixture(scope="module")
def oracle_runs():
    out = []
    for pos, case in enumerate(rc.CASES):
        img, cand = rc.make_data(case, pos)
        out.append((case, img, cand) + rp_oracle.clip_forward_probs_batched(img, cand, rc.SCALE, case.normalize, case.dtype, detail=True))
    return out


def _bits(x):
    return x.view(np.uint16 if x.dtype == np.float16 else np.uint32)


def test_cases_cover_what_they_must():
    for d in rc.D_VALUES:
        assert {(c.dtype, c.normalize) for c in rc.CASES if c.d == d} == {(t, z) for t in ("float16", "float32") for z in (True, False)}
    for c in rc.C_VALUES:
        assert {k.indexed for k in rc.CASES if k.c == c} == {True, False}
    for kmax in (8, 16):
        assert {k.n for k in rc.CASES if rc.instance(k.d) == kmax} >= set(rc.N_VALUES)
    assert max(k.n for k in rc.CASES) <= 260
    assert len({rc.case_id(k) + str(i) for i, k in enumerate(rc.CASES)}) == len(rc.CASES)


def test_batched_equals_per_item_bit_for_bit(oracle_runs):
    for case, img, cand, probs, _, _ in oracle_runs:
        for i in range(case.n):
            one = rp_oracle.clip_forward_probs(img[i], cand[i], rc.SCALE, case.normalize, np.dtype(case.dtype).type)
            assert np.array_equal(_bits(one), _bits(probs[i])), (rc.case_id(case), i)


def test_unsettled_items_stay_under_the_caps(oracle_runs):
    """Conditions on the DATA, counted by the oracle alone: no unsettled item in an fp16 case; at most 10 % of an fp32
    case and 2 % of all fp32 items; and no unsettled norm or dot product anywhere, because that moves the result by
    more than the one unit in the last place an unsettled item is allowed.  A seed that breaks one is replaced."""
    n32 = u32 = 0
    for case, _, _, probs, settled, flags in oracle_runs:
        assert not (flags["norm"] | flags["dot"]).any(), rc.case_id(case)
        if case.dtype == "float16":
            assert settled.all(), rc.case_id(case)
        else:
            assert (~settled).sum() <= 0.10 * case.n, rc.case_id(case)
            n32 += case.n
            u32 += int((~settled).sum())
        if case.c > 1 and case.n >= 8 and case.d >= 63:             # about half the items retrieve candidate 0 (d <= 2: no room)
            assert 0.2 <= float((np.argmax(probs, 1) == 0).mean()) <= 0.8, rc.case_id(case)
    assert u32 <= 0.02 * n32, (u32, n32)


def test_near_tie_items_are_decided_by_the_rounding(oracle_runs):
    """The built near-ties do both things somewhere: vanish in the dtype (exact tie, candidate 0 wins) and survive it."""
    tied = apart = 0
    for case, _, cand, probs, _, _ in oracle_runs:
        for i in range(0, case.n, 4):
            if case.c > 1:
                j = 1 + (i // 4) % (case.c - 1)
                same = _bits(probs[i, j]) == _bits(probs[i, 0])
                tied += int(same)
                apart += int(not same)
    assert tied >= 20 and apart >= 20, (tied, apart)


def test_guard_band_sees_midpoints():
    f = rp_oracle._unsettled
    mid32 = 1.0 + 2.0 ** -24                                             # half way between 1 and the next fp32 number
    assert f(np.array([mid32]), np.array([2.0 ** -50]), np.float32)[0]
    assert f(np.array([mid32 + 2.0 ** -45]), np.array([2.0 ** -44]), np.float32)[0]
    assert not f(np.array([mid32 + 2.0 ** -45]), np.array([2.0 ** -46]), np.float32)[0]
    assert not f(np.array([mid32]), np.array([0.0]), np.float32)[0]     # band 0: an exact tie is decided by the standard
    mid16 = 1.0 + 2.0 ** -11
    assert f(np.array([mid16 * (1 + 2.0 ** -40)]), np.array([2.0 ** -39]), np.float16)[0]
    assert not f(np.array([mid16 * (1 + 2.0 ** -30)]), np.array([2.0 ** -39]), np.float16)[0]
    # double rounding: just above an fp32 midpoint whose lower neighbour is an fp16 tie
    v = mid16 + 2.0 ** -24
    assert f(np.array([v + 2.0 ** -50]), np.array([2.0 ** -49]), np.float16)[0]
    assert not f(np.array([1.25 + 2.0 ** -24 + 2.0 ** -50]), np.array([2.0 ** -49]), np.float16)[0]
    # subnormals: the fp32 spacing stops at 2^-149, the fp16 one at 2^-24
    assert f(np.array([1.5 * 2.0 ** -149]), np.array([2.0 ** -200]), np.float32)[0]
    assert f(np.array([2.5 * 2.0 ** -24 + 2.0 ** -70]), np.array([2.0 ** -69]), np.float16)[0]
    # an exactly representable sum has no band: fp16 operands, every partial sum a multiple of 2^-48 below 2^5
    a = np.array([[1.0, 2.0 ** -12]], np.float16)
    t = np.array([[[1.0 + 2.0 ** -10, 2.0 ** -2]]], np.float16)           # dot = 1 + 2^-10 + 2^-14: an fp32 number
    _, settled = rp_oracle.clip_forward_probs_batched(a, t, 1.0, False, np.float16)
    assert settled.all()


def test_ulp_distance():
    one = np.float16(1.0)
    up = np.nextafter(one, np.float16(2))
    assert rp_oracle.ulp_distance(np.array([one, -one, np.float16(0.0), np.float16("nan")]),
                                  np.array([up, -up, np.float16(-0.0), np.float16("nan")])).tolist() == [1, 1, 0, 0]
    assert rp_oracle.ulp_distance(np.array([np.float32("nan")]), np.array([np.float32(1)]))[0] > 2 ** 32
    tiny = np.float32(2.0 ** -149)
    assert rp_oracle.ulp_distance(np.array([tiny]), np.array([-tiny]))[0] == 2


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_non_finite_items_are_all_nan_and_argmax_zero(dtype):
    rng = np.random.default_rng(5)
    img = rng.standard_normal((3, 64)).astype(dtype)
    cand = rng.standard_normal((3, 8, 64)).astype(dtype)
    img[0, 7] = np.nan
    cand[1, 5, 3] = np.nan
    img[2, :2] = 60000 if dtype == np.float16 else 3e38                 # the logit overflows: inf - inf
    cand[2, 4, :2] = 60000 if dtype == np.float16 else 3e38
    for normalize in (False, True):
        probs, _ = rp_oracle.clip_forward_probs_batched(img, cand, rc.SCALE, normalize, dtype)
        bad = (0, 1) if normalize else (0, 1, 2)
        for i in bad:
            assert np.isnan(probs[i]).all() and int(np.argmax(probs[i])) == 0
            one = rp_oracle.clip_forward_probs(img[i], cand[i], rc.SCALE, normalize, dtype)
            assert np.isnan(one).all()


def test_judge_is_as_strict_as_the_rule():
    probs = np.array([[0.25, 0.5, 0.25], [0.5, 0.25, 0.25]], np.float16)
    settled = np.array([True, False])
    ok_top, ok_p = np.array([1, 0], np.int32), np.array([0.25, 0.5], np.float32)
    assert rc.judge(ok_top, ok_p, probs, settled, np.float16) == []
    up = np.float32(np.nextafter(np.float16(0.25), np.float16(1)))
    assert rc.judge(ok_top, np.array([up, 0.5], np.float32), probs, settled, np.float16)          # settled: no ulp to give
    up = np.float32(np.nextafter(np.float16(0.5), np.float16(1)))
    assert rc.judge(ok_top, np.array([0.25, up], np.float32), probs, settled, np.float16) == []   # unsettled: one ulp
    up2 = np.float32(np.nextafter(np.nextafter(np.float16(0.5), np.float16(1)), np.float16(1)))
    assert rc.judge(ok_top, np.array([0.25, up2], np.float32), probs, settled, np.float16)
    assert rc.judge(np.array([0, 0], np.int32), ok_p, probs, settled, np.float16)                 # wrong top1, settled
    assert rc.judge(np.array([1, 1], np.int32), ok_p, probs, settled, np.float16)                 # unsettled, but far apart
    assert rc.judge(np.array([1, 3], np.int32), ok_p, probs, settled, np.float16)                 # outside [0, c)
    assert rc.judge(np.array([1, 0x7fffffff], np.int32), ok_p, probs, settled, np.float16)
    assert rc.judge(ok_top, np.array([0.25, 0.5 + 2.0 ** -20], np.float32), probs, settled, np.float16)   # not an fp16 number
    nanp = np.full((1, 3), np.nan, np.float16)
    assert rc.judge(np.array([0], np.int32), np.array([np.nan], np.float32), nanp, np.array([True]), np.float16) == []
    assert rc.judge(np.array([0], np.int32), np.array([0.5], np.float32), nanp, np.array([True]), np.float16)
