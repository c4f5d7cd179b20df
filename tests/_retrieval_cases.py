"""Cases of the retrieval kernel's pin (tests/test_gpu_retrieval_kernel.py) and of the batched oracle's own test
(tests/test_rp_oracle_batched.py): the shapes, the seeded data and the verdict on a kernel's output.  numpy only."""
import collections

import numpy as np

from oracle import rp_oracle

D_VALUES = (1, 2, 63, 64, 65, 100, 511, 512, 513, 768, 1023, 1024)      # one lane stride; the KMAX 8 / 16 switch; the limit
C_VALUES = (1, 2, 63, 64, 65, 100, 128, 1023, 1024)                      # one lane stride of the softmax pass; RT_MAXC
N_VALUES = (1, 2, 3, 4, 5, 7, 8, 9, 257)                                 # partly filled last workgroup
SCALE = 100.0

Case = collections.namedtuple("Case", "d c n dtype normalize indexed seed")


def instance(d):
    return 8 if d <= 512 else 16                                          # KMAX of cosine_top1_kernel


# c per d for (fp16 normalize / indexed, fp16 raw / contiguous, fp32 normalize / indexed, fp32 raw / contiguous): every c
# in both forms.  The large c sit at the large d in fp16, whose dot products are exact in fp64 (rp_oracle), and at
# d <= 2 in fp32, where an fp32 dot product over a thousand terms would too often be unsettled.
C_OF_D = {1: (1024, 1024, 1023, 1023), 2: (1023, 1023, 1024, 1024), 63: (1, 1, 2, 2), 64: (63, 63, 64, 64),
          65: (65, 65, 100, 100), 100: (128, 128, 1, 1), 511: (2, 2, 63, 63), 512: (64, 64, 65, 65),
          513: (100, 100, 128, 128), 768: (1023, 1024, 2, 2), 1023: (63, 63, 1, 1), 1024: (1024, 1023, 64, 64)}


def _cases():
    out = []
    small_n = [x for x in N_VALUES if x < 257]
    for d in D_VALUES:
        for k, (dtype, normalize) in enumerate([("float16", True), ("float16", False), ("float32", True), ("float32", False)]):
            out.append(Case(d, C_OF_D[d][k], small_n[(3 * len(out)) % len(small_n)], dtype, normalize, normalize, 0))
    # every n once per kernel instance
    for d in (100, 768):
        for i, n in enumerate(N_VALUES):
            out.append(Case(d, (2, 65)[i % 2], n, ("float16", "float32")[(i // 2) % 2], bool(i % 3), bool((i + 1) % 2), 0))
    return out


# Seeds: data seed = 1000 * position + Case.seed.  A seed is replaced (never the cap) when the oracle finds an fp16 item,
# an unsettled norm or dot product, or too many unsettled fp32 probabilities in the data it generates; the counts are
# asserted on the CPU by tests/test_rp_oracle_batched.py before any case reaches a device.
RESEED = {26: 1, 34: 1, 35: 1, 46: 1, 47: 2, 64: 1}
CASES = [c._replace(seed=RESEED.get(i, 0)) for i, c in enumerate(_cases())]


def case_id(case):
    return (f"d{case.d}-c{case.c}-n{case.n}-{case.dtype}-{'norm' if case.normalize else 'raw'}-"
            f"{'indexed' if case.indexed else 'contiguous'}")


def make_data(case, position):
    """-> img (n, d), cand (n, c, d) in the case's dtype.  Even items retrieve candidate 0 (true caption = image + noise);
    of those, every other one has a distractor that is the true caption's row plus 2^-8 ... 2^-20 in one element, so the
    roundings of the dtype decide (or erase) the difference."""
    rng = np.random.default_rng(1000 * position + case.seed)
    n, c, d = case.n, case.c, case.d
    img = rng.standard_normal((n, d))
    cand = rng.standard_normal((n, c, d))
    for i in range(0, n, 2):
        cand[i, 0] = img[i] + 0.7 * rng.standard_normal(d)
        if c > 1 and i % 4 == 0:
            j = 1 + (i // 4) % (c - 1)
            cand[i, j] = cand[i, 0]
            cand[i, j, (i // 4) % d] += 2.0 ** -(8 + (i // 4) % 13)
    if not case.normalize:                                               # the CLIs hand the kernel unit vectors
        img /= np.linalg.norm(img, axis=1, keepdims=True)
        cand /= np.linalg.norm(cand, axis=2, keepdims=True)
    return img.astype(case.dtype), cand.astype(case.dtype)


def judge(top1, p0, probs, settled, dtype, flipped=None, eps=None):
    """The acceptance rule.  Settled item: top1 == argmax of the oracle's probabilities and p0 == probs[0], bit for bit.
    Unsettled item: p0 within one unit in the last place; another top1 only between candidates whose oracle
    probabilities are within one such unit.  Returns a list of complaints (empty: accepted).

    `flipped` (fp32 runs too large to be seeded free of them) marks items with an unsettled DOT PRODUCT: a logit may
    then sit one fp32 spacing `eps` away, which no bound of one unit in the last place of p0 survives.  With every
    logit within eps, p_j = exp(l_j) / sum exp(l_k) stays within the factors exp(+-2 eps); those items get that
    interval, widened by the one unit, and nothing else does."""
    top1, p0 = np.asarray(top1), np.asarray(p0)
    n, c = probs.shape
    bad = []
    if not np.all((top1 >= 0) & (top1 < c)):
        return [f"top1 outside [0, {c}): {top1[(top1 < 0) | (top1 >= c)][:4].tolist()}"]
    with np.errstate(all="ignore"):
        pd = p0.astype(dtype)
    same = (pd.astype(np.float32).view(np.int32) == p0.view(np.int32)) | np.isnan(p0)
    if not same.all():
        bad.append(f"p0 is not a {np.dtype(dtype).name} number at items {np.flatnonzero(~same)[:4].tolist()}")
    want = np.argmax(probs, axis=1)
    dp = rp_oracle.ulp_distance(pd, probs[:, 0])
    rows = np.arange(n)
    dt = rp_oracle.ulp_distance(probs[rows, top1], probs[rows, want])
    allow = np.where(settled, 0, 1)
    if flipped is not None and flipped.any():
        p64 = probs.astype(np.float64)
        width = np.expm1(2 * eps) * p64.max(1) + 2 * np.spacing(probs.max(1)).astype(np.float64)
        close0 = np.abs(pd.astype(np.float64) - p64[:, 0]) <= np.expm1(2 * eps) * p64[:, 0] + np.spacing(probs[:, 0]).astype(np.float64)
        closet = np.abs(p64[rows, top1] - p64[rows, want]) <= width
        dp = np.where(flipped & close0, 0, dp)
        dt = np.where(flipped & closet, 0, dt)
        settled = settled & ~flipped
    for i in np.flatnonzero(dp > allow)[:4]:
        bad.append(f"item {i} ({'settled' if settled[i] else 'unsettled'}): p0 {p0[i]!r} vs {float(probs[i, 0])!r}, {int(dp[i])} ulp")
    wrong = (top1 != want) & (settled | (dt > 1))
    for i in np.flatnonzero(wrong)[:4]:
        bad.append(f"item {i} ({'settled' if settled[i] else 'unsettled'}): top1 {int(top1[i])} vs {int(want[i])}, "
                   f"probabilities {int(dt[i])} ulp apart")
    return bad
