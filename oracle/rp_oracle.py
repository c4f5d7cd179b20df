"""CPU restatement of the R-precision (RP-COCO) and positional-alignment (PA) reductions.

TEST INFRASTRUCTURE ONLY: imported by tests/, never by the product path (tise_toolbox_amd/ fails loudly
without the HIP library).

Follows the reference's own code around the CLIP towers:
  text_relevance/RP_coco.py:41-52   ten bins over the shuffled item ids, samples_per_bin = int(N / 10), the last bin
                                    takes the remainder
  text_relevance/RP_coco.py:68-80   candidates = [true caption] + mismatched captions; success iff
                                    np.argmax(softmax(logits_per_image)) == 0 (first maximum wins)
  text_relevance/RP_coco.py:79-88   bin score = successes / len(bin); result = mean and population std of the bins
  positional_alignment/PA.py:33-43  success iff softmax([true, false])[0] > 0.6
  positional_alignment/PA.py:52-67  per-phrase success rate, PA = mean over phrases
CLIP itself (third-party `clip` @ git master, README.md:43; ViT-B/32) is absent from /root/reference and from this
image: for the towers parity is UNPINNED.  The reductions are pinned by tests/golden/rp_stub_*.npz / pa_stub.json:
outputs of the reference scripts themselves, run with a stub `clip` module (tests/golden/make_golden_rp.py).
"""
import numpy as np


def clip_logits(img_emb, txt_emb, logit_scale=100.0, normalize=True):
    """logits_per_image of CLIP for one image against its candidates: scale * cosine (fp64)."""
    a = np.asarray(img_emb, dtype=np.float64)
    t = np.asarray(txt_emb, dtype=np.float64)
    if normalize:
        a = a / np.linalg.norm(a)
        t = t / np.linalg.norm(t, axis=-1, keepdims=True)
    return logit_scale * (t @ a)


def clip_forward_probs(img_emb, txt_emb, logit_scale=100.0, normalize=True, dtype=np.float16):
    """What the reference scripts compare (RP_coco.py:72-78, PA.py:37-42): CLIP.forward's
    `logit_scale * image_features @ text_features.t()` (third-party `clip` @ git master, model.py; Python evaluates it
    as (logit_scale * image_features) @ text_features.t()) followed by `.softmax(dim=-1).cpu().numpy()[0]`, with every
    stored tensor in the model's dtype -- fp16 for the model clip.load serves on a GPU, fp32 on the CPU path -- and
    fp32 arithmetic inside each op (torch's opmath for half tensors; accumulation order of the GEMM unspecified:
    float64 here).  Returns the probabilities as `dtype`: np.argmax of them is the first maximum of ROUNDED values."""
    a = np.asarray(img_emb, dtype=dtype)
    t = np.asarray(txt_emb, dtype=dtype)
    if normalize:                                           # x / x.norm(dim=1, keepdim=True) in the model's dtype
        na = np.sqrt((a.astype(np.float64) ** 2).sum()).astype(np.float32).astype(dtype)             # the norm is a tensor too
        nt = np.sqrt((t.astype(np.float64) ** 2).sum(-1, keepdims=True)).astype(np.float32).astype(dtype)
        a = (a.astype(np.float32) / na.astype(np.float32)).astype(dtype)
        t = (t.astype(np.float32) / nt.astype(np.float32)).astype(dtype)
    a = (np.float32(logit_scale) * a.astype(np.float32)).astype(dtype)
    logits = (t.astype(np.float64) @ a.astype(np.float64)).astype(np.float32).astype(dtype)
    z = logits.astype(np.float64) - float(logits.max())
    e = np.exp(z)
    return (e / e.sum()).astype(np.float32).astype(dtype)


def _gamma(k):
    """Higham's gamma_k = k u / (1 - k u), u = 2^-53: the relative error bound of a k-term fp64 sum of products."""
    return k * 2.0 ** -53 / (1.0 - k * 2.0 ** -53)


_FORMATS = {np.dtype(np.float32): (24, -126), np.dtype(np.float16): (11, -14)}     # significand bits, exponent of the least normal


def _near_midpoint(v, band, dtype):
    """True where the fp64 value v lies within `band` (absolute) of a rounding midpoint (k + 1/2) ulp of `dtype`
    (subnormals included: the spacing stops shrinking at the least normal exponent)."""
    p, emin = _FORMATS[np.dtype(dtype)]
    with np.errstate(all="ignore"):
        av = np.abs(v)
        _, e = np.frexp(av)                                     # av = m 2^e, m in [0.5, 1)
        e = np.where(av > 0, np.maximum(e - 1, emin), emin)
        ulp = np.ldexp(1.0, e - (p - 1))
        q = av / ulp                                            # a power-of-two scaling: exact
        dist = np.abs(q - np.floor(q) - 0.5) * ulp
        return np.isfinite(av) & (dist <= band)


def _quantum(x):
    """min over the last axis of the spacing of x's dtype at each non-zero element: every element is a multiple of it."""
    p, emin = _FORMATS[x.dtype]
    ax = np.abs(x.astype(np.float64))
    _, e = np.frexp(ax)
    q = np.ldexp(1.0, np.maximum(e - 1, emin) - (p - 1))
    return np.where((ax > 0) & np.isfinite(ax), q, np.inf).min(-1)


def _unsettled(v, band, dtype):
    """A step `fp64 value -> fp32 -> dtype`: can another correct evaluation (v moved by at most `band` > 0) round
    otherwise?  For fp32, if the band holds an fp32 midpoint.  For fp16, if it holds an fp16 midpoint, or if it holds an
    fp32 midpoint and one of the two fp32 numbers around v is an exact fp16 tie (the first rounding then decides which
    way the second one goes).  band == 0 marks a value that is known exactly: nothing can move it."""
    band = np.broadcast_to(np.asarray(band, dtype=np.float64), np.shape(v))
    near32 = _near_midpoint(v, band, np.float32) & (band > 0)
    if np.dtype(dtype) == np.float32:
        return near32
    with np.errstate(all="ignore"):
        v32 = np.asarray(v).astype(np.float32)
        other = np.nextafter(v32, np.where(v32 > v, -np.inf, np.inf).astype(np.float32))
    tie = _near_midpoint(v32.astype(np.float64), 0.0, np.float16) | _near_midpoint(other.astype(np.float64), 0.0, np.float16)
    return (_near_midpoint(v, band, np.float16) & (band > 0)) | (near32 & tie)


def clip_forward_probs_batched(img_emb, txt_emb, logit_scale=100.0, normalize=True, dtype=np.float16, detail=False):
    """clip_forward_probs for n items at once: img_emb (n, d), txt_emb (n, c, d) -> (probs (n, c) as `dtype`,
    settled (n,) bool).  The same roundings in the same places; bit-identical to the per-item function.

    `settled[i]` says that the oracle's own fp64 arithmetic cannot have decided a rounding of item i, so that ANY
    correct implementation of the same rounding model returns the same bits.  The model has two kinds of step:

    * elementwise steps (x / norm, logit_scale * x): one IEEE fp32 operation on operands that are known exactly,
      then fp32 -> dtype.  Both are correctly rounded operations with a unique result (ties go to even on every
      conforming machine; an fp32 number that is not an fp16 tie is at least 2^-24 relative away from one), so they
      leave no freedom and cannot unsettle an item.
    * steps whose input is an fp64 quantity that depends on evaluation order or on the libm: the norm
      sqrt(sum x^2), the dot product, and the probability exp(z_j) / sum_k exp(z_k).  Each is rounded
      fp64 -> fp32 -> dtype, and is unsettled when the fp64 value lies within a guard band of a rounding midpoint
      of fp32 or of the dtype.

    Guard bands (u = 2^-53, gamma_k = k u / (1 - k u); the products x_k y_k of fp16 / fp32 numbers are exact in fp64):
      dot product over d terms   any summation order, fused or not, errs by at most gamma_d * sum|x_k y_k| (Higham,
                                 Accuracy and Stability, section 3.1).  Band: 8 * gamma_d * sum|x_k y_k|.
      norm                       the sum of squares S as above (all terms positive: sum|terms| = S), carried through
                                 the square root: d sqrt(S) = dS / (2 sqrt(S)), plus the square root's own rounding.
                                 Band on sqrt(S): (4 gamma_d + 8 u) * sqrt(S).
      probability                z_j = logit_j - max is one correctly rounded fp64 subtraction of exact inputs (the same
                                 everywhere); exp errs by <= 1 ulp in a good libm, the c-term sum of positive terms by
                                 gamma_c relative, the division by u/2: at most (1 + c + 1 + 1) u <= (4 + c) u relative.
                                 Band: 8 * (4 + c) * u * p_j.
    The factor 8 is the margin over those worst-case bounds.  One sharper case is used: when every term is a multiple of
    a quantum q (the product of the operands' spacings) and sum|terms| < 2^53 q, every partial sum in every order, fused
    or not, is a multiple of q below 2^53 q and therefore exact in fp64: the sum has no error at all and its band is 0
    (the norm keeps the square root's 8 u).  That is the rule for almost every fp16 dot product, whose terms are
    multiples of 2^-48 at worst; without it the many fp16 sums that land EXACTLY on an fp32 midpoint -- a tie that
    round-to-nearest-even resolves identically everywhere -- would count as doubtful.  An unsettled norm or dot product changes everything
    after it by more than a unit in the last place, so callers that judge an implementation to within one such unit
    need inputs without them: `detail=True` adds a dict of per-item flags {"norm", "dot", "prob"} to tell them apart, and
    "eps", the fp32 spacing at the item's largest |logit|: if dot products flip, every fp32 logit moves by at most eps
    and every probability by a factor within exp(+-2 eps).
    Non-finite values settle nothing and unsettle nothing: NaN in, NaN out, in every order."""
    dtype = np.dtype(dtype)
    img = np.asarray(img_emb, dtype=dtype)
    txt = np.asarray(txt_emb, dtype=dtype)
    n, c, d = txt.shape
    assert img.shape == (n, d)
    u = 2.0 ** -53
    probs = np.empty((n, c), dtype)
    flags = {k: np.zeros(n, bool) for k in ("norm", "dot", "prob")}
    flags["eps"] = np.zeros(n)
    step = max(1, (1 << 21) // (c * d))                           # ~2 M candidate elements per slab
    with np.errstate(all="ignore"):
        for lo in range(0, n, step):
            a, t = img[lo:lo + step], txt[lo:lo + step]
            sl = slice(lo, lo + len(a))
            if normalize:
                va = np.sqrt((a.astype(np.float64) ** 2).sum(-1))
                vt = np.sqrt((t.astype(np.float64) ** 2).sum(-1))
                ba = np.where(va ** 2 < 2.0 ** 52 * _quantum(a) ** 2, 8 * u, 4 * _gamma(d) + 8 * u)
                bt = np.where(vt ** 2 < 2.0 ** 52 * _quantum(t) ** 2, 8 * u, 4 * _gamma(d) + 8 * u)
                flags["norm"][sl] = _unsettled(va, ba * va, dtype) | _unsettled(vt, bt * vt, dtype).any(-1)
                na = va.astype(np.float32).astype(dtype)
                nt = vt.astype(np.float32).astype(dtype)
                a = (a.astype(np.float32) / na.astype(np.float32)[:, None]).astype(dtype)
                t = (t.astype(np.float32) / nt.astype(np.float32)[:, :, None]).astype(dtype)
            a = (np.float32(logit_scale) * a.astype(np.float32)).astype(dtype)
            a64, t64 = a.astype(np.float64), t.astype(np.float64)
            dot = np.matmul(t64, a64[:, :, None])[:, :, 0]
            mag = np.matmul(np.abs(t64), np.abs(a64)[:, :, None])[:, :, 0]
            exact = mag < 2.0 ** 52 * (_quantum(a)[:, None] * _quantum(t))
            flags["dot"][sl] = _unsettled(dot, np.where(exact, 0.0, 8 * _gamma(d) * mag), dtype).any(-1)
            logits = dot.astype(np.float32).astype(dtype)
            flags["eps"][sl] = np.spacing(np.abs(dot).max(-1).astype(np.float32)).astype(np.float64)
            z = logits.astype(np.float64) - logits.max(-1, keepdims=True).astype(np.float64)
            e = np.exp(z)
            p = e / e.sum(-1, keepdims=True)
            flags["prob"][sl] = _unsettled(p, 8 * (4 + c) * u * p, dtype).any(-1)
            probs[sl] = p.astype(np.float32).astype(dtype)
    settled = ~(flags["norm"] | flags["dot"] | flags["prob"])
    return (probs, settled, flags) if detail else (probs, settled)


def ulp_distance(a, b):
    """Units in the last place between two arrays of one float dtype (0 where both are NaN; huge where one is)."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.dtype in (np.float16, np.float32)
    it = np.int16 if a.dtype == np.float16 else np.int32
    top = np.int64(np.iinfo(it).min)

    def ordered(x):                                             # sign-magnitude bits -> a monotone integer line
        i = x.view(it).astype(np.int64)
        return np.where(i < 0, top - i, i)
    dist = np.abs(ordered(a) - ordered(b))
    both, one = np.isnan(a) & np.isnan(b), np.isnan(a) ^ np.isnan(b)
    return np.where(both, 0, np.where(one, np.int64(1) << 40, dist))


def softmax(x):
    x = np.asarray(x, dtype=np.float64)
    e = np.exp(x - x.max())
    return e / e.sum()


def rp_bins(num_captions, perm, num_bins=10):
    """RP_coco.py:41-52.  perm: the shuffled list(range(num_captions))."""
    samples_per_bin = int(len(perm) / num_bins)
    bins = []
    for i in range(num_bins):
        if i == (num_bins - 1) and num_captions % num_bins != 0:
            bins.append(list(perm[i * samples_per_bin:]))
        else:
            bins.append(list(perm[i * samples_per_bin:(i + 1) * samples_per_bin]))
    return bins


def rp_score(success, perm, num_bins=10):
    """success[i] in {0, 1}: whether item i retrieved its true caption.  Returns (mean, std, bin scores)."""
    success = np.asarray(success)
    bins = rp_bins(len(success), list(perm), num_bins)
    scores = [float(np.sum(success[b])) * 1.0 / len(b) for b in bins]
    return float(np.mean(scores)), float(np.std(scores)), scores


def rp_success_from_logits(logits):
    """(N, 1 + mismatched) logits -> success flags (argmax of the softmax == 0)."""
    return np.array([int(np.argmax(softmax(row)) == 0) for row in np.asarray(logits)])


def rp_text(mean, std):
    return f"R-precision: {mean} +- {std}"                  # RP_coco.py:85,90


def pa_score(logits_by_phrase, threshold=0.6):
    """{phrase: (n, 2) logits [true, false]} -> (PA, {phrase: score})."""
    per = {}
    for phrase, rows in logits_by_phrase.items():
        ok = [1.0 if softmax(r)[0] > threshold else 0.0 for r in rows]
        per[phrase] = sum(ok) / len(ok)
    return float(np.mean([per[p] for p in per])), per
