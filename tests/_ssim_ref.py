"""numpy fp64 restatement of the paired-image definitions (include/tise_hip.h, tise_toolbox_amd/paired.py): PSNR, SSIM (Wang,
Bovik, Sheikh & Simoncelli 2004) and MS-SSIM (Wang, Simoncelli & Bovik 2003) of 8-bit RGB pairs, per channel, L = 255.  Restated
from the papers; no metric package is involved.  tests/test_paired_host.py pins it against an independent scipy route."""
import numpy as np

TAPS = 11
SIGMA = 1.5
C1 = (0.01 * 255.0) ** 2
C2 = (0.03 * 255.0) ** 2
MS_WEIGHTS = np.array([0.0448, 0.2856, 0.3001, 0.2363, 0.1333], dtype=np.float64)
MS_MIN_SIDE = 176                      # 176 -> 88 -> 44 -> 22 -> 11


def window():
    i = np.arange(TAPS, dtype=np.float64)
    g = np.exp(-(i - 5.0) ** 2 / (2.0 * SIGMA * SIGMA))
    return g / g.sum()


def blur_valid(z):
    """(h, w, c) fp64 -> (h - 10, w - 10, c): the separable 11-tap window at the valid positions, horizontal pass first."""
    g = window()
    h, w = z.shape[0], z.shape[1]
    t = np.zeros((h, w - 10) + z.shape[2:], dtype=np.float64)
    for k in range(TAPS):
        t += g[k] * z[:, k:k + w - 10]
    out = np.zeros((h - 10, w - 10) + z.shape[2:], dtype=np.float64)
    for k in range(TAPS):
        out += g[k] * t[k:k + h - 10]
    return out


def ssim_maps(x, y):
    """(h, w, 3) arrays of any real dtype -> (ssim map, cs map), each (h - 10, w - 10, 3) fp64."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if x.shape != y.shape or x.ndim != 3:
        raise ValueError(f"two (h, w, c) images of one shape (got {x.shape} and {y.shape})")
    if min(x.shape[0], x.shape[1]) < TAPS:
        raise ValueError(f"SSIM needs both sides >= {TAPS} (got {x.shape[0]} x {x.shape[1]})")
    mx, my = blur_valid(x), blur_valid(y)
    exx, eyy, exy = blur_valid(x * x), blur_valid(y * y), blur_valid(x * y)
    mxx, myy, mxy = mx * mx, my * my, mx * my
    sxx, syy, sxy = exx - mxx, eyy - myy, exy - mxy
    cs = (2.0 * sxy + C2) / (sxx + syy + C2)
    l = (2.0 * mxy + C1) / (mxx + myy + C1)
    return l * cs, cs


def ssim_means(x, y):
    """-> (3, 2) fp64: per channel the mean of the ssim map and the mean of the cs map (what tise_ssim_pairs writes per pair)."""
    s, cs = ssim_maps(x, y)
    return np.stack([s.mean(axis=(0, 1)), cs.mean(axis=(0, 1))], axis=1)


def ssim(x, y):
    return float(ssim_means(x, y)[:, 0].mean())


def pool2x2(z):
    """(h, w, c) -> (h // 2, w // 2, c) fp64: the mean of every whole 2 x 2 block; a last odd row or column is dropped."""
    z = np.asarray(z, dtype=np.float64)
    h2, w2 = z.shape[0] // 2, z.shape[1] // 2
    z = z[:2 * h2, :2 * w2]
    return (z[0::2, 0::2] + z[0::2, 1::2] + z[1::2, 0::2] + z[1::2, 1::2]) * 0.25


def ms_scale_means(x, y):
    """-> (5, 3) fp64: per scale and channel the cs mean (scales 1..4) or the ssim mean (scale 5)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if min(x.shape[0], x.shape[1]) < MS_MIN_SIDE:
        raise ValueError(f"MS-SSIM needs the smaller side >= {MS_MIN_SIDE} (got {x.shape[0]} x {x.shape[1]})")
    m = np.zeros((5, 3), dtype=np.float64)
    for s in range(5):
        means = ssim_means(x, y)
        m[s] = means[:, 1] if s < 4 else means[:, 0]
        if s < 4:
            x, y = pool2x2(x), pool2x2(y)
    return m


def ms_from_means(m):
    """(5, 3) scale means -> MS-SSIM: per channel prod_s max(m_s, 0) ^ w_s, then the mean over the channels."""
    m = np.maximum(np.asarray(m, dtype=np.float64), 0.0)
    return float(np.prod(m ** MS_WEIGHTS[:, None], axis=0).mean())


def ms_ssim(x, y):
    return ms_from_means(ms_scale_means(x, y))


def sse(x, y):
    d = np.asarray(x, dtype=np.int64) - np.asarray(y, dtype=np.int64)
    return int((d * d).sum())


def psnr_from_sse(s, h, w):
    """An exact integer SSE of an (h, w, 3) pair -> 10 log10(255^2 / (SSE / (3 h w))); inf for an identical pair."""
    if s == 0:
        return float("inf")
    return float(10.0 * np.log10(255.0 ** 2 / (float(s) / float(3 * h * w))))


def psnr(x, y):
    return psnr_from_sse(sse(x, y), np.shape(x)[0], np.shape(x)[1])


def smooth_pair(h, w, sigma_noise, seed):
    """The GPU tests' inputs: a smooth seeded uint8 image (box-blurred noise, several passes, rescaled to 0..255) and the same
    plus N(0, sigma_noise) noise, clipped.  (Independent noise images have cs ~ 0, which makes an MS-SSIM bound meaningless.)"""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((h + 16, w + 16, 3))
    for _ in range(3):                                       # three 5-tap box passes per axis ~ a Gaussian blur of sigma 2.4
        z = sum(np.roll(z, k, axis=0) for k in range(-2, 3)) / 5.0
        z = sum(np.roll(z, k, axis=1) for k in range(-2, 3)) / 5.0
    z = z[8:8 + h, 8:8 + w]
    lo, hi = z.min(), z.max()
    x = np.rint((z - lo) / (hi - lo) * 255.0).astype(np.uint8)
    y = np.clip(np.rint(x.astype(np.float64) + rng.normal(0.0, sigma_noise, x.shape)), 0, 255).astype(np.uint8)
    return x, y
