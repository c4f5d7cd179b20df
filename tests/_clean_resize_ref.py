"""numpy restatement of Pillow's resize of a 32-bit float image (mode "F"), the resize of clean-fid -- test infrastructure.

Written from Pillow's documented algorithm (Resample.c), not from the kernel:
  * precompute_coeffs: per output coordinate a window [xmin, xmin + cnt) of filter weights in double precision, normalised by
    their sum (``k[x] /= ww``); nothing is rounded to fixed point (that is the 8-bit path);
  * per output ``ss = 0.0; ss += (double)pixel * k[x]`` in ascending x, a multiply and an add (numpy's elementwise ``*`` and
    ``+`` on float64 arrays are exactly that); the result is stored as float32;
  * the horizontal pass first, the vertical pass on its float32 result; a pass whose size does not change is skipped;
  * ``Image.resize`` (PIL/Image.py, observed on Pillow 12.2.0) runs the vertical pass first, as two separate resizes, when
    ``h > 100 * w and oh < h``: ``vertical_first``.
tests/test_clean_resize_host.py pins this file to Pillow bit for bit; the GPU tests pin the kernel to this file."""
import numpy as np

FILTERS = ("bilinear", "bicubic")


def _bilinear(x):
    x = -x if x < 0.0 else x
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x):
    a = -0.5
    x = -x if x < 0.0 else x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coeffs(in_size, out_size, filter="bicubic"):
    """[(xmin, k)] per output coordinate: k float64, normalised; Resample.c precompute_coeffs in its own operation order."""
    f, support0 = (_bicubic, 2.0) if filter == "bicubic" else (_bilinear, 1.0)
    scale = in_size / out_size
    filterscale = 1.0 if scale < 1.0 else scale
    support = support0 * filterscale
    ss = 1.0 / filterscale
    out = []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k = np.array([f((x + xmin - center + 0.5) * ss) for x in range(xmax)], dtype=np.float64)
        ww = 0.0
        for v in k:
            ww += float(v)
        if ww != 0.0:
            k = k / ww
        out.append((xmin, k))
    return out


def _pass(img, out_size, axis, filter):
    """One pass along ``axis`` (0: vertical, 1: horizontal) of a float32 (h, w, c) image -> float32."""
    if img.shape[axis] == out_size:
        return img
    src = np.moveaxis(img, axis, 0)
    out = np.empty((out_size,) + src.shape[1:], dtype=np.float32)
    for xx, (xmin, k) in enumerate(coeffs(img.shape[axis], out_size, filter)):
        ss = np.zeros(src.shape[1:], dtype=np.float64)
        for x in range(len(k)):
            ss = ss + src[xmin + x].astype(np.float64) * k[x]
        out[xx] = ss.astype(np.float32)
    return np.ascontiguousarray(np.moveaxis(out, 0, axis))


def vertical_first(h, w, oh):
    """Image.resize's rule for a source more than 100 times taller than wide whose height shrinks."""
    return h > 100 * w and oh < h


def resize_f32(img_u8, out_hw, filter="bicubic", order=None):
    """(h, w, c) uint8 -> (oh, ow, c) float32, every channel resampled as a mode "F" image; not clipped, not quantised.
    ``order``: 0 horizontal first, 1 vertical first, None: Pillow's rule."""
    oh, ow = out_hw
    x = np.asarray(img_u8).astype(np.float32)
    if order is None:
        order = 1 if vertical_first(x.shape[0], x.shape[1], oh) else 0
    if order:
        return _pass(_pass(x, oh, 0, filter), ow, 1, filter)
    return _pass(_pass(x, ow, 1, filter), oh, 0, filter)


def affine(x, clip=(0, 255), sub=128, div=128):
    """clean-fid's ``np.clip(x, 0, 255)`` then ``x1 = x - 128; x2 = x1 / 128`` in float32."""
    x = np.clip(x, np.float32(clip[0]), np.float32(clip[1])).astype(np.float32)
    return ((x - np.float32(sub)) / np.float32(div)).astype(np.float32)


def clean_input(img_u8, out_hw, filter="bicubic", clip=(0, 255), sub=128, div=128, order=None):
    """(h, w, 3) uint8 -> (oh, ow, 3) float32 network input of the clean route."""
    return affine(resize_f32(img_u8, out_hw, filter, order), clip, sub, div)


def pil_resize_f32(img_u8, out_hw, filter="bicubic"):
    """The same through Pillow itself, channel by channel (clean-fid's resize_single_channel without its clip; a 2-D float32 array becomes a mode "F" image)."""
    from PIL import Image
    oh, ow = out_hw
    res = Image.BICUBIC if filter == "bicubic" else Image.BILINEAR
    x = np.asarray(img_u8)
    chans = [np.asarray(Image.fromarray(np.ascontiguousarray(x[:, :, c]).astype(np.float32)).resize((ow, oh), resample=res),
                        dtype=np.float32) for c in range(x.shape[2])]
    return np.stack(chans, axis=2)


def content(kind, seed, h, w):
    """Seeded (h, w, 3) uint8 test image: "rand" uniform bytes, "bw" only 0 and 255 (bicubic overshoot to about -70 and 326)."""
    rng = np.random.RandomState(seed)
    if kind == "bw":
        return (rng.randint(0, 2, size=(h, w, 3)) * 255).astype(np.uint8)
    return rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
