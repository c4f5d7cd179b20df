"""JPEG files for the host and GPU tests of the JPEG feed: the Pillow-written matrix and the hand-placed extremes of
tests/_jpeg_writer.py.  Every case is (name, file bytes); the ground truth is always Pillow's own decode of those bytes."""
import io
import os

import numpy as np
from PIL import Image

from . import _cases, _jpeg_writer as jw

SIZES = [(1, 1), (7, 5), (8, 8), (17, 33), (64, 33), (255, 257), (256, 256), (480, 640)]      # (w, h)


def pillow_rgb(blob):
    return np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"))


def _content(kind, w, h, seed):
    if kind == "smooth":
        return _cases.smooth_images(1, h, w, seed=seed)[0]
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def save_jpeg(img, path, **kw):
    """Pillow writes the file; ``optimize`` emits the scan in one piece, which for noise at quality 100 exceeds the encoder
    buffer Pillow sizes from the image ("Suspension not allowed here"), so the block size is raised for the call."""
    from PIL import ImageFile
    old, ImageFile.MAXBLOCK = ImageFile.MAXBLOCK, 1 << 23
    try:
        Image.fromarray(img).convert(kw.pop("mode", "RGB")).save(path, "JPEG", **kw)
    finally:
        ImageFile.MAXBLOCK = old
    with open(path, "rb") as f:
        return f.read()


def pillow_matrix(tmpdir):
    """The full product sizes x (4:4:4, 4:2:2, 4:2:0, gray) x quality x optimize x restart x content: 1024 files."""
    out = []
    tmp = os.path.join(str(tmpdir), "case.jpg")
    for (w, h) in SIZES:
        for kind in ("smooth", "noise"):
            img = _content(kind, w, h, seed=w + h)
            if kind == "noise" and w * h > 64 * 64:
                img = img // 2 + _content("smooth", w, h, seed=w) // 2        # halves the file size of the large noise cases
            for ss in (0, 1, 2, "L"):
                for q in (30, 75, 95, 100):
                    for opt in (False, True):
                        for rst in (0, 3):
                            kw = dict(quality=q, optimize=opt)
                            if ss == "L":
                                kw["mode"] = "L"
                            else:
                                kw["subsampling"] = ss
                            if rst:
                                kw["restart_marker_blocks"] = rst
                            out.append((f"{w}x{h}-{kind}-ss{ss}-q{q}-opt{int(opt)}-rst{rst}", save_jpeg(img, tmp, **kw)))
    return out


LAYOUTS = {"gray": [(1, 1)], "444": [(1, 1)] * 3, "422": [(2, 1), (1, 1), (1, 1)], "420": [(2, 2), (1, 1), (1, 1)]}


def _blank(w, h, sampling):
    return [np.zeros(s + (64,), dtype=np.int32) for s in jw.blocks_shape(w, h, sampling)]


def writer_extremes():
    """Exact coefficient values: clamp saturation on both sides, DC-only blocks, one maximal AC term in every position
    (product 129 * 127 = 16383, the guard itself), for every layout and with a restart interval."""
    out = []
    rng = np.random.default_rng(5)
    for name, sampling in LAYOUTS.items():
        w, h = 21, 19
        nc = len(sampling)
        ones = [np.ones(64, dtype=np.int32)] * nc
        q127 = [np.full(64, 127, dtype=np.int32)] * nc
        # DC-only blocks over the whole useful range, both signs (quantiser 1 and 16)
        for q in (1, 16):
            b = _blank(w, h, sampling)
            for c in range(nc):
                b[c][..., 0] = rng.integers(-(1023 // q), 1023 // q + 1, b[c].shape[:2])
            out.append((f"{name}-dc-q{q}", jw.write_jpeg(w, h, b, [np.full(64, q, dtype=np.int32)] * nc, sampling)))
        # saturation: large DC with opposing AC terms drives samples far beyond 0 and 255 inside one block
        b = _blank(w, h, sampling)
        for c in range(nc):
            b[c][..., 0] = rng.choice([-1000, 1000], b[c].shape[:2])
            b[c][..., 1] = rng.choice([-600, 600], b[c].shape[:2])
            b[c][..., 8] = rng.choice([-600, 600], b[c].shape[:2])
            b[c][..., 63] = rng.choice([-300, 300], b[c].shape[:2])
        out.append((f"{name}-saturate", jw.write_jpeg(w, h, b, ones, sampling, restart=2)))
        # realistic dense blocks with a restart interval and no JFIF marker (ids 1 2 3) / an Adobe marker with transform 1
        b = _blank(w, h, sampling)
        for c in range(nc):
            b[c][...] = rng.integers(-6, 7, b[c].shape)
            b[c][..., 0] = rng.integers(-60, 61, b[c].shape[:2])
        q = [np.arange(3, 67, dtype=np.int32)] * nc
        out.append((f"{name}-dense-nomarker", jw.write_jpeg(w, h, b, q, sampling, restart=1, marker=None)))
        out.append((f"{name}-dense-adobe1-sof1", jw.write_jpeg(w, h, b, q, sampling, marker="adobe" if nc == 3 else "jfif", sof=0xC1)))
    # one maximal term (|coefficient * quantiser| = 16383) in every position and sign, one block per position (4:2:0 and gray)
    for name in ("gray", "420"):
        sampling = LAYOUTS[name]
        w, h = 64, 64
        nc = len(sampling)
        for sign in (1, -1):
            b = _blank(w, h, sampling)
            flat = b[0].reshape(-1, 64)
            for pos in range(64):
                flat[pos, pos] = sign * 129
                if pos:
                    flat[pos, 0] = 3                                           # a small DC beside it
            for c in range(1, nc):
                fc = b[c].reshape(-1, 64)
                for pos in range(fc.shape[0]):
                    fc[pos, (pos * 5) % 64] = -sign * 129
            out.append((f"{name}-max-term-{'pos' if sign > 0 else 'neg'}", jw.write_jpeg(w, h, b, [np.full(64, 127, dtype=np.int32)] * nc, sampling)))
    return out


def tiny_chroma(tmpdir):
    """Chroma planes at most 2 samples wide (replicated, not filtered, by libjpeg) and the first widths beyond."""
    out = []
    for (w, h) in ((2, 2), (3, 3), (4, 9), (5, 4), (6, 2)):
        img = np.random.default_rng(w * h).integers(0, 256, (h, w, 3), dtype=np.uint8)
        for ss in (1, 2):
            out.append((f"{w}x{h}-ss{ss}", save_jpeg(img, os.path.join(str(tmpdir), "t.jpg"), quality=90, subsampling=ss)))
    return out


def beyond_guard():
    """128 * 128 = 16384: one past the guard -> UNSUPPORTED."""
    b = _blank(16, 16, LAYOUTS["444"])
    b[0][0, 0, 9] = 128
    return jw.write_jpeg(16, 16, b, [np.full(64, 128, dtype=np.int32)] * 3, LAYOUTS["444"])


def unsupported_layouts():
    rng = np.random.default_rng(2)
    out = []
    for name, sampling, scans in (("440", [(1, 2), (1, 1), (1, 1)], None), ("411", [(4, 1), (1, 1), (1, 1)], None),
                                  ("two-scans", [(1, 1)] * 3, [[0], [1, 2]])):
        b = _blank(40, 24, sampling)
        for c in range(3):
            b[c][..., 0] = rng.integers(-50, 50, b[c].shape[:2])
        out.append((name, jw.write_jpeg(40, 24, b, [np.full(64, 8, dtype=np.int32)] * 3, sampling, scans=scans)))
    b = _blank(16, 16, LAYOUTS["444"])
    out.append(("ids-RGB", jw.write_jpeg(16, 16, b, [np.ones(64, dtype=np.int32)] * 3, LAYOUTS["444"], marker=None, ids=[82, 71, 66])))
    out.append(("adobe-transform-0", jw.write_jpeg(16, 16, b, [np.ones(64, dtype=np.int32)] * 3, LAYOUTS["444"], marker="adobe0")))
    return out
