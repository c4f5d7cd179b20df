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


def _distinct_tables(cr_takes_cb):
    out = []
    for li, name in enumerate(("444", "422", "420")):
        sampling = LAYOUTS[name]
        w, h = 38, 29                                                          # even (a right chroma edge), not a multiple of 16
        for fi, form in enumerate(("all-three", "chroma-only")):
            rng = np.random.default_rng([11, li, fi])
            q = [rng.integers(1, 32, 64).astype(np.int32) for _ in range(3)]
            for t in q:
                t[0] = rng.integers(2, 9)
            if form == "chroma-only":
                q[0] = q[1].copy()                                             # only Cr's table differs from the others
            assert not np.array_equal(q[1], q[2])
            b = _blank(w, h, sampling)
            for c in range(3):
                b[c][...] = rng.integers(-3, 4, b[c].shape) * (rng.random(b[c].shape) < 0.3)
                b[c][..., 0] = rng.integers(-40, 41, b[c].shape[:2])
            if cr_takes_cb:
                q[2] = q[1]
            out.append((f"{name}-tables-{form}", jw.write_jpeg(w, h, b, q, sampling)))
    return out


def distinct_tables():
    """Three different random quantisation tables for Y, Cb and Cr (Pillow's own files share one between Cb and Cr), and a form
    in which only Cr's table differs from the other two."""
    return _distinct_tables(False)


def distinct_tables_cr_takes_cb():
    """The same files with Cr's table replaced by Cb's: what a decoder that read the wrong table would make of distinct_tables().
    Pillow's pixels of the two must differ, else distinct_tables() proves nothing."""
    return _distinct_tables(True)


DENSE_BOUNDS = (2047, 4095, 8191, 16383)


def dense_out_of_range():
    """Blocks with MANY products near the guard (TISE_JPEG_MAX_PRODUCT): the regime in which libjpeg-turbo's 16-bit lanes
    wrap (rows 1..7 all zero) or saturate (otherwise) and the row pass leaves 32 bits.  The writer's Annex K tables carry AC
    values of at most 10 bits and DC differences of at most 11, so the quantiser is ceil(bound / 1023) and every coefficient,
    DC included, lies in +-(bound // q) <= 1023.  Four layouts x bounds x densities, row-0-only and column-0-only blocks,
    and a checkerboard of row-0-only blocks (wrap) beside blocks with one more term in rows 1..7 (saturate), products exactly
    at the guard (129 * 127), so that the 8-lane groups of one wave disagree."""
    out = []
    w, h = 45, 27
    for li, (name, sampling) in enumerate(LAYOUTS.items()):
        nc = len(sampling)
        for bound in DENSE_BOUNDS:
            q = -(-bound // 1023)
            m = bound // q
            qt = [np.full(64, q, dtype=np.int32)] * nc
            rng = np.random.default_rng([23, li, bound])
            forms = [(f"d{d}", None, d) for d in (0.05, 0.3, 1.0)] + [("row0", np.arange(8), 1.0), ("col0", np.arange(0, 64, 8), 1.0)]
            for form, keep, density in forms:
                b = _blank(w, h, sampling)
                for c in range(nc):
                    v = rng.integers(-m, m + 1, b[c].shape) * (rng.random(b[c].shape) < density)
                    if keep is not None:
                        mask = np.zeros(64, dtype=bool)
                        mask[keep] = True
                        v = v * mask
                    b[c][...] = v
                out.append((f"{name}-dense-{bound}-{form}", jw.write_jpeg(w, h, b, qt, sampling)))
        rng = np.random.default_rng([29, li])
        for extra in ("small", "guard"):
            b = _blank(w, h, sampling)
            for c in range(nc):
                bh, bw = b[c].shape[:2]
                b[c][..., :8] = rng.choice([-129, 129], (bh, bw, 8))
                for by in range(bh):
                    for bx in range(bw):
                        if (by + bx) & 1:                                      # one more term below row 0: this block saturates
                            b[c][by, bx, int(rng.integers(8, 64))] = int(rng.choice([-1, 1])) * (1 if extra == "small" else 129)
            out.append((f"{name}-checkerboard-{extra}", jw.write_jpeg(w, h, b, [np.full(64, 127, dtype=np.int32)] * nc, sampling)))
    return out


LONG_EDGES = ((65500, 1, "gray"), (1, 65500, "gray"), (65500, 3, "420"), (2, 65500, "422"), (65500, 2, "444"))


def long_edges():
    """libjpeg's largest dimension on either axis, a few low-frequency terms per block."""
    out = []
    for k, (w, h, name) in enumerate(LONG_EDGES):
        sampling = LAYOUTS[name]
        rng = np.random.default_rng([31, k])
        b = _blank(w, h, sampling)
        for c in range(len(sampling)):
            b[c][..., 0] = rng.integers(-100, 101, b[c].shape[:2])
            for pos in (1, 8, 9):
                b[c][..., pos] = rng.integers(-12, 13, b[c].shape[:2])
        out.append((f"{w}x{h}-{name}", jw.write_jpeg(w, h, b, [np.full(64, 6, dtype=np.int32)] * len(sampling), sampling)))
    return out


def beyond_libjpeg_dimension():
    """Sizes a SOF marker can state and libjpeg refuses (JPEG_MAX_DIMENSION = 65500): Pillow raises OSError for them."""
    out = []
    for w, h in ((65501, 1), (65535, 1), (1, 65535)):
        b = _blank(w, h, LAYOUTS["gray"])
        b[0][..., 0] = 9
        out.append((f"{w}x{h}-gray", jw.write_jpeg(w, h, b, [np.full(64, 8, dtype=np.int32)])))
    return out


# ---- launches: where each image lies in the output, and which branches of the two kernels a launch reaches -----------------
PIXEL_SLOT = (23, 31)                                                          # (w, h) of the mode-0 slot the matrix launch carries


def matrix_cases(tmpdir):
    """The files of the GPU matrix launch (tests/test_gpu_jpeg.py); the launch adds one mode-0 slot of PIXEL_SLOT pixels."""
    return pillow_matrix(tmpdir) + writer_extremes() + tiny_chroma(tmpdir) + distinct_tables() + dense_out_of_range()


def plan_offsets(sizes, align=16, residue=0):
    """Byte offset of every (h, w) image in the output and the extent: images ``align`` apart, the first at ``residue``."""
    offs, pos = np.zeros(len(sizes), dtype=np.int64), int(residue)
    for i, (h, w) in enumerate(sizes):
        offs[i] = pos
        pos += (h * w * 3 + align - 1) // align * align
    return offs, pos


LAYOUT_NAMES = ("gray", "444", "422", "420")                                   # by TISE_JPEG_GRAY .. TISE_JPEG_420
CENSUS_ROWS = (["gray", "1x1", "mode0-copy"] + [f"{s}-{e}" for s in ("2x1", "2x2") for e in ("narrow", "left", "interior", "right")]
               + ["2x2-oy-top", "2x2-oy-bottom", "2x2-oy-free", "store-npx1", "store-npx2", "store-npx3", "store-npx4-dword",
                  "store-npx4-bytes", "idct-groups-live", "idct-groups-shadow", "idct-workgroups-idle"])


def branch_census(items):
    """Pixels / threads / groups / workgroups of ONE launch that fall into each branch of jpeg_colour_kernel and
    jpeg_idct_kernel (csrc/jpeg_idct.hip).  ``items``: (w, h, layout, output offset) per image, layout one of LAYOUT_NAMES
    or "pix" (a mode-0 slot); the offset counts from a 4-byte-aligned address.  Plain counting from the kernels' index
    arithmetic as documented; the tests assert that no row is empty for the launches that are meant to cover them."""
    n = dict.fromkeys(CENSUS_ROWS, 0)
    blocks = []
    for w, h, layout, off in items:
        hs, vs = {"gray": (1, 1), "444": (1, 1), "422": (2, 1), "420": (2, 2), "pix": (1, 1)}[layout]
        if layout == "pix":
            n["mode0-copy"] += w * h
            blocks.append(0)
        else:
            mx, my = -(-w // (8 * hs)), -(-h // (8 * vs))
            blocks.append(mx * hs * my * vs + (0 if layout == "gray" else 2 * mx * my))
            if layout == "gray":
                n["gray"] += w * h
            elif hs == 1:
                n["1x1"] += w * h
            else:
                s = f"{hs}x{vs}"
                dsw, dsh = (w + 1) // 2, (h + vs - 1) // vs
                if dsw <= 2:
                    n[s + "-narrow"] += w * h
                else:
                    left, right = h, (h if w % 2 == 0 else 0)                  # x = 0; x = w - 1 odd with x >> 1 == dsw - 1
                    n[s + "-left"] += left
                    n[s + "-right"] += right
                    n[s + "-interior"] += w * h - left - right
                    if vs == 2:
                        top, bottom = w, (w if h % 2 == 0 else 0)              # y = 0; y = h - 1 odd with (y >> 1) + 1 == dsh
                        n["2x2-oy-top"] += top
                        n["2x2-oy-bottom"] += bottom
                        n["2x2-oy-free"] += w * h - top - bottom
        if w % 4:
            n[f"store-npx{w % 4}"] += h
        aligned = int(np.count_nonzero(((int(off) + 3 * w * np.arange(h, dtype=np.int64)) & 3) == 0))   # 12 bytes per thread: a row's phase
        n["store-npx4-dword"] += (w // 4) * aligned
        n["store-npx4-bytes"] += (w // 4) * (h - aligned)
    gx = -(-max(blocks) // 32)
    for t in blocks:
        if t:
            n["idct-groups-live"] += t
            n["idct-groups-shadow"] += -(-t // 32) * 32 - t
        n["idct-workgroups-idle"] += gx - -(-t // 32)
    return n
