"""CPU: the entry points of the paired-image kernels (csrc/ssim.hip) are declared, bound and exported, reject bad arguments before
touching the device, and size their workspace by the documented formula (the sibling of tests/test_cabi_symbols_nn.py)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tise_pair_sse_u8", "tise_ssim_pairs", "tise_pool2x2_pairs", "tise_ssim_workspace_bytes")
MAX_SIDE, MAX_PAIRS, TILE = 16384, 65535, 64


def test_declared_bound_and_exported():
    from tise_toolbox_amd import _lib, build, device
    raw_text = open(os.path.join(ROOT, "include", "tise_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw_text, flags=re.S)
    declared = set(re.findall(r"\b(tise_[a-z0-9_]+)\s*\(", text))
    assert "ssim.hip" in build.SOURCES
    build.build(force=False, verbose=False)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in declared and name in _lib.SIGNATURES
        getattr(raw, name)
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [6, 9, 7, 4]
    assert len(_lib.SIGNATURES["tise_resize_ragged_torch_f32"][1]) == 8                       # the pattern it follows stays
    # the header's constants, device.py's mirror of them, and the table record
    macros = dict(re.findall(r"#define (TISE_SSIM_[A-Z_]+) (\d+)", raw_text))
    assert {k: int(v) for k, v in macros.items()} == {"TISE_SSIM_TAPS": 11, "TISE_SSIM_TILE": TILE, "TISE_SSIM_MAX_SIDE": MAX_SIDE,
                                                       "TISE_SSIM_MAX_PAIRS": MAX_PAIRS}
    assert (device.SSIM_TAPS, device.SSIM_TILE, device.SSIM_MAX_SIDE, device.SSIM_MAX_PAIRS) == (11, TILE, MAX_SIDE, MAX_PAIRS)
    assert device._PAIR.itemsize == 24 and [device._PAIR.fields[k][1] for k in ("x", "y", "h", "w")] == [0, 8, 16, 20]
    assert re.search(r"typedef struct tise_pair \{\s*const void\* x;\s*const void\* y;\s*int32_t h, w;\s*\} tise_pair_t;", text)


def _tiles(side):
    return (side - 10 + TILE - 1) // TILE


def test_workspace_formula():
    """bytes = 48 n tiles(max_h) tiles(max_w), tiles(s) = ceil((s - 10) / 64)."""
    from tise_toolbox_amd import _lib
    lib = _lib.load()
    nb = ctypes.c_size_t(7)
    for n, h, w in ((1, 11, 11), (1, 74, 74), (1, 75, 74), (1, 74, 75), (50, 256, 256), (3, 139, 203), (0, 11, 11), (65535, 74, 74),
                    (1, 16384, 16384), (64, 16384, 16384), (7, 11, 16384), (1000, 1080, 1920)):
        assert lib.tise_ssim_workspace_bytes(n, h, w, ctypes.byref(nb)) == _lib.TISE_OK, (n, h, w)
        assert nb.value == 48 * n * _tiles(h) * _tiles(w), (n, h, w)
    for kw in ((-1, 11, 11), (1, 10, 11), (1, 11, 10), (1, 0, 64), (1, 64, -5)):
        assert lib.tise_ssim_workspace_bytes(*kw, ctypes.byref(nb)) == _lib.TISE_ERR_INVALID_ARG, kw
    assert lib.tise_ssim_workspace_bytes(1, 11, 11, None) == _lib.TISE_ERR_INVALID_ARG
    for kw in ((1, MAX_SIDE + 1, 11), (1, 11, MAX_SIDE + 1), (MAX_PAIRS + 1, 11, 11), (65, 16384, 16384)):       # 65 * 256 * 256 > 2^22
        assert lib.tise_ssim_workspace_bytes(*kw, ctypes.byref(nb)) == _lib.TISE_ERR_UNSUPPORTED, kw


def test_argument_validation_without_a_gpu():
    """Fake device addresses; every call has exactly one defect and must come back with its code before any HIP call (a launch
    would need a device this test does not have)."""
    from tise_toolbox_amd import _lib
    lib = _lib.load()
    bad, unsupported = _lib.TISE_ERR_INVALID_ARG, _lib.TISE_ERR_UNSUPPORTED
    T, T2, O, W = (0x7f0000000000 + i * 0x10000000 for i in range(4))       # 16-byte aligned

    def ssim(t=T, n=5, h=256, w=256, f32=0, out=O, ws=W, ws_bytes=1 << 40):
        return lib.tise_ssim_pairs(t, n, h, w, f32, out, ws, ws_bytes, None)
    need = 48 * 5 * 16
    for kw in (dict(t=None), dict(out=None), dict(ws=None), dict(n=-1), dict(h=10), dict(w=10), dict(h=0), dict(w=-3),
               dict(f32=2), dict(f32=-1), dict(t=T + 4), dict(out=O + 4), dict(ws=W + 4), dict(ws=W + 1),
               dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(n=6, ws_bytes=need)):
        assert ssim(**kw) == bad, kw
    for kw in (dict(h=MAX_SIDE + 1), dict(w=MAX_SIDE + 1), dict(n=MAX_PAIRS + 1), dict(n=65, h=MAX_SIDE, w=MAX_SIDE)):
        assert ssim(**kw) == unsupported, kw
    assert ssim(n=0) == _lib.TISE_OK and ssim(n=0, ws_bytes=0) == _lib.TISE_OK                 # nothing to do: no HIP call

    def sse(t=T, n=5, h=256, w=256, out=O):
        return lib.tise_pair_sse_u8(t, n, h, w, out, None)
    for kw in (dict(t=None), dict(out=None), dict(n=-1), dict(h=0), dict(w=0), dict(h=-1), dict(t=T + 4), dict(out=O + 4)):
        assert sse(**kw) == bad, kw
    for kw in (dict(h=MAX_SIDE + 1), dict(w=MAX_SIDE + 1), dict(n=MAX_PAIRS + 1)):
        assert sse(**kw) == unsupported, kw
    assert sse(n=0) == _lib.TISE_OK

    def pool(t=T, o=T2, n=5, h=256, w=256, f32=1):
        return lib.tise_pool2x2_pairs(t, o, n, h, w, f32, None)
    for kw in (dict(t=None), dict(o=None), dict(n=-1), dict(h=1), dict(w=1), dict(h=0), dict(f32=2), dict(f32=-1), dict(t=T + 4),
               dict(o=T2 + 2)):
        assert pool(**kw) == bad, kw
    for kw in (dict(h=MAX_SIDE + 1), dict(w=MAX_SIDE + 1), dict(n=MAX_PAIRS + 1)):
        assert pool(**kw) == unsupported, kw
    assert pool(n=0) == _lib.TISE_OK
