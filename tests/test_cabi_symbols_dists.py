"""CPU: the entry points of the DISTS kernels (csrc/dists.hip) are declared, bound and exported, reject bad arguments before
touching the device, and size their workspace by the documented formula (the sibling of tests/test_cabi_symbols_lpips.py)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tise_l2pool3s2_split_nhwc", "tise_dists_workspace_bytes", "tise_dists_layer", "tise_dists_image_sums_u8")
MAX_SIDE, MAX_PAIRS, WG, MAX_C, SUM_PIX = 16384, 32767, 512, 512, 4096


def test_declared_bound_and_exported():
    from tise_toolbox_amd import _lib, build, device
    raw_text = open(os.path.join(ROOT, "include", "tise_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw_text, flags=re.S)
    declared = set(re.findall(r"\b(tise_[a-z0-9_]+)\s*\(", text))
    assert "dists.hip" in build.SOURCES
    build.build(force=False, verbose=False)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in declared and name in _lib.SIGNATURES
        getattr(raw, name)
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [11, 5, 11, 6]
    assert _lib.SIGNATURES["tise_l2pool3s2_split_nhwc"] == _lib.SIGNATURES["tise_maxpool2s2_split_nhwc"]     # its siblings' arguments
    assert _lib.SIGNATURES["tise_l2pool3s2_split_nhwc"] == _lib.SIGNATURES["tise_maxpool3s2_split_nhwc"]
    macros = dict(re.findall(r"#define (TISE_DISTS_[A-Z_]+) (\d+)", raw_text))
    assert {k: int(v) for k, v in macros.items()} == {"TISE_DISTS_MAX_SIDE": MAX_SIDE, "TISE_DISTS_MAX_PAIRS": MAX_PAIRS,
                                                       "TISE_DISTS_WG_PIXELS": WG, "TISE_DISTS_MAX_CHANNELS": MAX_C,
                                                       "TISE_DISTS_SUM_PIXELS": SUM_PIX}
    assert (device.DISTS_MAX_SIDE, device.DISTS_MAX_PAIRS, device.DISTS_WG_PIXELS, device.DISTS_MAX_CHANNELS,
            device.DISTS_SUM_PIXELS) == (MAX_SIDE, MAX_PAIRS, WG, MAX_C, SUM_PIX)


def test_workspace_formula():
    """bytes = 8 n C (7 ceil(h w / 512) + 2)."""
    from tise_toolbox_amd import _lib
    lib = _lib.load()
    nb = ctypes.c_size_t(7)
    for n, h, w, c in ((1, 1, 1, 16), (1, 16, 16, 64), (1, 1, 513, 64), (3, 16, 33, 48), (50, 256, 256, 64), (0, 16, 16, 64),
                       (MAX_PAIRS, 35, 67, 512), (1, MAX_SIDE, MAX_SIDE, 64), (MAX_PAIRS, MAX_SIDE, MAX_SIDE, MAX_C)):
        assert lib.tise_dists_workspace_bytes(n, h, w, c, ctypes.byref(nb)) == _lib.TISE_OK, (n, h, w, c)
        assert nb.value == 8 * n * c * (7 * ((h * w + WG - 1) // WG) + 2), (n, h, w, c)
    for kw in ((-1, 16, 16, 64), (1, 0, 16, 64), (1, 16, 0, 64), (1, -3, 16, 64), (1, 16, 16, 0), (1, 16, 16, 8), (1, 16, 16, 24),
               (1, 16, 16, -16)):
        assert lib.tise_dists_workspace_bytes(*kw, ctypes.byref(nb)) == _lib.TISE_ERR_INVALID_ARG, kw
    assert lib.tise_dists_workspace_bytes(1, 16, 16, 64, None) == _lib.TISE_ERR_INVALID_ARG
    for kw in ((1, MAX_SIDE + 1, 16, 64), (1, 16, MAX_SIDE + 1, 64), (MAX_PAIRS + 1, 16, 16, 64), (1, 16, 16, MAX_C + 16)):
        assert lib.tise_dists_workspace_bytes(*kw, ctypes.byref(nb)) == _lib.TISE_ERR_UNSUPPORTED, kw


def test_argument_validation_without_a_gpu():
    """Fake device addresses; every call has exactly one defect and must come back with its code before any HIP call (a launch
    would need a device this test does not have)."""
    from tise_toolbox_amd import _lib
    lib = _lib.load()
    bad, unsupported = _lib.TISE_ERR_INVALID_ARG, _lib.TISE_ERR_UNSUPPORTED
    T, A, O, F, B, S = (0x7f0000000000 + i * 0x10000000 for i in range(6))       # 16-byte aligned

    def pool(x=F, x_ld=64, x_off=0, n=2, h=16, w=16, c=64, out=O, out_ld=64, out_off=0):
        return lib.tise_l2pool3s2_split_nhwc(x, x_ld, x_off, n, h, w, c, out, out_ld, out_off, None)
    for kw in (dict(x=None), dict(out=None), dict(n=-1), dict(h=0), dict(w=0), dict(h=-1), dict(c=0), dict(c=60), dict(c=-8), dict(x_ld=72),
               dict(out_ld=72), dict(x_off=4), dict(out_off=4), dict(x_off=8), dict(out_off=8), dict(c=72), dict(x_off=-8, c=8),
               dict(x=F + 8), dict(out=O + 2), dict(x_ld=1 << 32, c=64)):
        assert pool(**kw) == bad, kw
    assert pool(n=65536) == unsupported
    assert pool(n=0) == _lib.TISE_OK and pool(n=0, h=1, w=1) == _lib.TISE_OK                      # sides from 1 up
    assert pool(n=0, x_off=16, c=48, out_ld=96, out_off=48) == _lib.TISE_OK                       # a slice into a slice at an offset
    assert pool(n=0, x_off=24, c=48, out_ld=96, out_off=48) == bad                                # 24 + 48 > 64

    def layer(f=F, n=5, h=16, w=33, c=64, al=A, be=B, out=O, ws=S, ws_bytes=1 << 40):
        return lib.tise_dists_layer(f, n, h, w, c, al, be, out, ws, ws_bytes, None)
    need = 8 * 5 * 64 * (7 * 2 + 2)
    for kw in (dict(f=None), dict(al=None), dict(be=None), dict(out=None), dict(ws=None), dict(n=-1), dict(h=0), dict(w=0), dict(w=-1),
               dict(c=0), dict(c=8), dict(c=24), dict(c=72), dict(c=-16), dict(f=F + 8), dict(al=A + 4), dict(be=B + 4), dict(be=B + 1),
               dict(out=O + 4), dict(ws=S + 4), dict(ws=S + 1), dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(n=6, ws_bytes=need)):
        assert layer(**kw) == bad, kw
    for kw in (dict(h=MAX_SIDE + 1), dict(w=MAX_SIDE + 1), dict(n=MAX_PAIRS + 1), dict(c=MAX_C + 16), dict(c=1024)):
        assert layer(**kw) == unsupported, kw
    assert layer(n=0) == _lib.TISE_OK and layer(n=0, ws_bytes=0) == _lib.TISE_OK                 # nothing to do: no HIP call

    def sums(t=T, n=5, h=16, w=16, out=O):
        return lib.tise_dists_image_sums_u8(t, n, h, w, out, None)
    for kw in (dict(t=None), dict(out=None), dict(n=-1), dict(h=0), dict(w=0), dict(h=-2), dict(t=T + 4), dict(out=O + 4), dict(out=O + 2)):
        assert sums(**kw) == bad, kw
    for kw in (dict(h=MAX_SIDE + 1), dict(w=MAX_SIDE + 1), dict(n=MAX_PAIRS + 1)):
        assert sums(**kw) == unsupported, kw
    assert sums(n=0) == _lib.TISE_OK
