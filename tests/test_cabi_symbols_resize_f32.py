"""CPU: the float32 resize entry points (csrc/resize_f32.hip) are declared, bound and exported, and reject bad arguments
before touching the device (the sibling of tests/test_cabi_symbols.py for tise_resize_f32 / tise_resize_ragged_f32)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tise_resize_f32", "tise_resize_ragged_f32")


def test_declared_bound_and_exported():
    from tise_toolbox_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tise_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tise_[a-z0-9_]+)\s*\(", text))
    build.build(force=False, verbose=False)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in declared and name in _lib.SIGNATURES
        getattr(raw, name)
    assert len(_lib.SIGNATURES["tise_resize_f32"][1]) == 15
    assert len(_lib.SIGNATURES["tise_resize_ragged_f32"][1]) == 19


def test_argument_validation_without_a_gpu():
    from tise_toolbox_amd import _lib
    lib = _lib.load()
    bad, ok = _lib.TISE_ERR_INVALID_ARG, _lib.TISE_OK
    S, D = 0x7f0000000000, 0x7f0000100000                      # fake device addresses: every call below returns before a launch

    def f32(src=S, n=1, h=8, w=8, dst=D, oh=4, ow=4, nhwc=1, filt=1, lo=0.0, hi=255.0, sub=128.0, div=128.0, order=0):
        return lib.tise_resize_f32(src, n, h, w, dst, oh, ow, nhwc, filt, lo, hi, sub, div, order, None)
    assert f32(n=0) == ok                                       # nothing to do, no launch
    for kw in (dict(n=-1), dict(h=0), dict(w=0), dict(oh=0), dict(ow=-3), dict(src=None), dict(dst=None), dict(filt=2), dict(filt=-1),
               dict(order=2), dict(order=-1), dict(lo=1.0, hi=0.0), dict(lo=float("nan")), dict(hi=float("nan")), dict(div=0.0),
               dict(div=float("inf")), dict(sub=float("nan"))):
        assert f32(**kw) == bad, kw
    assert f32(n=0, filt=2) == bad                              # arguments are checked before the n = 0 exit
    assert f32(n=65536) == _lib.TISE_ERR_UNSUPPORTED

    ptrs = (ctypes.c_uint64 * 2)(S, S + 4096)
    hs, ws, orders = (ctypes.c_int32 * 2)(8, 9), (ctypes.c_int32 * 2)(8, 7), (ctypes.c_int32 * 2)(0, 0)
    W = 0x7f0000200000
    need = 2 * (64 + 4 * 4) + 16
    idx = ctypes.c_int64(7)

    def ragged(p=ptrs, h=hs, w=ws, o=orders, n=2, dst=D, oh=4, ow=4, filt=1, lo=0.0, hi=255.0, div=128.0, wsp=W, wsb=need, pin=None):
        return lib.tise_resize_ragged_f32(ctypes.addressof(p) if p is not None else None, ctypes.addressof(h), ctypes.addressof(w),
                                          ctypes.addressof(o) if o is not None else None, n, dst, oh, ow, 1, filt, lo, hi, 128.0, div,
                                          wsp, wsb, pin, ctypes.byref(idx), None)
    assert ragged(n=0) == ok and idx.value == -1
    for kw in (dict(n=-1), dict(oh=0), dict(filt=3), dict(lo=2.0, hi=1.0), dict(div=0.0), dict(p=None), dict(o=None), dict(dst=None),
               dict(wsp=None), dict(wsp=W + 8), dict(wsb=need - 1), dict(pin=0x7f0000300008)):
        assert ragged(**kw) == bad, kw
    assert ragged(h=(ctypes.c_int32 * 2)(8, 0)) == bad and idx.value == 1          # names the image
    assert ragged(o=(ctypes.c_int32 * 2)(0, 2)) == bad and idx.value == 1
    assert ragged(p=(ctypes.c_uint64 * 2)(0, S)) == bad and idx.value == 0
    # a size of which not even one output row per workgroup fits LDS is refused before anything is enqueued
    assert ragged(w=(ctypes.c_int32 * 2)(8, 1 << 19)) == _lib.TISE_ERR_UNSUPPORTED and idx.value == 1
