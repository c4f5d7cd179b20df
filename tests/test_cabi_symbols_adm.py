"""CPU: the entry points of the ADM sample-batch suite (csrc/resize_tf1.hip, tise_split_tap_rows of csrc/trunk_ops.hip) are
declared, bound and exported, and reject bad arguments before touching the device (the sibling of
tests/test_cabi_symbols_resize_f32.py)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tise_resize_tf1_f32", "tise_split_tap_rows")


def test_declared_bound_and_exported():
    from tise_toolbox_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tise_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tise_[a-z0-9_]+)\s*\(", text))
    assert "resize_tf1.hip" in build.SOURCES
    build.build(force=False, verbose=False)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in declared and name in _lib.SIGNATURES
        getattr(raw, name)
    assert len(_lib.SIGNATURES["tise_resize_tf1_f32"][1]) == 10
    assert len(_lib.SIGNATURES["tise_split_tap_rows"][1]) == 9


def test_argument_validation_without_a_gpu():
    from tise_toolbox_amd import _lib
    lib = _lib.load()
    bad, ok = _lib.TISE_ERR_INVALID_ARG, _lib.TISE_OK
    S, D = 0x7f0000000000, 0x7f0000100000                      # fake device addresses: every call below returns before a launch

    def tf1(src=S, n=1, h=8, w=8, dst=D, oh=4, ow=4, sub=128.0, mul=2.0 ** -7):
        return lib.tise_resize_tf1_f32(src, n, h, w, dst, oh, ow, sub, mul, None)
    assert tf1(n=0) == ok                                       # nothing to do, no launch
    for kw in (dict(n=-1), dict(h=0), dict(w=0), dict(h=-2), dict(oh=0), dict(ow=-3), dict(src=None), dict(dst=None),
               dict(sub=float("nan")), dict(mul=float("inf"))):
        assert tf1(**kw) == bad, kw
    assert tf1(n=0, oh=0) == bad                                # arguments are checked before the n = 0 exit

    def tap(x=S, n=1, hw=289, C=768, c0=0, nc=7, out=D, ld=2048):
        return lib.tise_split_tap_rows(x, n, hw, C, c0, nc, out, ld, None)
    assert tap(n=0) == ok
    for kw in (dict(n=-1), dict(hw=0), dict(C=0), dict(C=24), dict(c0=-1), dict(nc=0), dict(c0=762), dict(c0=768, nc=1),
               dict(ld=2022), dict(x=None), dict(out=None), dict(c0=2 ** 31 - 4, nc=7)):
        assert tap(**kw) == bad, kw
    assert tap(n=0, ld=2022) == bad
