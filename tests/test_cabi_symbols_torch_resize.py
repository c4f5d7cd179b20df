"""CPU: the entry points of pytorch-fid's input route (csrc/resize_torch.hip) are declared, bound and exported, and reject bad
arguments before touching the device (the sibling of tests/test_cabi_symbols_adm.py)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tise_resize_torch_f32", "tise_resize_ragged_torch_f32")


def test_declared_bound_and_exported():
    from tise_toolbox_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tise_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tise_[a-z0-9_]+)\s*\(", text))
    assert "resize_torch.hip" in build.SOURCES
    build.build(force=False, verbose=False)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in declared and name in _lib.SIGNATURES
        getattr(raw, name)
    assert len(_lib.SIGNATURES["tise_resize_torch_f32"][1]) == 10
    assert len(_lib.SIGNATURES["tise_resize_ragged_torch_f32"][1]) == 8
    # the table entry the ragged launch reads: { const uint8_t* src; int32_t h, w; } = 16 bytes, what device.py builds
    assert re.search(r"typedef struct tise_torch_image \{\s*const uint8_t\* src;\s*int32_t h, w;\s*\} tise_torch_image_t;", text)
    from tise_toolbox_amd import device
    assert device._TORCH_IMAGE.itemsize == 16 and device._TORCH_IMAGE.names == ("src", "h", "w")
    assert [device._TORCH_IMAGE.fields[k][1] for k in ("src", "h", "w")] == [0, 8, 12]


def test_argument_validation_without_a_gpu():
    from tise_toolbox_amd import _lib
    lib = _lib.load()
    bad, ok, unsupported = _lib.TISE_ERR_INVALID_ARG, _lib.TISE_OK, _lib.TISE_ERR_UNSUPPORTED
    S, D = 0x7f0000000000, 0x7f0000100000                      # fake device addresses: every call below returns before a launch

    def plain(src=S, n=1, h=8, w=8, dst=D, oh=4, ow=4, mul=2.0, sub=1.0):
        return lib.tise_resize_torch_f32(src, n, h, w, dst, oh, ow, mul, sub, None)
    assert plain(n=0) == ok                                     # nothing to do, no launch
    for kw in (dict(n=-1), dict(h=0), dict(w=0), dict(h=-2), dict(w=-1), dict(oh=0), dict(ow=-3), dict(src=None), dict(dst=None),
               dict(mul=float("nan")), dict(mul=float("inf")), dict(sub=float("nan")), dict(sub=float("-inf"))):
        assert plain(**kw) == bad, kw
    assert plain(n=0, oh=0) == bad                              # arguments are checked before the n = 0 exit
    assert plain(n=0, src=None) == bad
    assert plain(oh=1 << 16, ow=1 << 15) == unsupported         # oh * ow = 2^31: the index inside an image is 32-bit

    def ragged(table=S, n=1, dst=D, oh=4, ow=4, mul=2.0, sub=1.0):
        return lib.tise_resize_ragged_torch_f32(table, n, dst, oh, ow, mul, sub, None)
    assert ragged(n=0) == ok
    for kw in (dict(n=-1), dict(oh=0), dict(ow=0), dict(oh=-1), dict(table=None), dict(dst=None), dict(mul=float("nan")),
               dict(mul=float("inf")), dict(sub=float("nan")), dict(sub=float("inf"))):
        assert ragged(**kw) == bad, kw
    assert ragged(n=0, ow=0) == bad
    assert ragged(n=0, table=None) == bad
    assert ragged(oh=1 << 16, ow=1 << 15) == unsupported
