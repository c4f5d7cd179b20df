"""CPU: the entry point of the CountSeg head (csrc/countseg.hip) is declared, bound and exported, and rejects bad arguments -- the
limit of 1024 pixels per map among them -- before touching the device (the sibling of tests/test_cabi_symbols_dists.py)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "tise_countseg_head"
MAX_PIXELS, MAX_WIDTH, MAX_CLASSES, MAX_IMAGES, GROUP = 1024, 1024, 4096, 65535, 4


def test_declared_bound_and_exported():
    from tise_toolbox_amd import _lib, build, device
    raw_text = open(os.path.join(ROOT, "include", "tise_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw_text, flags=re.S)
    declared = set(re.findall(r"\b(tise_[a-z0-9_]+)\s*\(", text))
    assert "countseg.hip" in build.SOURCES
    build.build(force=False, verbose=False)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert NAME in declared and NAME in _lib.SIGNATURES
    getattr(raw, NAME)
    assert len(_lib.SIGNATURES[NAME][1]) == 18
    macros = dict(re.findall(r"#define (TISE_COUNTSEG_[A-Z_]+) (\d+)", raw_text))
    assert {k: int(v) for k, v in macros.items()} == {"TISE_COUNTSEG_MAX_PIXELS": MAX_PIXELS, "TISE_COUNTSEG_MAX_WIDTH": MAX_WIDTH,
                                                       "TISE_COUNTSEG_MAX_CLASSES": MAX_CLASSES, "TISE_COUNTSEG_MAX_IMAGES": MAX_IMAGES,
                                                       "TISE_COUNTSEG_CLASS_GROUP": GROUP}
    assert (device.COUNTSEG_MAX_PIXELS, device.COUNTSEG_MAX_WIDTH, device.COUNTSEG_MAX_CLASSES, device.COUNTSEG_MAX_IMAGES,
            device.COUNTSEG_CLASS_GROUP) == (MAX_PIXELS, MAX_WIDTH, MAX_CLASSES, MAX_IMAGES, GROUP)


def test_argument_validation_without_a_gpu():
    """Fake device addresses; every call has exactly one defect and must come back with its code before any HIP call (a launch
    would need a device this test does not have)."""
    from tise_toolbox_amd import _lib
    lib = _lib.load()
    bad, unsupported = _lib.TISE_ERR_INVALID_ARG, _lib.TISE_ERR_UNSUPPORTED
    X, BM, WC, BC, WD, BD, CF, DN, PK, MP = (0x7f0000000000 + i * 0x10000000 for i in range(10))      # 16-byte aligned

    def head(mix=X, ld=240, off=0, b_mix=BM, w_cls=WC, b_cls=BC, w_den=WD, b_den=BD, n=0, h=14, w=14, P=120, C=80, conf=CF, den=DN,
             peaks=PK, maps=MP):
        return lib.tise_countseg_head(mix, ld, off, b_mix, w_cls, b_cls, w_den, b_den, n, h, w, P, C, conf, den, peaks, maps, None)
    assert head() == _lib.TISE_OK and head(maps=None) == _lib.TISE_OK                    # n == 0: nothing to do, no HIP call
    assert head(h=32, w=32) == _lib.TISE_OK and head(h=1, w=1024) == _lib.TISE_OK and head(h=1, w=1) == _lib.TISE_OK
    assert head(ld=256, off=16) == _lib.TISE_OK and head(P=8, C=1, ld=16) == _lib.TISE_OK
    assert head(n=MAX_IMAGES + 1) == unsupported                                         # (checked before n == 0 returns)
    for kw in (dict(mix=None), dict(b_mix=None), dict(w_cls=None), dict(b_cls=None), dict(w_den=None), dict(b_den=None), dict(conf=None),
               dict(den=None), dict(peaks=None), dict(n=-1), dict(h=0), dict(w=0), dict(h=-3), dict(P=0), dict(P=2), dict(P=122),
               dict(P=-4), dict(C=0), dict(C=-1), dict(off=-4), dict(off=2), dict(ld=242), dict(ld=0), dict(ld=236), dict(ld=256, off=20),
               dict(ld=1 << 32), dict(mix=X + 4), dict(mix=X + 8), dict(b_mix=BM + 2), dict(w_cls=WC + 1), dict(b_cls=BC + 2),
               dict(w_den=WD + 2), dict(b_den=BD + 1), dict(conf=CF + 4), dict(den=DN + 4), dict(peaks=PK + 2), dict(maps=MP + 4)):
        assert head(**kw) == bad, kw
        if "n" not in kw:
            assert head(n=3, **kw) == bad, kw
    for kw in (dict(h=33, w=32), dict(h=1, w=1025), dict(h=1025, w=1), dict(h=16384, w=16384), dict(P=MAX_WIDTH + 4, ld=4096),
               dict(C=MAX_CLASSES + 1), dict(n=MAX_IMAGES + 1)):
        assert head(n=kw.pop("n", 3), **kw) == unsupported, kw
