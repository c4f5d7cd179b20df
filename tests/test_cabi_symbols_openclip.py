"""CPU: the entry points CLIPScore and the open_clip tower add (csrc/clip_ops.hip) are declared, bound and exported, and reject
bad arguments before touching the device (the sibling of tests/test_cabi_symbols_dinov2.py)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tise_layernorm_wide_f16", "tise_paired_cosine")


def test_declared_bound_and_exported():
    from tise_toolbox_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tise_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tise_[a-z0-9_]+)\s*\(", text))
    build.build(force=False, verbose=False)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in declared and name in _lib.SIGNATURES
        getattr(raw, name)
    assert _lib.SIGNATURES["tise_layernorm_wide_f16"] == _lib.SIGNATURES["tise_layernorm_f16"]
    assert len(_lib.SIGNATURES["tise_paired_cosine"][1]) == 7
    assert len(_lib.SIGNATURES["tise_attention_long_f16"][1]) == 7          # the signature stays


def test_argument_validation_without_a_gpu():
    """Fake device addresses, every call has exactly one defect and must come back TISE_ERR_INVALID_ARG before any HIP call (a
    launch would need a device this test does not have); rows = 0 / n = 0 / batch = 0 return TISE_OK after the checks."""
    from tise_toolbox_amd import _lib
    lib = _lib.load()
    bad, ok = _lib.TISE_ERR_INVALID_ARG, _lib.TISE_OK
    A, W, B, O = (0x7f0000000000 + i * 0x100000 for i in range(4))           # 16-byte aligned

    def ln(x=A, ldx=1280, out=O, ldo=1280, rows=0, c=1280, g=W, b=B, fn=lib.tise_layernorm_wide_f16):
        return fn(x, ldx, g, b, out, ldo, rows, c, ctypes.c_float(1e-5), None)
    assert ln() == ok and ln(c=2048, ldx=2048, ldo=2048) == ok and ln(c=8, ldx=16, ldo=24) == ok and ln(c=1032, ldx=1032, ldo=1040) == ok
    for kw in (dict(c=2056, ldx=2056, ldo=2056), dict(c=12, ldx=16, ldo=16), dict(c=0), dict(c=-8), dict(ldx=1272), dict(ldo=1272),
               dict(ldx=1284), dict(ldo=1284), dict(x=A + 8), dict(x=A + 2), dict(out=O + 8), dict(g=W + 8), dict(b=B + 8),
               dict(x=None), dict(out=None), dict(g=None), dict(b=None), dict(rows=-1)):
        assert ln(**kw) == bad, kw
    # the narrow entry is what it was
    assert ln(c=1024, ldx=1024, ldo=1024, fn=lib.tise_layernorm_f16) == ok
    assert ln(fn=lib.tise_layernorm_f16) == bad and ln(c=1032, ldx=1032, ldo=1032, fn=lib.tise_layernorm_f16) == bad

    def cos(a=A, b=B, n=0, d=512, f16=1, out=O):
        return lib.tise_paired_cosine(a, b, n, d, f16, out, None)
    assert cos() == ok and cos(f16=0) == ok and cos(d=1) == ok and cos(a=A + 2, b=B + 6) == ok and cos(f16=0, a=A + 4) == ok
    for kw in (dict(a=None), dict(b=None), dict(out=None), dict(n=-1), dict(d=0), dict(d=-4), dict(f16=2), dict(f16=-1), dict(a=A + 1),
               dict(b=B + 1), dict(f16=0, a=A + 2), dict(f16=0, b=B + 2), dict(out=O + 4)):
        assert cos(**kw) == bad, kw

    def att(q=A, batch=0, seq=257, heads=16, hd=80, out=O):
        return lib.tise_attention_long_f16(q, batch, seq, heads, hd, out, None)
    assert att() == ok and att(hd=64) == ok
    for kw in (dict(hd=72), dict(hd=96), dict(hd=32), dict(hd=128), dict(hd=0), dict(q=A + 8), dict(out=O + 8), dict(seq=0), dict(heads=0),
               dict(batch=-1), dict(q=None), dict(out=None)):
        assert att(**kw) == bad, kw
    assert lib.tise_attention_f16(A, 0, 77, 16, 80, 1, O, None) == bad        # the short / causal kernel stays at 64
