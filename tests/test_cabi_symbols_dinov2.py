"""CPU: the entry points of the DINOv2 tower's fp32 residual stream (csrc/clip_ops.hip) are declared, bound and exported, and
reject bad arguments before touching the device (the sibling of tests/test_cabi_symbols_adm.py)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tise_gemm_f16_act", "tise_gemm_f16_res32", "tise_layernorm_f32", "tise_vit_tokens_f32", "tise_gather_rows_f32")


def test_declared_bound_and_exported():
    from tise_toolbox_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tise_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tise_[a-z0-9_]+)\s*\(", text))
    build.build(force=False, verbose=False)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in declared and name in _lib.SIGNATURES
        getattr(raw, name)
    assert len(_lib.SIGNATURES["tise_gemm_f16_res32"][1]) == 14
    assert _lib.SIGNATURES["tise_gemm_f16_act"] == _lib.SIGNATURES["tise_gemm_f16"]
    assert len(_lib.SIGNATURES["tise_layernorm_f32"][1]) == 11
    assert len(_lib.SIGNATURES["tise_vit_tokens_f32"][1]) == 8
    assert len(_lib.SIGNATURES["tise_gather_rows_f32"][1]) == 6


def test_argument_validation_without_a_gpu():
    """Fake device addresses, every call has exactly one defect and must come back TISE_ERR_INVALID_ARG before any HIP call (a
    launch would need a device this test does not have)."""
    from tise_toolbox_amd import _lib
    lib = _lib.load()
    bad, ok = _lib.TISE_ERR_INVALID_ARG, _lib.TISE_OK
    A, W, B, S, R, O = (0x7f0000000000 + i * 0x100000 for i in range(6))      # 16-byte aligned
    m, n, k = 128, 256, 192

    def res32(a=A, lda=k, w=W, ldw=k, bias=B, scale=S, res=R, ldr=n, out=O, ldo=n, mm=m, nn=n, kk=k):
        return lib.tise_gemm_f16_res32(a, lda, w, ldw, bias, scale, res, ldr, out, ldo, mm, nn, kk, None)
    assert res32(mm=0) == ok                                            # M = 0: nothing to do, no launch
    assert res32(mm=0, bias=None, scale=None) == ok                     # both are optional
    assert res32(mm=0, out=R) == ok                                     # in place
    assert res32(mm=0, bias=B + 8) == ok                                # an 8-byte aligned bias is enough
    assert res32(mm=0, ldr=n + 4, ldo=n + 12) == ok                     # fp32 rows: strides in steps of four elements
    assert res32(mm=0, lda=k - 8) == bad                                # arguments are checked before the M = 0 exit
    for kw in (dict(a=A + 8), dict(a=A + 2), dict(w=W + 8), dict(res=R + 8), dict(res=R + 4), dict(out=O + 8), dict(out=O + 4),
               dict(scale=S + 8), dict(scale=S + 4), dict(bias=B + 4), dict(bias=B + 2),
               dict(kk=200, lda=200, ldw=200), dict(kk=32, lda=64, ldw=64), dict(kk=0), dict(nn=252), dict(nn=4), dict(nn=0),
               dict(lda=k - 8), dict(ldw=k - 8), dict(lda=k + 4), dict(ldr=n - 4), dict(ldo=n - 4), dict(ldr=n + 2), dict(ldo=n + 2),
               dict(ldr=0), dict(res=None), dict(out=None), dict(a=None), dict(w=None), dict(mm=-1)):
        assert res32(**kw) == bad, kw

    def gemm_act(a=A, lda=k, w=W, ldw=k, bias=B, res=R, ldr=n, out=O, ldo=n, mm=0, act=2, fn=lib.tise_gemm_f16_act):
        return fn(a, lda, w, ldw, bias, res, ldr, out, ldo, mm, n, k, act, None)
    assert [gemm_act(act=a) for a in (0, 1, 2)] == [ok, ok, ok]         # 2: exact GELU
    for kw in (dict(act=3), dict(act=-1), dict(lda=k - 8), dict(ldw=k - 8), dict(ldo=n - 8), dict(ldr=n - 8), dict(a=A + 8),
               dict(w=W + 8), dict(out=O + 8), dict(res=R + 8), dict(bias=B + 4)):
        assert gemm_act(**kw) == bad, kw                                # tise_gemm_f16's refusals
    # tise_gemm_f16 itself is what it was: act 0 and 1
    assert [gemm_act(act=a, fn=lib.tise_gemm_f16) for a in (0, 1, 2, 3)] == [ok, ok, bad, bad]

    def ln(x=A, ldx=1024, out=O, ldo=1024, rows=4, c=1024, g=W, b=B, f32=0):
        return lib.tise_layernorm_f32(x, ldx, g, b, out, ldo, rows, c, ctypes.c_float(1e-6), f32, None)
    assert ln(rows=0) == ok and ln(rows=0, f32=1) == ok
    assert ln(rows=0, c=8, ldx=12, ldo=16) == ok and ln(rows=0, c=8, ldx=12, ldo=12, f32=1) == ok
    for kw in (dict(c=1032, ldx=1032, ldo=1032), dict(c=2048, ldx=2048, ldo=2048), dict(c=12, ldx=16, ldo=16), dict(c=0),
               dict(ldx=1016), dict(ldo=1016), dict(ldx=1026), dict(c=8, ldx=8, ldo=12), dict(c=8, ldx=8, ldo=10, f32=1),
               dict(x=A + 8), dict(x=A + 4), dict(out=O + 8), dict(g=W + 8), dict(b=B + 4), dict(x=None), dict(out=None),
               dict(g=None), dict(b=None), dict(rows=-1), dict(f32=2)):
        assert ln(**kw) == bad, kw
    assert ln(rows=0, ldx=1016) == bad

    def tok(p=A, cls=W, pos=B, batch=2, npatch=256, width=1024, x=O):
        return lib.tise_vit_tokens_f32(p, cls, pos, batch, npatch, width, x, None)
    assert tok(batch=0) == ok
    for kw in (dict(p=None), dict(cls=None), dict(pos=None), dict(x=None), dict(batch=-1), dict(npatch=0), dict(width=0),
               dict(p=A + 1), dict(cls=W + 2), dict(pos=B + 1), dict(x=O + 2)):
        assert tok(**kw) == bad, kw

    def gather(x=A, idx=W, cnt=4, width=1024, out=O):
        return lib.tise_gather_rows_f32(x, idx, cnt, width, out, None)
    assert gather(cnt=0) == ok
    for kw in (dict(x=None), dict(idx=None), dict(out=None), dict(cnt=-1), dict(width=0), dict(x=A + 2), dict(out=O + 1), dict(idx=W + 4)):
        assert gather(**kw) == bad, kw
