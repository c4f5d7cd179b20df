"""CPU: libtise_hip.so loads and exports exactly what include/tise_hip.h declares (no compute calls)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "tise_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(tise_[a-z0-9_]+)\s*\(", text)))


def test_header_and_binding_table_agree():
    from tise_toolbox_amd import _lib
    declared = _declared_symbols()
    assert len(declared) >= 20
    assert sorted(_lib.SIGNATURES) == declared, "tise_toolbox_amd/_lib.py SIGNATURES must mirror include/tise_hip.h"


def test_library_loads_and_exports_every_symbol():
    from tise_toolbox_amd import _lib, build
    build.build(force=False, verbose=False)            # hipcc cross-compiles gfx950 without a GPU
    lib = _lib.load()
    for name in _declared_symbols():
        assert hasattr(lib, name), name
    assert lib.tise_version() == 1
    assert lib.tise_status_string(0) == b"ok"
    assert lib.tise_status_string(-1) == b"invalid argument"
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in _declared_symbols():
        getattr(raw, name)


def test_argument_validation_without_a_gpu():
    """Entry points reject bad arguments before touching the device."""
    from tise_toolbox_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.tise_stats_create(0, ctypes.byref(h)) == _lib.TISE_ERR_INVALID_ARG
    assert lib.tise_frechet_create(-3, ctypes.byref(h)) == _lib.TISE_ERR_INVALID_ARG
    r, unpivoted = ctypes.c_int(), ctypes.c_int()
    assert lib.tise_frechet_factor(None, 0x7f0000000000, ctypes.byref(r), ctypes.byref(unpivoted), None) == _lib.TISE_ERR_INVALID_ARG
    assert lib.tise_stats_update(None, None, 4, 4, None) == _lib.TISE_ERR_INVALID_ARG
    assert lib.tise_is_finalize(None, 10, 10, 10, 0, None, None) == _lib.TISE_ERR_INVALID_ARG
    assert lib.tise_is_update(None, 4, 8, 8, 0.0, 0, 0, 4, 10, 0, None, None, None) == _lib.TISE_ERR_INVALID_ARG
    lut = (ctypes.c_float * 768)()
    assert lib.tise_resize_bilinear_u8(None, 1, 0, 5, None, 299, 299, 1, lut, None, None) == _lib.TISE_ERR_INVALID_ARG


def test_clip_entries_reject_strides_and_misalignment_without_a_gpu():
    """The CLIP tower entries (csrc/clip_ops.hip) refuse leading dimensions shorter than a row and pointers the kernels'
    16-byte (8-byte: gemm bias) accesses cannot take, before any HIP call: fake device addresses, every call has exactly
    one defect, and each must come back TISE_ERR_INVALID_ARG (a launch would need a device this test does not have)."""
    from tise_toolbox_amd import _lib
    lib = _lib.load()
    bad = _lib.TISE_ERR_INVALID_ARG
    A, W, B, R, O = 0x7f0000000000, 0x7f0000100000, 0x7f0000200000, 0x7f0000300000, 0x7f0000400000   # 16-byte aligned
    m, n, k = 128, 256, 192

    def gemm(a=A, lda=k, w=W, ldw=k, bias=B, res=R, ldr=n, out=O, ldo=n, mm=m, act=0):
        return lib.tise_gemm_f16(a, lda, w, ldw, bias, res, ldr, out, ldo, mm, n, k, act, None)
    assert gemm(mm=0) == _lib.TISE_OK                                 # M = 0: nothing to do, no launch
    assert gemm(mm=0, lda=k - 8) == bad                               # arguments are checked before the M = 0 exit
    for kw in (dict(lda=k - 8), dict(lda=8), dict(ldw=k - 8), dict(ldo=n - 8), dict(ldr=n - 8), dict(ldr=0),
               dict(a=A + 8), dict(a=A + 2), dict(w=W + 8), dict(out=O + 8), dict(res=R + 8), dict(bias=B + 4),
               dict(bias=B + 2), dict(act=2)):
        assert gemm(**kw) == bad, kw
    assert gemm(res=None, ldr=0, mm=0) == _lib.TISE_OK                # no residual: ldr is not read
    assert gemm(bias=B + 8, mm=0) == _lib.TISE_OK                     # 8-byte aligned bias is enough

    def ln(x=A, ldx=520, out=O, ldo=520, rows=4, c=520, g=W, b=B):
        return lib.tise_layernorm_f16(x, ldx, g, b, out, ldo, rows, c, ctypes.c_float(1e-5), None)
    assert ln(rows=0) == _lib.TISE_OK
    for kw in (dict(ldx=512), dict(ldo=512), dict(ldx=8), dict(x=A + 8), dict(out=O + 8), dict(g=W + 8), dict(b=B + 8),
               dict(c=1032, ldx=1032, ldo=1032), dict(c=12, ldx=16, ldo=16)):
        assert ln(**kw) == bad, kw

    def attn(qkv=A, out=O, batch=2, seq=77, heads=8, hd=64):
        return lib.tise_attention_f16(qkv, batch, seq, heads, hd, 1, out, None)
    assert attn(batch=0) == _lib.TISE_OK
    for kw in (dict(qkv=A + 8), dict(qkv=A + 2), dict(out=O + 8), dict(seq=97), dict(seq=0), dict(hd=32), dict(hd=128)):
        assert attn(**kw) == bad, kw

    def patchify(img=A, out=O, batch=2, res=224, patch=32):
        return lib.tise_patchify_f16(img, batch, res, patch, out, None)
    assert patchify(batch=0) == _lib.TISE_OK
    for kw in (dict(img=A + 8), dict(out=O + 8), dict(out=O + 2), dict(patch=12, res=48), dict(res=230)):
        assert patchify(**kw) == bad, kw


def test_product_refuses_to_run_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import numpy as np
    from tise_toolbox_amd import _lib, fid_score, inception_score
    with pytest.raises(_lib.TiseLibraryError):
        fid_score.calculate_frechet_distance(np.zeros(2), np.eye(2), np.zeros(2), np.eye(2))
    with pytest.raises(_lib.TiseLibraryError):
        inception_score.inception_score_from_logits(np.zeros((4, 3), np.float32))
    with pytest.raises(_lib.TiseLibraryError):
        fid_score.get_activations([], None, cuda=False)


def test_product_never_imports_the_oracle():
    """The product package must not route through oracle/ (or any CPU fallback)."""
    pkg = os.path.join(ROOT, "tise_toolbox_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M), f
                assert "from tests" not in text, f


def test_png_library_exports_its_header():
    """libtise_png.so (gcc, csrc/png_decode.c): every symbol include/tise_png.h declares, bound as _png_worker binds them."""
    from tise_toolbox_amd import _png_worker, build
    build.build_png(force=False, verbose=False)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tise_png.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(tise_png_[a-z0-9_]+)\s*\(", text)))
    assert declared == ["tise_png_decode_rgb8", "tise_png_inflate_backend", "tise_png_inflate_slot", "tise_png_probe",
                        "tise_png_scratch_bytes", "tise_png_slot_bytes"]
    raw = ctypes.CDLL(build.PNG_LIB)
    for name in declared:
        getattr(raw, name)
    lib = _png_worker.load_decoder()
    assert lib is not None and lib.tise_png_inflate_backend() in (0, 1)
