"""CPU: the entry points of the nearest-row search (csrc/knn.hip) are declared, bound and exported, reject bad arguments before
touching the device, and size their workspace by the documented formula (the sibling of tests/test_cabi_symbols_openclip.py)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tise_nn_workspace_bytes", "tise_nn_argmin")


def test_declared_bound_and_exported():
    from tise_toolbox_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tise_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tise_[a-z0-9_]+)\s*\(", text))
    build.build(force=False, verbose=False)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in declared and name in _lib.SIGNATURES
        getattr(raw, name)
    assert len(_lib.SIGNATURES["tise_nn_workspace_bytes"][1]) == 4 and len(_lib.SIGNATURES["tise_nn_argmin"][1]) == 14
    assert len(_lib.SIGNATURES["tise_knn_radius2"][1]) == 10 and len(_lib.SIGNATURES["tise_prdc_counts"][1]) == 16      # the parents stay


def _splits(rows_q, rows_b, col_splits):
    """The header's rule: the caller's value or ceil(1024 / query row tiles), capped at the base row tiles and at 1024."""
    tq, tb = (rows_q + 63) // 64, (rows_b + 63) // 64
    s = col_splits if col_splits > 0 else (1024 + tq - 1) // tq
    return max(1, min(s, tb, 1024))


def test_workspace_formula():
    from tise_toolbox_amd import _lib
    lib = _lib.load()
    for rows_q, rows_b, cs in ((1, 1, 0), (300, 260, 0), (300, 260, 2), (300, 260, 7), (64, 65, 1), (6, 700, 0), (700, 6, 3), (50000, 50000, 0),
                               (1 << 24, 1 << 24, 0), (1 << 24, 1, 1024), (100000, 70000, 1024)):
        nb = ctypes.c_size_t(0)
        assert lib.tise_nn_workspace_bytes(rows_q, rows_b, cs, ctypes.byref(nb)) == _lib.TISE_OK
        assert nb.value == 8 * (rows_q + rows_b) + 12 * rows_q * _splits(rows_q, rows_b, cs), (rows_q, rows_b, cs)
    nb = ctypes.c_size_t(0)
    for kw in ((0, 5, 0), (5, 0, 0), (-1, 5, 0), (5, 5, -1), (5, 5, 1025)):
        assert lib.tise_nn_workspace_bytes(*kw, ctypes.byref(nb)) == _lib.TISE_ERR_INVALID_ARG, kw
    assert lib.tise_nn_workspace_bytes(5, 5, 0, None) == _lib.TISE_ERR_INVALID_ARG
    assert lib.tise_nn_workspace_bytes((1 << 24) + 1, 5, 0, ctypes.byref(nb)) == _lib.TISE_ERR_UNSUPPORTED
    assert lib.tise_nn_workspace_bytes(5, (1 << 24) + 1, 0, ctypes.byref(nb)) == _lib.TISE_ERR_UNSUPPORTED


def test_argument_validation_without_a_gpu():
    """Fake device addresses; every call has exactly one defect and must come back with its code before any HIP call (a launch
    would need a device this test does not have)."""
    from tise_toolbox_amd import _lib
    lib = _lib.load()
    bad, unsupported = _lib.TISE_ERR_INVALID_ARG, _lib.TISE_ERR_UNSUPPORTED
    Q, B, D, I, W = (0x7f0000000000 + i * 0x10000000 for i in range(5))       # 16-byte aligned

    def need(rows_q, rows_b, cs):
        nb = ctypes.c_size_t(0)
        assert lib.tise_nn_workspace_bytes(rows_q, rows_b, cs, ctypes.byref(nb)) == _lib.TISE_OK
        return nb.value

    def nn(q=Q, rows_q=100, ld_q=64, b=B, rows_b=100, ld_b=64, d=64, ex=0, cs=0, d2=D, idx=I, ws=W, ws_bytes=None):
        if ws_bytes is None:
            ws_bytes = 1 << 40
        return lib.tise_nn_argmin(q, rows_q, ld_q, b, rows_b, ld_b, d, ex, cs, d2, idx, ws, ws_bytes, None)
    for kw in (dict(q=None), dict(b=None), dict(d2=None), dict(idx=None), dict(ws=None),
               dict(rows_q=0), dict(rows_b=0), dict(rows_q=-3), dict(rows_b=-1),
               dict(d=0), dict(d=-4),
               dict(ld_q=60), dict(ld_b=60), dict(ld_q=66), dict(ld_b=70), dict(d=62, ld_q=62),
               dict(q=Q + 4), dict(q=Q + 8), dict(b=B + 4), dict(b=B + 8),
               dict(cs=-1), dict(cs=1025),
               dict(ex=2), dict(ex=-1), dict(ex=1, rows_b=101), dict(ex=1, rows_q=99),
               dict(d2=D + 4), dict(idx=I + 2), dict(ws=W + 4),
               dict(ws_bytes=need(100, 100, 0) - 1), dict(ws_bytes=0), dict(cs=2, ws_bytes=need(100, 100, 1))):
        assert nn(**kw) == bad, kw
    assert nn(rows_q=(1 << 24) + 1) == unsupported and nn(rows_b=(1 << 24) + 1) == unsupported
    assert nn(ex=1, rows_q=(1 << 24) + 1, rows_b=(1 << 24) + 1) == unsupported
