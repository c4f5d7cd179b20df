"""CPU: the entry points of the ResNet kernels (csrc/resnet.hip, the 7 x 7 stem of csrc/conv_pipe.hip) are declared, bound and
exported, and reject bad arguments before touching the device (the sibling of tests/test_cabi_symbols_lpips.py)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tise_stem_conv7x7s2_split_u8_mfma", "tise_residual_relu_split_nhwc", "tise_maxpool3s2p1_split_nhwc", "tise_resnet_input_split")


def test_declared_bound_and_exported():
    from tise_toolbox_amd import _lib, build
    raw_text = open(os.path.join(ROOT, "include", "tise_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw_text, flags=re.S)
    declared = set(re.findall(r"\b(tise_[a-z0-9_]+)\s*\(", text))
    assert "resnet.hip" in build.SOURCES and "conv_pipe.hip" in build.SOURCES
    build.build(force=False, verbose=False)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in declared and name in _lib.SIGNATURES
        getattr(raw, name)
        m = re.search(name + r"\s*\(([^)]*)\)", text)
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [10, 17, 11, 7]
    assert _lib.SIGNATURES["tise_maxpool3s2p1_split_nhwc"] == _lib.SIGNATURES["tise_maxpool3s2_split_nhwc"]          # its sibling's arguments
    assert _lib.SIGNATURES["tise_stem_conv7x7s2_split_u8_mfma"] == _lib.SIGNATURES["tise_stem_conv3x3s2_split_u8_mfma"]
    getattr(raw, "tise_internal_split_flag_resnet")                        # the residual kernel's range-guard word has its reader


def test_argument_validation_without_a_gpu():
    """Fake device addresses; every call has exactly one defect and must come back with its code before any HIP call (a launch
    would need a device this test does not have)."""
    from tise_toolbox_amd import _lib
    lib = _lib.load()
    bad, unsupported, ok = _lib.TISE_ERR_INVALID_ARG, _lib.TISE_ERR_UNSUPPORTED, _lib.TISE_OK
    X, L, W, S, B, O, R, I = (0x7f0000000000 + i * 0x10000000 for i in range(8))       # 16-byte aligned

    def stem(x=X, lut=L, n=0, h=32, w=32, ws=W, sc=S, bs=B, out=O):
        return lib.tise_stem_conv7x7s2_split_u8_mfma(x, lut, n, h, w, ws, sc, bs, out, None)
    for kw in (dict(x=None), dict(lut=None), dict(ws=None), dict(sc=None), dict(bs=None), dict(out=None), dict(n=-1), dict(h=0), dict(w=0),
               dict(h=-3), dict(lut=L + 2), dict(ws=W + 8), dict(sc=S + 4), dict(bs=B + 8), dict(out=O + 8)):
        assert stem(**kw) == bad, kw
    assert stem() == ok and stem(x=X + 1) == ok and stem(h=1, w=1) == ok            # any address, down to one pixel; n = 0: no HIP call
    assert stem(n=1 << 20, h=1 << 12, w=1 << 12) == unsupported                    # 2^20 x 2^11 x 2^11 output pixels

    def inp(x=X, lut=L, n=0, h=32, w=32, out=O):
        return lib.tise_resnet_input_split(x, lut, n, h, w, out, None)
    for kw in (dict(x=None), dict(lut=None), dict(out=None), dict(n=-1), dict(h=0), dict(w=0), dict(lut=L + 2), dict(out=O + 8)):
        assert inp(**kw) == bad, kw
    assert inp() == ok and inp(x=X + 3) == ok
    assert inp(n=65536) == unsupported and inp(n=1, h=1 << 14, w=(1 << 13) + 1) == unsupported

    def pool(x=R, x_ld=64, x_off=0, n=0, h=16, w=16, c=64, out=O, out_ld=64, out_off=0):
        return lib.tise_maxpool3s2p1_split_nhwc(x, x_ld, x_off, n, h, w, c, out, out_ld, out_off, None)
    for kw in (dict(x=None), dict(out=None), dict(n=-1), dict(h=0), dict(w=0), dict(c=0), dict(c=60), dict(c=-8), dict(x_ld=72),
               dict(out_ld=72), dict(x_off=4), dict(out_off=4), dict(x_off=8), dict(out_off=8), dict(c=72), dict(x_off=-8, c=8),
               dict(x=R + 8), dict(out=O + 2), dict(x_ld=1 << 32, c=64), dict(out=R)):
        assert pool(**kw) == bad, kw
    assert pool() == ok and pool(h=1, w=1) == ok
    assert pool(x_off=16, c=48, out_ld=96, out_off=48) == ok                       # a slice into a slice at an offset
    assert pool(x_off=24, c=48, out_ld=96, out_off=48) == bad                      # 24 + 48 > 64
    assert pool(n=65536) == unsupported

    def res(raw=R, raw_ld=64, raw_off=0, bias=B, ids=I, id_ld=64, id_off=0, idr=None, idr_ld=0, idr_off=0, idb=None, pixels=0, c=64,
            out=O, out_ld=64, out_off=0):
        return lib.tise_residual_relu_split_nhwc(raw, raw_ld, raw_off, bias, ids, id_ld, id_off, idr, idr_ld, idr_off, idb, pixels, c,
                                                 out, out_ld, out_off, None)
    rawid = dict(ids=None, id_ld=0, idr=I, idr_ld=64, idb=S)                       # the raw-identity form
    assert res() == ok and res(**rawid) == ok
    assert res(raw_ld=96, raw_off=32, id_ld=80, id_off=32, c=48, out_ld=112, out_off=64) == ok          # slices; 16-wide tails
    for kw in (dict(raw=None), dict(bias=None), dict(out=None), dict(pixels=-1), dict(c=0), dict(c=60), dict(c=-8),
               dict(ids=None), dict(idr=I, idr_ld=64, idb=S),                     # no identity; two identities
               dict(raw_ld=66), dict(raw_off=2, c=56), dict(raw_off=8), dict(raw_off=-8, c=8), dict(raw=R + 4), dict(bias=B + 4),
               dict(out_ld=72), dict(out_off=4, c=56), dict(out_off=8), dict(out_off=-8, c=8), dict(out=O + 8), dict(out_ld=1 << 32),
               dict(id_ld=72), dict(id_off=4, c=56), dict(id_off=8), dict(id_off=-8, c=8), dict(ids=I + 8), dict(id_ld=1 << 32),
               dict(out=I), dict(out=R)):
        assert res(**kw) == bad, kw
    for kw in (dict(idb=None), dict(idr_ld=66), dict(idr_off=2, c=56), dict(idr_off=8), dict(idr_off=-8, c=8), dict(idr=I + 4),
               dict(idb=S + 4), dict(out=I)):
        assert res(**{**rawid, **kw}) == bad, kw
    assert res(pixels=1 << 40, c=1 << 12, raw_ld=1 << 12, id_ld=1 << 12, out_ld=1 << 12) == unsupported
