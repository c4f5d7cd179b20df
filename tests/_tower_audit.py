"""Launch recorder, fp64 references and wiring check of the transformer towers (clip_hip.HipTowers, dinov2_hip.HipDino) for
tests/test_gpu_tower_launches.py (helper, no tests), modelled on tests/_trunk_audit.py.

While a tower's forward runs, ``Recorder`` wraps ``_lib.call`` and the pointer helper ``_p`` (bound in clip_hip AND, by name,
in dinov2_hip) and keeps the operands of every launch AS THAT LAUNCH SAW THEM: a clone of every input taken before the call
(``tise_gemm_f16_res32`` runs in place on the stream, ``layernorm32(..., out=y)`` overwrites a buffer an earlier launch read), a
clone of every destination before and after, and every integer and float argument by position.  Each launch is handed to a
``Checker`` as soon as it is recorded and its tensors are dropped afterwards: a 24-layer forward never holds more than one
launch, plus the latest output of each role of the graph (stream, y, qkv, o, f), which the wiring check needs.

What the Checker asserts of launch k against step k of a PLAN -- the module's graph written out as the expected launch sequence
(``dino_plan``, ``clip_image_plan``, ``clip_text_plan``), built from the MODULE's parameters rounded as the tower documents
(weights and Linear biases fp16; LayerNorm, LayerScale, class token and position table fp32 for DINOv2 and fp16 for CLIP), never
from the copies held by ``_Block`` / ``HipTowers`` / ``HipDino``, which would test the copying with itself:

  name      the entry point is the step's;
  scalar    every integer and float argument equals the module's: eps bit for bit as a float, act, causal, heads, seq,
            out_fp32, M / N / K and every row stride;
  input     every input is bit-equal to the "after" clone of the destination of the launch the graph names as its producer,
            or to the rounded module parameter, the image, the token ids or the gather index the graph implies; a pointer
            the graph leaves out is null;
  changed   no launch changes the bits of any of its inputs (the res32 residual when ``out is res`` is the one exception,
            and there the two pointers must be one);
  numeric   the launch's destination against the operation in fp64 computed from the launch's OWN recorded activation inputs
            and the module's parameters, at the bound the project derived for that kernel on its own (none is taken from what
            a tower gives): tests/_clip_gemm_child.check (rounding interval and magnitude), tests/_dinov2_gemm_child.check_res32
            and check_act2, test_gpu_clip_kernels._ln_check and _attention_ref, test_gpu_dinov2_kernels._ln32_check,
            test_gpu_attention_long.attention_long_ref (with its flat 3e-3), and bit equality for patchify, the three
            token-assembly kernels and both gathers.

The kernel INSTANCE of a GEMM launch cannot be read back from the library; as in tests/_clip_gemm_child.py it is the restated
rule ``instance_for`` (M, N, act and the process environment), kept per launch so that the tests can say which instances ran
on a tower's operands.

Nothing here touches a device at import time.  ``python tests/_tower_audit.py`` audits the tiny towers under the environment
it was started with and prints one JSON record (the GEMM instance switches are read once per process).
"""
import ctypes
import json
import os
import sys
import time

import torch

# name -> (input pointer positions, destination pointer positions) among the arguments of _lib.call(name, *args)
KNOWN = {
    "tise_gemm_f16": ((0, 2, 4, 5), (7,)),
    "tise_gemm_f16_act": ((0, 2, 4, 5), (7,)),
    "tise_gemm_f16_res32": ((0, 2, 4, 5, 6), (8,)),
    "tise_layernorm_f16": ((0, 2, 3), (4,)),
    "tise_layernorm_f32": ((0, 2, 3), (4,)),
    "tise_attention_f16": ((0,), (6,)),
    "tise_attention_long_f16": ((0,), (5,)),
    "tise_patchify_f16": ((0,), (4,)),
    "tise_patchify_pad_f16": ((0,), (5,)),
    "tise_vit_tokens_f16": ((0, 1, 2), (6,)),
    "tise_vit_tokens_f32": ((0, 1, 2), (6,)),
    "tise_text_tokens_f16": ((0, 1, 2), (6,)),
    "tise_gather_rows_f16": ((0, 1), (4,)),
    "tise_gather_rows_f32": ((0, 1), (4,)),
}
LAUNCH_NOTHING = ("tise_attention_long_key_tile",)      # entry points of the towers' sources that launch no kernel

# the arguments by position (the trailing stream left out): what a failure message calls them
_GEMM = ("a", "lda", "w", "ldw", "bias", "res", "ldr", "out", "ldo", "m", "n", "k", "act")
_LN16 = ("x", "ldx", "gamma", "beta", "out", "ldo", "rows", "C", "eps")
_TOK = ("patch_out", "cls", "pos", "batch", "npatch", "width", "out")
ARGS = {
    "tise_gemm_f16": _GEMM,
    "tise_gemm_f16_act": _GEMM,
    "tise_gemm_f16_res32": ("a", "lda", "w", "ldw", "bias", "scale", "res", "ldr", "out", "ldo", "m", "n", "k"),
    "tise_layernorm_f16": _LN16,
    "tise_layernorm_f32": _LN16 + ("out_fp32",),
    "tise_attention_f16": ("qkv", "batch", "seq", "heads", "head_dim", "causal", "out"),
    "tise_attention_long_f16": ("qkv", "batch", "seq", "heads", "head_dim", "out"),
    "tise_patchify_f16": ("x", "batch", "res", "patch", "out"),
    "tise_patchify_pad_f16": ("x", "batch", "res", "patch", "kpad", "out"),
    "tise_vit_tokens_f16": _TOK,
    "tise_vit_tokens_f32": _TOK,
    "tise_text_tokens_f16": ("tok", "table", "pos", "rows", "seq", "width", "out"),
    "tise_gather_rows_f16": ("x", "index", "n", "width", "out"),
    "tise_gather_rows_f32": ("x", "index", "n", "width", "out"),
}
GEMMS = ("tise_gemm_f16", "tise_gemm_f16_act", "tise_gemm_f16_res32")
ALL_INSTANCES = {"gemm16_f16_kernel<false>", "gemm16_f16_kernel<true>", "gemm_f16_kernel", "gemm_f16_big_kernel"}
FLAT_TOL_LONG = 3e-3                                    # test_gpu_attention_long.py's check 2

# the tiny towers of tests/test_gpu_dinov2.py and tests/test_gpu_clip_l14.py (the test module asserts they are the same)
TINY154 = dict(width=128, layers=2, heads=2, patch=14, resolution=154)
TINY84 = dict(width=128, layers=2, heads=2, patch=14, resolution=84)
TINY_CLIP = dict(resolution=154, patch=14, width=128, layers=2, heads=2, embed_dim=64, text_width=64, text_layers=1, text_heads=1)
CAPTIONS = ("a bird", "two dogs run over a green field", "a red bus", "the quick brown fox jumps over the lazy dog again and again",
            "a plate of food on a wooden table")


def bits(t):
    """The tensor's bit patterns (uninitialised memory may hold NaNs, which never compare equal as numbers)."""
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64, 1: torch.uint8}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


# ------------------------------------------------------------------------------------------------------- recording
class Launch:
    """One kernel launch: ``name``, ``inputs`` / ``dsts`` keyed by the argument's name (``inputs[label]`` the clone taken before
    the call, or None for a null pointer; ``dsts[label]`` = (before, after)), ``scalars`` = every integer and float argument by
    name, ``changed`` = the inputs whose bits the call changed, ``aliased`` = the inputs that share a destination's address."""

    def __init__(self, index, name):
        self.index, self.name = index, name
        self.inputs, self.dsts, self.scalars = {}, {}, {}
        self.changed, self.aliased = [], []
        self.instance = None
        self.figure = None

    def __repr__(self):
        return f"{self.name} {self.scalars}"

    def drop(self):
        self.inputs, self.dsts = {}, {}


class Recorder:
    """``with Recorder(on_launch) as rec: towers.encode_image(x)`` -> ``rec.launches`` (tensors dropped once ``on_launch``
    has seen them; kept when there is no callback).  A ``tise_*`` name outside ``KNOWN`` is an error: a future kernel cannot
    slip past the audit."""

    def __init__(self, on_launch=None):
        self.launches = []
        self.on_launch = on_launch
        self._tensors = {}

    def __enter__(self):
        from tise_toolbox_amd import _lib, clip_hip, dinov2_hip
        rec = self
        self._orig = (_lib.call, clip_hip._p, dinov2_hip._p)
        orig_call, orig_p = self._orig[0], self._orig[1]
        assert self._orig[2] is orig_p, "dinov2_hip._p is no longer clip_hip._p: the recorder patches one helper under two names"

        def p(t):                                                  # remember which tensor a raw pointer is
            if t is not None:
                rec._tensors[t.data_ptr()] = t
            return orig_p(t)

        def clone(t):
            torch.cuda.synchronize()
            return t.detach().clone()

        def lib_call(name, *args):
            if name not in KNOWN:
                raise AssertionError(f"a tower reached {name}, which the launch recorder does not know")
            ins, outs = KNOWN[name]
            labels = ARGS[name]
            assert len(args) == len(labels) + 1, (name, len(args))     # + the stream
            L = Launch(len(rec.launches), name)

            def tensor(i):
                if args[i] is None or args[i].value is None:
                    return None
                t = rec._tensors.get(args[i].value)
                assert t is not None, f"{name}: argument {labels[i]} is a pointer no _p() call produced"
                return t
            live_in = {labels[i]: tensor(i) for i in ins}
            live_out = {labels[i]: tensor(i) for i in outs}
            L.inputs = {k: (clone(t) if t is not None else None) for k, t in live_in.items()}
            before = {k: clone(t) for k, t in live_out.items()}
            for i, v in enumerate(args[:-1]):
                if isinstance(v, bool):
                    raise AssertionError(f"{name}: argument {labels[i]} is a bool")
                if isinstance(v, int):
                    L.scalars[labels[i]] = v
                elif isinstance(v, ctypes.c_float):
                    L.scalars[labels[i]] = v.value
            out_ptrs = {t.data_ptr(): k for k, t in live_out.items()}
            L.aliased = [(k, out_ptrs[t.data_ptr()]) for k, t in live_in.items() if t is not None and t.data_ptr() in out_ptrs]
            r = orig_call(name, *args)
            L.dsts = {k: (before[k], clone(t)) for k, t in live_out.items()}
            L.changed = [k for k, t in live_in.items() if t is not None and not same_bits(t, L.inputs[k])]
            rec._tensors.clear()
            rec.launches.append(L)
            if rec.on_launch is not None:
                rec.on_launch(L)
                L.drop()
            return r

        _lib.call, clip_hip._p, dinov2_hip._p = lib_call, p, p
        return self

    def __exit__(self, *exc):
        from tise_toolbox_amd import _lib, clip_hip, dinov2_hip
        _lib.call, clip_hip._p, dinov2_hip._p = self._orig
        self._tensors.clear()


# ------------------------------------------------------------------------------------------------------ references
# one function per entry point: (step, launch) -> {figure name: value}; raises AssertionError beyond the kernel's own bound.
# Activations come from the launch's recorded inputs, parameters and scalars from the step (the module).
def _gemm_env():
    return {k: os.environ[k] for k in ("TISE_GEMM_SHAPE", "TISE_GEMM_BIG") if k in os.environ}


def ref_gemm(S, L):
    from tests import _clip_gemm_child as gc
    from tests import _dinov2_gemm_child as dc
    a, out, act = L.inputs["a"], L.dsts["out"][1], S.scalars["act"]
    w, b = S.params["w"], S.params.get("bias")
    r = L.inputs["res"] if S.ins["res"] is not None else None
    assert torch.isfinite(out).all(), "non-finite output"
    if act == 2:
        assert r is None
        ratio, _ = dc.check_act2(a, w, b, out)
        outside = 0
    else:
        ratio, outside = gc.check(a, w, b, r, act, out)
    assert outside == 0, f"{outside} elements outside the rounding interval"
    assert ratio <= 1.0, f"|out - fp64| is {ratio:.3f} x the bound"
    return {"ratio": ratio}


def ref_res32(S, L):
    from tests import _dinov2_gemm_child as dc
    out = L.dsts["out"][1]
    assert torch.isfinite(out).all(), "non-finite output"
    ratio = dc.check_res32(L.inputs["a"], S.params["w"], S.params.get("bias"), S.params.get("scale"), L.inputs["res"], out)
    assert ratio <= 1.0, f"|out - fp64| is {ratio:.3f} x the bound"
    return {"ratio": ratio}


def ref_ln16(S, L):
    from tests.test_gpu_clip_kernels import _ln_check
    out = L.dsts["out"][1]
    assert torch.isfinite(out).all(), "non-finite output"
    ratio, _ = _ln_check(L.inputs["x"], S.params["gamma"], S.params["beta"], S.eps, out)
    assert ratio <= 1.0, f"|out - fp64| is {ratio:.3f} x the bound"
    return {"ratio": ratio}


def ref_ln32(S, L):
    from tests.test_gpu_dinov2_kernels import _ln32_check
    out = L.dsts["out"][1]
    assert out.dtype == (torch.float32 if S.scalars["out_fp32"] else torch.float16), out.dtype
    assert torch.isfinite(out).all(), "non-finite output"
    ratio = _ln32_check(L.inputs["x"], S.params["gamma"], S.params["beta"], S.eps, out)
    assert ratio <= 1.0, f"|out - fp64| is {ratio:.3f} x the bound"
    return {"ratio": ratio}


def ref_attention(S, L):
    from tests.test_gpu_clip_kernels import _attention_ref
    sc = S.scalars
    got = L.dsts["out"][1]
    ref, bound, _ = _attention_ref(L.inputs["qkv"], sc["batch"], sc["seq"], sc["heads"], bool(sc["causal"]))
    ratio = ((got.double() - ref).abs() / bound).max().item()
    assert torch.isfinite(got).all() and ratio <= 1.0, f"|out - fp64| is {ratio:.3f} x the bound"
    return {"ratio": ratio}


def ref_attention_long(S, L):
    from tests.test_gpu_attention_long import attention_long_ref
    from tise_toolbox_amd import clip_hip
    sc = S.scalars
    got = L.dsts["out"][1]
    ref, bound, _ = attention_long_ref(L.inputs["qkv"], sc["batch"], sc["seq"], sc["heads"], clip_hip.ATTN_LONG_KEY_TILE)
    err = (got.double() - ref).abs()
    ratio = (err / bound).max().item()
    flat = (err.max() / max(1.0, ref.abs().max().item())).item()
    assert torch.isfinite(got).all() and ratio <= 1.0, f"|out - fp64| is {ratio:.3f} x the bound"
    assert flat <= FLAT_TOL_LONG, f"flat error {flat:.3e} > {FLAT_TOL_LONG}"
    return {"ratio": ratio, "flat": flat}


def _exact(got, want, what):
    assert same_bits(got, want), f"not bit-equal to {what}"
    return {"ratio": 0.0}


def ref_patchify(S, L):
    """Patch matrix [B G^2][3 P^2], columns (c, ky, kx), zero columns up to kpad (tise_patchify_pad_f16)."""
    x, sc = L.inputs["x"], S.scalars
    b, p = sc["batch"], sc["patch"]
    g = sc["res"] // p
    want = x.unfold(2, p, p).unfold(3, p, p).permute(0, 2, 3, 1, 4, 5).reshape(b * g * g, -1)
    if "kpad" in sc:
        wide = torch.zeros((b * g * g, sc["kpad"]), dtype=x.dtype, device=x.device)
        wide[:, :want.shape[1]] = want
        want = wide
    return _exact(L.dsts["out"][1], want.contiguous(), "unfold of the image")


def ref_vit_tokens(S, L):
    """x[b][0] = cls + pos[0], x[b][1 + p] = patch_out[b NP + p] + pos[1 + p]: one fp32 add (and one fp16 rounding for CLIP)."""
    sc = S.scalars
    b, npch, w = sc["batch"], sc["npatch"], sc["width"]
    pe, cls, pos = L.inputs["patch_out"], S.params["cls"], S.params["pos"]
    seqs = torch.cat([cls.float().expand(b, 1, w), pe.float().view(b, npch, w)], 1) + pos.float()
    want = seqs.view(b * (npch + 1), w)
    if L.name == "tise_vit_tokens_f16":
        want = want.half()
    return _exact(L.dsts["out"][1], want, "cat(cls, patch rows) + pos")


def ref_text_tokens(S, L):
    sc = S.scalars
    tok = L.inputs["tok"].long().view(-1, sc["seq"])
    want = (S.params["table"][tok].float() + S.params["pos"][:sc["seq"]].float()).half().view(sc["rows"], sc["width"])
    return _exact(L.dsts["out"][1], want, "table[tok] + pos")


def ref_gather(S, L):
    return _exact(L.dsts["out"][1], L.inputs["x"][S.given["index"]], "x[index]")


REFS = {
    "tise_gemm_f16": ref_gemm, "tise_gemm_f16_act": ref_gemm, "tise_gemm_f16_res32": ref_res32,
    "tise_layernorm_f16": ref_ln16, "tise_layernorm_f32": ref_ln32,
    "tise_attention_f16": ref_attention, "tise_attention_long_f16": ref_attention_long,
    "tise_patchify_f16": ref_patchify, "tise_patchify_pad_f16": ref_patchify,
    "tise_vit_tokens_f16": ref_vit_tokens, "tise_vit_tokens_f32": ref_vit_tokens, "tise_text_tokens_f16": ref_text_tokens,
    "tise_gather_rows_f16": ref_gather, "tise_gather_rows_f32": ref_gather,
}
assert set(REFS) == set(KNOWN) == set(ARGS)


# ---------------------------------------------------------------------------------------------------------- the plan
class Step:
    """One expected launch.  ``ins``: argument name -> ("act", role) | ("param", key of ``params``) | ("given", key of ``given``)
    | None (a null pointer); ``scalars``: argument name -> the module's value; ``out``: the role its destination plays;
    ``inplace``: the residual and the destination are one tensor; ``where``: the module path, for messages."""

    def __init__(self, name, where, ins, scalars, out, params=None, given=None, eps=None, inplace=False):
        self.name, self.where, self.ins, self.scalars, self.out = name, where, ins, scalars, out
        self.params, self.given, self.eps, self.inplace = params or {}, given or {}, eps, inplace
        if eps is not None:
            self.scalars["eps"] = ctypes.c_float(eps).value            # what the C ABI receives: the fp32 nearest to the module's
        assert set(ins) == {ARGS[name][i] for i in KNOWN[name][0]}, (name, sorted(ins))
        assert set(self.scalars) == {a for i, a in enumerate(ARGS[name]) if i not in KNOWN[name][0] + KNOWN[name][1]}, (name, sorted(self.scalars))


def _gemm_step(kind, where, a_role, w, bias, out, m, res_role=None, act=0, scale=None):
    """A GEMM of the plan: ``kind`` "f16" / "act" / "res32"; w (N, K) and bias the module's, rounded to fp16."""
    n, k = w.shape
    params = {"w": w}
    ins = {"a": ("act", a_role), "w": ("param", "w"), "bias": None}
    if bias is not None:
        params["bias"] = bias
        ins["bias"] = ("param", "bias")
    if kind == "res32":
        ins["scale"] = None
        if scale is not None:
            params["scale"] = scale
            ins["scale"] = ("param", "scale")
        ins["res"] = ("act", res_role)
        sc = dict(lda=k, ldw=k, ldr=n, ldo=n, m=m, n=n, k=k)
        return Step("tise_gemm_f16_res32", where, ins, sc, out, params, inplace=True)
    ins["res"] = ("act", res_role) if res_role else None
    sc = dict(lda=k, ldw=k, ldr=n if res_role else 0, ldo=n, m=m, n=n, k=k, act=act)
    return Step("tise_gemm_f16_act" if kind == "act" else "tise_gemm_f16", where, ins, sc, out, params)


def _ln_step(name, where, x_role, ln, cast, rows, out, out_fp32=None):
    c = ln.weight.shape[0]
    sc = dict(ldx=c, ldo=c, rows=rows, C=c)
    if out_fp32 is not None:
        sc["out_fp32"] = out_fp32
    return Step(name, where, {"x": ("act", x_role), "gamma": ("param", "gamma"), "beta": ("param", "beta")}, sc, out,
                {"gamma": cast(ln.weight), "beta": cast(ln.bias)}, eps=ln.eps)


def _attention_step(where, batch, seq, heads, causal):
    from tise_toolbox_amd import clip_hip
    if seq > clip_hip.ATTN_SHORT_MAX_SEQ:                              # the long kernel exactly beyond the short one's limit
        assert not causal
        return Step("tise_attention_long_f16", where, {"qkv": ("act", "qkv")}, dict(batch=batch, seq=seq, heads=heads, head_dim=64), "o")
    return Step("tise_attention_f16", where, {"qkv": ("act", "qkv")},
                dict(batch=batch, seq=seq, heads=heads, head_dim=64, causal=1 if causal else 0), "o")


def dino_plan(model, image, dev):
    """The launch sequence of HipDino.encode_image(image) from the module ``model`` (dinov2_model.DinoVisionTransformer)."""
    h = lambda t: t.detach().to(dev, torch.float16).contiguous()
    f = lambda t: t.detach().to(dev, torch.float32).contiguous()
    x16 = image.to(dev, torch.float16).contiguous()
    b, _, r, _ = x16.shape
    w, p = model.out_dim, model.patch
    g = r // p
    npatch, seq = g * g, g * g + 1
    kcols = 3 * p * p
    kpad = (kcols + 63) // 64 * 64
    wp = torch.zeros((w, kpad), dtype=torch.float16, device=dev)
    wp[:, :kcols] = h(model.patch_embed.proj.weight.flatten(1))
    steps = [Step("tise_patchify_pad_f16", "patch_embed (unfold)", {"x": ("given", "image")}, dict(batch=b, res=r, patch=p, kpad=kpad), "pm",
                  given={"image": x16}),
             _gemm_step("f16", "patch_embed.proj", "pm", wp, h(model.patch_embed.proj.bias), "pe", b * npatch),
             Step("tise_vit_tokens_f32", "cls_token / pos", {"patch_out": ("act", "pe"), "cls": ("param", "cls"), "pos": ("param", "pos")},
                  dict(batch=b, npatch=npatch, width=w), "x", {"cls": f(model.cls_token.reshape(-1)), "pos": f(model.pos)})]
    rows = b * seq
    for i, blk in enumerate(model.blocks):
        at = f"blocks.{i}."
        steps += [
            _ln_step("tise_layernorm_f32", at + "norm1", "x", blk.norm1, f, rows, "y", out_fp32=0),
            _gemm_step("f16", at + "attn.qkv", "y", h(blk.attn.qkv.weight), h(blk.attn.qkv.bias), "qkv", rows),
            _attention_step(at + "attn", b, seq, blk.attn.heads, False),
            _gemm_step("res32", at + "attn.proj + ls1", "o", h(blk.attn.proj.weight), h(blk.attn.proj.bias), "x", rows, res_role="x",
                       scale=f(blk.ls1.gamma)),
            _ln_step("tise_layernorm_f32", at + "norm2", "x", blk.norm2, f, rows, "y", out_fp32=0),
            _gemm_step("act", at + "mlp.fc1", "y", h(blk.mlp.fc1.weight), h(blk.mlp.fc1.bias), "f", rows, act=2),
            _gemm_step("res32", at + "mlp.fc2 + ls2", "f", h(blk.mlp.fc2.weight), h(blk.mlp.fc2.bias), "x", rows, res_role="x",
                       scale=f(blk.ls2.gamma)),
        ]
    idx = torch.arange(b, device=dev, dtype=torch.int64) * seq
    steps += [Step("tise_gather_rows_f32", "class rows", {"x": ("act", "x"), "index": ("given", "index")}, dict(n=b, width=w), "c",
                   given={"index": idx}),
              _ln_step("tise_layernorm_f32", "norm", "c", model.norm, f, b, "feat", out_fp32=1)]
    return steps


def _clip_blocks(blocks, prefix, b, seq, causal, h):
    steps = []
    rows = b * seq
    for i, blk in enumerate(blocks):
        at = f"{prefix}resblocks.{i}."
        steps += [
            _ln_step("tise_layernorm_f16", at + "ln_1", "x", blk.ln_1, h, rows, "y"),
            _gemm_step("f16", at + "attn.in_proj", "y", h(blk.attn.in_proj_weight), h(blk.attn.in_proj_bias), "qkv", rows),
            _attention_step(at + "attn", b, seq, blk.attn.heads, causal),
            _gemm_step("f16", at + "attn.out_proj", "o", h(blk.attn.out_proj.weight), h(blk.attn.out_proj.bias), "x", rows, res_role="x"),
            _ln_step("tise_layernorm_f16", at + "ln_2", "x", blk.ln_2, h, rows, "y"),
            _gemm_step("f16", at + "mlp.c_fc", "y", h(blk.mlp.c_fc.weight), h(blk.mlp.c_fc.bias), "f", rows, act=1),
            _gemm_step("f16", at + "mlp.c_proj", "f", h(blk.mlp.c_proj.weight), h(blk.mlp.c_proj.bias), "x", rows, res_role="x"),
        ]
    return steps


def clip_image_plan(model, image, dev):
    """The launch sequence of HipTowers.encode_image(image) from the module ``model`` (clip_model.CLIP)."""
    h = lambda t: t.detach().to(dev, torch.float16).contiguous()
    v = model.visual
    x16 = image.to(dev, torch.float16).contiguous()
    b, _, r, _ = x16.shape
    p, w = v.conv1.kernel_size[0], v.conv1.out_channels
    g = r // p
    npatch, seq = g * g, g * g + 1
    kcols = 3 * p * p
    wp = h(v.conv1.weight.flatten(1))
    if kcols % 64 == 0 and p % 8 == 0:                                 # tise_patchify_f16 moves 8 halves, the GEMM steps K by 64
        first = Step("tise_patchify_f16", "visual.conv1 (unfold)", {"x": ("given", "image")}, dict(batch=b, res=r, patch=p), "pm",
                     given={"image": x16})
    else:
        kpad = (kcols + 63) // 64 * 64
        wide = torch.zeros((w, kpad), dtype=torch.float16, device=dev)
        wide[:, :kcols] = wp
        wp = wide
        first = Step("tise_patchify_pad_f16", "visual.conv1 (unfold)", {"x": ("given", "image")}, dict(batch=b, res=r, patch=p, kpad=kpad),
                     "pm", given={"image": x16})
    steps = [first,
             _gemm_step("f16", "visual.conv1", "pm", wp, None, "pe", b * npatch),
             Step("tise_vit_tokens_f16", "visual.class_embedding / positional_embedding",
                  {"patch_out": ("act", "pe"), "cls": ("param", "cls"), "pos": ("param", "pos")}, dict(batch=b, npatch=npatch, width=w), "tok",
                  {"cls": h(v.class_embedding), "pos": h(v.positional_embedding)}),
             _ln_step("tise_layernorm_f16", "visual.ln_pre", "tok", v.ln_pre, h, b * seq, "x")]
    steps += _clip_blocks(v.transformer.resblocks, "visual.transformer.", b, seq, False, h)
    idx = torch.arange(b, device=dev, dtype=torch.int64) * seq
    steps += [Step("tise_gather_rows_f16", "class rows", {"x": ("act", "x"), "index": ("given", "index")}, dict(n=b, width=w), "c",
                   given={"index": idx}),
              _ln_step("tise_layernorm_f16", "visual.ln_post", "c", v.ln_post, h, b, "cn"),
              _gemm_step("f16", "visual.proj", "cn", h(v.proj.t()), None, "feat", b)]
    return steps


def clip_text_plan(model, text, dev):
    """The launch sequence of HipTowers.encode_text(text) from the module: ``text`` (B, seq <= 77) token ids."""
    h = lambda t: t.detach().to(dev, torch.float16).contiguous()
    text = text.to(dev)
    b, seq = text.shape
    w = model.token_embedding.weight.shape[1]
    steps = [Step("tise_text_tokens_f16", "token_embedding / positional_embedding",
                  {"tok": ("given", "tok"), "table": ("param", "table"), "pos": ("param", "pos")}, dict(rows=b * seq, seq=seq, width=w), "x",
                  {"table": h(model.token_embedding.weight), "pos": h(model.positional_embedding)},
                  given={"tok": text.to(torch.int32).contiguous()})]
    steps += _clip_blocks(model.transformer.resblocks, "transformer.", b, seq, True, h)
    idx = torch.arange(b, device=dev, dtype=torch.int64) * seq + text.argmax(-1).to(torch.int64)
    steps += [Step("tise_gather_rows_f16", "end-of-text rows", {"x": ("act", "x"), "index": ("given", "index")}, dict(n=b, width=w), "e",
                   given={"index": idx}),
              _ln_step("tise_layernorm_f16", "ln_final", "e", model.ln_final, h, b, "en"),
              _gemm_step("f16", "text_projection", "en", h(model.text_projection.t()), None, "feat", b)]
    return steps


# ------------------------------------------------------------------------------------------------------ the checker
class Checker:
    """Checks launch k against step k as it is recorded (module docstring).  ``failures`` = [(launch index, reason, message)]
    with reason one of "name", "scalar:<argument>", "input:<argument>", "changed:<argument>", "inplace", "numeric", "count";
    ``worst`` = entry point -> the largest ratio to its bound; ``instances`` = the GEMM instances the launches select;
    ``stream_stats`` = (largest |x|, median |x|) of the fp32 stream after its last update.  ``numerics``: None = every launch,
    or the entry points whose launches are compared with fp64 (the wiring is checked for all)."""

    def __init__(self, plan, numerics=None):
        self.plan, self.numerics = plan, numerics
        self.failures, self.rows = [], []
        self.worst, self.names, self.instances = {}, [], {}
        self.state = {}
        self.broken = False
        self.stream_stats = None
        self.seconds = 0.0

    def fail(self, k, reason, msg):
        self.failures.append((k, reason, f"launch {k} ({msg})"))

    def __call__(self, L):
        t0 = time.time()
        k = L.index
        self.names.append(L.name)
        if self.broken:
            return
        if k >= len(self.plan):
            self.broken = True
            return self.fail(k, "count", f"{L.name}: the module's graph has {len(self.plan)} launches")
        S = self.plan[k]
        if L.name != S.name:
            self.broken = True                                     # nothing after this can be lined up with the graph
            return self.fail(k, "name", f"{S.where}: {L.name} where the module's graph has {S.name}")
        at = f"{S.where}, {L.name}"
        for a in sorted(set(S.scalars) | set(L.scalars)):
            got, want = L.scalars.get(a), S.scalars.get(a)
            if got != want or type(got) is not type(want):
                self.fail(k, f"scalar:{a}", f"{at}: argument {a} is {got!r}, the module gives {want!r}")
        for a, src in S.ins.items():
            got = L.inputs[a]
            if src is None:
                if got is not None:
                    self.fail(k, f"input:{a}", f"{at}: argument {a} is set, the module has nothing there")
                continue
            kind, key = src
            want = self.state.get(key) if kind == "act" else (S.params if kind == "param" else S.given)[key]
            what = {"act": f"the output of the launch that produced '{key}'", "param": f"the module's rounded parameter ({S.where}: {key})",
                    "given": f"the {key} the graph implies"}[kind]
            if got is None or want is None or not same_bits(got, want):
                self.fail(k, f"input:{a}", f"{at}: argument {a} is not bit-equal to {what}")
        inplace = [(a, d) for a, d in L.aliased]
        if S.inplace:
            if inplace != [("res", "out")]:
                self.fail(k, "inplace", f"{at}: the residual is not updated in place (aliases {inplace})")
        elif inplace:
            self.fail(k, "inplace", f"{at}: input {inplace} shares its destination's address")
        for a in L.changed:
            if not (S.inplace and a == "res"):
                self.fail(k, f"changed:{a}", f"{at}: the launch changed the bits of its input {a}")
        if L.name in GEMMS:
            from tests import _dinov2_gemm_child as dc
            L.instance = dc.instance_for(S.scalars["m"], S.scalars["n"], _gemm_env(), act=S.scalars.get("act", 0))
            self.instances.setdefault(L.instance, []).append(k)
        if self.numerics is None or L.name in self.numerics:
            try:
                fig = REFS[L.name](S, L)
            except (AssertionError, RuntimeError, KeyError, TypeError) as e:
                fig = None
                self.fail(k, "numeric", f"{at}: {type(e).__name__}: {e}")
            if fig is not None:
                L.figure = fig
                self.worst[L.name] = max(self.worst.get(L.name, 0.0), fig["ratio"])
                self.rows.append((k, L.name, S.where, fig["ratio"], L.instance))
        after = L.dsts["out"][1]
        self.state[S.out] = after
        if S.out == "x" and after.dtype == torch.float32:          # the fp32 stream: its largest entry so far, its latest median
            a = after.abs().flatten()
            self.stream_stats = (max(a.max().item(), self.stream_stats[0] if self.stream_stats else 0.0), a.median().item())
        self.seconds += time.time() - t0

    def finish(self):
        if not self.broken and len(self.names) != len(self.plan):
            self.fail(len(self.names), "count", f"{len(self.names)} launches, the module's graph has {len(self.plan)}")
        self.state.clear()
        for S in self.plan:                                        # the plan's parameter copies go with it
            S.params, S.given = {}, {}
        self.plan = [(S.name, S.where) for S in self.plan]
        return self

    def summary(self):
        return dict(launches=len(self.names), worst={k: round(v, 4) for k, v in sorted(self.worst.items())},
                    instances=sorted(self.instances), failures=[m for _, _, m in self.failures])


def check_assembly(plan, forward, numerics=None):
    """Run ``forward()`` under the recorder against ``plan``: -> (Checker, what forward returned)."""
    chk = Checker(plan, numerics)
    with Recorder(chk):
        out = forward()
    torch.cuda.synchronize()
    return chk.finish(), out


# ------------------------------------------------------------------------------------------------- parameter sets
def fill_defaults_(model, seed=1):
    """clip_model.seeded_init_ leaves every Linear bias at 0 and every LayerNorm at (1, 0): a bias taken from the neighbouring
    Linear would be the same bits.  Seeded values for exactly those, so that no two parameters of one shape are equal."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if p.dim() != 1 or name == "visual.class_embedding":
                continue
            v = torch.randn(p.shape, generator=g)
            if bool((p == 0).all()):
                p.copy_((0.02 * v).to(p))
            elif bool((p == 1).all()):
                p.copy_((1 + 0.1 * v).to(p))
    return model


OUTLIER_CHANNELS = (5, 77)
OUTLIER_MAGNITUDE = 3000.0
OUTLIER_FC2_SCALE = 40.0
OUTLIER_CLASS_MAGNITUDE = 50.0


def make_outliers_(model, magnitude=OUTLIER_MAGNITUDE, fc2_scale=OUTLIER_FC2_SCALE, class_magnitude=OUTLIER_CLASS_MAGNITUDE):
    """The seeded DINOv2 module with its stream driven large on a few tokens and channels: ``magnitude`` (signs alternating)
    added to channels OUTLIER_CHANNELS of the position rows of the class token and of two patch tokens, and block 0's fc2 rows
    (and bias entries) of those channels scaled by ``fc2_scale``, so that the first MLP writes into the very channels that
    carry the outliers on every token.  In place; returns the module."""
    with torch.no_grad():
        n = model.pos.shape[0]
        rows = [0, 1 + (n - 1) // 3, n - 2]
        for j, c in enumerate(OUTLIER_CHANNELS):
            for i, r in enumerate(rows):
                model.pos[r, c] += (class_magnitude if r == 0 else magnitude) * (-1.0) ** (i + j)
            model.blocks[0].mlp.fc2.weight[c] *= fc2_scale
            model.blocks[0].mlp.fc2.bias[c] *= fc2_scale
    return model


# ----------------------------------------------------------------------------------------- the tiny audits (child process)
def seeded_images(n, res, seed, dev):
    return torch.randn((n, 3, res, res), generator=torch.Generator(device="cpu").manual_seed(seed)).to(dev)


def audit_dino(model, image, dev, mutate=None, numerics=None):
    """HipDino over ``model`` audited on ``image``: -> (Checker, features).  ``mutate(tower)`` runs on the built instance first."""
    from tise_toolbox_amd import dinov2_hip
    tower = dinov2_hip.HipDino(model, dev)
    if mutate is not None:
        mutate(tower)
    return check_assembly(dino_plan(model, image, dev), lambda: tower.encode_image(image.half()), numerics)


def audit_clip_image(model, image, dev, towers=None, numerics=None):
    from tise_toolbox_amd import clip_hip
    towers = towers or clip_hip.HipTowers(model, dev)
    return check_assembly(clip_image_plan(model, image, dev), lambda: towers.encode_image(image), numerics)


def audit_clip_text(model, text, dev, towers=None):
    from tise_toolbox_amd import clip_hip
    towers = towers or clip_hip.HipTowers(model, dev)
    return check_assembly(clip_text_plan(model, text, dev), lambda: towers.encode_text(text))


def run_tiny_audits(dev):
    """The tiny DINOv2 towers (122 and 37 tokens, 3 images) and the tiny CLIP tower (image: 122 tokens, 3 images; text: 5
    captions at 77 tokens) under this process's environment: {configuration: Checker.summary()}."""
    from tise_toolbox_amd import clip_model, dinov2_model
    out = {}
    for name, cfg in (("dinov2-tiny154", TINY154), ("dinov2-tiny84", TINY84)):
        model = dinov2_model.build_dinov2(None, 0, cfg).to(dev)
        out[name] = audit_dino(model, seeded_images(3, cfg["resolution"], 5, dev), dev)[0].summary()
    model = fill_defaults_(clip_model.build_clip(None, 0, TINY_CLIP)).to(dev)
    out["clip-tiny154-image"] = audit_clip_image(model, seeded_images(3, TINY_CLIP["resolution"], 5, dev), dev)[0].summary()
    text = clip_model.HashTokenizer()(list(CAPTIONS)).to(dev)
    out["clip-tiny-text77"] = audit_clip_text(model, text, dev)[0].summary()
    return out


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    from tise_toolbox_amd import _lib
    assert torch.cuda.is_available(), "no HIP device"
    _lib.load()
    json.dump(dict(env=_gemm_env(), audits=run_tiny_audits(torch.device("cuda", 0))), sys.stdout)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()
