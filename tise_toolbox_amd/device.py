"""Torch-tensor front ends of the libtise_hip.so entry points.

PyTorch is only plumbing here (device memory, streams): every function passes raw
``data_ptr()`` values and the current HIP stream through the C ABI; the arithmetic is in
``csrc/*.hip``.  All functions raise if the tensors are not on a GPU -- there is no CPU
path in the product (see ``_lib.TiseLibraryError``).
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib

# image_realism/FID/inception.py:120-124 (applied to [0,1] pixels)
NORM_SCALE = (0.229 / 0.5, 0.224 / 0.5, 0.225 / 0.5)
NORM_BIAS = ((0.485 - 0.5) / 0.5, (0.456 - 0.5) / 0.5, (0.406 - 0.5) / 0.5)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


_FEED_STREAMS = {}


def _pick_independent_stream(dev):
    """A normal-priority stream whose hardware queue is NOT the one the current stream's kernels sit in, found by trying:
    a ~1.5 ms spin kernel goes to the current stream, one tiny host->device copy to each of eight pool streams, and the
    first stream whose copy completes while the spin is still running is taken (None when none overtakes)."""
    import time
    cur = torch.cuda.current_stream(dev)
    cands = [torch.cuda.Stream(device=dev) for _ in range(8)]
    src = torch.zeros(64, dtype=torch.uint8).pin_memory()
    dst = torch.empty(64, dtype=torch.uint8, device=dev)
    for st in cands:                                           # first use creates a stream's queue (milliseconds): not inside the measurement
        with torch.cuda.stream(st):
            dst.copy_(src, non_blocking=True)
        st.synchronize()
    cur.synchronize()
    torch.cuda._sleep(8_000_000)                               # ~4 ms of cycles on the current stream
    end = torch.cuda.Event()
    end.record(cur)
    evs = []
    for st in cands:
        with torch.cuda.stream(st):
            dst.copy_(src, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(st)
        evs.append(ev)
    chosen, t0 = None, time.perf_counter()
    while chosen is None and not end.query() and time.perf_counter() - t0 < 0.1:
        for i, ev in enumerate(evs):
            if ev.query():
                chosen = i
                break
    end.synchronize()
    for st in cands:
        st.synchronize()
    if os.environ.get("TISE_FEED_DEBUG") == "1":
        import sys
        print(f"[tise] feed stream probe: stream {chosen} of {len(cands)} overtook the compute stream", file=sys.stderr)
    return cands[chosen] if chosen is not None else None


def feed_stream(dev):
    """THE side stream of the image feeds on ``dev`` (host->device copies of decoded chunks, the PNG unfilter kernel, the
    gather copies of coalesce_u8): one per device and process.

    Round 6 measurement (tools/png_feed_probe.py, profiles/r06c_png_feed_timeline.txt): a fresh ``torch.cuda.Stream()`` per
    loader comes from torch's round-robin pool and HIP maps streams onto four hardware queues; every FOURTH stream shares
    its queue with the stream the trunk runs on, and its 1 500 chunk copies (1.6 MB each) then queued BEHIND the convolution
    launches -- 451 ms waiting for copies in a 470 ms job, 16 k images/s instead of 23 k, for every second loader of the
    probe.  A HIGH-priority stream always has a queue of its own, but its operations hold the compute queue up while they
    run: bench.py's host_feed leg (600 gather copies of 9.8 MB) fell from 0.98 to 0.89 of the resident rate
    (tools/host_feed_ab.sh, profiles/r06i_feed_stream_ab.txt).  So: a normal-priority stream that is PROVEN to overtake a
    kernel on the current stream (_pick_independent_stream, ~2 ms once per process); the high-priority stream only when
    none does.  TISE_FEED_PRIORITY=high | normal forces either without the probe."""
    dev = torch.device(dev)
    key = (dev.index if dev.index is not None else torch.cuda.current_device())
    st = _FEED_STREAMS.get(key)
    if st is None:
        lo, hi = torch.cuda.Stream.priority_range()            # (lowest, highest) = (0, -1) on this runtime
        mode = os.environ.get("TISE_FEED_PRIORITY", "auto")
        if mode == "auto":
            st = _pick_independent_stream(dev)
        elif mode == "normal":
            st = torch.cuda.Stream(device=dev)
        if st is None:
            st = torch.cuda.Stream(device=dev, priority=hi)
        _FEED_STREAMS[key] = st
    return st


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise _lib.TiseLibraryError("tise_toolbox_amd runs on MI355X only: tensor is not on a HIP device")


def make_lut(normalize_input=True, scale_pm1=False, network="torchvision"):
    """3x256 fp32 table: byte -> network input value, with the reference's own op order.

    ToTensor (fid_score.py:211): fp32(v) / 255 (true division, fp32).  Then either the
    inception.py:120-124 affine ``x * (s/0.5) + (m-0.5)/0.5`` (fp32 multiply, fp32 add, Python
    scalars rounded to fp32 first, as torch does for tensor-scalar ops) or, for O-IS,
    Normalize((.5,.5,.5),(.5,.5,.5)) = (x - 0.5) / 0.5 (object_centric_inception_score.py:91).
    ``network="inception-2015"`` (with ``normalize_input``): the 2015 graph's input map (v - 128) / 128 on the byte value v,
    every channel (fp32; constants in inception.INCEPTION_2015_INPUT_SUB / _DIV).
    ``network="slim"`` (with ``normalize_input``): the bird script's ``img.astype(np.float32) / 127.5 - 1.0``
    (inception_score_star_bird.py:69-70) on the byte value, every channel, fp32 in that order.
    """
    if network == "slim" and normalize_input and not scale_pm1:
        from .inception import SLIM_INPUT_DIV, SLIM_INPUT_SUB
        b = np.arange(256, dtype=np.uint8).astype(np.float32)
        row = b / np.float32(SLIM_INPUT_DIV) - np.float32(SLIM_INPUT_SUB)
        return np.ascontiguousarray(np.tile(row, (3, 1)).astype(np.float32))
    if network == "inception-2015" and normalize_input and not scale_pm1:
        from .inception import INCEPTION_2015_INPUT_DIV, INCEPTION_2015_INPUT_SUB
        b = np.arange(256, dtype=np.float32)
        row = (b - np.float32(INCEPTION_2015_INPUT_SUB)) / np.float32(INCEPTION_2015_INPUT_DIV)
        return np.ascontiguousarray(np.tile(row, (3, 1)).astype(np.float32))
    if network not in ("torchvision", "inception-2015", "slim"):
        raise ValueError(f"unknown network {network!r}")
    v = np.arange(256, dtype=np.float32) / np.float32(255.0)
    lut = np.empty((3, 256), dtype=np.float32)
    for c in range(3):
        if scale_pm1:
            lut[c] = (v - np.float32(0.5)) / np.float32(0.5)
        elif normalize_input:
            lut[c] = v * np.float32(NORM_SCALE[c]) + np.float32(NORM_BIAS[c])
        else:
            lut[c] = v
    return np.ascontiguousarray(lut)


_IDENTITY_LUT = np.ascontiguousarray(np.tile(np.arange(256, dtype=np.float32) / np.float32(255.0), (3, 1)))
_FILTERS = {"bilinear": 0, "bicubic": 1}


def pillow_vertical_first(h, w, oh):
    """Pillow's ``Image.resize`` (PIL/Image.py, read from 12.2.0) resizes a source more than 100 times taller than wide whose
    height shrinks to (w, oh) first and to (ow, oh) second: ``if self.size[1] > self.size[0] * 100 and size[1] < self.size[1]``.
    Everywhere else the horizontal pass runs first, which is the order the kernel states.  The uint8 intermediate makes the
    order visible (about one byte in five differs by 1 for 480 x 4 -> 299 x 299), and the host roads (DataLoader,
    clip_model.preprocess) call Pillow for the same pixels, so the device road follows the rule: _vertical_pass_first."""
    return h > 100 * w and oh < h


def _vertical_pass_first(src_u8, oh, filter):
    """Inside Pillow's rule: (N,h,w,3) -> (N,oh,w,3) uint8, a launch of its own whose horizontal pass is the identity; the
    caller's launch then sees h == oh and runs the horizontal pass only.  Outside the rule: ``src_u8`` itself."""
    n, h, w, _ = src_u8.shape
    if not pillow_vertical_first(h, w, oh):
        return src_u8
    mid = torch.empty((n, oh, w, 3), dtype=torch.uint8, device=src_u8.device)
    _lib.call("tise_resize_u8", _ptr(src_u8), n, h, w, None, oh, w, 1,
              _IDENTITY_LUT.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), _ptr(mid), _FILTERS[filter], _stream())
    return mid


def resize_bilinear_u8(src_u8, out_hw=(299, 299), lut=None, channels_last=True, return_u8=False):
    """(N,H,W,3) uint8 CUDA tensor -> (N,3,oh,ow) fp32 network input (PIL-exact bilinear).

    Fuses transforms.Resize + ToTensor (fid_score.py:208-213) and the input affine
    (inception.py:120-124) through ``lut`` (see make_lut).  With ``channels_last`` the
    result is an NCHW tensor in torch.channels_last memory format.
    """
    _require_cuda(src_u8)
    if src_u8.dtype != torch.uint8 or src_u8.dim() != 4 or src_u8.shape[3] != 3:
        raise ValueError("src_u8 must be (N,H,W,3) uint8")
    oh, ow = out_hw
    src_u8 = _vertical_pass_first(src_u8.contiguous(), oh, "bilinear")
    n, h, w, _ = src_u8.shape
    if lut is None:
        lut = make_lut(True)
    lut = np.ascontiguousarray(lut, dtype=np.float32)
    if channels_last:
        store = torch.empty((n, oh, ow, 3), dtype=torch.float32, device=src_u8.device)
        out = store.permute(0, 3, 1, 2)
    else:
        store = torch.empty((n, 3, oh, ow), dtype=torch.float32, device=src_u8.device)
        out = store
    u8 = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device=src_u8.device) if return_u8 else None
    _lib.call("tise_resize_bilinear_u8", _ptr(src_u8), n, h, w, _ptr(store), oh, ow, 1 if channels_last else 0,
              lut.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), _ptr(u8) if u8 is not None else None, _stream())
    return (out, u8) if return_u8 else out


def resize_u8_lut(src_u8, out_hw, lut, filter="bicubic", channels_last=False, return_u8=False):
    """(N,H,W,3) uint8 CUDA tensor -> (N,3,oh,ow) fp32 through a 3x256 byte -> value table, with Pillow's 8-bit two-pass
    resample for ``filter`` "bilinear" or "bicubic" (tise_resize_u8).  The CLIP metrics' preprocess on the device:
    clip._transform = Resize(224, BICUBIC) -> CenterCrop (a no-op for square images) -> ToTensor -> Normalize."""
    _require_cuda(src_u8)
    if src_u8.dtype != torch.uint8 or src_u8.dim() != 4 or src_u8.shape[3] != 3:
        raise ValueError("src_u8 must be (N,H,W,3) uint8")
    oh, ow = out_hw
    src_u8 = _vertical_pass_first(src_u8.contiguous(), oh, filter)
    n, h, w, _ = src_u8.shape
    lut = np.ascontiguousarray(lut, dtype=np.float32)
    if channels_last:
        store = torch.empty((n, oh, ow, 3), dtype=torch.float32, device=src_u8.device)
        out = store.permute(0, 3, 1, 2)
    else:
        store = torch.empty((n, 3, oh, ow), dtype=torch.float32, device=src_u8.device)
        out = store
    u8 = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device=src_u8.device) if return_u8 else None
    _lib.call("tise_resize_u8", _ptr(src_u8), n, h, w, _ptr(store), oh, ow, 1 if channels_last else 0,
              lut.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), _ptr(u8) if u8 is not None else None,
              _FILTERS[filter], _stream())
    return (out, u8) if return_u8 else out


def resize_u8_only(src_u8, out_hw=(299, 299), out=None):
    """(N,H,W,3) uint8 CUDA tensor -> the Pillow-exact resized uint8 image (N,oh,ow,3); no float output (the stem
    convolution applies the input table itself: SplitTrunk.forward_u8).  ``out``: preallocated contiguous
    (N,oh,ow,3) uint8 destination (a slice of a batch buffer when crops of different sizes are stacked)."""
    _require_cuda(src_u8)
    if src_u8.dtype != torch.uint8 or src_u8.dim() != 4 or src_u8.shape[3] != 3:
        raise ValueError("src_u8 must be (N,H,W,3) uint8")
    oh, ow = out_hw
    src_u8 = _vertical_pass_first(src_u8.contiguous(), oh, "bilinear")
    n, h, w, _ = src_u8.shape
    if out is None:
        u8 = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device=src_u8.device)
    else:
        u8 = out
        if u8.dtype != torch.uint8 or tuple(u8.shape) != (n, oh, ow, 3) or not u8.is_contiguous() or not u8.is_cuda:
            raise ValueError("out must be a contiguous (N,oh,ow,3) uint8 CUDA tensor")
    lut = _IDENTITY_LUT                                                   # unused by the kernel when dst is NULL
    _lib.call("tise_resize_bilinear_u8", _ptr(src_u8), n, h, w, None, oh, ow, 1,
              lut.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), _ptr(u8), _stream())
    return u8


_RAGGED_TABLES = {}        # device index -> [[pinned table, event of the launch that last read it], ...] (two, used in turn)


def resize_ragged_u8(crops, out_hw=(299, 299), out=None, filter="bilinear"):
    """List of (H_i,W_i,3) uint8 CUDA tensors of any sizes -> the Pillow-exact resized uint8 batch (B,oh,ow,3) in ONE launch
    (tise_resize_ragged_u8), byte for byte what ``resize_u8_only`` gives crop by crop.  A crop inside Pillow's vertical-first
    rule (pillow_vertical_first: more than 100 times taller than wide) gets its vertical pass in a launch of its own first, as
    there.  A size the plan builder refuses raises before anything of the batch is enqueued, naming the crop."""
    if len(crops) == 0:
        raise ValueError("empty batch")
    oh, ow = out_hw
    dev = crops[0].device
    srcs = []
    for i, c in enumerate(crops):
        _require_cuda(c)
        if c.dim() == 4 and c.shape[0] == 1:
            c = c[0]
        if c.dtype != torch.uint8 or c.dim() != 3 or c.shape[2] != 3:
            raise ValueError(f"crop {i} must be (H,W,3) uint8")
        c = c.contiguous()
        if pillow_vertical_first(c.shape[0], c.shape[1], oh):
            c = _vertical_pass_first(c.unsqueeze(0), oh, filter)[0]
        srcs.append(c)
    n = len(srcs)
    if out is None:
        out = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (n, oh, ow, 3) or not out.is_contiguous() or not out.is_cuda:
        raise ValueError("out must be a contiguous (N,oh,ow,3) uint8 CUDA tensor")
    ptrs = np.fromiter((c.data_ptr() for c in srcs), dtype=np.uint64, count=n)
    hs = np.fromiter((c.shape[0] for c in srcs), dtype=np.int32, count=n)
    ws = np.fromiter((c.shape[1] for c in srcs), dtype=np.int32, count=n)
    need = n * (64 + 4 * oh) + 16 * (n // 4096 + 1)
    ws_dev = torch.empty(need, dtype=torch.uint8, device=dev)
    # the table is built in page-locked memory and copied asynchronously (the host does not wait for the stream: the trunk
    # passes of earlier batches are still queued there); two buffers in turn, each reused once its last copy has run
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    ring = _RAGGED_TABLES.setdefault(key, [[None, None], [None, None]])
    slot = ring.pop(0)
    ring.append(slot)
    if slot[1] is not None:
        slot[1].synchronize()
    if slot[0] is None or slot[0].numel() < need:
        slot[0] = torch.empty(max(need, 1 << 16), dtype=torch.uint8).pin_memory()
    bad = ctypes.c_int64(-1)
    st = _lib.load().tise_resize_ragged_u8(ptrs.ctypes.data, hs.ctypes.data, ws.ctypes.data, n, _ptr(out), oh, ow, _FILTERS[filter],
                                           _ptr(ws_dev), need, slot[0].data_ptr(), ctypes.byref(bad), _stream())
    if st != _lib.TISE_OK:
        if bad.value >= 0:
            raise _lib.TiseStatusError(f"tise_resize_ragged_u8 (image {bad.value} of the batch, {int(hs[bad.value])} x {int(ws[bad.value])})",
                                       st, _lib.load().tise_status_string(st).decode())
        _lib.check("tise_resize_ragged_u8", st)
    slot[1] = torch.cuda.Event()
    slot[1].record(torch.cuda.current_stream(dev))
    return out


def _f32_out(n, oh, ow, channels_last, dev):
    if channels_last:
        store = torch.empty((n, oh, ow, 3), dtype=torch.float32, device=dev)
        return store, store.permute(0, 3, 1, 2)
    store = torch.empty((n, 3, oh, ow), dtype=torch.float32, device=dev)
    return store, store


def resize_f32(src_u8, out_hw=(299, 299), filter="bicubic", clip=(0, 255), sub=128, div=128, channels_last=True):
    """(N,H,W,3) uint8 CUDA tensor -> (N,3,oh,ow) fp32 network input of clean-fid's route (tise_resize_f32): every channel
    resampled as Pillow resamples a float32 (mode "F") image, NOT quantised, clipped to ``clip`` and mapped ``(x - sub) / div``
    in fp32.  Pillow's vertical-first rule (pillow_vertical_first) is applied here: the kernel takes the order as an argument.
    With ``channels_last`` the result is an NCHW tensor in torch.channels_last memory format (what the trunk's stem reads)."""
    _require_cuda(src_u8)
    if src_u8.dtype != torch.uint8 or src_u8.dim() != 4 or src_u8.shape[3] != 3:
        raise ValueError("src_u8 must be (N,H,W,3) uint8")
    oh, ow = out_hw
    src_u8 = src_u8.contiguous()
    n, h, w, _ = src_u8.shape
    store, out = _f32_out(n, oh, ow, channels_last, src_u8.device)
    _lib.call("tise_resize_f32", _ptr(src_u8), n, h, w, _ptr(store), oh, ow, 1 if channels_last else 0, _FILTERS[filter],
              float(clip[0]), float(clip[1]), float(sub), float(div), 1 if pillow_vertical_first(h, w, oh) else 0, _stream())
    return out


def resize_ragged_f32(crops, out_hw=(299, 299), filter="bicubic", clip=(0, 255), sub=128, div=128, channels_last=True):
    """List of (H_i,W_i,3) uint8 CUDA tensors of any sizes -> the (B,3,oh,ow) fp32 batch ``resize_f32`` gives image by image, bit
    for bit, in ONE launch (tise_resize_ragged_f32); Pillow's vertical-first rule is applied per image.  A size the plan builder
    refuses raises before anything of the batch is enqueued, naming the image."""
    if len(crops) == 0:
        raise ValueError("empty batch")
    oh, ow = out_hw
    dev = crops[0].device
    srcs = []
    for i, c in enumerate(crops):
        _require_cuda(c)
        if c.dim() == 4 and c.shape[0] == 1:
            c = c[0]
        if c.dtype != torch.uint8 or c.dim() != 3 or c.shape[2] != 3:
            raise ValueError(f"crop {i} must be (H,W,3) uint8")
        srcs.append(c.contiguous())
    n = len(srcs)
    store, out = _f32_out(n, oh, ow, channels_last, dev)
    ptrs = np.fromiter((c.data_ptr() for c in srcs), dtype=np.uint64, count=n)
    hs = np.fromiter((c.shape[0] for c in srcs), dtype=np.int32, count=n)
    ws = np.fromiter((c.shape[1] for c in srcs), dtype=np.int32, count=n)
    orders = np.fromiter((1 if pillow_vertical_first(c.shape[0], c.shape[1], oh) else 0 for c in srcs), dtype=np.int32, count=n)
    need = n * (64 + 4 * oh) + 16 * (n // 4096 + 1)
    ws_dev = torch.empty(need, dtype=torch.uint8, device=dev)
    # the pinned table ring of resize_ragged_u8: built in page-locked memory, copied asynchronously, two buffers in turn
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    ring = _RAGGED_TABLES.setdefault(key, [[None, None], [None, None]])
    slot = ring.pop(0)
    ring.append(slot)
    if slot[1] is not None:
        slot[1].synchronize()
    if slot[0] is None or slot[0].numel() < need:
        slot[0] = torch.empty(max(need, 1 << 16), dtype=torch.uint8).pin_memory()
    bad = ctypes.c_int64(-1)
    st = _lib.load().tise_resize_ragged_f32(ptrs.ctypes.data, hs.ctypes.data, ws.ctypes.data, orders.ctypes.data, n, _ptr(store), oh, ow,
                                            1 if channels_last else 0, _FILTERS[filter], float(clip[0]), float(clip[1]), float(sub),
                                            float(div), _ptr(ws_dev), need, slot[0].data_ptr(), ctypes.byref(bad), _stream())
    if st != _lib.TISE_OK:
        if bad.value >= 0:
            raise _lib.TiseStatusError(f"tise_resize_ragged_f32 (image {bad.value} of the batch, {int(hs[bad.value])} x {int(ws[bad.value])})",
                                       st, _lib.load().tise_status_string(st).decode())
        _lib.check("tise_resize_ragged_f32", st)
    slot[1] = torch.cuda.Event()
    slot[1].record(torch.cuda.current_stream(dev))
    return out


def resize_tf1_f32(src_u8, out_hw=(299, 299), sub=128, mul=2.0 ** -7, channels_last=True):
    """(N,H,W,3) uint8 CUDA tensor -> (N,3,oh,ow) fp32 network input of the ADM evaluator's route (tise_resize_tf1_f32):
    TensorFlow 1's legacy ResizeBilinear (float32, align_corners=False, no half-pixel centres, no antialiasing), then
    ``(v - sub) * mul``, every multiply and add a separate fp32 operation (tests/_tf1_resize_ref.py is the definition).  The
    kernel writes NHWC: with ``channels_last`` the result is its NCHW view (torch.channels_last memory format, what the trunk's
    stem reads); otherwise a contiguous NCHW copy."""
    _require_cuda(src_u8)
    if src_u8.dtype != torch.uint8 or src_u8.dim() != 4 or src_u8.shape[3] != 3:
        raise ValueError("src_u8 must be (N,H,W,3) uint8")
    oh, ow = (int(v) for v in out_hw)
    src_u8 = src_u8.contiguous()
    n, h, w, _ = src_u8.shape
    if h <= 0 or w <= 0 or oh <= 0 or ow <= 0:
        raise ValueError(f"resize_tf1_f32: sizes must be positive (got {h} x {w} -> {oh} x {ow})")
    store = torch.empty((n, oh, ow, 3), dtype=torch.float32, device=src_u8.device)
    if n:
        _lib.call("tise_resize_tf1_f32", _ptr(src_u8), n, h, w, _ptr(store), oh, ow, float(sub), float(mul), _stream())
    out = store.permute(0, 3, 1, 2)
    return out if channels_last else out.contiguous()


def resize_torch_f32(src_u8, out_hw=(299, 299), mul=2.0, sub=1.0, channels_last=True):
    """(N,H,W,3) uint8 CUDA tensor -> (N,3,oh,ow) fp32 network input of pytorch-fid's route (tise_resize_torch_f32): ToTensor's
    byte / 255, torch's float32 bilinear interpolation (align_corners=False, no antialiasing; the bits of torch's CPU kernel,
    tests/_torch_resize_ref.py is the definition), then ``v * mul - sub``.  The kernel writes NHWC: with ``channels_last`` the
    result is its NCHW view (torch.channels_last memory format, what the trunk's stem reads); otherwise a contiguous NCHW copy."""
    _require_cuda(src_u8)
    if src_u8.dtype != torch.uint8 or src_u8.dim() != 4 or src_u8.shape[3] != 3:
        raise ValueError("src_u8 must be (N,H,W,3) uint8")
    oh, ow = (int(v) for v in out_hw)
    src_u8 = src_u8.contiguous()
    n, h, w, _ = src_u8.shape
    if h <= 0 or w <= 0 or oh <= 0 or ow <= 0:
        raise ValueError(f"resize_torch_f32: sizes must be positive (got {h} x {w} -> {oh} x {ow})")
    store = torch.empty((n, oh, ow, 3), dtype=torch.float32, device=src_u8.device)
    if n:
        _lib.call("tise_resize_torch_f32", _ptr(src_u8), n, h, w, _ptr(store), oh, ow, float(mul), float(sub), _stream())
    out = store.permute(0, 3, 1, 2)
    return out if channels_last else out.contiguous()


_TORCH_IMAGE = np.dtype([("src", "<u8"), ("h", "<i4"), ("w", "<i4")])       # tise_torch_image_t (include/tise_hip.h)


def resize_ragged_torch_f32(crops, out_hw=(299, 299), mul=2.0, sub=1.0, channels_last=True):
    """List of (H_i,W_i,3) uint8 CUDA tensors of any sizes -> the (B,3,oh,ow) fp32 batch ``resize_torch_f32`` gives image by
    image, bit for bit, in ONE launch (tise_resize_ragged_torch_f32).  The (pointer, h, w) table is built in page-locked memory
    and copied on the current stream, in front of the launch; a wrong dtype or shape raises before anything is enqueued."""
    if len(crops) == 0:
        raise ValueError("empty batch")
    oh, ow = (int(v) for v in out_hw)
    if oh <= 0 or ow <= 0:
        raise ValueError(f"resize_ragged_torch_f32: sizes must be positive (got -> {oh} x {ow})")
    dev = crops[0].device
    srcs = []
    for i, c in enumerate(crops):
        _require_cuda(c)
        if c.dim() == 4 and c.shape[0] == 1:
            c = c[0]
        if c.dtype != torch.uint8 or c.dim() != 3 or c.shape[2] != 3 or c.shape[0] <= 0 or c.shape[1] <= 0:
            raise ValueError(f"crop {i} must be (H,W,3) uint8")
        srcs.append(c.contiguous())
    n = len(srcs)
    table = np.empty(n, dtype=_TORCH_IMAGE)
    table["src"] = np.fromiter((c.data_ptr() for c in srcs), dtype=np.uint64, count=n)
    table["h"] = np.fromiter((c.shape[0] for c in srcs), dtype=np.int32, count=n)
    table["w"] = np.fromiter((c.shape[1] for c in srcs), dtype=np.int32, count=n)
    # (torch's caching host allocator keeps the page-locked block until the copy that reads it has run)
    table_dev = torch.from_numpy(table.view(np.uint8)).pin_memory().to(dev, non_blocking=True)
    store = torch.empty((n, oh, ow, 3), dtype=torch.float32, device=dev)
    _lib.call("tise_resize_ragged_torch_f32", _ptr(table_dev), n, _ptr(store), oh, ow, float(mul), float(sub), _stream())
    out = store.permute(0, 3, 1, 2)
    return out if channels_last else out.contiguous()


def split_tap_rows(t, c0, nc, ld):
    """Channels [c0, c0 + nc) of a split tensor (N,H,W,2C) (conv_split.py) as fp32 rows (N, ld) (tise_split_tap_rows): row i
    holds ``conv_split.merge(t)[i, :, :, c0:c0+nc]`` flattened in h, w, c order -- the same bits -- and zeros from column
    H*W*nc on."""
    _require_cuda(t)
    if t.dtype != torch.float16 or t.dim() != 4 or t.shape[3] % 32 or not t.is_contiguous():
        raise ValueError("t must be a contiguous split tensor (N,H,W,2C) fp16 with C % 16 == 0")
    n, h, w, c2 = t.shape
    c0, nc, ld = int(c0), int(nc), int(ld)
    if h * w <= 0 or c0 < 0 or nc <= 0 or c0 + nc > c2 // 2 or ld < h * w * nc:
        raise ValueError(f"split_tap_rows: channels [{c0}, {c0 + nc}) of {c2 // 2} into rows of {ld} < {h * w * nc} columns"
                         if ld < h * w * nc else f"split_tap_rows: channels [{c0}, {c0 + nc}) outside 0..{c2 // 2}")
    out = torch.empty((n, ld), dtype=torch.float32, device=t.device)
    if n:
        _lib.call("tise_split_tap_rows", _ptr(t), n, h * w, c2 // 2, c0, nc, _ptr(out), ld, _stream())
    return out


def read_split_overflow():
    """Read-and-clear the range guard of the split-fp16 activation format (csrc/common.h): True when any kernel
    since the last read converted a value above the fp16 range (65504) into a split tensor.  A NaN raises it only in
    split_mean (the pool3 row); every other writer's ReLU turns a NaN into 0 first -- the trunks refuse non-finite parameters
    for that reason, and with finite parameters a NaN can only follow an overflow, which raises the flag.  Synchronises the
    current stream."""
    flag = ctypes.c_int(0)
    _lib.call("tise_split_overflow_check", ctypes.byref(flag), _stream())
    return bool(flag.value)


def check_split_overflow(what="InceptionV3 trunk", flag=None):
    """Raise when the range guard fired: the hi half would hold +inf and every later layer would be silently wrong."""
    if flag is None:
        flag = read_split_overflow()
    if flag:
        raise FloatingPointError(
            f"{what}: an activation exceeded the fp16 range of the split-precision format (|v| > 65504); "
            "the CLIs finish such a job on the exact-fp32 path by themselves (engine.run_with_exact_fallback); library callers: "
            "TISE_CONV=miopen / --conv exact")


class StatsAccumulator:
    """fp64 running {n, sum x, sum x x^T} on the device (tise_stats_* in include/tise_hip.h)."""

    def __init__(self, dims, device=None):
        self.dims = int(dims)
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda":
            raise _lib.TiseLibraryError("StatsAccumulator needs a HIP device")
        self._h = ctypes.c_void_p()
        self._pid = os.getpid()
        with torch.cuda.device(self.device):
            _lib.call("tise_stats_create", self.dims, ctypes.byref(self._h))
        self._keep = []

    def close(self):
        # Only the process that created the handle may destroy it: a forked child (a DataLoader worker of the ragged-crop
        # path) inherits this object, and when ITS garbage collector finalises an unreachable copy the destroy would call
        # hipFree in a process that must not touch the parent's HIP context (crash: "DataLoader worker exited unexpectedly")
        if self._h and os.getpid() == getattr(self, "_pid", None):
            _lib.load().tise_stats_destroy(self._h)
        self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        _lib.call("tise_stats_reset", self._h, _stream())

    def _check_feats(self, feats):
        _require_cuda(feats)
        if feats.dim() != 2 or feats.shape[1] != self.dims or feats.dtype != torch.float32:
            raise ValueError(f"feats must be (rows,{self.dims}) float32")
        return feats if feats.stride(1) == 1 else feats.contiguous()

    def update(self, feats):
        """feats: (rows, dims) fp32 CUDA tensor (row stride may exceed dims)."""
        feats = self._check_feats(feats)
        _lib.call("tise_stats_update", self._h, _ptr(feats), feats.shape[0], feats.stride(0), _stream())

    def update_parts(self, feats, cov=True, col_sum=True):
        """The two kernels of update() separately (bench.py brackets the MFMA one with HIP events); same checks as update()."""
        feats = self._check_feats(feats)
        if cov:
            _lib.call("tise_stats_update_cov", self._h, _ptr(feats), feats.shape[0], feats.stride(0), _stream())
        if col_sum:
            _lib.call("tise_stats_update_sum", self._h, _ptr(feats), feats.shape[0], feats.stride(0), _stream())

    def buffer(self):
        """The contiguous fp64 device buffer [S | s | n | pad] as a torch tensor VIEW (no copy);
        this is what the data-parallel driver all-reduces over RCCL."""
        p = ctypes.c_void_p()
        n = ctypes.c_size_t()
        _lib.call("tise_stats_buffer", self._h, ctypes.byref(p), ctypes.byref(n))
        return _wrap_device_doubles(p.value, n.value, self.device, owner=self)

    def count(self):
        return float(self.buffer()[self.dims * self.dims + self.dims].item())

    def finalize(self):
        """-> (mu (d,), sigma (d,d)) fp64 CUDA tensors; np.mean / np.cov(ddof=1) of everything fed."""
        mu = torch.empty(self.dims, dtype=torch.float64, device=self.device)
        sigma = torch.empty((self.dims, self.dims), dtype=torch.float64, device=self.device)
        _lib.call("tise_stats_finalize", self._h, _ptr(mu), _ptr(sigma), _stream())
        return mu, sigma


def stats_update_grouped(accs, feats_sorted, offsets):
    """ONE launch: rows [offsets[g], offsets[g + 1]) of ``feats_sorted`` (fp32 CUDA (rows, d), sorted by group) are folded into
    ``accs[g]`` (StatsAccumulator) for every g (tise_stats_update_grouped)."""
    _require_cuda(feats_sorted)
    ng = len(accs)
    if ng == 0:
        return
    if feats_sorted.dim() != 2 or feats_sorted.dtype != torch.float32 or feats_sorted.shape[1] != accs[0].dims:
        raise ValueError("feats_sorted must be (rows, dims) float32")
    if feats_sorted.stride(1) != 1:
        feats_sorted = feats_sorted.contiguous()
    offs = [int(o) for o in offsets]
    if len(offs) != ng + 1 or offs[0] != 0 or offs[-1] != feats_sorted.shape[0]:
        raise ValueError("offsets must run from 0 to the row count, one more entry than groups")
    handles = (ctypes.c_void_p * ng)(*[a._h for a in accs])
    arr = (ctypes.c_int64 * (ng + 1))(*offs)
    _lib.call("tise_stats_update_grouped", handles, ng, _ptr(feats_sorted), arr, feats_sorted.stride(0), _stream())


def mmd_offsets(offsets, limit, what):
    """Host check of one side's group offsets: n_groups + 1 ascending entries from >= 0 up to at most ``limit`` -> int64 array."""
    offs = np.asarray(offsets, dtype=np.int64).reshape(-1)
    if offs.size < 1 or offs[0] < 0 or np.any(np.diff(offs) < 0) or offs[-1] > limit:
        raise ValueError(f"{what}: offsets must ascend from >= 0 to at most {limit} (got {offs[:4].tolist()}.. {offs[-1:].tolist()})")
    return np.ascontiguousarray(offs)


def mmd_index(index, rows, what):
    """Host check of a row index BEFORE it is uploaded (the kernel trusts a device index: include/tise_hip.h): integers in
    [0, rows), one dimension -> contiguous int64 array.  Runs without a GPU."""
    if isinstance(index, torch.Tensor):
        if index.is_cuda:
            raise TypeError(f"{what}: pass the index as a host array; it is validated on the host and uploaded here")
        index = index.numpy()
    idx = np.asarray(index)
    if idx.ndim != 1 or not np.issubdtype(idx.dtype, np.integer):
        raise ValueError(f"{what}: the index must be a one-dimensional integer array")
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    if idx.size and (int(idx.min()) < 0 or int(idx.max()) >= rows):
        raise ValueError(f"{what}: index values must lie in [0, {rows}) (got {int(idx.min())} .. {int(idx.max())})")
    return idx


def _rows_side(t, what):
    """A (rows, d) float32 CUDA tensor as the gathered-row fetch of csrc/rows_tile.h needs it: unit column stride, row stride a
    multiple of 4 and >= d, 16-byte aligned base -- the tensor itself when it already is, else a copy (padded when d % 4 != 0)."""
    _require_cuda(t)
    if t.dim() != 2 or t.dtype != torch.float32:
        raise ValueError(f"{what} must be a (rows, d) float32 tensor")
    if t.shape[0] and (t.stride(1) != 1 or t.stride(0) % 4 or t.stride(0) < t.shape[1] or t.data_ptr() % 16):
        t = t.contiguous()
        if t.stride(0) % 4 or t.data_ptr() % 16:                 # d % 4 != 0: pad the rows to the fetch's alignment
            p = torch.zeros((t.shape[0], (t.shape[1] + 3) // 4 * 4), dtype=torch.float32, device=t.device)
            p[:, :t.shape[1]] = t
            t = p[:, :t.shape[1]]
    return t


class _RowsTileUser:
    """What the classes over the gathered-row tile (csrc/rows_tile.h) share on this side: the device check and one grow-only
    byte workspace."""

    def __init__(self, device=None):
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda":
            raise _lib.TiseLibraryError(f"{type(self).__name__} needs a HIP device")
        self._ws = None

    def _workspace(self, nbytes):
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = torch.empty(max(256, nbytes), dtype=torch.uint8, device=self.device)
        return self._ws


class _GroupedMMD(_RowsTileUser):
    """What the grouped kernel-sum entry points of csrc/mmd.hip share on this side: the host checks and ``sums``."""

    _FN = None                                                    # C ABI prefix: <_FN>_workspace_bytes, <_FN>_grouped

    def _kernel_args(self):
        """The kernel function's own arguments, between ``d`` and ``out_dev`` in the C signature."""
        return ()

    def sums(self, X, Y, offsets_x, offsets_y, index_x=None, index_y=None):
        """X (rows_x, d), Y (rows_y, d): fp32 CUDA tensors (row stride may exceed d).  offsets_*: n_groups + 1 host integers
        per side.  index_* (host integer arrays, optional): with an index, group g of that side is the rows
        index[offsets[g]:offsets[g + 1]], else the contiguous rows offsets[g]:offsets[g + 1].  -> (n_groups, 3) fp64 CUDA tensor
        [Sxx, Syy, Sxy]; the groups' sizes come back as two int64 arrays in ``last_counts``."""
        X, Y = _rows_side(X, "X"), _rows_side(Y, "Y")
        if X.shape[1] != Y.shape[1] or X.shape[1] < 1:
            raise ValueError("X and Y must have the same, positive number of columns")
        ix = mmd_index(index_x, X.shape[0], "index_x") if index_x is not None else None
        iy = mmd_index(index_y, Y.shape[0], "index_y") if index_y is not None else None
        ox = mmd_offsets(offsets_x, ix.size if ix is not None else X.shape[0], "offsets_x")
        oy = mmd_offsets(offsets_y, iy.size if iy is not None else Y.shape[0], "offsets_y")
        if ox.size != oy.size:
            raise ValueError("both sides need the same number of groups")
        ng = ox.size - 1
        self.last_counts = (np.diff(ox), np.diff(oy))
        out = torch.zeros((ng, 3), dtype=torch.float64, device=self.device)
        if ng == 0:
            return out
        with torch.cuda.device(self.device):
            ixd = torch.from_numpy(ix).to(self.device) if ix is not None else None           # ONE upload per side
            iyd = torch.from_numpy(iy).to(self.device) if iy is not None else None
            pox = ox.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
            poy = oy.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
            nbytes = ctypes.c_size_t()
            _lib.call(self._FN + "_workspace_bytes", pox, poy, ng, ctypes.byref(nbytes))
            ws = self._workspace(nbytes.value)
            _lib.call(self._FN + "_grouped",
                      _ptr(X), X.shape[0], X.stride(0) if X.shape[0] else X.shape[1] + (-X.shape[1]) % 4, _ptr(ixd) if ixd is not None else None,
                      ix.size if ix is not None else 0, pox,
                      _ptr(Y), Y.shape[0], Y.stride(0) if Y.shape[0] else Y.shape[1] + (-Y.shape[1]) % 4, _ptr(iyd) if iyd is not None else None,
                      iy.size if iy is not None else 0, poy, ng, int(X.shape[1]), *self._kernel_args(), _ptr(out), _ptr(ws),
                      ws.numel(), _stream())
        return out


class PolynomialMMD(_GroupedMMD):
    """Grouped sums of the KID kernel k(a, b) = (a.b / d + 1)^3 on resident fp32 rows (tise_mmd_poly3_grouped in
    include/tise_hip.h): every group's Sxx, Syy, Sxy from one launch pair, bitwise reproducible."""

    _FN = "tise_mmd_poly3"

    def mmd2(self, X, Y, offsets_x, offsets_y, index_x=None, index_y=None):
        """The unbiased estimator per group, Sxx / (n (n - 1)) + Syy / (m (m - 1)) - 2 Sxy / (n m): (n_groups,) fp64 CUDA tensor;
        NaN -- not an exception -- for a group with n < 2 or m < 2 (the callers decide what a skipped group means)."""
        s = self.sums(X, Y, offsets_x, offsets_y, index_x, index_y)
        n = torch.from_numpy(self.last_counts[0].astype(np.float64)).to(self.device)
        m = torch.from_numpy(self.last_counts[1].astype(np.float64)).to(self.device)
        v = s[:, 0] / (n * (n - 1.0)) + s[:, 1] / (m * (m - 1.0)) - 2.0 * s[:, 2] / (n * m)
        return torch.where((n < 2) | (m < 2), torch.full_like(v, float("nan")), v)


class GaussianMMD(_GroupedMMD):
    """Grouped sums of the Gaussian kernel k(a, b) = exp(-gamma |a - b|^2) on resident fp32 rows (tise_mmd_rbf_grouped in
    include/tise_hip.h): the kernel of CMMD (cmmd.py).  ``sums`` is PolynomialMMD's, argument for argument; the estimators over
    the sums are cmmd.cmmd_from_sums."""

    _FN = "tise_mmd_rbf"

    def __init__(self, device=None, gamma=None):
        if gamma is None or not np.isfinite(gamma) or gamma < 0:
            raise ValueError(f"gamma must be finite and >= 0 (got {gamma})")
        super().__init__(device)
        self.gamma = float(gamma)

    def _kernel_args(self):
        return (ctypes.c_double(self.gamma),)


class KnnManifold(_RowsTileUser):
    """k-nearest-neighbour radii, the precision / recall / density / coverage counts and the nearest row of another set on
    resident fp32 rows (tise_knn_radius2, tise_prdc_counts and tise_nn_argmin in include/tise_hip.h; csrc/knn.hip).  Owns the
    workspace; bitwise reproducible."""

    def radius2(self, X, k, col_splits=0):
        """X (n, d) fp32 CUDA tensor (row stride may exceed d), n >= k + 1, 1 <= k <= 16 -> (n,) fp64 CUDA tensor: the squared
        distance from every row to its k-th nearest OTHER row.  ``col_splits``: 0 = chosen by the library.  A row that holds a
        NaN or an infinity gets NaN and is no other row's neighbour (include/tise_hip.h, "Non-finite feature rows")."""
        X = _rows_side(X, "X")
        k, col_splits = int(k), int(col_splits)
        if X.shape[1] < 1:
            raise ValueError("X needs at least one column")
        if not 1 <= k <= 16 or X.shape[0] < k + 1:
            raise ValueError(f"radius2 needs 1 <= k <= 16 and at least k + 1 rows (got k = {k}, {X.shape[0]} rows)")
        r2 = torch.empty(X.shape[0], dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            nbytes = ctypes.c_size_t()
            _lib.call("tise_knn_workspace_bytes", X.shape[0], k, col_splits, ctypes.byref(nbytes))
            ws = self._workspace(nbytes.value)
            _lib.call("tise_knn_radius2", _ptr(X), X.shape[0], X.stride(0), int(X.shape[1]), k, col_splits, _ptr(r2), _ptr(ws),
                      ws.numel(), _stream())
        return r2

    def counts(self, R, r2R, F, r2F, col_splits=0):
        """R (n, d), F (m, d) fp32 CUDA tensors with their squared radii (fp64, from radius2) -> (cnt (n,) int32, rec (n,) bool,
        prec (m,) bool) CUDA tensors: cnt[i] = number of F rows strictly inside R_i's ball, rec[i] = R_i lies strictly inside
        some F row's ball, prec[j] = F_j lies strictly inside some R row's ball."""
        R, F = _rows_side(R, "R"), _rows_side(F, "F")
        if R.shape[1] != F.shape[1] or R.shape[1] < 1 or not R.shape[0] or not F.shape[0]:
            raise ValueError("R and F need rows and the same, positive number of columns")
        r2R = r2R.to(self.device, torch.float64).contiguous()
        r2F = r2F.to(self.device, torch.float64).contiguous()
        if r2R.shape != (R.shape[0],) or r2F.shape != (F.shape[0],):
            raise ValueError("one squared radius per row of each side")
        cnt = torch.empty(R.shape[0], dtype=torch.int32, device=self.device)
        rec = torch.empty(R.shape[0], dtype=torch.int32, device=self.device)
        prec = torch.empty(F.shape[0], dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            ws = self._workspace(8 * (R.shape[0] + F.shape[0]))
            _lib.call("tise_prdc_counts", _ptr(R), R.shape[0], R.stride(0), _ptr(r2R), _ptr(F), F.shape[0], F.stride(0), _ptr(r2F),
                      int(R.shape[1]), int(col_splits), _ptr(cnt), _ptr(rec), _ptr(prec), _ptr(ws), ws.numel(), _stream())
        return cnt, rec != 0, prec != 0

    def nearest(self, Q, B, exclude_diagonal=False, col_splits=0):
        """Q (n, d), B (m, d) fp32 CUDA tensors (row stride may exceed d) -> (d2 (n,) fp64, idx (n,) int32) CUDA tensors
        (tise_nn_argmin): the squared distance from every row of Q to its nearest row of B and that row's number, the smallest
        one on a tie.  ``exclude_diagonal``: the within-set pass -- row i skips base row i; needs n == m, and d2 then has the bits
        of ``radius2(k = 1)``.  The result does not depend on ``col_splits``.  A non-finite base row is nobody's nearest row; a
        non-finite query row gets (NaN, -1); a query row without any candidate (+inf, -1)."""
        Q, B = _rows_side(Q, "Q"), _rows_side(B, "B")
        if Q.shape[1] != B.shape[1] or Q.shape[1] < 1 or not Q.shape[0] or not B.shape[0]:
            raise ValueError("Q and B need rows and the same, positive number of columns")
        if exclude_diagonal and Q.shape[0] != B.shape[0]:
            raise ValueError(f"exclude_diagonal is the within-set pass: the row counts must agree (got {Q.shape[0]} and {B.shape[0]})")
        col_splits = int(col_splits)
        d2 = torch.empty(Q.shape[0], dtype=torch.float64, device=self.device)
        idx = torch.empty(Q.shape[0], dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            nbytes = ctypes.c_size_t()
            _lib.call("tise_nn_workspace_bytes", Q.shape[0], B.shape[0], col_splits, ctypes.byref(nbytes))
            ws = self._workspace(nbytes.value)
            _lib.call("tise_nn_argmin", _ptr(Q), Q.shape[0], Q.stride(0), _ptr(B), B.shape[0], B.stride(0), int(Q.shape[1]),
                      1 if exclude_diagonal else 0, col_splits, _ptr(d2), _ptr(idx), _ptr(ws), ws.numel(), _stream())
        return d2, idx


def _wrap_device_doubles(ptr, n, device, owner=None):
    """Zero-copy torch view of `n` doubles at device address `ptr` (__cuda_array_interface__)."""
    class _Holder:
        pass
    holder = _Holder()
    holder.__cuda_array_interface__ = {
        "shape": (int(n),), "typestr": "<f8", "data": (int(ptr), False), "version": 3, "strides": None,
    }
    holder._owner = owner
    t = torch.as_tensor(holder, device=device)
    return t


class FrechetSolver:
    """Device Frechet distance (tise_frechet_* in include/tise_hip.h)."""

    def __init__(self, dims, device=None):
        self.dims = int(dims)
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda":
            raise _lib.TiseLibraryError("FrechetSolver needs a HIP device")
        self._h = ctypes.c_void_p()
        self._pid = os.getpid()
        with torch.cuda.device(self.device):
            _lib.call("tise_frechet_create", self.dims, ctypes.byref(self._h))

    def close(self):
        if self._h and os.getpid() == getattr(self, "_pid", None):      # never from a forked child (StatsAccumulator.close)
            _lib.load().tise_frechet_destroy(self._h)
        self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _prep(self, t, shape):
        t = torch.as_tensor(t, dtype=torch.float64, device=self.device).contiguous()
        if tuple(t.shape) != shape:
            raise ValueError(f"expected shape {shape}, got {tuple(t.shape)}")
        return t

    def distance(self, mu1, sigma1, mu2, sigma2, diag_offset=0.0):
        """-> dict(fid, tr_covmean, diff2, tr1, tr2, rank, n_negative, flags); one device->host read."""
        d = self.dims
        mu1 = self._prep(mu1, (d,)); mu2 = self._prep(mu2, (d,))
        sigma1 = self._prep(sigma1, (d, d)); sigma2 = self._prep(sigma2, (d, d))
        out = torch.empty(_lib.TISE_FRECHET_OUT_DOUBLES, dtype=torch.float64, device=self.device)
        _lib.call("tise_frechet_distance", self._h, _ptr(mu1), _ptr(sigma1), _ptr(mu2), _ptr(sigma2),
                  float(diag_offset), _ptr(out), _stream())
        o = out.cpu().numpy()
        return {"fid": np.float64(o[0]), "tr_covmean": float(o[1]), "diff2": float(o[2]), "tr1": float(o[3]),
                "tr2": float(o[4]), "rank": int(o[5]), "n_negative": int(o[6]), "flags": int(o[7])}

    def prefactor(self, sigma, stream=None):
        """Start the pivoted Cholesky of ``sigma`` (d,d fp64 CUDA tensor, kept alive by the solver) on ``stream``
        (default: a private side stream, so it overlaps whatever the current stream is doing).  The host blocks
        until that stream has finished the factorisation (the numerical rank is read back), not the device."""
        sigma = self._prep(sigma, (self.dims, self.dims))
        if stream is None:
            if getattr(self, "_side", None) is None:
                self._side = torch.cuda.Stream(device=self.device)
            stream = self._side
        stream.wait_stream(torch.cuda.current_stream(self.device))        # sigma may still be in flight there
        self._pf_sigma = sigma
        _lib.call("tise_frechet_prefactor", self._h, _ptr(sigma), ctypes.c_void_p(stream.cuda_stream))
        sigma.record_stream(stream)
        return self

    def distance_prefactored(self, mu_f, mu_o, sigma_o):
        """Frechet distance between (mu_f, the sigma given to prefactor()) and (mu_o, sigma_o)."""
        d = self.dims
        if getattr(self, "_pf_sigma", None) is None:
            raise RuntimeError("prefactor() has not been called")
        mu_f = self._prep(mu_f, (d,)); mu_o = self._prep(mu_o, (d,))
        sigma_o = self._prep(sigma_o, (d, d))
        out = torch.empty(_lib.TISE_FRECHET_OUT_DOUBLES, dtype=torch.float64, device=self.device)
        _lib.call("tise_frechet_distance_prefactored", self._h, _ptr(mu_f), _ptr(self._pf_sigma), _ptr(mu_o), _ptr(sigma_o),
                  _ptr(out), _stream())
        o = out.cpu().numpy()
        return {"fid": np.float64(o[0]), "tr_covmean": float(o[1]), "diff2": float(o[2]), "tr1": float(o[3]),
                "tr2": float(o[4]), "rank": int(o[5]), "n_negative": int(o[6]), "flags": int(o[7])}

    def prefactor_ms(self):
        ms = ctypes.c_double()
        _lib.call("tise_frechet_prefactor_ms", self._h, ctypes.byref(ms))
        return ms.value

    def set_profiling(self, on=True):
        _lib.call("tise_frechet_set_profiling", self._h, 1 if on else 0)

    def phase_ms(self):
        """HIP-event phase times of the last distance() call: dict(pchol, gemm, sytrd, bisect, finish, rank)."""
        ms = (ctypes.c_double * 5)()
        r = ctypes.c_int()
        _lib.call("tise_frechet_phase_ms", self._h, ms, ctypes.byref(r))
        return {"pchol": ms[0], "gemm": ms[1], "sytrd": ms[2], "bisect": ms[3], "finish": ms[4], "rank": r.value}

    def eigvalsh(self, a):
        a = torch.as_tensor(a, dtype=torch.float64, device=self.device).contiguous()
        n = a.shape[0]
        w = torch.empty(n, dtype=torch.float64, device=self.device)
        _lib.call("tise_eigvalsh", self._h, _ptr(a), n, _ptr(w), _stream())
        return w

    def pivoted_cholesky(self, sigma):
        sigma = self._prep(sigma, (self.dims, self.dims))
        lt = torch.empty_like(sigma)
        r = ctypes.c_int()
        _lib.call("tise_pivoted_cholesky", self._h, _ptr(sigma), _ptr(lt), ctypes.byref(r), _stream())
        return lt, r.value

    def factor(self):
        """The factor prefactor() left: (L^T (d,d) fp64 CUDA tensor, rows >= rank zero; rank; unpivoted) where
        unpivoted tells which factorisation produced it (True: natural order, L^T upper triangular)."""
        if getattr(self, "_pf_sigma", None) is None:
            raise RuntimeError("prefactor() has not been called")
        lt = torch.empty((self.dims, self.dims), dtype=torch.float64, device=self.device)
        r, unpivoted = ctypes.c_int(), ctypes.c_int()
        _lib.call("tise_frechet_factor", self._h, _ptr(lt), ctypes.byref(r), ctypes.byref(unpivoted), _stream())
        return lt, r.value, bool(unpivoted.value)


class InceptionScoreAccumulator:
    """Per-split additive IS* sums on the device (tise_is_update / tise_is_finalize)."""

    RULES = {"coco": 0, "bird": 0, "ois": 1}

    def __init__(self, num_classes, n_total, temperature, splits=10, rule="coco", drop_first_class=False, device=None):
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda":
            raise _lib.TiseLibraryError("InceptionScoreAccumulator needs a HIP device")
        self.C = int(num_classes)
        self.drop = 1 if drop_first_class else 0
        self.Ce = self.C - self.drop
        self.n_total = int(n_total)
        self.T = float(temperature)
        self.splits = int(splits)
        self.rule = self.RULES[rule] if isinstance(rule, str) else int(rule)
        self.acc = torch.zeros(self.splits * (1 + self.Ce), dtype=torch.float64, device=self.device)
        self._ws = None

    def update(self, logits, idx_base):
        """logits: (rows, C) fp32 CUDA tensor whose rows have global indices idx_base..idx_base+rows-1."""
        _require_cuda(logits)
        if logits.dim() != 2 or logits.shape[1] != self.C or logits.dtype != torch.float32:
            raise ValueError(f"logits must be (rows,{self.C}) float32")
        if logits.stride(1) != 1:
            logits = logits.contiguous()
        rows = logits.shape[0]
        if self._ws is None or self._ws.numel() < 2 * rows:
            self._ws = torch.empty(2 * max(rows, 1024), dtype=torch.float64, device=self.device)
        _lib.call("tise_is_update", _ptr(logits), rows, logits.stride(0), self.C, self.T, self.drop, int(idx_base),
                  self.n_total, self.splits, self.rule, _ptr(self.acc), _ptr(self._ws), _stream())

    def finalize(self):
        """-> (mean, std, scores[splits]) as Python floats / numpy."""
        out = torch.empty(2 + self.splits, dtype=torch.float64, device=self.device)
        _lib.call("tise_is_finalize", _ptr(self.acc), self.Ce, self.n_total, self.splits, self.rule, _ptr(out), _stream())
        o = out.cpu().numpy()
        return float(o[0]), float(o[1]), o[2:].copy()


class CalibrationEvaluator:
    """NLL / dNLL/dT / ECE bins of temperature-scaled logits (tise_calib_eval): one pass over resident logits per call.

    logits: (rows, ld) fp32 CUDA tensor (row stride ld, unit column stride); the classes are columns [c0, c0 + C) with
    C = ld - c0 unless given.  labels: (rows,) integer class indices, kept on the device as int32; a non-integer dtype
    or a value outside int32 raises ValueError (a value inside int32 but outside [0, C) is the device's to count)."""

    def __init__(self, logits, labels, c0=0, num_classes=None, n_bins=15):
        _require_cuda(logits)
        if logits.dim() != 2 or logits.dtype != torch.float32 or logits.stride(1) != 1:
            raise ValueError("logits must be a (rows, C) float32 tensor with unit column stride")
        self.logits = logits
        self.rows = int(logits.shape[0])
        self.c0 = int(c0)
        self.C = int(num_classes) if num_classes is not None else int(logits.shape[1]) - self.c0
        if self.C < 1 or self.c0 < 0 or self.c0 + self.C > logits.shape[1]:
            raise ValueError(f"classes [{self.c0}, {self.c0 + self.C}) do not fit a row of {logits.shape[1]} logits")
        labels = torch.as_tensor(labels)
        if labels.shape != (self.rows,):
            raise ValueError(f"labels must have shape ({self.rows},), not {tuple(labels.shape)}")
        # the int32 conversion below wraps (2**32 + 3 -> 3) and truncates (1.7 -> 1): a label the device would have
        # counted as bad must not turn into a valid class on the way there
        if labels.dtype in (getattr(torch, "uint16", None), getattr(torch, "uint32", None)):
            labels = labels.to(torch.int64)
        if labels.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
            raise ValueError(f"labels must be integer class indices, not a {labels.dtype} tensor")
        if labels.dtype == torch.int64 and self.rows:
            lo, hi = (int(v) for v in torch.aminmax(labels))
            for v in (lo, hi):
                if not -2 ** 31 <= v < 2 ** 31:
                    raise ValueError(f"label {v} does not fit the device's int32 labels")
        self.labels = labels.to(logits.device, torch.int32).contiguous()
        self.n_bins = int(n_bins)
        # the reference's bin edges: torch.linspace(0, 1, n_bins + 1) in fp32 on the CPU (temperature_scaling.py:96)
        self.edges = torch.linspace(0, 1, self.n_bins + 1).to(logits.device)
        nbytes = ctypes.c_size_t()
        _lib.call("tise_calib_workspace_bytes", self.rows, self.C, self.n_bins, ctypes.byref(nbytes))
        self._ws = torch.empty(max(1, nbytes.value), dtype=torch.uint8, device=logits.device)
        self._out = torch.empty(4 + 3 * self.n_bins, dtype=torch.float64, device=logits.device)

    def raw(self, temperature):
        """One evaluation -> the 4 + 3 n_bins fp64 sums of tise_calib_eval (numpy)."""
        _lib.call("tise_calib_eval", _ptr(self.logits), self.rows, self.logits.stride(0), self.c0, self.C,
                  _ptr(self.labels), float(temperature), _ptr(self.edges), self.n_bins, _ptr(self._out),
                  _ptr(self._ws), self._ws.numel(), _stream())
        return self._out.cpu().numpy()

    def __call__(self, temperature):
        """-> dict(nll_sum, grad_sum, count, conf_sum, correct_sum); raises ValueError on a non-finite logit or a label
        outside [0, C) (the device counts such rows and leaves them out of every sum)."""
        o = self.raw(temperature)
        nb = self.n_bins
        if o[2] or o[3]:
            raise ValueError(f"calibration input: {int(o[2])} row(s) with a non-finite logit, {int(o[3])} row(s) with a "
                             f"label outside [0, {self.C})")
        return {"nll_sum": float(o[0]), "grad_sum": float(o[1]), "count": o[4:4 + nb].copy(),
                "conf_sum": o[4 + nb:4 + 2 * nb].copy(), "correct_sum": o[4 + 2 * nb:4 + 3 * nb].copy()}


def gemm_f64(a, b):
    """C = A @ B in fp64 through the MFMA tile kernel (any strides); test/bench helper."""
    _require_cuda(a, b)
    m, k = a.shape
    k2, n = b.shape
    assert k == k2 and a.dtype == torch.float64 and b.dtype == torch.float64
    c = torch.empty((m, n), dtype=torch.float64, device=a.device)
    _lib.call("tise_gemm_f64", _ptr(a), a.stride(0), a.stride(1), _ptr(b), b.stride(0), b.stride(1), _ptr(c), n,
              m, n, k, _stream())
    return c


def cosine_top1(img_emb, txt_emb, txt_index=None, normalize=True, logit_scale=100.0, want_p0=True):
    """Top-1 text retrieval (RP_coco.py:72-78 / PA.py:37-42) for all items at once.

    img_emb (n, d), txt_emb (rows, d): fp32 or fp16 device tensors; txt_index (n, c) int32 rows of txt_emb per item,
    candidate 0 = true caption (None: txt_emb is (n*c, d), item-major).  Returns (top1 int32 (n,), p0 fp32 (n,) or None).
    An item with a non-finite logit gets what the reference's np.argmax of all-NaN probabilities gives: top1 0, p0 NaN.
    Raises ValueError, before anything is launched, when txt_index names a row outside the table (one min/max
    reduction and a host sync per call) or when the contiguous form's table does not hold exactly n * c rows.
    """
    _require_cuda(img_emb, txt_emb, txt_index)
    assert img_emb.dim() == 2 and txt_emb.dim() == 2 and img_emb.shape[1] == txt_emb.shape[1]
    assert img_emb.dtype == txt_emb.dtype and img_emb.dtype in (torch.float32, torch.float16)
    img_emb, txt_emb = img_emb.contiguous(), txt_emb.contiguous()
    n, d = img_emb.shape
    if txt_index is not None:
        assert txt_index.dtype == torch.int32 and txt_index.dim() == 2 and txt_index.shape[0] == n
        txt_index = txt_index.contiguous()
        c = txt_index.shape[1]
        if txt_index.numel():
            lo, hi = (int(v) for v in torch.aminmax(txt_index))
            if lo < 0 or hi >= txt_emb.shape[0]:
                raise ValueError(f"txt_index holds values in [{lo}, {hi}]: outside the {txt_emb.shape[0]} rows of txt_emb")
    else:
        c = txt_emb.shape[0] // max(n, 1)
        if n and (c == 0 or c * n != txt_emb.shape[0]):
            raise ValueError(f"txt_emb has {txt_emb.shape[0]} rows: not n * c for n = {n} items")
    top1 = torch.empty(n, dtype=torch.int32, device=img_emb.device)
    p0 = torch.empty(n, dtype=torch.float32, device=img_emb.device) if want_p0 else None
    _lib.call("tise_cosine_top1", _ptr(img_emb), _ptr(txt_emb), _ptr(txt_index) if txt_index is not None else None,
              ctypes.c_int64(n), int(c), int(d), 0 if img_emb.dtype == torch.float32 else 1, 1 if normalize else 0,
              ctypes.c_float(logit_scale), _ptr(top1), _ptr(p0) if p0 is not None else None, _stream())
    return top1, p0


def paired_cosine(img_emb, txt_emb):
    """cos(img_emb[i], txt_emb[i]) for every row of two (n, d) device tables, fp16 or fp32 alike -> (n,) float64 on the device
    (csrc/clip_ops.hip, tise_paired_cosine: fp64 products and sums in a fixed order, one wave per row, no atomics -- two calls
    give the same bits, and no n x n product is formed).  A zero row gives NaN, as numpy's 0 / 0."""
    _require_cuda(img_emb, txt_emb)
    if img_emb.dim() != 2 or img_emb.shape != txt_emb.shape:
        raise ValueError(f"paired rows need two (n, d) tables of one shape (got {tuple(img_emb.shape)} and {tuple(txt_emb.shape)})")
    if img_emb.dtype != txt_emb.dtype or img_emb.dtype not in (torch.float32, torch.float16):
        raise ValueError(f"both tables fp16 or both fp32 (got {img_emb.dtype} and {txt_emb.dtype})")
    img_emb, txt_emb = img_emb.contiguous(), txt_emb.contiguous()
    n, d = img_emb.shape
    out = torch.empty(n, dtype=torch.float64, device=img_emb.device)
    if n == 0:                                                              # an empty shard: nothing to launch (and no pointer to pass)
        return out
    _lib.call("tise_paired_cosine", _ptr(img_emb), _ptr(txt_emb), ctypes.c_int64(n), int(d),
              1 if img_emb.dtype == torch.float16 else 0, _ptr(out), _stream())
    return out


_PAIR = np.dtype([("x", "<u8"), ("y", "<u8"), ("h", "<i4"), ("w", "<i4")])       # tise_pair_t (include/tise_hip.h)
SSIM_TAPS, SSIM_TILE, SSIM_MAX_SIDE, SSIM_MAX_PAIRS = 11, 64, 16384, 65535       # TISE_SSIM_* of the header


def _pair_images(xs, ys, what, min_side, dtypes):
    """Two (N,H,W,3) tensors or two lists of (H,W,3) tensors -> (x side, y side, dtype): a side stays ONE contiguous (N,H,W,3)
    tensor (no per-image work on the host) or becomes a list of contiguous images.  One dtype of ``dtypes`` for all, pair by
    pair one size, every side within min_side .. SSIM_MAX_SIDE, at most SSIM_MAX_PAIRS pairs.  A wrong dtype, shape or size
    raises before anything is enqueued."""
    if isinstance(xs, torch.Tensor) != isinstance(ys, torch.Tensor):
        raise ValueError(f"{what}: both sides a (N,H,W,3) tensor or both a list of (H,W,3) tensors")
    stacked = isinstance(xs, torch.Tensor)
    if stacked:
        if xs.dim() != 4 or xs.shape != ys.shape or xs.shape[3] != 3:
            raise ValueError(f"{what}: two (N,H,W,3) tensors of one shape (got {tuple(xs.shape)} and {tuple(ys.shape)})")
        pairs = [(xs, ys)]
    else:
        if len(xs) != len(ys):
            raise ValueError(f"{what}: {len(xs)} images on side one, {len(ys)} on side two")
        pairs = list(zip(xs, ys))
    if len(xs) == 0:
        raise ValueError("empty batch")
    if len(xs) > SSIM_MAX_PAIRS:
        raise ValueError(f"{what}: at most {SSIM_MAX_PAIRS} pairs per launch (got {len(xs)})")
    dtype = pairs[0][0].dtype
    if dtype not in dtypes:
        raise ValueError(f"{what}: images must be {' or '.join(str(d) for d in dtypes)} (got {dtype})")
    outx, outy = [], []
    for i, (a, b) in enumerate(pairs):
        _require_cuda(a, b)
        for t in (a, b):
            if t.dtype != dtype or t.dim() != (4 if stacked else 3) or t.shape[-1] != 3:
                raise ValueError(f"{what}: image {i} must be (H,W,3) {dtype} (got {tuple(t.shape)} {t.dtype})")
        if a.shape != b.shape:
            raise ValueError(f"{what}: pair {i} has two sizes ({a.shape[0]} x {a.shape[1]} and {b.shape[0]} x {b.shape[1]})")
        h, w = a.shape[-3], a.shape[-2]
        if min(h, w) < min_side:
            raise ValueError(f"{what}: pair {i} is {h} x {w}; the smaller side must be at least {min_side}")
        if max(h, w) > SSIM_MAX_SIDE:
            raise ValueError(f"{what}: pair {i} is {h} x {w}; a side may be at most {SSIM_MAX_SIDE}")
        outx.append(a.contiguous())
        outy.append(b.contiguous())
    return (outx[0], outy[0], dtype) if stacked else (outx, outy, dtype)


def _pair_geometry(side):
    """(pointers uint64, h int32, w int32) of the images of a side: a contiguous (N,H,W,3) tensor or a list of images."""
    if isinstance(side, torch.Tensor):
        n, h, w = side.shape[:3]
        step = h * w * 3 * side.element_size()
        return (np.uint64(side.data_ptr()) + np.arange(n, dtype=np.uint64) * np.uint64(step), np.full(n, h, dtype=np.int32),
                np.full(n, w, dtype=np.int32))
    n = len(side)
    return (np.fromiter((t.data_ptr() for t in side), dtype=np.uint64, count=n),
            np.fromiter((t.shape[0] for t in side), dtype=np.int32, count=n),
            np.fromiter((t.shape[1] for t in side), dtype=np.int32, count=n))


def _pair_table(xs, ys, dev):
    """The tise_pair_t table of the pairs on ``dev`` (built in page-locked memory, copied on the current stream in front of the
    launch that reads it) and the largest h and w."""
    px, hs, ws = _pair_geometry(xs)
    table = np.empty(len(px), dtype=_PAIR)
    table["x"], table["y"], table["h"], table["w"] = px, _pair_geometry(ys)[0], hs, ws
    # (torch's caching host allocator keeps the page-locked block until the copy that reads it has run)
    return torch.from_numpy(table.view(np.uint8)).pin_memory().to(dev, non_blocking=True), int(hs.max()), int(ws.max())


def _side_device(side):
    return side.device if isinstance(side, torch.Tensor) else side[0].device


def pair_sse_u8(xs, ys, out=None):
    """Two (N,H,W,3) uint8 CUDA tensors, or two lists of (H_i,W_i,3) uint8 CUDA tensors (pair by pair one size) -> (N,) int64 on
    the device: the sum over a pair's bytes of (x - y)^2, exact (tise_pair_sse_u8; one launch for the list).  ``out``: N int64 to
    write into."""
    xs, ys, _ = _pair_images(xs, ys, "pair_sse_u8", 1, (torch.uint8,))
    n, dev = len(xs), _side_device(xs)
    table, mh, mw = _pair_table(xs, ys, dev)
    if out is None:
        out = torch.empty(n, dtype=torch.int64, device=dev)
    elif out.dtype != torch.int64 or out.shape != (n,) or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"pair_sse_u8: out must be {n} contiguous int64 on {dev}")
    _lib.call("tise_pair_sse_u8", _ptr(table), ctypes.c_int64(n), mh, mw, _ptr(out), _stream())
    return out


def ssim_workspace_bytes(n, max_h, max_w):
    nb = ctypes.c_size_t(0)
    _lib.call("tise_ssim_workspace_bytes", ctypes.c_int64(n), int(max_h), int(max_w), ctypes.byref(nb))
    return nb.value


def ssim_pairs(xs, ys, out=None, workspace=None):
    """Two (N,H,W,3) CUDA tensors or two lists of (H_i,W_i,3) CUDA tensors, all uint8 (scale 1) or all float32 (a pyramid level),
    pair by pair one size, every side >= 11 -> (N,3,2) float64 on the device: per pair and channel the mean of the SSIM map and
    the mean of its contrast-structure (cs) map over the valid positions of the 11 x 11 Gaussian window (tise_ssim_pairs: fp64 in
    a fixed order, an identical pair gives exactly 1.0; one launch for the list).  ``out`` / ``workspace``: buffers to use
    ((N,3,2) float64; uint8 of at least ssim_workspace_bytes(N, max h, max w))."""
    xs, ys, dtype = _pair_images(xs, ys, "ssim_pairs", SSIM_TAPS, (torch.uint8, torch.float32))
    n, dev = len(xs), _side_device(xs)
    table, mh, mw = _pair_table(xs, ys, dev)
    need = ssim_workspace_bytes(n, mh, mw)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    elif workspace.dtype != torch.uint8 or workspace.numel() < need or not workspace.is_contiguous() or workspace.device != dev:
        raise ValueError(f"ssim_pairs: workspace must be at least {need} contiguous uint8 on {dev}")
    if out is None:
        out = torch.empty((n, 3, 2), dtype=torch.float64, device=dev)
    elif out.dtype != torch.float64 or out.shape != (n, 3, 2) or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"ssim_pairs: out must be ({n},3,2) contiguous float64 on {dev}")
    _lib.call("tise_ssim_pairs", _ptr(table), ctypes.c_int64(n), mh, mw, 1 if dtype == torch.float32 else 0, _ptr(out),
              _ptr(workspace), ctypes.c_size_t(workspace.numel()), _stream())
    return out


def pool2x2_sizes(xs):
    """Floats of the pooled level of every image of a list (or of a (N,H,W,3) tensor): (h // 2) * (w // 2) * 3."""
    return [(t.shape[0] // 2) * (t.shape[1] // 2) * 3 for t in xs]


def pool2x2_pairs(xs, ys, out=None):
    """Two (N,H,W,3) CUDA tensors or two lists of (H_i,W_i,3) CUDA tensors, uint8 or float32, every side >= 2 -> the next
    pyramid level of both sides as float32: the mean of every whole 2 x 2 block, (h // 2, w // 2, 3), a last odd row or column
    dropped; exact (tise_pool2x2_pairs, one launch for the list).  Tensors in, two (N,H//2,W//2,3) tensors out; lists in, two
    lists out -- views of ONE float32 store, side one's levels first (``out``: that store, 2 * sum(pool2x2_sizes(xs)) floats)."""
    xs, ys, dtype = _pair_images(xs, ys, "pool2x2_pairs", 2, (torch.uint8, torch.float32))
    n, dev = len(xs), _side_device(xs)
    _, hs, ws = _pair_geometry(xs)
    sizes = (hs // 2).astype(np.int64) * (ws // 2) * 3
    total = int(sizes.sum())
    if out is None:
        out = torch.empty(2 * total, dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or out.shape != (2 * total,) or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"pool2x2_pairs: out must be {2 * total} contiguous float32 on {dev}")
    if isinstance(xs, torch.Tensor):
        shape = (n, int(hs[0]) // 2, int(ws[0]) // 2, 3)
        ox, oy = out[:total].view(shape), out[total:].view(shape)
    else:
        ox, oy, at = [], [], 0
        for h, w, sz in zip(hs.tolist(), ws.tolist(), sizes.tolist()):
            ox.append(out[at:at + sz].view(h // 2, w // 2, 3))
            oy.append(out[total + at:total + at + sz].view(h // 2, w // 2, 3))
            at += sz
    table, mh, mw = _pair_table(xs, ys, dev)
    out_table, _, _ = _pair_table(ox, oy, dev)
    _lib.call("tise_pool2x2_pairs", _ptr(table), _ptr(out_table), ctypes.c_int64(n), mh, mw, 1 if dtype == torch.float32 else 0,
              _stream())
    return ox, oy


LPIPS_MAX_SIDE, LPIPS_MAX_PAIRS, LPIPS_WG_PIXELS, LPIPS_MAX_CHANNELS = 16384, 32767, 256, 512       # TISE_LPIPS_* of the header
# TISE_DISTS_* of the header
DISTS_MAX_SIDE, DISTS_MAX_PAIRS, DISTS_WG_PIXELS, DISTS_MAX_CHANNELS, DISTS_SUM_PIXELS = 16384, 32767, 512, 512, 4096


def _one_size_pairs(xs, ys, fn, max_pairs):
    """_pair_images' uint8 sides for a launch that takes pairs of ONE size, at most ``max_pairs`` -> (xs, ys, n, device, h, w)."""
    xs, ys, _ = _pair_images(xs, ys, fn, 1, (torch.uint8,))
    n, dev = len(xs), _side_device(xs)
    _, hs, ws = _pair_geometry(xs)
    h, w = int(hs[0]), int(ws[0])
    if bool((hs != h).any()) or bool((ws != w).any()):
        raise ValueError(f"{fn}: all pairs of a launch must have one size")
    if n > max_pairs:
        raise ValueError(f"{fn}: at most {max_pairs} pairs per launch (got {n})")
    return xs, ys, n, dev, h, w


def _require_split(x, fn, pairs=False):
    """A contiguous split tensor (N,H,W,2C), C % 16 == 0; ``pairs``: (2N,h,w,2C), both sides of N pairs."""
    if x.dtype != torch.float16 or x.dim() != 4 or (pairs and x.shape[0] % 2) or x.shape[3] % 32 or not x.is_contiguous():
        raise ValueError(f"{fn}: a contiguous split tensor {'(2N,h,w,2C)' if pairs else '(N,H,W,2C)'} fp16, C % 16 == 0 "
                         f"(got {tuple(x.shape)} {x.dtype})")


def _pool_split(fn, symbol, min_side, out_side, x, out, out_off, x_off, channels):
    """The body of a split-tensor pool: (N,H,W,2C) -> (N,out_side(H),out_side(W),2C') through the C entry point ``symbol``."""
    _require_cuda(x)
    _require_split(x, fn)
    n, h, w, c2 = x.shape
    if h < min_side or w < min_side:
        raise ValueError(f"{fn}: both sides must be at least {min_side} (got {h} x {w})")
    oh, ow = out_side(h), out_side(w)
    c = c2 // 2 - x_off if channels is None else int(channels)
    if out is None:
        out = torch.empty((n, oh, ow, 2 * (out_off + c)), dtype=torch.float16, device=x.device)
    elif (out.dtype != torch.float16 or out.dim() != 4 or out.shape[:3] != (n, oh, ow) or out.shape[3] % 32
          or not out.is_contiguous() or out.device != x.device):
        raise ValueError(f"{fn}: out must be a contiguous split tensor ({n},{oh},{ow},2C') on {x.device}")
    _lib.call(symbol, _ptr(x), c2 // 2, int(x_off), n, h, w, c, _ptr(out), out.shape[3] // 2, int(out_off), _stream())
    return out


def _layer_buffers(fn, out, workspace, n, dev, need):
    """The ``out`` and ``workspace`` arguments of a *_layer call on N pairs -> the workspace to use (a fresh one of ``need()``
    bytes by default), or None when N == 0 and there is nothing to launch."""
    if out.dtype != torch.float64 or out.shape != (n,) or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"{fn}: out must be {n} contiguous float64 on {dev}")
    if n == 0:
        return None
    need = need()
    if workspace is None:
        return torch.empty(need, dtype=torch.uint8, device=dev)
    if workspace.dtype != torch.uint8 or workspace.numel() < need or not workspace.is_contiguous() or workspace.device != dev:
        raise ValueError(f"{fn}: workspace must be at least {need} contiguous uint8 on {dev}")
    return workspace


def lpips_input_split(xs, ys, lut, out=None):
    """Two (N,H,W,3) uint8 CUDA tensors or two lists of (H,W,3) uint8 CUDA tensors, ALL of one size, and the (3,256) float32
    input table -> the split tensor (2N,H,W,64) fp16 conv1_1 reads (tise_lpips_input_split): images 0..N-1 side one, N..2N-1
    side two; channels 0..2 = lut[c][byte] in split form, channels 3..31 zero in both halves."""
    xs, ys, n, dev, h, w = _one_size_pairs(xs, ys, "lpips_input_split", LPIPS_MAX_PAIRS)
    _require_cuda(lut)
    if lut.dtype != torch.float32 or lut.shape != (3, 256) or not lut.is_contiguous() or lut.device != dev:
        raise ValueError(f"lpips_input_split: the table must be (3,256) contiguous float32 on {dev}")
    if out is None:
        out = torch.empty((2 * n, h, w, 64), dtype=torch.float16, device=dev)
    elif out.dtype != torch.float16 or out.shape != (2 * n, h, w, 64) or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"lpips_input_split: out must be ({2 * n},{h},{w},64) contiguous float16 on {dev}")
    table, _, _ = _pair_table(xs, ys, dev)
    _lib.call("tise_lpips_input_split", _ptr(table), ctypes.c_int64(n), h, w, _ptr(lut), _ptr(out), _stream())
    return out


def maxpool2s2_split(x, out=None, out_off=0, x_off=0, channels=None):
    """max_pool2d(2, stride 2) (floor) of ``channels`` channels from ``x_off`` of a split tensor (N,H,W,2C) into the channels from
    ``out_off`` of a split tensor (N,H//2,W//2,2C') (tise_maxpool2s2_split_nhwc; default: all channels into a fresh tensor)."""
    return _pool_split("maxpool2s2_split", "tise_maxpool2s2_split_nhwc", 2, lambda s: s // 2, x, out, out_off, x_off, channels)


def lpips_workspace_bytes(n, h, w):
    nb = ctypes.c_size_t(0)
    _lib.call("tise_lpips_workspace_bytes", ctypes.c_int64(n), int(h), int(w), ctypes.byref(nb))
    return nb.value


def lpips_layer(feat, weight, out, workspace=None):
    """One LPIPS tap: split features (2N,h,w,2C) fp16 (images 0..N-1 side one, N..2N-1 side two), ``weight`` C float32 ->
    out[i] += mean over the pixels of sum_c w_c (a_c / n(a) - b_c / n(b))^2, n(v) = sqrt(sum_c v_c^2) + 1e-10 (tise_lpips_layer:
    fp64 in a fixed order, no atomics; an identical pair adds exactly 0.0).  ``out``: N float64, ``workspace``: uint8 of at least
    lpips_workspace_bytes(N, h, w)."""
    _require_cuda(feat, weight, out)
    _require_split(feat, "lpips_layer", pairs=True)
    if feat.shape[3] // 2 > LPIPS_MAX_CHANNELS:
        raise ValueError(f"lpips_layer: at most {LPIPS_MAX_CHANNELS} channels (got {feat.shape[3] // 2})")
    n, h, w, c = feat.shape[0] // 2, feat.shape[1], feat.shape[2], feat.shape[3] // 2
    dev = feat.device
    if weight.dtype != torch.float32 or weight.shape != (c,) or not weight.is_contiguous() or weight.device != dev:
        raise ValueError(f"lpips_layer: weight must be {c} contiguous float32 on {dev}")
    workspace = _layer_buffers("lpips_layer", out, workspace, n, dev, lambda: lpips_workspace_bytes(n, h, w))
    if workspace is not None:
        _lib.call("tise_lpips_layer", _ptr(feat), ctypes.c_int64(n), h, w, c, _ptr(weight), _ptr(out), _ptr(workspace),
                  ctypes.c_size_t(workspace.numel()), _stream())
    return out


def l2pool3s2_split(x, out=None, out_off=0, x_off=0, channels=None):
    """DISTS's L2 (Hanning) pool, sqrt(conv(x^2, [[1,2,1],[2,4,2],[1,2,1]] / 16, stride 2, zero padding 1) + 1e-12), of ``channels``
    channels from ``x_off`` of a split tensor (N,H,W,2C) into the channels from ``out_off`` of a split tensor
    (N,ceil(H/2),ceil(W/2),2C') (tise_l2pool3s2_split_nhwc: fp64 in a fixed order, one rounding to fp32, split again; default: all
    channels into a fresh tensor)."""
    return _pool_split("l2pool3s2_split", "tise_l2pool3s2_split_nhwc", 1, lambda s: (s + 1) // 2, x, out, out_off, x_off, channels)


def dists_workspace_bytes(n, h, w, c):
    nb = ctypes.c_size_t(0)
    _lib.call("tise_dists_workspace_bytes", ctypes.c_int64(n), int(h), int(w), int(c), ctypes.byref(nb))
    return nb.value


def dists_layer(feat, alpha, beta, out, workspace=None):
    """One DISTS stage: split features (2N,h,w,2C) fp16 (images 0..N-1 side one, N..2N-1 side two), ``alpha`` and ``beta`` C float64
    each (already divided by sum alpha + sum beta) -> out[i] += sum_c alpha_c (1 - S1_c) + beta_c (1 - S2_c), S1 and S2 from the
    per-channel means, centered variances and covariance over the pixels (tise_dists_layer: fp64 in a fixed order, two passes, no
    atomics; an identical pair adds exactly 0.0).  ``out``: N float64, ``workspace``: uint8 of at least
    dists_workspace_bytes(N, h, w, C)."""
    _require_cuda(feat, alpha, beta, out)
    _require_split(feat, "dists_layer", pairs=True)
    if feat.shape[3] // 2 > DISTS_MAX_CHANNELS:
        raise ValueError(f"dists_layer: at most {DISTS_MAX_CHANNELS} channels (got {feat.shape[3] // 2})")
    n, h, w, c = feat.shape[0] // 2, feat.shape[1], feat.shape[2], feat.shape[3] // 2
    dev = feat.device
    for name, t in (("alpha", alpha), ("beta", beta)):
        if t.dtype != torch.float64 or t.shape != (c,) or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"dists_layer: {name} must be {c} contiguous float64 on {dev}")
    workspace = _layer_buffers("dists_layer", out, workspace, n, dev, lambda: dists_workspace_bytes(n, h, w, c))
    if workspace is not None:
        _lib.call("tise_dists_layer", _ptr(feat), ctypes.c_int64(n), h, w, c, _ptr(alpha), _ptr(beta), _ptr(out), _ptr(workspace),
                  ctypes.c_size_t(workspace.numel()), _stream())
    return out


def dists_image_sums(xs, ys, out=None):
    """Two (N,H,W,3) uint8 CUDA tensors or two lists of (H,W,3) uint8 CUDA tensors, ALL of one size -> (N,3,5) int64 on the
    device: per pair and colour the sums over the pixels of bx, by, bx^2, by^2, bx by (tise_dists_image_sums_u8: exact) -- DISTS's
    stage 0, from which the host forms S1 and S2."""
    xs, ys, n, dev, h, w = _one_size_pairs(xs, ys, "dists_image_sums", DISTS_MAX_PAIRS)
    if out is None:
        out = torch.empty((n, 3, 5), dtype=torch.int64, device=dev)
    elif out.dtype != torch.int64 or out.shape != (n, 3, 5) or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"dists_image_sums: out must be ({n},3,5) contiguous int64 on {dev}")
    table, _, _ = _pair_table(xs, ys, dev)
    _lib.call("tise_dists_image_sums_u8", _ptr(table), ctypes.c_int64(n), h, w, _ptr(out), _stream())
    return out


# ---- ResNet (csrc/resnet.hip, the 7 x 7 stem of csrc/conv_pipe.hip; resnet_hip.py) --------------------------------------------

def _require_u8_batch(x, fn):
    _require_cuda(x)
    if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3 or x.stride(3) != 1 or x.stride(2) != 3 \
            or x.stride(1) != 3 * x.shape[2] or (x.shape[0] > 1 and x.stride(0) != 3 * x.shape[1] * x.shape[2]):
        raise ValueError(f"{fn}: a dense (N,H,W,3) uint8 batch (got {tuple(x.shape)} {x.dtype}, strides {tuple(x.stride())})")


def _require_table(lut, dev, fn):
    _require_cuda(lut)
    if lut.dtype != torch.float32 or lut.shape != (3, 256) or not lut.is_contiguous() or lut.device != dev:
        raise ValueError(f"{fn}: the table must be (3,256) contiguous float32 on {dev}")


def stem_conv7x7s2_supported(x):
    """Whether tise_stem_conv7x7s2_split_u8_mfma takes this dense (N,H,W,3) uint8 batch: any address, H and W >= 1, fewer than
    2^31 - 256 output pixels (the header's refusals, mirrored so that a caller can choose its route before any launch)."""
    n, h, w, _ = x.shape
    return h >= 1 and w >= 1 and n * ((h - 1) // 2 + 1) * ((w - 1) // 2 + 1) < 0x7fffff00


def stem_conv7x7s2_split_u8(x, lut, wsplit, scale, bias, out=None):
    """ResNet's stem on the matrix cores (tise_stem_conv7x7s2_split_u8_mfma): a dense (N,H,W,3) uint8 batch at any address and the
    (3,256) table -> the split tensor (N,(H-1)//2+1,(W-1)//2+1,128) fp16 of max(scale conv + bias, 0), zero padding 3 of the table
    values.  ``wsplit``: 28672 fp16 in the kernel's order (resnet_hip.pack_stem7_mfma), ``scale`` / ``bias``: 64 fp32."""
    _require_u8_batch(x, "stem_conv7x7s2_split_u8")
    _require_table(lut, x.device, "stem_conv7x7s2_split_u8")
    n, h, w, _ = x.shape
    if wsplit.dtype != torch.float16 or wsplit.numel() != 28672 or not wsplit.is_contiguous() or wsplit.device != x.device:
        raise ValueError("stem_conv7x7s2_split_u8: wsplit must be 28672 contiguous float16 on the batch's device")
    for t in (scale, bias):
        if t.dtype != torch.float32 or t.shape != (64,) or not t.is_contiguous() or t.device != x.device:
            raise ValueError("stem_conv7x7s2_split_u8: scale and bias must be 64 contiguous float32 on the batch's device")
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    if out is None:
        out = torch.empty((n, oh, ow, 128), dtype=torch.float16, device=x.device)
    elif out.dtype != torch.float16 or out.shape != (n, oh, ow, 128) or not out.is_contiguous() or out.device != x.device:
        raise ValueError(f"stem_conv7x7s2_split_u8: out must be ({n},{oh},{ow},128) contiguous float16 on {x.device}")
    _lib.call("tise_stem_conv7x7s2_split_u8_mfma", _ptr(x), _ptr(lut), n, h, w, _ptr(wsplit), _ptr(scale), _ptr(bias), _ptr(out), _stream())
    return out


def resnet_input_split(x, lut, out=None):
    """A dense (N,H,W,3) uint8 batch at any address and the (3,256) table -> the split tensor (N,H,W,64) fp16 a 32-channel first
    layer reads (tise_resnet_input_split): channels 0..2 = lut[c][byte] in split form, channels 3..31 zero in both halves."""
    _require_u8_batch(x, "resnet_input_split")
    _require_table(lut, x.device, "resnet_input_split")
    n, h, w, _ = x.shape
    if out is None:
        out = torch.empty((n, h, w, 64), dtype=torch.float16, device=x.device)
    elif out.dtype != torch.float16 or out.shape != (n, h, w, 64) or not out.is_contiguous() or out.device != x.device:
        raise ValueError(f"resnet_input_split: out must be ({n},{h},{w},64) contiguous float16 on {x.device}")
    _lib.call("tise_resnet_input_split", _ptr(x), _ptr(lut), n, h, w, _ptr(out), _stream())
    return out


def resize_u8_filter_only(src_u8, out_hw, filter="bicubic"):
    """(N,H,W,3) uint8 CUDA tensor -> the Pillow-exact resized uint8 image (N,oh,ow,3) for ``filter`` "bilinear" or "bicubic"
    (tise_resize_u8 with no float output: the bytes ``resize_u8_lut(..., return_u8=True)`` returns)."""
    _require_cuda(src_u8)
    if src_u8.dtype != torch.uint8 or src_u8.dim() != 4 or src_u8.shape[3] != 3:
        raise ValueError("src_u8 must be (N,H,W,3) uint8")
    oh, ow = (int(v) for v in out_hw)
    src_u8 = _vertical_pass_first(src_u8.contiguous(), oh, filter)
    n, h, w, _ = src_u8.shape
    u8 = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device=src_u8.device)
    _lib.call("tise_resize_u8", _ptr(src_u8), n, h, w, None, oh, ow, 1, _IDENTITY_LUT.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
              _ptr(u8), _FILTERS[filter], _stream())
    return u8


def maxpool3s2p1_split(x, out=None, out_off=0, x_off=0, channels=None):
    """max_pool2d(3, stride 2, padding 1) of ``channels`` channels from ``x_off`` of a split tensor (N,H,W,2C) into the channels from
    ``out_off`` of a split tensor (N,(H-1)//2+1,(W-1)//2+1,2C') (tise_maxpool3s2p1_split_nhwc; default: all channels into a fresh
    tensor).  The padding does not take part: an all-negative window keeps its largest value."""
    return _pool_split("maxpool3s2p1_split", "tise_maxpool3s2p1_split_nhwc", 1, lambda s: (s - 1) // 2 + 1, x, out, out_off, x_off, channels)


def residual_relu_split(raw, bias, identity, id_bias=None, out=None, raw_off=0, id_off=0, out_off=0, channels=None):
    """The end of a bottleneck block (tise_residual_relu_split_nhwc): out = split(max((raw + bias) + u, 0)) in fp32, in that order.
    ``raw``: fp32 (..., Cr) -- a convolution's mode-1 output -- channels from ``raw_off``; ``bias``: C fp32.  ``identity``: a split
    tensor (..., 2 Ci) fp16 (u = hi + lo 2^-11, ``id_bias`` None) or fp32 (..., Ci) with ``id_bias`` (u = identity + id_bias),
    channels from ``id_off``.  ``out``: a split tensor (..., 2 Co), channels from ``out_off`` (default: a fresh one of C channels).
    The leading dimensions of the three tensors must agree.  The range guard is raised where the sum is NaN or beyond +-65504."""
    _require_cuda(raw, bias, identity, id_bias, out)
    if raw.dtype != torch.float32 or raw.dim() < 2 or not raw.is_contiguous():
        raise ValueError("residual_relu_split: raw must be contiguous float32 (..., C)")
    lead = tuple(raw.shape[:-1])
    pixels = 1
    for s in lead:
        pixels *= int(s)
    c = raw.shape[-1] - raw_off if channels is None else int(channels)
    if bias.dtype != torch.float32 or bias.shape != (c,) or not bias.is_contiguous():
        raise ValueError(f"residual_relu_split: bias must be {c} contiguous float32")
    split_id = identity.dtype == torch.float16
    if split_id == (id_bias is not None) or identity.dtype not in (torch.float16, torch.float32) or not identity.is_contiguous() \
            or tuple(identity.shape[:-1]) != lead:
        raise ValueError("residual_relu_split: identity is a contiguous split tensor (fp16, no id_bias) or fp32 with id_bias, of raw's "
                         "leading dimensions")
    if id_bias is not None and (id_bias.dtype != torch.float32 or id_bias.shape != (c,) or not id_bias.is_contiguous()):
        raise ValueError(f"residual_relu_split: id_bias must be {c} contiguous float32")
    if out is None:
        out = torch.empty(lead + (2 * (out_off + c),), dtype=torch.float16, device=raw.device)
    elif out.dtype != torch.float16 or tuple(out.shape[:-1]) != lead or not out.is_contiguous() or out.device != raw.device:
        raise ValueError("residual_relu_split: out must be a contiguous split tensor of raw's leading dimensions on its device")
    null = ctypes.c_void_p(None)
    if split_id:
        ids = (_ptr(identity), ctypes.c_int64(identity.shape[-1] // 2), int(id_off), null, ctypes.c_int64(0), 0, null)
    else:
        ids = (null, ctypes.c_int64(0), 0, _ptr(identity), ctypes.c_int64(identity.shape[-1]), int(id_off), _ptr(id_bias))
    _lib.call("tise_residual_relu_split_nhwc", _ptr(raw), ctypes.c_int64(raw.shape[-1]), int(raw_off), _ptr(bias), *ids,
              ctypes.c_int64(pixels), c, _ptr(out), ctypes.c_int64(out.shape[-1] // 2), int(out_off), _stream())
    return out


# ---- counting alignment (csrc/countseg.hip; countseg_hip.py) --------------------------------------------------------------------
COUNTSEG_MAX_PIXELS, COUNTSEG_MAX_WIDTH, COUNTSEG_MAX_CLASSES, COUNTSEG_MAX_IMAGES, COUNTSEG_CLASS_GROUP = 1024, 1024, 4096, 65535, 4


def countseg_head(mix, b_mix, w_cls, b_cls, w_den, b_den, off=0, want_maps=False):
    """CountSeg's two branches and peak stimulation (tise_countseg_head) on ``mix``: the raw fp32 result (N,h,w,ld) of the mix
    convolution (SplitConv mode 1: scale * conv, no bias), channels [off, off + 2P).  ``b_mix``: 2P fp32; ``w_cls`` / ``w_den``:
    (C,P) fp32; ``b_cls`` / ``b_den``: C fp32.  -> (conf (N,C) fp64, den (N,C) fp64, peaks (N,C) int32[, maps (N,2C,h w) fp64: the
    class maps, then the density maps]).  conf = the mean of the local maxima of a class map that reach its lower median, den = the
    mean of a density map; a NaN in a class map gives conf NaN and 0 peaks for that image and class only.  h w <= 1024."""
    _require_cuda(mix, b_mix, w_cls, b_cls, w_den, b_den)
    if mix.dtype != torch.float32 or mix.dim() != 4 or not mix.is_contiguous():
        raise ValueError(f"countseg_head: mix must be contiguous float32 (N,h,w,ld) (got {tuple(mix.shape)} {mix.dtype})")
    n, h, w, ld = mix.shape
    dev = mix.device
    if w_cls.dim() != 2:
        raise ValueError("countseg_head: w_cls must be (C,P) float32")
    c, p = w_cls.shape
    if h * w > COUNTSEG_MAX_PIXELS:
        raise ValueError(f"countseg_head: at most {COUNTSEG_MAX_PIXELS} pixels per map (got {h} x {w})")
    for name, t, shape in (("b_mix", b_mix, (2 * p,)), ("w_cls", w_cls, (c, p)), ("b_cls", b_cls, (c,)), ("w_den", w_den, (c, p)),
                           ("b_den", b_den, (c,))):
        if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"countseg_head: {name} must be {shape} contiguous float32 on {dev}")
    conf = torch.empty((n, c), dtype=torch.float64, device=dev)
    den = torch.empty((n, c), dtype=torch.float64, device=dev)
    peaks = torch.empty((n, c), dtype=torch.int32, device=dev)
    maps = torch.empty((n, 2 * c, h * w), dtype=torch.float64, device=dev) if want_maps else None
    _lib.call("tise_countseg_head", _ptr(mix), ctypes.c_int64(ld), int(off), _ptr(b_mix), _ptr(w_cls), _ptr(b_cls), _ptr(w_den),
              _ptr(b_den), ctypes.c_int64(n), h, w, p, c, _ptr(conf), _ptr(den), _ptr(peaks),
              _ptr(maps) if want_maps else ctypes.c_void_p(None), _stream())
    return (conf, den, peaks, maps) if want_maps else (conf, den, peaks)
