"""The two kernels of tise_jpeg_reconstruct_rgb8 (csrc/jpeg_idct.hip) alone: a batch of coefficient slots resident in HBM,
reconstructed repeatedly; device-event time per call, bytes moved per call and the rate against a device-to-device copy
measured in the same process.  Run it under ``rocprofv3 --kernel-trace --stats -- python tools/jpeg_kernel_probe.py`` for
the split between jpeg_idct_kernel and jpeg_colour_kernel (result: profiles/*_jpeg_kernel_stats.txt).

Bytes per call (algorithmic): coefficients read (2 per sample) + planes written and read again (1 + 1 per sample) + RGB
written (3 per pixel); per kernel: A = coefficients + planes written, B = planes read + RGB written."""
import argparse
import ctypes
import io
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    import torch
    from PIL import Image
    from tise_toolbox_amd import _lib, jpeg_feed
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from jpeg_feed_probe import synthetic
    lib = jpeg_feed.load_decoder()
    dev = torch.device("cuda", 0)
    # the copy rate of this box: 1 GiB device to device (read + write)
    a, b = torch.empty(1 << 30, dtype=torch.uint8, device=dev), torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    b.copy_(a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    copy_rate = 10 * 2 * (1 << 30) / (e0.elapsed_time(e1) * 1e-3)
    print(f"device-to-device copy: {copy_rate / 1e12:.2f} TB/s (read + write)", flush=True)
    del a, b
    for name, n, sizes in (("50 x 256x256 (one loader batch)", 50, [(256, 256)]), ("1000 x 256x256", 1000, [(256, 256)]),
                           ("50 ragged 640x480 / 500x375 / 480x640 / 375x500", 50, [(640, 480), (500, 375), (480, 640), (375, 500)])):
        blobs = []
        for (w, h) in sizes:
            buf = io.BytesIO()
            Image.fromarray(synthetic(1, h, w, seed=w)[0]).save(buf, "JPEG", quality=75, subsampling=2)
            blobs.append((buf.getvalue(), w, h))
        sb = max(int(lib.tise_jpeg_slot_bytes(w, h, 3)) for _, w, h in blobs)
        arena = np.zeros((n, sb), dtype=np.uint8)
        offs, pos, samples, pixels = np.zeros(n, dtype=np.int64), 0, 0, 0
        for i in range(n):
            blob, w, h = blobs[i % len(blobs)]
            assert lib.tise_jpeg_entropy_decode(blob, len(blob), arena[i].ctypes.data, sb, None, None) == 0
            offs[i] = pos
            pos += (h * w * 3 + 15) & ~15
            samples += int(arena[i, :64].view(np.int32)[12]) // 2
            pixels += h * w
        raw = torch.from_numpy(arena.reshape(-1)).to(dev)
        out = torch.empty(pos, dtype=torch.uint8, device=dev)
        wsb = ctypes.c_size_t()
        _lib.call("tise_jpeg_workspace_bytes", n, sb, ctypes.byref(wsb))
        ws = torch.empty(wsb.value, dtype=torch.uint8, device=dev)
        table = torch.empty(n * 64, dtype=torch.uint8).pin_memory()
        st = torch.cuda.current_stream().cuda_stream

        def call():
            _lib.call("tise_jpeg_reconstruct_rgb8", raw.data_ptr(), n, sb, arena.ctypes.data, sb, offs.ctypes.data, out.data_ptr(), pos,
                      ws.data_ptr(), wsb.value, table.data_ptr(), st)
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.reps):
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        ms = float(np.median(times))
        bytes_a, bytes_b = 3 * samples, samples + 3 * pixels
        print(f"{name}: {ms:.3f} ms per call (median of {args.reps}, min {min(times):.3f}, max {max(times):.3f}; table copy + both kernels), "
              f"{(bytes_a + bytes_b) / 1e6:.1f} MB moved = {(bytes_a + bytes_b) / ms / 1e9 * 1e3 / 1e3:.3f} TB/s = "
              f"{(bytes_a + bytes_b) / (ms * 1e-3) / copy_rate:.2f} of the copy rate; {n / ms * 1e3:.0f} images/s; "
              f"bytes of kernel A {bytes_a / 1e6:.1f} MB, of kernel B {bytes_b / 1e6:.1f} MB", flush=True)


if __name__ == "__main__":
    main()
