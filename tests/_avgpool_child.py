"""Child-process entry point of tests/test_gpu_pool_kernels.py and tests/test_gpu_nonfinite.py.

``TISE_AVGPOOL_PER_OUTPUT`` is read once per process (csrc/trunk_ops.hip, avgpool_split_launch), so the per-output split
average-pool kernel can only be reached from a fresh process: ``python tests/_avgpool_child.py IN.npz OUT.npz`` runs every
case of IN.npz (``save_cases``) through ``tise_avgpool3[_excl]_bias_relu_split_nhwc`` under the environment it was started
with and writes each case's whole output tensor and the range guard's flag after it to OUT.npz.  ``run_cases`` is the same
loop for the calling process (the column-walking kernel).  Not collected by pytest (no ``test_`` prefix)."""
import ctypes
import os
import sys

import numpy as np

SENTINEL = np.float16(-3.0)
META = ("n", "h", "w", "C", "x_ld", "x_off", "out_C", "out_off", "excl")


def save_cases(path, cases):
    """cases: dicts with x (n, h, w, x_ld) fp32, bias (C,) fp32 and the META integers."""
    arrs = {"count": np.array(len(cases))}
    for i, c in enumerate(cases):
        arrs[f"x{i}"] = c["x"]
        arrs[f"b{i}"] = c["bias"]
        arrs[f"m{i}"] = np.array([int(c[k]) for k in META], dtype=np.int64)
    np.savez(path, **arrs)


def load_cases(path):
    z = np.load(path)
    out = []
    for i in range(int(z["count"])):
        c = dict(zip(META, (int(v) for v in z[f"m{i}"])))
        c.update(x=z[f"x{i}"], bias=z[f"b{i}"])
        out.append(c)
    return out


def run_cases(cases, dev, read_flag=True):
    """-> list of (out (n, h, w, 2 * out_C) fp16 numpy, sentinel-filled outside the written slice; guard flag after the launch,
    or None with ``read_flag`` False: the flag is then left for the caller to read)."""
    import torch
    from tise_toolbox_amd import _lib, device
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    if read_flag:
        device.read_split_overflow()
    res = []
    for c in cases:
        x = torch.from_numpy(np.ascontiguousarray(c["x"], dtype=np.float32)).to(dev)
        b = torch.from_numpy(np.ascontiguousarray(c["bias"], dtype=np.float32)).to(dev)
        out = torch.full((c["n"], c["h"], c["w"], 2 * c["out_C"]), float(SENTINEL), dtype=torch.float16, device=dev)
        assert x.shape == (c["n"], c["h"], c["w"], c["x_ld"]) and b.numel() == c["C"] and x.data_ptr() % 16 == 0
        fn = "tise_avgpool3_excl_bias_relu_split_nhwc" if c["excl"] else "tise_avgpool3_bias_relu_split_nhwc"
        _lib.call(fn, P(x), c["x_ld"], c["x_off"], c["n"], c["h"], c["w"], c["C"], P(b), P(out), c["out_C"], c["out_off"],
                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        flag = device.read_split_overflow() if read_flag else None
        res.append((out.cpu().numpy(), flag))
    return res


def main():
    import torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    from tise_toolbox_amd import _lib
    assert torch.cuda.is_available(), "no HIP device"
    _lib.load()
    res = run_cases(load_cases(sys.argv[1]), torch.device("cuda", 0))
    arrs = {"per_output": np.array("TISE_AVGPOOL_PER_OUTPUT" in os.environ)}
    for i, (out, flag) in enumerate(res):
        arrs[f"o{i}"] = out
        arrs[f"f{i}"] = np.array(flag)
    np.savez(sys.argv[2], **arrs)


if __name__ == "__main__":
    main()
