"""GPU: lpips_hip.HipLpips and dists_hip.HipDists on their shared runner (vgg_pairs_hip.HipVGG16Pairs) in one process: neither
metric's bits depend on the other having run, on an earlier call, or on the chunking."""
import numpy as np
import pytest
import torch

SIZES = [(16, 16), (17, 19), (16, 16), (33, 16)]        # ragged: two pairs share a size, two stand alone; odd at every pool level


@pytest.mark.gpu
def test_interleaved_metrics_carry_no_state(cuda_device):
    from tise_toolbox_amd import dists_model, lpips_model, vgg_pairs_hip
    from tise_toolbox_amd.dists_hip import HipDists
    from tise_toolbox_amd.lpips_hip import HipLpips
    g = torch.Generator().manual_seed(0)
    xs = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).to(cuda_device) for h, w in SIZES]
    ys = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).to(cuda_device) for h, w in SIZES]
    lm, dm = lpips_model.LpipsVGG16().init_synthetic(0), dists_model.DistsVGG16().init_synthetic(0)
    alone = {"lpips": HipLpips(lm, cuda_device)(xs, ys), "dists": HipDists(dm, cuda_device)(xs, ys)}       # each in a fresh runner
    for v in alone.values():
        assert v.dtype == np.float64 and v.shape == (len(SIZES),) and np.isfinite(v).all() and (v > 0).all(), v
    assert alone["lpips"].tobytes() != alone["dists"].tobytes()
    default = {"lpips": HipLpips(lm, cuda_device), "dists": HipDists(dm, cuda_device)}
    tiny = {"lpips": HipLpips(lm, cuda_device, budget=1), "dists": HipDists(dm, cuda_device, budget=1)}     # every pair its own chunk
    assert isinstance(default["lpips"], vgg_pairs_hip.HipVGG16Pairs) and isinstance(default["dists"], vgg_pairs_hip.HipVGG16Pairs)
    got = {"lpips": [], "dists": []}
    for order in (("lpips", "dists"), ("dists", "lpips")):                  # interleaved, each runner called twice
        for runners in (default, tiny):
            for name in order:
                got[name].append(runners[name](xs, ys))
    for name, values in got.items():
        assert len(values) == 4
        for k, v in enumerate(values):
            assert v.tobytes() == alone[name].tobytes(), (name, k, v, alone[name])
