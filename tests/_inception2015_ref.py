"""CPU restatement of the Inception-2015 graph's forward (test infrastructure for ``--network inception-2015``).

Works from a state_dict in pytorch-fid's key layout (torchvision Inception3 names, no AuxLogits, fc 1008 x 2048) with
``torch.nn.functional`` only, in fp64 by default, and deliberately shares no code with ``tise_toolbox_amd/inception.py``
(module tree, BatchNorm folding, pool-branch switch) or with ``oracle/inception_oracle.py`` (the torchvision graph).

What differs from torchvision's graph, written out here independently of the package:
  * input: the uint8 image v -> (v - 128) / 128 on every channel (the graph's Sub / Mul nodes);
  * the average-pool branches of Mixed_5b..5d, 6b..6e and 7b exclude the padding (TensorFlow SAME average);
  * Mixed_7c's pool branch is a 3x3 / stride 1 / pad 1 max pool (padding = -inf) before its 1x1 conv;
  * the classifier is fc 2048 -> 1008.
"""
import numpy as np
import torch
import torch.nn.functional as F


def to_input(u8_nhwc, dtype=torch.float64):
    """(N, H, W, 3) uint8 -> (N, 3, H, W) network input."""
    x = torch.as_tensor(np.ascontiguousarray(u8_nhwc)).to(dtype).permute(0, 3, 1, 2)
    return (x - 128.0) / 128.0


def _cbr(sd, name, x, stride=1, padding=0):
    dt = x.dtype
    y = F.conv2d(x, sd[name + ".conv.weight"].to(dt), None, stride, padding)
    y = F.batch_norm(y, sd[name + ".bn.running_mean"].to(dt), sd[name + ".bn.running_var"].to(dt),
                     sd[name + ".bn.weight"].to(dt), sd[name + ".bn.bias"].to(dt), False, 0.0, 0.001)
    return F.relu(y)


def _avg_same(x):
    return F.avg_pool2d(x, 3, 1, 1, count_include_pad=False)


def _mixed_a(sd, p, x):
    b1 = _cbr(sd, p + ".branch1x1", x)
    b5 = _cbr(sd, p + ".branch5x5_2", _cbr(sd, p + ".branch5x5_1", x), padding=2)
    b3 = _cbr(sd, p + ".branch3x3dbl_3", _cbr(sd, p + ".branch3x3dbl_2", _cbr(sd, p + ".branch3x3dbl_1", x), padding=1),
              padding=1)
    return torch.cat([b1, b5, b3, _cbr(sd, p + ".branch_pool", _avg_same(x))], 1)


def _mixed_b(sd, p, x):
    b3 = _cbr(sd, p + ".branch3x3", x, stride=2)
    bd = _cbr(sd, p + ".branch3x3dbl_3", _cbr(sd, p + ".branch3x3dbl_2", _cbr(sd, p + ".branch3x3dbl_1", x), padding=1),
              stride=2)
    return torch.cat([b3, bd, F.max_pool2d(x, 3, 2)], 1)


def _mixed_c(sd, p, x):
    b1 = _cbr(sd, p + ".branch1x1", x)
    b7 = _cbr(sd, p + ".branch7x7_1", x)
    b7 = _cbr(sd, p + ".branch7x7_3", _cbr(sd, p + ".branch7x7_2", b7, padding=(0, 3)), padding=(3, 0))
    bd = _cbr(sd, p + ".branch7x7dbl_1", x)
    for k, pad in ((2, (3, 0)), (3, (0, 3)), (4, (3, 0)), (5, (0, 3))):
        bd = _cbr(sd, p + f".branch7x7dbl_{k}", bd, padding=pad)
    return torch.cat([b1, b7, bd, _cbr(sd, p + ".branch_pool", _avg_same(x))], 1)


def _mixed_d(sd, p, x):
    b3 = _cbr(sd, p + ".branch3x3_2", _cbr(sd, p + ".branch3x3_1", x), stride=2)
    b7 = _cbr(sd, p + ".branch7x7x3_1", x)
    b7 = _cbr(sd, p + ".branch7x7x3_2", b7, padding=(0, 3))
    b7 = _cbr(sd, p + ".branch7x7x3_3", b7, padding=(3, 0))
    b7 = _cbr(sd, p + ".branch7x7x3_4", b7, stride=2)
    return torch.cat([b3, b7, F.max_pool2d(x, 3, 2)], 1)


def _mixed_e(sd, p, x, max_pool):
    b1 = _cbr(sd, p + ".branch1x1", x)
    b3 = _cbr(sd, p + ".branch3x3_1", x)
    b3 = torch.cat([_cbr(sd, p + ".branch3x3_2a", b3, padding=(0, 1)), _cbr(sd, p + ".branch3x3_2b", b3, padding=(1, 0))], 1)
    bd = _cbr(sd, p + ".branch3x3dbl_2", _cbr(sd, p + ".branch3x3dbl_1", x), padding=1)
    bd = torch.cat([_cbr(sd, p + ".branch3x3dbl_3a", bd, padding=(0, 1)), _cbr(sd, p + ".branch3x3dbl_3b", bd, padding=(1, 0))], 1)
    pooled = F.max_pool2d(x, 3, 1, 1) if max_pool else _avg_same(x)
    return torch.cat([b1, b3, bd, _cbr(sd, p + ".branch_pool", pooled)], 1)


@torch.no_grad()
def pool3(sd, x):
    """(N, 3, 299, 299) network input (``to_input``) -> (N, 2048) pool3 features in x's dtype."""
    x = _cbr(sd, "Conv2d_1a_3x3", x, stride=2)
    x = _cbr(sd, "Conv2d_2a_3x3", x)
    x = F.max_pool2d(_cbr(sd, "Conv2d_2b_3x3", x, padding=1), 3, 2)
    x = _cbr(sd, "Conv2d_4a_3x3", _cbr(sd, "Conv2d_3b_1x1", x))
    x = F.max_pool2d(x, 3, 2)
    for name in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
        x = _mixed_a(sd, name, x)
    x = _mixed_b(sd, "Mixed_6a", x)
    for name in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
        x = _mixed_c(sd, name, x)
    x = _mixed_d(sd, "Mixed_7a", x)
    x = _mixed_e(sd, "Mixed_7b", x, max_pool=False)
    x = _mixed_e(sd, "Mixed_7c", x, max_pool=True)
    return x.mean(dim=(2, 3))


@torch.no_grad()
def logits(sd, feats, bias=False):
    """pool3 -> 1008 logits; ``bias=False`` is the IS* for COCO head (weight matrix only)."""
    w = sd["fc.weight"].to(feats.dtype)
    return F.linear(feats, w, sd["fc.bias"].to(feats.dtype) if bias else None)


def features_of_u8(sd, u8_nhwc, dtype=torch.float64, chunk=8):
    """uint8 299 x 299 images -> (pool3, W-only logits) as numpy arrays, in chunks of ``chunk`` images."""
    fs, ls = [], []
    for i in range(0, len(u8_nhwc), chunk):
        f = pool3(sd, to_input(u8_nhwc[i:i + chunk], dtype))
        fs.append(f.numpy())
        ls.append(logits(sd, f).numpy())
    return np.concatenate(fs), np.concatenate(ls)


def pytorch_fid_shapes():
    """{key: shape} of pytorch-fid's pt_inception-2015-12-05-6726825d.pth, derived from the published topology: every
    BasicConv2d contributes conv.weight and bn.{weight, bias, running_mean, running_var, num_batches_tracked}; fc is
    1008 x 2048 with bias; there is no AuxLogits."""
    convs = {"Conv2d_1a_3x3": (32, 3, 3, 3), "Conv2d_2a_3x3": (32, 32, 3, 3), "Conv2d_2b_3x3": (64, 32, 3, 3),
             "Conv2d_3b_1x1": (80, 64, 1, 1), "Conv2d_4a_3x3": (192, 80, 3, 3)}
    for name, cin, pf in (("Mixed_5b", 192, 32), ("Mixed_5c", 256, 64), ("Mixed_5d", 288, 64)):
        convs.update({f"{name}.branch1x1": (64, cin, 1, 1), f"{name}.branch5x5_1": (48, cin, 1, 1),
                      f"{name}.branch5x5_2": (64, 48, 5, 5), f"{name}.branch3x3dbl_1": (64, cin, 1, 1),
                      f"{name}.branch3x3dbl_2": (96, 64, 3, 3), f"{name}.branch3x3dbl_3": (96, 96, 3, 3),
                      f"{name}.branch_pool": (pf, cin, 1, 1)})
    convs.update({"Mixed_6a.branch3x3": (384, 288, 3, 3), "Mixed_6a.branch3x3dbl_1": (64, 288, 1, 1),
                  "Mixed_6a.branch3x3dbl_2": (96, 64, 3, 3), "Mixed_6a.branch3x3dbl_3": (96, 96, 3, 3)})
    for name, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        convs.update({f"{name}.branch1x1": (192, 768, 1, 1), f"{name}.branch7x7_1": (c7, 768, 1, 1),
                      f"{name}.branch7x7_2": (c7, c7, 1, 7), f"{name}.branch7x7_3": (192, c7, 7, 1),
                      f"{name}.branch7x7dbl_1": (c7, 768, 1, 1), f"{name}.branch7x7dbl_2": (c7, c7, 7, 1),
                      f"{name}.branch7x7dbl_3": (c7, c7, 1, 7), f"{name}.branch7x7dbl_4": (c7, c7, 7, 1),
                      f"{name}.branch7x7dbl_5": (192, c7, 1, 7), f"{name}.branch_pool": (192, 768, 1, 1)})
    convs.update({"Mixed_7a.branch3x3_1": (192, 768, 1, 1), "Mixed_7a.branch3x3_2": (320, 192, 3, 3),
                  "Mixed_7a.branch7x7x3_1": (192, 768, 1, 1), "Mixed_7a.branch7x7x3_2": (192, 192, 1, 7),
                  "Mixed_7a.branch7x7x3_3": (192, 192, 7, 1), "Mixed_7a.branch7x7x3_4": (192, 192, 3, 3)})
    for name, cin in (("Mixed_7b", 1280), ("Mixed_7c", 2048)):
        convs.update({f"{name}.branch1x1": (320, cin, 1, 1), f"{name}.branch3x3_1": (384, cin, 1, 1),
                      f"{name}.branch3x3_2a": (384, 384, 1, 3), f"{name}.branch3x3_2b": (384, 384, 3, 1),
                      f"{name}.branch3x3dbl_1": (448, cin, 1, 1), f"{name}.branch3x3dbl_2": (384, 448, 3, 3),
                      f"{name}.branch3x3dbl_3a": (384, 384, 1, 3), f"{name}.branch3x3dbl_3b": (384, 384, 3, 1),
                      f"{name}.branch_pool": (192, cin, 1, 1)})
    shapes = {}
    for name, shp in convs.items():
        shapes[name + ".conv.weight"] = shp
        for k in ("weight", "bias", "running_mean", "running_var"):
            shapes[f"{name}.bn.{k}"] = (shp[0],)
        shapes[name + ".bn.num_batches_tracked"] = ()
    shapes["fc.weight"] = (1008, 2048)
    shapes["fc.bias"] = (1008,)
    return shapes


def random_state_dict(seed=0):
    """A state_dict with pytorch-fid's keys and shapes (random values: key / shape tests only)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shp in pytorch_fid_shapes().items():
        sd[k] = torch.zeros((), dtype=torch.long) if k.endswith("num_batches_tracked") else torch.rand(shp, generator=g) + 0.5
    return sd
