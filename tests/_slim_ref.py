"""CPU restatement of the TF-slim InceptionV3 forward of the reference's IS* for CUB birds (test infrastructure for
``--network slim``).

Works from the TensorFlow-layout checkpoint tensors themselves -- ``{"<scope>/weights/ExponentialMovingAverage":
[kh, kw, cin, cout], ".../BatchNorm/beta", "moving_mean", "moving_variance", "logits/logits/weights": [2048, C],
"biases"}`` -- with ``torch.nn.functional`` only, fp64 by default, and shares no code with ``tise_toolbox_amd/inception.py``
(module tree, name map, BatchNorm folding) or ``oracle/``.  The graph, as inception_model.py / ops.py build it:
  * input: the uint8 image v -> v / 127.5 - 1 on every channel (inception_score_star_bird.py:70);
  * conv (no bias) -> BatchNorm with beta and moving statistics, NO gamma, eps 0.001 -> ReLU;
  * every 3x3 / stride 1 SAME pool of a mixed block is an average that excludes the padding, Mixed_7c's too;
  * 8 x 8 VALID average -> fc 2048 -> C with bias.
"""
import numpy as np
import torch
import torch.nn.functional as F

EMA = "/ExponentialMovingAverage"


def to_input(u8_nhwc, dtype=torch.float64):
    x = torch.as_tensor(np.ascontiguousarray(u8_nhwc)).to(dtype).permute(0, 3, 1, 2)
    return x / 127.5 - 1.0


def _t(tf, name, dt):
    return torch.as_tensor(np.asarray(tf[name + EMA])).to(dt)


def _cbr(tf, scope, x, stride=1, padding="SAME"):
    dt = x.dtype
    w = _t(tf, scope + "/weights", dt)                         # [kh, kw, cin, cout]
    kh, kw = w.shape[0], w.shape[1]
    pad = (0, 0) if padding == "VALID" else (kh // 2, kw // 2)
    y = F.conv2d(x, w.permute(3, 2, 0, 1), None, stride, pad)
    mean, var = _t(tf, scope + "/BatchNorm/moving_mean", dt), _t(tf, scope + "/BatchNorm/moving_variance", dt)
    beta = _t(tf, scope + "/BatchNorm/beta", dt)
    y = (y - mean.view(1, -1, 1, 1)) / torch.sqrt(var.view(1, -1, 1, 1) + 0.001) + beta.view(1, -1, 1, 1)
    return F.relu(y)


def _avg_same(x):
    return F.avg_pool2d(x, 3, 1, 1, count_include_pad=False)


def _chain(tf, scope, x, kinds):
    for i, _ in enumerate(kinds):
        x = _cbr(tf, f"{scope}/Conv" + (f"_{i}" if i else ""), x)
    return x


def _mixed_35(tf, s, x):
    return torch.cat([_chain(tf, s + "/branch1x1", x, "a"), _chain(tf, s + "/branch5x5", x, "ab"),
                      _chain(tf, s + "/branch3x3dbl", x, "abc"), _cbr(tf, s + "/branch_pool/Conv", _avg_same(x))], 1)


def _mixed_17a(tf, s, x):
    b3 = _cbr(tf, s + "/branch3x3/Conv", x, 2, "VALID")
    d = _cbr(tf, s + "/branch3x3dbl/Conv_1", _cbr(tf, s + "/branch3x3dbl/Conv", x))
    d = _cbr(tf, s + "/branch3x3dbl/Conv_2", d, 2, "VALID")
    return torch.cat([b3, d, F.max_pool2d(x, 3, 2)], 1)


def _mixed_17(tf, s, x):
    return torch.cat([_chain(tf, s + "/branch1x1", x, "a"), _chain(tf, s + "/branch7x7", x, "abc"),
                      _chain(tf, s + "/branch7x7dbl", x, "abcde"), _cbr(tf, s + "/branch_pool/Conv", _avg_same(x))], 1)


def _mixed_17x17x1280a(tf, s, x):
    b3 = _cbr(tf, s + "/branch3x3/Conv_1", _cbr(tf, s + "/branch3x3/Conv", x), 2, "VALID")
    b7 = _chain(tf, s + "/branch7x7x3", x, "abc")
    b7 = _cbr(tf, s + "/branch7x7x3/Conv_3", b7, 2, "VALID")
    return torch.cat([b3, b7, F.max_pool2d(x, 3, 2)], 1)


def _mixed_8(tf, s, x):
    b3 = _cbr(tf, s + "/branch3x3/Conv", x)
    b3 = torch.cat([_cbr(tf, s + "/branch3x3/Conv_1", b3), _cbr(tf, s + "/branch3x3/Conv_2", b3)], 1)
    d = _cbr(tf, s + "/branch3x3dbl/Conv_1", _cbr(tf, s + "/branch3x3dbl/Conv", x))
    d = torch.cat([_cbr(tf, s + "/branch3x3dbl/Conv_2", d), _cbr(tf, s + "/branch3x3dbl/Conv_3", d)], 1)
    return torch.cat([_cbr(tf, s + "/branch1x1/Conv", x), b3, d, _cbr(tf, s + "/branch_pool/Conv", _avg_same(x))], 1)


def pool3(tf, x):
    x = _cbr(tf, "conv0", x, 2, "VALID")
    x = _cbr(tf, "conv1", x, 1, "VALID")
    x = _cbr(tf, "conv2", x)
    x = F.max_pool2d(x, 3, 2)
    x = _cbr(tf, "conv3", x, 1, "VALID")
    x = _cbr(tf, "conv4", x, 1, "VALID")
    x = F.max_pool2d(x, 3, 2)
    for s in ("mixed_35x35x256a", "mixed_35x35x288a", "mixed_35x35x288b"):
        x = _mixed_35(tf, s, x)
    x = _mixed_17a(tf, "mixed_17x17x768a", x)
    for s in ("mixed_17x17x768b", "mixed_17x17x768c", "mixed_17x17x768d", "mixed_17x17x768e"):
        x = _mixed_17(tf, s, x)
    x = _mixed_17x17x1280a(tf, "mixed_17x17x1280a", x)
    for s in ("mixed_8x8x2048a", "mixed_8x8x2048b"):
        x = _mixed_8(tf, s, x)
    assert x.shape[-2:] == (8, 8)
    return F.avg_pool2d(x, 8).flatten(1)


def logits(tf, feats):
    dt = feats.dtype
    return feats @ _t(tf, "logits/logits/weights", dt) + _t(tf, "logits/logits/biases", dt)


def features_of_u8(tf, u8_nhwc, dtype=torch.float64, chunk=8):
    """(N, 299, 299, 3) uint8 -> (pool3 (N, 2048), biased logits (N, C)) as numpy arrays of ``dtype``."""
    fs, ls = [], []
    with torch.no_grad():
        for i in range(0, len(u8_nhwc), chunk):
            f = pool3(tf, to_input(u8_nhwc[i:i + chunk], dtype))
            fs.append(f)
            ls.append(logits(tf, f))
    return torch.cat(fs).numpy(), torch.cat(ls).numpy()
