"""CPU: --network slim (the TF-slim InceptionV3 of the reference's IS* for CUB birds) and the inception_score_bird CLI.

Name map against the variable list the reference's own code creates (tests/golden/slim_inception_v3_variables.json), the
product's module tree against the slim listing (tests/golden/inception_v3_topology.json) with NO normalisation of the pool
divisor or of the BatchNorm gamma, the checkpoint loader, the input table, the bird sampling rule and fid_score's refusal."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tise_toolbox_amd import build

from ._tf_ckpt_writer import slim_checkpoint_tensors, write_v1, write_v2

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EMA = "/ExponentialMovingAverage"


@pytest.fixture(scope="module", autouse=True)
def _host_lib():
    build.build_png(verbose=False)


def _variables():
    return json.load(open(os.path.join(GOLDEN, "slim_inception_v3_variables.json")))["variables"]


def _pool3_logits_ancestor_scopes():
    """Scopes of the conv and fc layers that are ancestors of logits in the slim listing (no aux head)."""
    t = json.load(open(os.path.join(GOLDEN, "inception_v3_topology.json")))
    nodes = {n["id"]: n for n in t["nodes"]}
    fc = [n for n in t["nodes"] if n["op"] == "fc" and n["scope"].endswith("logits/logits")]
    assert len(fc) == 1
    keep, stack = set(), [fc[0]["id"]]
    while stack:
        i = stack.pop()
        if i not in keep:
            keep.add(i)
            stack.extend(nodes[i]["inputs"])
    return [nodes[i] for i in sorted(keep) if nodes[i]["op"] in ("conv2d", "fc")]


def test_name_map_covers_exactly_the_pool3_and_logits_ancestors():
    from tise_toolbox_amd.inception import Inception3, slim_variable_map
    variables = {v["name"]: v for v in _variables()}
    # TF1 ExponentialMovingAverage.variables_to_restore(): trainable or moving-average variables read from their shadows
    restore = {}
    for v in variables.values():
        shadow = "trainable_variables" in v["collections"] or "moving_average_variables" in v["collections"]
        restore[v["name"] + EMA if shadow else v["name"]] = v
    vmap = slim_variable_map()
    names = [n for n, _ in vmap.values()]
    assert len(names) == len(set(names))
    assert all(n in restore and n.endswith(EMA) for n in names)
    # the listing's logits ancestors: 94 BatchNorm'd convolutions and the classifier (the topology golden does not carry
    # the uniquified Conv_<i> scope names, the variable list does); every other variable belongs to the auxiliary head
    anc = _pool3_logits_ancestor_scopes()
    assert sum(1 for n in anc if n["op"] == "conv2d") == 94 and sum(1 for n in anc if n["op"] == "fc") == 1
    wanted = {n for n in variables if not n.startswith("aux_logits/")}
    assert {n[:-len(EMA)] for n in names} == wanted
    assert len(wanted) == 94 * 4 + 2
    assert {n.split("/")[0] for n in variables} - {n.split("/")[0] for n in wanted} == {"aux_logits"}
    assert not any(n.startswith("aux_logits") for n in wanted)
    assert not any(n.endswith("/gamma") for n in variables)                 # scale=False: no gamma in the graph
    # TF shapes match the module tree through the layout rule
    sd = Inception3(num_classes=51, aux_logits=False, network="slim").state_dict()
    for key, (name, layout) in vmap.items():
        shape = variables[name[:-len(EMA)]]["shape"]
        want = list(sd[key].shape)
        got = [shape[3], shape[2], shape[0], shape[1]] if layout == "conv" else (shape[::-1] if layout == "fc" else shape)
        assert got == want, (key, name, shape)


def _random_slim_state(seed=0):
    from tise_toolbox_amd.inception import Inception3
    g = torch.Generator().manual_seed(seed)
    net = Inception3(num_classes=51, aux_logits=False, network="slim")
    sd = {}
    for k, v in net.state_dict().items():
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.zeros((), dtype=torch.long)
        elif k.endswith("bn.weight"):
            sd[k] = torch.ones_like(v)
        elif k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(v.shape, generator=g)
        else:
            sd[k] = torch.randn(v.shape, generator=g) * 0.1
    return sd


@pytest.mark.parametrize("fmt", ["V1", "V2"])
def test_checkpoint_loads_into_the_module_tree(tmp_path, fmt):
    from tise_toolbox_amd.inception import build_inception3
    sd = _random_slim_state(1)
    path = str(tmp_path / "model.ckpt")
    tensors = slim_checkpoint_tensors(sd)
    (write_v1 if fmt == "V1" else write_v2)(path, tensors, compression=1 if fmt == "V1" else 0, block_size=65536)
    net = build_inception3(weights=path, network="slim")
    assert not hasattr(net, "AuxLogits") and net.fc.out_features == 51
    got = net.state_dict()
    assert set(got) == set(sd)
    for k, v in sd.items():
        assert torch.equal(got[k], v), k
    assert all(bool((m.weight == 1.0).all()) for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d))
    # a head of another width is refused with the tensor's name
    tensors["logits/logits/weights" + EMA] = np.zeros((2048, 11), np.float32)
    write_v2(str(tmp_path / "bad"), tensors)
    with pytest.raises(ValueError, match="logits/logits/weights/ExponentialMovingAverage"):
        build_inception3(weights=str(tmp_path / "bad"), network="slim")


def _pad(n):
    """Pixels of padding per side: SAME occurs only at stride 1 in this graph, where it is (k - 1) / 2."""
    if n["padding"] == "VALID":
        return (0, 0)
    assert n["stride"] == [1, 1]
    return (n["kernel"][0] // 2, n["kernel"][1] // 2)


def _reference_canon():
    """The slim listing's logits ancestors as an op list, taken as it is: TF SAME average pools exclude the padding, the
    BatchNorms have no gamma."""
    t = json.load(open(os.path.join(GOLDEN, "inception_v3_topology.json")))
    nodes = {n["id"]: n for n in t["nodes"]}
    final = [n for n in t["nodes"] if n["op"] == "avg_pool" and n["scope"].endswith("logits/pool")][0]
    keep, stack = set(), [final["id"]]
    while stack:
        i = stack.pop()
        if i not in keep:
            keep.add(i)
            stack.extend(nodes[i]["inputs"])
    canon, where = [], {}
    for n in t["nodes"]:
        if n["id"] not in keep:
            continue
        ins = tuple(where[i] for i in n["inputs"])
        if n["op"] == "input":
            canon.append(("input",))
        elif n["op"] == "conv2d":
            canon.append(("conv", n["cin"], n["cout"], *n["kernel"], *n["stride"], *_pad(n), *n["out_shape"][:2], ins))
        elif n["op"] == "batch_norm":
            canon.append(("bn", n["epsilon"], n["has_gamma"], n["has_beta"], ins))
        elif n["op"] == "relu":
            canon.append(("relu", ins))
        elif n["id"] == final["id"]:
            canon.append(("global_avg", ins))
        elif n["op"] in ("max_pool", "avg_pool"):
            # TensorFlow's SAME average divides by the in-image tap count: it excludes the padding
            excl = n["op"] == "avg_pool" and n["padding"] == "SAME"
            canon.append((n["op"], *n["kernel"], *n["stride"], *_pad(n), excl, *n["out_shape"][:2], ins))
        elif n["op"] == "concat":
            canon.append(("concat", tuple(n["widths"]), ins))
        else:
            raise AssertionError(n["op"])
        where[n["id"]] = len(canon) - 1
    return canon


class _Tracer:
    def __init__(self):
        self.ops = []

    def tag(self, t, entry):
        self.ops.append(entry)
        t._node = len(self.ops) - 1
        return t

    def __enter__(self):
        o = self.o = {n: getattr(F, n) for n in ("conv2d", "batch_norm", "relu", "max_pool2d", "avg_pool2d", "adaptive_avg_pool2d")}
        o["cat"] = torch.cat
        tr = self

        def pad_name(k, padding):
            return (padding, padding) if isinstance(padding, int) else tuple(padding)

        def conv2d(x, w, b=None, stride=1, padding=0, *a, **k):
            y = o["conv2d"](x, w, b, stride, padding, *a, **k)
            s = (stride, stride) if isinstance(stride, int) else tuple(stride)
            return tr.tag(y, ("conv", w.shape[1], w.shape[0], w.shape[2], w.shape[3], *s, *pad_name(tuple(w.shape[2:]), padding),
                              y.shape[2], y.shape[3], (x._node,)))

        def batch_norm(x, rm, rv, weight=None, bias=None, training=False, momentum=0.1, eps=1e-5):
            has_gamma = weight is not None and not bool((weight == 1.0).all())      # exactly 1: no gamma
            return tr.tag(o["batch_norm"](x, rm, rv, weight, bias, training, momentum, eps),
                          ("bn", eps, has_gamma, bias is not None, (x._node,)))

        def relu(x, inplace=False):
            return tr.tag(o["relu"](x, inplace), ("relu", (x._node,)))

        def pool(kind):
            def f(x, kernel_size, stride=None, padding=0, *a, **k):
                y = o[kind + "2d"](x, kernel_size, stride, padding, *a, **k)
                # avg_pool2d(input, kernel_size, stride, padding, ceil_mode, count_include_pad, divisor_override)
                count_include_pad = k.get("count_include_pad", a[1] if len(a) > 1 else True)
                ks = (kernel_size, kernel_size) if isinstance(kernel_size, int) else tuple(kernel_size)
                st = (stride, stride) if isinstance(stride, int) else tuple(stride)
                excl = kind == "avg_pool" and not count_include_pad
                return tr.tag(y, (kind, *ks, *st, *pad_name(ks, padding), excl, y.shape[2], y.shape[3], (x._node,)))
            return f

        def adaptive(x, size):
            return tr.tag(o["adaptive_avg_pool2d"](x, size), ("global_avg", (x._node,)))

        def cat(ts, dim=0):
            return tr.tag(o["cat"](ts, dim), ("concat", tuple(t.shape[1] for t in ts), tuple(t._node for t in ts)))
        F.conv2d, F.batch_norm, F.relu = conv2d, batch_norm, relu
        F.max_pool2d, F.avg_pool2d, F.adaptive_avg_pool2d = pool("max_pool"), pool("avg_pool"), adaptive
        torch.cat = cat
        return self

    def __exit__(self, *exc):
        for name, fn in self.o.items():
            setattr(torch if name == "cat" else F, name, fn)


def test_product_tree_is_the_slim_listing_without_normalisation(tmp_path):
    from tise_toolbox_amd.inception import InceptionV3
    path = str(tmp_path / "model.ckpt")
    write_v2(path, slim_checkpoint_tensors(_random_slim_state(2), extra=False))
    m = InceptionV3([3], weights=path, network="slim").eval()
    with _Tracer() as tr, torch.no_grad():
        x = torch.rand(1, 3, 299, 299)
        x = tr.tag(x, ("input",))
        m(x, prenormalized=True)
    assert tr.ops == _reference_canon()
    # the default network is NOT the slim listing taken as it is (its pools include the padding, its BN has gamma)
    assert sum(1 for op in tr.ops if op[0] == "avg_pool" and op[7]) == 9


def test_slim_input_table_bit_exact():
    from tise_toolbox_amd import device
    lut = device.make_lut(network="slim")
    want = np.arange(256, dtype=np.uint8).astype(np.float32) / 127.5 - 1.0
    assert lut.shape == (3, 256) and lut.dtype == np.float32
    for c in range(3):
        assert lut[c].tobytes() == want.tobytes()
    assert device.make_lut().tobytes() != lut.tobytes()


def test_slim_network_constants():
    from tise_toolbox_amd import weights
    from tise_toolbox_amd.inception import NETWORK_CLASSES, POOL_BRANCHES, network_classes
    assert network_classes("slim") == 51 and "slim" not in NETWORK_CLASSES
    assert [network_classes(n) for n in ("torchvision", "inception-2015")] == [1000, 1008]
    assert set(POOL_BRANCHES["slim"].values()) == {"avg_excl"} and len(POOL_BRANCHES["slim"]) == 9
    assert weights.inception_kind("slim") == "slim"
    assert weights._KINDS["slim"][1]() == [os.path.join("IS", "bird", "inception_finetuned_models", "birds_valid299", "model.ckpt")]


def test_weights_resolve_takes_a_v2_prefix(tmp_path):
    from tise_toolbox_amd import weights
    p = str(tmp_path / "model.ckpt")
    with pytest.raises(RuntimeError, match="Invalid path"):
        weights.resolve(p, False, "slim")
    open(p + ".index", "wb").close()
    assert weights.resolve(p, False, "slim") == (p, "")
    with pytest.raises(RuntimeError, match="mutually exclusive"):
        weights.resolve(p, True, "slim")


def test_bird_order_is_the_references_shuffle():
    from tise_toolbox_amd.inception_score_bird import bird_order, bird_selection
    gold = np.load(os.path.join(GOLDEN, "is_ref_bird_150.npz"))
    files = [f"f{i:03d}.png" for i in range(150)]
    sel = bird_selection(files, 64, seed=13)
    assert len(sel) == 128 == int(gold["batch_size"]) * (150 // int(gold["batch_size"]))
    assert sel == [files[i] for i in gold["shuffle"][:128]]
    assert bird_order(150, 13).tolist() == gold["shuffle"].tolist()
    np.random.seed(13)                                        # unseeded: the global generator, as the reference uses it
    assert bird_order(150).tolist() == gold["shuffle"].tolist()
    assert bird_selection(files[:63], 64, seed=1) == []


def test_fid_score_refuses_slim(capsys):
    from tise_toolbox_amd import fid_score
    with pytest.raises(SystemExit):
        fid_score._build_parser().parse_args(["--path2", "x", "--network", "slim"])
    assert "slim network" in capsys.readouterr().err
    assert fid_score._build_parser().parse_args(["--path2", "x", "--network", "inception-2015"]).network == "inception-2015"


def test_cli_flags_follow_the_reference():
    from tise_toolbox_amd import calibration, inception_score, inception_score_bird as bird
    a = bird._build_parser().parse_args([])
    assert (a.checkpoint_dir, a.num_classes, a.splits, a.batch_size, a.gpu, a.saved_file, a.shuffle_seed) == \
        (os.path.join("IS", "bird", "inception_finetuned_models", "birds_valid299", "model.ckpt"), 50, 10, 64, 0, "", None)
    assert inception_score._build_parser().parse_args(["--network", "slim"]).network == "slim"
    assert calibration._build_parser().parse_args(["--network", "slim", "--rule", "bird", "--image_dir", "d"]).network == "slim"
