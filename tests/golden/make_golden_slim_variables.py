#!/usr/bin/env python3
"""Every variable of the reference's TF-slim InceptionV3 -> tests/golden/slim_inception_v3_variables.json.

The reference's IS* for CUB birds restores its network from a TensorFlow checkpoint by variable NAME
(image_realism/IS/bird/inception_score_star_bird.py:196-201: ``ExponentialMovingAverage(0.9999).variables_to_restore()``).
Those names are whatever ``inception_model.py`` / ``ops.py`` / ``scopes.py`` / ``variables.py`` create under TF1's scoping
rules, so this script EXECUTES those four reference files by path, under a stub ``tensorflow`` that models exactly the parts
of TF1 the names depend on:

* ``tf.variable_scope(name)`` opens ``name`` inside the current variable scope (no uniquifying: a named scope is re-entered);
  ``tf.variable_scope(None, default_name)`` picks ``default_name``, ``default_name_1``, ... unique within the enclosing
  variable scope, counted per full scope name as TF1's variable-scope store does;
* ``tf.name_scope`` adds nothing to variable names -- the model's outer ``name_scope(scope, "inception_v3")`` included;
* ``tf.get_variable`` names a variable ``<variable scope>/<name>`` and puts it in the collections it is given, plus
  ``trainable_variables`` when it is trainable (tf.Variable's rule); ``ops.batch_norm`` puts the moving statistics into
  ``moving_average_variables`` itself.

The graph is built with the bird script's own arguments (``inference``, :147-169: weight decay 0.00004, stddev 0.1, ReLU,
BatchNorm decay 0.9997 / epsilon 0.001 on every conv; ``inception_v3(images, dropout_keep_prob=0.8, num_classes=51,
is_training=False, restore_logits=True)``).  Stored: names, shapes, collections and the trainable flag -- no reference
source text.

    python tests/golden/make_golden_slim_variables.py REFERENCE_CHECKOUT
"""
import contextlib
import importlib.util
import json
import os
import re
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
SLIM_REL = os.path.join("image_realism", "IS", "bird", "inception", "slim")
sys.dont_write_bytecode = True

GLOBAL_VARIABLES = "variables"
TRAINABLE_VARIABLES = "trainable_variables"
MOVING_AVERAGE_VARIABLES = "moving_average_variables"

VAR_SCOPE = []            # names of the open variable scopes
SCOPE_COUNTS = {}         # full variable-scope name -> times opened (TF1 _VariableScopeStore.variable_scopes_count)
COLLECTIONS = {}
VARIABLES = []


class TensorShape:
    def __init__(self, dims):
        self.dims = list(dims)

    def __getitem__(self, i):
        r = self.dims[i]
        return TensorShape(r) if isinstance(i, slice) else r

    def __len__(self):
        return len(self.dims)

    def __iter__(self):
        return iter(self.dims)

    def num_elements(self):
        n = 1
        for d in self.dims:
            n *= d
        return n

    def as_list(self):
        return list(self.dims)


class Tensor:
    def __init__(self, shape):
        self.shape = list(shape)

    def get_shape(self):
        return TensorShape(self.shape)

    def set_shape(self, s):
        pass


class Variable(Tensor):
    def __init__(self, name, shape):
        super().__init__(shape)
        self.name = name + ":0"
        self.op = types.SimpleNamespace(name=name)


def _out_hw(h, w, k, s, padding):
    if padding == "SAME":
        return -(-h // s[0]), -(-w // s[1])
    return (h - k[0]) // s[0] + 1, (w - k[1]) // s[1] + 1


def _conv2d(x, w, strides, padding):
    oh, ow = _out_hw(x.shape[1], x.shape[2], w.shape[:2], strides[1:3], padding)
    return Tensor([x.shape[0], oh, ow, w.shape[3]])


def _pool(x, ksize, strides, padding):
    oh, ow = _out_hw(x.shape[1], x.shape[2], ksize[1:3], strides[1:3], padding)
    return Tensor([x.shape[0], oh, ow, x.shape[3]])


def _scope_name():
    return "/".join(VAR_SCOPE)


def _open(name):
    full = f"{_scope_name()}/{name}" if VAR_SCOPE else name
    SCOPE_COUNTS[full] = SCOPE_COUNTS.get(full, 0) + 1
    VAR_SCOPE.append(name)


def _unique(prefix):
    """TF1 _get_unique_variable_scope: ``prefix`` if no scope of that full name was opened yet, else the first free
    ``prefix_<i>``."""
    base = f"{_scope_name()}/{prefix}" if VAR_SCOPE else prefix
    if SCOPE_COUNTS.get(base, 0) == 0:
        return prefix
    i = 1
    while SCOPE_COUNTS.get(f"{base}_{i}", 0) > 0:
        i += 1
    return f"{prefix}_{i}"


@contextlib.contextmanager
def variable_scope(name_or_scope, default_name=None, values=None, reuse=None):
    _open(name_or_scope if name_or_scope is not None else _unique(default_name))
    try:
        yield types.SimpleNamespace(name=_scope_name())
    finally:
        VAR_SCOPE.pop()


@contextlib.contextmanager
def name_scope(name, default_name=None, values=None):
    yield name or default_name                                  # no effect on variable names


def get_variable(name, shape=None, dtype=None, initializer=None, regularizer=None, trainable=True, collections=None, **kw):
    full = f"{_scope_name()}/{name}" if VAR_SCOPE else name
    if any(v["name"] == full for v in VARIABLES):
        raise ValueError(f"Variable {full} already exists")
    colls = set(collections or [GLOBAL_VARIABLES])
    if trainable:
        colls.add(TRAINABLE_VARIABLES)
    var = Variable(full, list(shape))
    VARIABLES.append({"name": full, "shape": [int(d) for d in shape], "collections": sorted(colls), "trainable": bool(trainable)})
    for c in colls:
        COLLECTIONS.setdefault(c, []).append(var)
    return var


def get_collection(key, scope=None):
    items = COLLECTIONS.get(key, [])
    if scope is None:
        return list(items)
    return [v for v in items if re.match(scope, v.op.name)]


def add_to_collection(key, value):
    COLLECTIONS.setdefault(key, []).append(value)
    if isinstance(value, Variable):
        for v in VARIABLES:
            if v["name"] == value.op.name and key not in v["collections"]:
                v["collections"] = sorted(v["collections"] + [key])


def build_stubs():
    tf = types.ModuleType("tensorflow")
    tf.TensorShape = TensorShape
    tf.float32, tf.int64 = "float32", "int64"
    tf.GraphKeys = types.SimpleNamespace(GLOBAL_VARIABLES=GLOBAL_VARIABLES, TRAINABLE_VARIABLES=TRAINABLE_VARIABLES,
                                         MOVING_AVERAGE_VARIABLES=MOVING_AVERAGE_VARIABLES, GLOBAL_STEP="global_step",
                                         VARIABLES=GLOBAL_VARIABLES)
    tf.nn = types.SimpleNamespace(
        conv2d=_conv2d, max_pool=_pool, avg_pool=_pool, relu=lambda x, name=None: x,
        batch_normalization=lambda x, mean, var, offset, scale, eps: x,
        softmax=lambda x, name=None: x,
        xw_plus_b=lambda x, w, b: Tensor([x.shape[0], w.shape[1]]),
        dropout=lambda x, keep_prob: x, bias_add=lambda x, b: x)
    tf.matmul = lambda x, w: Tensor([x.shape[0], w.shape[1]])
    tf.variable_scope = variable_scope
    tf.name_scope = name_scope
    tf.get_variable = get_variable
    tf.get_variable_scope = lambda: types.SimpleNamespace(name=_scope_name())
    tf.get_collection = get_collection
    tf.add_to_collection = add_to_collection
    tf.device = lambda d: contextlib.nullcontext()
    tf.NodeDef = lambda **k: types.SimpleNamespace(**k)
    tf.concat = lambda values, axis: Tensor(values[0].shape[:3] + [sum(v.shape[3] for v in values)])
    tf.identity = lambda x: x
    tf.reshape = lambda x, s: Tensor([x.shape[0], s[1]])
    for n in ("truncated_normal_initializer", "constant_initializer", "zeros_initializer", "ones_initializer"):
        setattr(tf, n, lambda *a, **k: None)
    fw_ops = types.ModuleType("tensorflow.python.framework.ops")
    fw_ops.get_collection = get_collection
    fw_ops.add_to_collection = add_to_collection
    mods = {"tensorflow": tf, "tensorflow.python": types.ModuleType("tensorflow.python"),
            "tensorflow.python.framework": types.ModuleType("tensorflow.python.framework"),
            "tensorflow.python.framework.ops": fw_ops,
            "tensorflow.python.training": types.ModuleType("tensorflow.python.training"),
            "tensorflow.python.training.moving_averages": types.ModuleType("tensorflow.python.training.moving_averages"),
            "inception": types.ModuleType("inception"), "inception.slim": types.ModuleType("inception.slim"),
            "inception.slim.losses": types.ModuleType("inception.slim.losses")}
    mods["tensorflow.python.framework"].ops = fw_ops
    mods["tensorflow.python.training"].moving_averages = mods["tensorflow.python.training.moving_averages"]
    mods["inception.slim.losses"].l2_regularizer = lambda wd: None
    mods["inception.slim"].losses = mods["inception.slim.losses"]
    mods["inception"].slim = mods["inception.slim"]
    sys.modules.update(mods)


def load_reference(slim_dir, name):
    """Execute a reference slim file by path as module inception.slim.<name>."""
    spec = importlib.util.spec_from_file_location(f"inception.slim.{name}", os.path.join(slim_dir, f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[f"inception.slim.{name}"] = mod
    setattr(sys.modules["inception.slim"], name, mod)
    spec.loader.exec_module(mod)
    return mod


def main(argv):
    if len(argv) != 2:
        raise SystemExit(__doc__.strip().splitlines()[-1])
    slim_dir = os.path.join(argv[1], SLIM_REL)
    build_stubs()
    scopes = load_reference(slim_dir, "scopes")
    load_reference(slim_dir, "variables")
    ops = load_reference(slim_dir, "ops")
    model = load_reference(slim_dir, "inception_model")
    import tensorflow as tf
    images = Tensor([64, 299, 299, 3])
    # inception_score_star_bird.py:147-164 (inference) with num_classes = 50 + 1 (:181)
    with scopes.arg_scope([ops.conv2d, ops.fc], weight_decay=0.00004):
        with scopes.arg_scope([ops.conv2d], stddev=0.1, activation=tf.nn.relu,
                              batch_norm_params={"decay": 0.9997, "epsilon": 0.001}):
            model.inception_v3(images, dropout_keep_prob=0.8, num_classes=51, is_training=False, restore_logits=True,
                               scope=None)
    out = {"source": "image_realism/IS/bird/inception/slim/{inception_model,ops,scopes,variables}.py executed under stub "
                     "tensorflow (tests/golden/make_golden_slim_variables.py), arguments of inception_score_star_bird.py "
                     "inference() with num_classes 51",
           "variables": VARIABLES}
    path = os.path.join(HERE, "slim_inception_v3_variables.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print(f"{len(VARIABLES)} variables -> {path}")


if __name__ == "__main__":
    main(sys.argv)
