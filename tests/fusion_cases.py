"""Case table for the kernels that csrc/runtime/fusion.cpp generates (a data module).

Every case names the route it must take: the region kind (an elementwise
region or a row reduction), the ops inside, the index width, thread or wave
per row, and how each leaf is read. tests/test_fusion_routes.py checks on the
host that every case plans onto that route and that the table covers every op
x dtype of `_C.fusible_ops()` and every route; tests/test_gpu_fusion_routes.py
runs the cases on the device against exact references.

The partner op of the op sweep is a multiplication by the scalar placeholder
`one` (fed 1): it is exact, keeps NaN and the sign of zero, and makes the
smallest region that still fuses (two compute ops).

A case's `ref(feeds)` is the reference in numpy, one array per fetch, and
`check` names how it is compared:
  exact   bit for bit (NaN wherever the reference has NaN)
  exact0  as exact, but +0.0 equals -0.0: for max / min / relu of zeros of
          both signs IEEE 754 leaves the sign open, and numpy's own choice
          is not a rule of this engine
  ulp     against a higher-precision reference, within a limit measured on
          the host executor (see the GPU test)
  device  no numpy reference (f64 Erf): fused equals op by op only
  rowred  row reductions: exact ops exactly, float Sum / Mean / Prod within
          the bound of any summation order
"""
import math
from collections import namedtuple

import numpy as np

from tensorframes_amd import tf
from tensorframes_amd.graph import dsl

DTYPES = ("float32", "float64", "int32", "int64")
FLOATS = ("float32", "float64")
TF_DT = {"float32": tf.float32, "float64": tf.float64, "int32": tf.int32, "int64": tf.int64, "uint8": tf.uint8}

# build() -> (graph, fetch names, feed names); feeds() -> {feed name: array}
Case = namedtuple("Case", "id build feeds ref check kind ops idx row leaves op dtype")


def line_of(case):
    """What the plan line of the case's region must contain after its name."""
    s = "[%s] " % case.ops
    tail = " idx%d%s leaves[%s]" % (case.idx, " " + case.row if case.row else "", ",".join(case.leaves))
    return s, tail


# ------------------------------------------------------------------ feeds
def float_edges(dtype):
    """The edge values every float case is fed (see the issue list in the module
    docstring of the GPU test), followed by ordinary values of both signs."""
    dt = np.dtype(dtype).type
    fi = np.finfo(dt)
    up = lambda v: np.nextafter(dt(v), dt(np.inf))    # noqa: E731
    dn = lambda v: np.nextafter(dt(v), dt(-np.inf))   # noqa: E731
    v = [np.nan, np.inf, -np.inf, 0.0, -0.0, fi.tiny, -fi.tiny, fi.tiny / 4, -fi.tiny / 4, fi.max, -fi.max,
         1.0, -1.0, 6.0, up(0), dn(0), up(6), dn(6), up(20), dn(20), 20.0, 21.0, 30.0, 36.0, 37.0, 40.0,
         0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 2.0, 3.0, -2.0, -3.0, -6.0, -20.0, -37.0, -40.0, 88.0, 89.0, -104.0,
         709.0, 710.0, -746.0, 0.1, -0.1, 1e-3, -1e-3, 0.999, 1e4, -1e4, math.pi, -math.pi / 2]
    rng = np.random.default_rng(7)
    return np.concatenate([np.array(v, dtype=dt), (rng.standard_normal(20) * 3).astype(dt)])


def int_edges(dtype):
    ii = np.iinfo(dtype)
    v = [ii.min, ii.max, 0, -1, 1, 2, -2, 5, 6, 7, -6, ii.min + 1, ii.max - 1, 46341, -46341, 65536, 3037000500 % ii.max,
         12345, -12345, 100]
    return np.array(v, dtype=dtype)


def edges(dtype):
    return float_edges(dtype) if dtype in FLOATS else int_edges(dtype)


def grid(dtype):
    """(x, y): every pair of edge values."""
    e = edges(dtype)
    return np.repeat(e, e.size), np.tile(e, e.size)


ONE = lambda dtype: np.ones((), dtype)  # noqa: E731


# ------------------------------------------------------------------ references of the op sweep
def _sign(x):
    # Sign(NaN) is 0: `(x > 0) - (x < 0)` on the device and in ATen alike (numpy gives NaN)
    with np.errstate(invalid="ignore"):
        return ((x > 0).astype(x.dtype) - (x < 0).astype(x.dtype)).astype(x.dtype)


def _relu(x):
    return np.where(x < 0, x.dtype.type(0), x)


def _relu6(x):
    return np.where(x < 0, x.dtype.type(0), np.where(x > 6, x.dtype.type(6), x))


def _leaky(x):
    alpha = x.dtype.type(np.float32(0.2))  # the attribute is a float32
    return np.where(x >= 0, x, x * alpha)


def _nanmax(a, b):
    return np.where(np.isnan(a) | np.isnan(b), a + b, np.where(a > b, a, b)) if a.dtype.kind == "f" else np.maximum(a, b)


def _nanmin(a, b):
    return np.where(np.isnan(a) | np.isnan(b), a + b, np.where(a < b, a, b)) if a.dtype.kind == "f" else np.minimum(a, b)


def _divnonan(a, b):
    return np.where(b == 0, a.dtype.type(0), a / np.where(b == 0, a.dtype.type(1), b))


def _hi(x):
    return x.astype(np.longdouble if x.dtype == np.float64 else np.float64)


_SELU_SCALE = "1.0507009873554804934193349852946"
_SELU_ALPHA = "1.6732632423543772848170429916717"


def _selu(h):
    s, a = h.dtype.type(_SELU_SCALE), h.dtype.type(_SELU_ALPHA)
    return np.where(h > 0, s * h, s * a * np.expm1(h))


def _softplus(h):
    return np.maximum(h, 0) + np.log1p(np.exp(-np.abs(h)))


def _erf(h):
    return np.array([math.erf(v) for v in h.astype(np.float64)], np.float64)


# op -> (reference, check). "ulp" references take and return the higher precision.
UNARY_REF = {
    "Neg": (lambda x: -x, "exact"),
    "Abs": (np.abs, "exact"),
    "Square": (lambda x: x * x, "exact"),
    "Sqrt": (np.sqrt, "exact"),
    "Rsqrt": (lambda x: x.dtype.type(1) / np.sqrt(x), "exact"),
    "Exp": (np.exp, "ulp"),
    "Log": (np.log, "ulp"),
    "Log1p": (np.log1p, "ulp"),
    "Expm1": (np.expm1, "ulp"),
    "Reciprocal": (lambda x: x.dtype.type(1) / x, "exact"),
    "Inv": (lambda x: x.dtype.type(1) / x, "exact"),
    "Relu": (_relu, "exact0"),
    "Relu6": (_relu6, "exact0"),
    "Elu": (lambda h: np.where(h > 0, h, np.expm1(h)), "ulp"),
    "Selu": (_selu, "ulp"),
    "Sigmoid": (lambda h: 1 / (1 + np.exp(-h)), "ulp"),
    "Tanh": (np.tanh, "ulp"),
    "Softplus": (_softplus, "ulp"),
    "Softsign": (lambda x: x / (x.dtype.type(1) + np.abs(x)), "exact"),
    "Floor": (np.floor, "exact"),
    "Ceil": (np.ceil, "exact"),
    "Rint": (np.rint, "exact"),
    "Round": (np.rint, "exact"),      # half to even, as TensorFlow's Round
    "Sign": (_sign, "exact"),
    "Sin": (np.sin, "ulp"),
    "Cos": (np.cos, "ulp"),
    "Erf": (_erf, "ulp"),             # float32 only; float64 is "device"
    "LeakyRelu": (_leaky, "exact"),
}
BINARY_REF = {
    "Add": (lambda a, b: a + b, "exact"),
    "AddV2": (lambda a, b: a + b, "exact"),
    "BiasAdd": (lambda a, b: a + b, "exact"),
    "Sub": (lambda a, b: a - b, "exact"),
    "Mul": (lambda a, b: a * b, "exact"),
    "Div": (lambda a, b: a / b, "exact"),
    "RealDiv": (lambda a, b: a / b, "exact"),
    "Maximum": (_nanmax, "exact0"),
    "Minimum": (_nanmin, "exact0"),
    "SquaredDifference": (lambda a, b: (a - b) * (a - b), "exact"),
    "Pow": (np.power, "ulp"),
    "DivNoNan": (_divnonan, "exact"),
}
VIEW_OPS = ("Identity", "Snapshot", "StopGradient", "PreventGradient")


def quiet(f):
    def g(*a):
        with np.errstate(all="ignore"):
            return f(*a)
    return g


# ------------------------------------------------------------------ graph helpers
def _ph(dtype, shape, name):
    return tf.placeholder(TF_DT[dtype], shape, name=name)


def _unary(op, x, name=None):
    if op == "LeakyRelu":
        return tf.nn.leaky_relu(x, 0.2, name=name)
    return dsl._unary(op, x, name)


def _graph(body):
    """build() of a case from `body(g) -> (fetch names, feed names)`."""
    def build():
        g = tf.Graph()
        with g.as_default():
            fetches, feeds = body()
        return g, fetches, feeds
    return build


def _mk(id, body, feeds, ref, check, kind, ops, leaves, idx=32, row=None, op=None, dtype=None):
    return Case(id, _graph(body), feeds, quiet(ref), check, kind, ops, idx, row, tuple(leaves), op, dtype)


C, S, X = "contiguous", "scalar", "strided"


# ------------------------------------------------------------------ op sweep
def _sweep_unary(op, dtype):
    ref, check = UNARY_REF[op]
    if op == "Erf" and dtype == "float64":
        check = "device"

    def body():
        y = _unary(op, _ph(dtype, [None], "x"))
        tf.multiply(y, _ph(dtype, [], "one"), name="y")
        return ["y"], ["x", "one"]

    def reference(f):
        x = f["x"]
        if check in ("ulp", "device"):
            return [ref(_hi(x))]
        return [ref(x)]
    return _mk("sweep-%s-%s" % (op, dtype), body, lambda: {"x": edges(dtype), "one": ONE(dtype)}, reference, check,
               "FUSED", op + " Mul", [C, S], op=op, dtype=dtype)


def _sweep_binary(op, dtype):
    ref, check = BINARY_REF[op]
    if op == "BiasAdd":
        def body():
            y = tf.nn.bias_add(_ph(dtype, [None, edges(dtype).size], "x"), _ph(dtype, [edges(dtype).size], "b"))
            tf.multiply(y, _ph(dtype, [], "one"), name="y")
            return ["y"], ["x", "b", "one"]

        def feeds():
            e = edges(dtype)
            return {"x": np.repeat(e, e.size).reshape(e.size, e.size), "b": e, "one": ONE(dtype)}
        return _mk("sweep-BiasAdd-" + dtype, body, feeds, lambda f: [f["x"] + f["b"]], check, "FUSED", "BiasAdd Mul",
                   [C, X, S], op=op, dtype=dtype)

    def body():
        y = dsl._binary(op, _ph(dtype, [None], "x"), _ph(dtype, [None], "z"), None)
        tf.multiply(y, _ph(dtype, [], "one"), name="y")
        return ["y"], ["x", "z", "one"]

    def feeds():
        x, z = grid(dtype)
        return {"x": x, "z": z, "one": ONE(dtype)}

    def reference(f):
        if check == "ulp":
            return [ref(_hi(f["x"]), _hi(f["z"]))]
        return [ref(f["x"], f["z"])]
    return _mk("sweep-%s-%s" % (op, dtype), body, feeds, reference, check, "FUSED", op + " Mul", [C, C, S],
               op=op, dtype=dtype)


def _sweep_view(op, dtype):
    """Views and broadcasts in regions whose result depends on their indexing:
    a [n] (or [m]) vector meets a full [n, m] matrix through the op."""
    n, m = 7, 5

    def mat():
        e = edges(dtype)
        return np.resize(e, n * m).reshape(n, m)

    def vec(k, shape):
        e = edges(dtype)[::-1]
        return np.resize(e, k).reshape(shape).copy()
    one = lambda: _ph(dtype, [], "one")  # noqa: E731
    if op in VIEW_OPS:
        def body():
            y = _unary(op, tf.multiply(_ph(dtype, [None], "x"), one()))
            tf.multiply(y, _ph(dtype, [], "one2"), name="y")
            return ["y"], ["x", "one", "one2"]
        return _mk("sweep-%s-%s" % (op, dtype), body,
                   lambda: {"x": edges(dtype), "one": ONE(dtype), "one2": ONE(dtype)}, lambda f: [f["x"]], "exact",
                   "FUSED", "Mul %s Mul" % op, [C, S, S], op=op, dtype=dtype)
    spec = {
        # op: (shape of a, how a reaches [n, m], numpy view of a)
        "ExpandDims": ([n], lambda a: tf.expand_dims(a, 1), lambda a: a.reshape(n, 1)),
        "Squeeze": ([1, n, 1], lambda a: tf.squeeze(a, [0]), lambda a: a.reshape(n, 1)),
        "Reshape": ([n], lambda a: tf.reshape(a, [n, 1]), lambda a: a.reshape(n, 1)),
        "Tile": ([1, m], lambda a: tf.tile(a, [n, 1]), lambda a: a.reshape(1, m)),
        "BroadcastTo": ([m], lambda a: tf.broadcast_to(a, [n, m]), lambda a: a.reshape(1, m)),
    }[op]

    def body():
        a = spec[1](_ph(dtype, spec[0], "a"))
        tf.multiply(tf.add(a, _ph(dtype, [n, m], "c")), one(), name="y")
        return ["y"], ["a", "c", "one"]
    return _mk("sweep-%s-%s" % (op, dtype), body,
               lambda: {"a": vec(int(np.prod(spec[0])), spec[0]), "c": mat(), "one": ONE(dtype)},
               lambda f: [spec[2](f["a"]) + f["c"]], "exact", "FUSED", "%s Add Mul" % op, [X, C, S], op=op, dtype=dtype)


def cast_values(src, dst):
    """In-range inputs only: out-of-range and NaN float -> int are undefined."""
    if src == "uint8":
        return np.array([0, 1, 2, 127, 128, 200, 254, 255], np.uint8)
    if src in FLOATS:
        if dst in FLOATS:
            return float_edges(src)
        big = 2.0 ** 30 if dst == "int32" or src == "float32" else 2.0 ** 52
        return np.array([0.0, -0.0, 0.5, -0.5, 0.999, -0.999, 1.0, -1.0, 1.5, -1.5, 2.5, -2.5, 1e-30, 100.75, -100.75,
                         big, -big, 2.0 ** 24 + 2, -(2.0 ** 24) - 2], src)
    v = int_edges(src)
    if dst == "int32" and src == "int64":
        v = v[(v >= np.iinfo(np.int32).min) & (v <= np.iinfo(np.int32).max)]
    extra = np.array([2 ** 24 + 1, 2 ** 24 + 3, -(2 ** 24) - 1, 2 ** 30 + 65], src)  # ties and odd bits for -> f32
    if src == "int64":
        extra = np.concatenate([extra, np.array([2 ** 53 + 1, 2 ** 53 + 3, -(2 ** 53) - 1, 2 ** 62 + 2 ** 9 + 1], src)])
        if dst == "int32":
            extra = extra[:0]
    return np.concatenate([v, extra])


def _sweep_cast(src, dst):
    def body():
        y = tf.cast(_ph(src, [None], "x"), TF_DT[dst])
        tf.multiply(y, _ph(dst, [], "one"), name="y")
        return ["y"], ["x", "one"]
    return _mk("sweep-Cast-%s-to-%s" % (src, dst), body, lambda: {"x": cast_values(src, dst), "one": ONE(dst)},
               lambda f: [f["x"].astype(dst)], "exact", "FUSED", "Cast Mul", [C, S], op="Cast", dtype=dst)


def sweep_cases(fusible):
    """One case per op x dtype of `fusible` (the dict `_C.fusible_ops()` returns)."""
    out = []
    for op, facts in sorted(fusible.items()):
        for dtype in DTYPES:
            if facts["float_only"] and dtype not in FLOATS:
                continue
            if facts["kind"] == "unary":
                out.append(_sweep_unary(op, dtype))
            elif facts["kind"] == "binary":
                out.append(_sweep_binary(op, dtype))
            elif facts["kind"] in ("view", "broadcast"):
                out.append(_sweep_view(op, dtype))
    for dst in DTYPES:
        for src in DTYPES + ("uint8",):
            if src != dst:
                out.append(_sweep_cast(src, dst))
    return out


# ------------------------------------------------------------------ element loop geometry
# block 256 x 4 elements per thread: around one thread row, one block, and three blocks with a ragged tail
GEOMETRY_N = (1, 255, 256, 257, 1023, 1024, 1025, 2 * 1024 + 517)


def _geometry(n, dtype):
    def body():
        tf.multiply(tf.negative(_ph(dtype, [None], "x")), _ph(dtype, [], "one"), name="y")
        return ["y"], ["x", "one"]

    def feeds():
        x = np.arange(n).astype(dtype) - dtype_mid(dtype)
        return {"x": x, "one": ONE(dtype)}
    # with one output element every stride is zero, and a leaf whose strides equal the output's is read as p[i]
    return _mk("geometry-n%d-%s" % (n, dtype), body, feeds, lambda f: [-f["x"]], "exact", "FUSED", "Neg Mul",
               [C, C] if n == 1 else [C, S])


def dtype_mid(dtype):
    return np.dtype(dtype).type(3)


# ------------------------------------------------------------------ leaf kinds and index decomposition
DIMS4 = (3, 5, 7, 11)  # no power of two: a wrong divisor shows


def _vals(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-9, 10, size=shape).astype(dtype)  # small integers: every result is exact


def _leaves_strided(dtype):
    """Contiguous, scalar and strided leaves in one region; the strided ones
    broadcast over the last, a middle, the first and two non-adjacent dims of
    a rank-4 output, so collapse() can merge no pair of dims."""
    d = DIMS4
    shapes = {"x": list(d), "a": [d[0], d[1], d[2], 1], "b": [d[0], 1, d[2], d[3]], "c": [d[1], d[2], d[3]],
              "d": [1, d[1], 1, d[3]]}

    def body():
        p = {k: _ph(dtype, s, k) for k, s in shapes.items()}
        y = tf.add(tf.subtract(tf.multiply(tf.add(p["x"], p["a"]), p["b"]), p["c"]), p["d"])
        tf.multiply(y, _ph(dtype, [], "one"), name="y")
        return ["y"], list(shapes) + ["one"]

    def feeds():
        f = {k: _vals(s, dtype, i) for i, (k, s) in enumerate(shapes.items())}
        f["one"] = ONE(dtype)
        return f
    return _mk("leaves-rank4-strided-" + dtype, body, feeds,
               lambda f: [((f["x"] + f["a"]) * f["b"] - f["c"]) + f["d"]], "exact", "FUSED", "Add Mul Sub Add Mul",
               [C, X, X, X, X, S])


def _leaves_mergeable(dtype):
    d = list(DIMS4)

    def body():
        y = tf.subtract(tf.multiply(_ph(dtype, d, "x"), _ph(dtype, d, "a")), _ph(dtype, d, "b"))
        tf.multiply(y, _ph(dtype, [], "one"), name="y")
        return ["y"], ["x", "a", "b", "one"]

    def feeds():
        return {"x": _vals(d, dtype, 1), "a": _vals(d, dtype, 2), "b": _vals(d, dtype, 3), "one": ONE(dtype)}
    return _mk("leaves-rank4-mergeable-" + dtype, body, feeds, lambda f: [f["x"] * f["a"] - f["b"]], "exact", "FUSED",
               "Mul Sub Mul", [C, C, C, S])


def _leaf_twice(dtype):
    n = 5

    def body():
        v = _ph(dtype, [n], "v")
        y = tf.subtract(tf.expand_dims(v, 0), tf.multiply(tf.expand_dims(v, 1), _ph(dtype, [], "two")))
        tf.identity(y, name="y")
        return ["y"], ["v", "two"]
    return _mk("leaf-twice-" + dtype, body,
               lambda: {"v": np.array([1, -2, 3, 5, -7], dtype), "two": np.array(2, dtype)},
               lambda f: [f["v"][None, :] - f["v"][:, None] * f["two"]], "exact", "FUSED",
               "ExpandDims ExpandDims Mul Sub Identity", [X, X, S])


def _unit_dims(dtype):
    def body():
        y = tf.multiply(tf.negative(_ph(dtype, [1, 1], "x")), _ph(dtype, [], "one"))
        tf.identity(y, name="y")
        return ["y"], ["x", "one"]
    return _mk("unit-dims-" + dtype, body, lambda: {"x": np.array([[5]], dtype), "one": ONE(dtype)},
               lambda f: [-f["x"]], "exact", "FUSED", "Neg Mul Identity", [C, C])  # one element: see _geometry


# ------------------------------------------------------------------ row reductions
RED_OPS = ("Sum", "Mean", "Min", "Max", "Prod", "ArgMin", "ArgMax")
RED_FN = {"Sum": tf.reduce_sum, "Mean": tf.reduce_mean, "Min": tf.reduce_min, "Max": tf.reduce_max,
          "Prod": tf.reduce_prod, "ArgMin": tf.argmin, "ArgMax": tf.argmax}
# 256 is the smallest row count that fuses; 302 is no multiple of the 4 rows of a wave block
ROWRED_SHAPES = [(256, i) for i in (1, 3, 16, 17, 63, 64, 65, 129, 1000)] + \
                [(257, 16), (257, 17), (257, 129), (302, 16), (302, 65), (302, 1000)]


def rowred_feed(dtype, outer, inner):
    """[outer, inner] with the rows where a reduction goes wrong first; the
    other rows hold ordinary values (magnitudes around 1, so that a product of
    1000 of them stays finite)."""
    rng = np.random.default_rng(outer * 1009 + inner)
    last = inner - 1
    if dtype in FLOATS:
        x = (rng.uniform(0.5, 1.5, size=(outer, inner)) * rng.choice([-1.0, 1.0], size=(outer, inner))).astype(dtype)
        x[0, :] = 1.0                                      # a whole row of ties: the first index
        x[1, :] = 1.0
        x[1, [min(2, last), last]] = 3.0                   # partial ties of the maximum ...
        x[1, [min(1, last), max(last - 1, 0)]] = -3.0      # ... and of the minimum
        x[2, 0] = np.nan                                   # NaN at index 0
        x[3, 64 if inner > 64 else min(1, last)] = np.nan  # lane 0's second element (a wave strides by 64)
        x[4, min(5, last)] = np.nan                        # a lane other than 0
        x[5, last] = np.nan                                # the last element
        x[6, :] = np.nan                                   # all NaN
        x[7, :] = np.inf
        x[8, :] = -np.inf
        x[9, ::2] = np.inf                                 # +inf and, from inner 2, -inf: Sum is NaN
        x[9, 1::2] = -np.inf
        x[10, ::2] = -0.0                                  # ties of zeros of both signs
        x[10, 1::2] = 0.0
        x[11, :] = 1.0
        x[11, [min(3, last), last]] = np.nan               # two NaNs: the first one
        x[11, min(1, last)] = np.inf
        x[12, last] = np.inf                               # an infinity after ordinary values
        x[13, 0] = -np.inf
        return x
    ii = np.iinfo(dtype)
    x = rng.integers(-3, 4, size=(outer, inner)).astype(dtype)
    x[0, :] = 7
    x[1, :] = 0
    x[1, [min(2, last), last]] = 9
    x[1, [min(1, last), max(last - 1, 0)]] = -9
    x[2, :] = ii.max                                       # Sum wraps
    x[3, :] = ii.min
    x[4, :] = 3                                            # Prod wraps from inner 21 (int32) / 41 (int64)
    x[5, :] = -1
    x[5, 0] = -5                                           # Mean of a negative sum truncates towards zero
    x[6, :] = 46341                                        # squares past int32
    x[7, 0], x[7, last] = ii.min, ii.max
    x[8, :] = -2
    return x


def _trunc_div(s, n):
    q = s // n
    return q + ((s % n != 0) & (s < 0))


def rowred_reference(op, x):
    """Reference of one row reduction over the last axis of a 2-d array.
    Float Sum / Mean / Prod come back in longdouble (the caller applies the
    bound); everything else is exact in the output dtype."""
    fl = x.dtype.kind == "f"
    with np.errstate(all="ignore"):
        if op in ("ArgMin", "ArgMax"):
            r = (np.argmin if op == "ArgMin" else np.argmax)(x, axis=1)  # the first NaN, else the first extremum
            return r.astype(np.int64)
        if op in ("Min", "Max"):
            return (np.min if op == "Min" else np.max)(x, axis=1)       # NaN propagates
        if fl:
            h = x.astype(np.longdouble)
            return {"Sum": h.sum(1), "Mean": h.sum(1) / x.shape[1], "Prod": h.prod(1)}[op]
        if op == "Prod":
            return np.prod(x, axis=1, dtype=x.dtype)                     # wraps
        s = np.sum(x.astype(np.int64), axis=1, dtype=np.int64)           # wraps at 64 bits only
        if op == "Sum":
            return s.astype(x.dtype)                                     # the low bits: wraps
        return _trunc_div(s, x.shape[1]).astype(x.dtype)                 # Mean: truncated quotient of the 64-bit sum


def _rowred(dtype, outer, inner, prologue):
    def body():
        x = _ph(dtype, [None, inner], "x")
        v = tf.multiply(x, _ph(dtype, [], "one")) if prologue else x
        for op in RED_OPS:
            RED_FN[op](v, 1, name="y" + op)
        return ["y" + op for op in RED_OPS], ["x", "one"] if prologue else ["x"]

    def feeds():
        f = {"x": rowred_feed(dtype, outer, inner)}
        if prologue:
            f["one"] = ONE(dtype)
        return f
    ops = ("Mul -> " if prologue else "") + " ".join(RED_OPS)
    return _mk("rowred-%s-%dx%d-%s" % (dtype, outer, inner, "prologue" if prologue else "siblings"), body, feeds,
               lambda f: [rowred_reference(op, f["x"]) for op in RED_OPS], "rowred", "FUSED-ROWRED", ops,
               [C, S] if prologue else [C], row="wave" if inner > 16 else "thread")


def _rowred_nd(dtype, xshape, cshape, axes, red, row, outer_strided):
    """Reductions over trailing axes of a rank-3 / rank-4 tensor whose prologue
    adds a strided leaf, so the reduced (or the outer) dims cannot collapse and
    the kernel decomposes the index (`jj % D`, `rr % D`)."""
    def body():
        v = tf.add(_ph(dtype, list(xshape), "x"), _ph(dtype, list(cshape), "c"))
        for op in red:
            RED_FN[op](v, axes if len(axes) > 1 else axes[0], name="y" + op)
        return ["y" + op for op in red], ["x", "c"]

    def reference(f):
        v = f["x"] + f["c"]
        outer = int(np.prod(xshape[:axes[0]]))
        out = [rowred_reference(op, v.reshape(outer, -1)).reshape(xshape[:axes[0]]) for op in red]
        return out
    return _mk("rowred-nd-%s-%s-%s" % (dtype, "x".join(map(str, xshape)), "outer" if outer_strided else "inner"), body,
               lambda: {"x": _vals(xshape, dtype, 11), "c": _vals(cshape, dtype, 12)}, reference, "rowred",
               "FUSED-ROWRED", "Add -> " + " ".join(red), [C, X], row=row)


# ------------------------------------------------------------------ the table
def with_index64(case):
    return case._replace(id=case.id + "-idx64", idx=64)


def build_cases(fusible):
    sweep = sweep_cases(fusible)
    geometry = [_geometry(n, dt) for dt in ("float32", "int64") for n in GEOMETRY_N]
    leaves = [f(dt) for dt in ("float32", "float64", "int32", "int64")
              for f in (_leaves_strided, _leaves_mergeable, _leaf_twice, _unit_dims)]
    rowred = [_rowred(dt, o, i, p) for dt in DTYPES for (o, i) in ROWRED_SHAPES for p in (True, False)]
    for dt in DTYPES:
        rowred += [
            _rowred_nd(dt, (260, 3, 5), (3, 1), [1, 2], ("Sum", "Mean", "Min", "Max", "Prod"), "thread", False),
            _rowred_nd(dt, (64, 5, 3, 7), (3, 1), [2, 3], ("Sum", "Mean", "Min", "Max", "Prod"), "wave", False),
            _rowred_nd(dt, (52, 5, 33), (5, 1), [2], RED_OPS, "wave", True),
            _rowred_nd(dt, (52, 5, 7), (5, 1), [2], RED_OPS, "thread", True),
        ]
    # the 64-bit index variant: every geometry, leaf and row-reduction case again, and of the op sweep one
    # unary, one binary, one view and one cast region per dtype (the index type does not enter a formula)
    wide = [c for c in sweep if c.op in ("Abs", "Maximum", "Tile", "BiasAdd")]
    wide += [c for c in sweep if c.op == "Cast" and c.id.startswith("sweep-Cast-uint8")]
    return sweep + geometry + leaves + rowred + [with_index64(c) for c in wide + geometry + leaves + rowred]
