"""Every dispatch route of csrc/kernels/reduce.hip on the device against plain
numpy references in higher precision (tests/reduce_cases.py is the case table;
tests/test_reduce_routes.py proves on the host that it covers every route).

One fetch per program, fed straight from a placeholder, and every program's
plan is checked to hold the reduction as a plain op: nothing here runs inside a
generated (fused) region. The data is chosen so that the result is exact:
nonzero integers of magnitude <= 1000 held in the dtype (every partial sum is
exact in the f64 / int64 accumulator), products of powers of two, unique
extremes and special values placed at every position where a kernel changes
what it does (slice boundaries, vector lanes, the scalar tail, the unrolled
chains). A dropped, repeated or misrouted element changes the result."""
import functools
import math
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import reduce_cases as rc  # noqa: E402
from tensorframes_amd import engine, tf  # noqa: E402
from tensorframes_amd._native import _C  # noqa: E402

DEV = torch.device("cuda", 0)
CPU = torch.device("cpu")
NP = {"float32": np.float32, "float64": np.float64, "int32": np.int32, "int64": np.int64, "bool": np.bool_}
NUMERIC = [c for c in rc.REDUCE_CASES if c.dtype != "bool"]
FLOAT = [c for c in NUMERIC if c.dtype.startswith("float")]
BOOL = [c for c in rc.REDUCE_CASES if c.dtype == "bool"]
RED_FN = {"Sum": tf.reduce_sum, "Mean": tf.reduce_mean, "Min": tf.reduce_min, "Max": tf.reduce_max,
          "Prod": tf.reduce_prod, "All": tf.reduce_all, "Any": tf.reduce_any}


def seed_of(*parts):
    return zlib.crc32("/".join(map(str, parts)).encode())


def make_program(build, fetches, names, op_name, sample):
    """A program with its plan checked: `op_name` runs as a plain op, no fused region."""
    g = tf.Graph()
    with g.as_default():
        build()
    prog = engine.program(g.serialize(), fetches, names)
    plan = prog.describe([torch.as_tensor(s) for s in sample], as_gpu=True)
    assert "FUSED" not in plan and " 0 fused regions" in plan, plan
    assert ("OP   %s " % op_name) in plan, plan
    return prog


def run(prog, arrays, device=DEV):
    outs = engine.run_program(prog, [torch.as_tensor(np.ascontiguousarray(a)) for a in arrays], device)
    return [o.cpu().numpy() for o in outs]


def same(got, want):
    """== plus isnan: NaN matches NaN, the sign of a zero is not pinned."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind == "f":
        return bool(np.all((got == want) | (np.isnan(got) & np.isnan(want))))
    return bool(np.array_equal(got, want))


def assert_same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not same(got, want):
        bad = ~((got == want) | ((got != got) & (want != want))) if got.dtype.kind == "f" else got != want
        idx = np.argwhere(bad)
        first = tuple(idx[0])
        raise AssertionError("%s: %d of %d differ, first at %s: got %r, want %r"
                             % (what, len(idx), got.size, first, got[first], want[first]))


# ------------------------------------------------------------------ [outer, r, inner] <-> the op's input
def from_canonical(x3, case):
    """The op's input whose reduction the kernel sees as x3 [outer, r, inner]."""
    shape, axes = case.shape, sorted(case.axes)
    outer, r, inner, adjacent = rc.canonical(shape, axes)
    if adjacent:
        return x3.reshape(shape)
    kept = [i for i in range(len(shape)) if i not in axes]
    perm = kept + axes
    x = x3.reshape([shape[i] for i in perm])
    return np.ascontiguousarray(np.transpose(x, np.argsort(perm)))


def out_shape(case):
    if case.keep_dims:
        return tuple(1 if i in case.axes else d for i, d in enumerate(case.shape))
    return tuple(d for i, d in enumerate(case.shape) if i not in case.axes)


@functools.lru_cache(maxsize=None)
def reduce_program(op, dtype, rank, axes, keep):
    def build():
        x = tf.placeholder(NP[dtype], [None] * rank, name="x")
        RED_FN[op](x, list(axes), keep_dims=keep, name="y")
    sample = np.zeros((1,) * rank, NP[dtype])
    return make_program(build, ["y"], ["x"], op, [sample])


def device_reduce(op, case, x3):
    prog = reduce_program(op, case.dtype, len(case.shape), tuple(case.axes), case.keep_dims)
    (y,) = run(prog, [from_canonical(x3, case)])
    assert y.shape == out_shape(case), (y.shape, out_shape(case))
    return y.reshape(x3.shape[0], x3.shape[2])


def ref_reduce(op, x3):
    """numpy in the accumulator's precision or better. For the exact data of
    these tests the order of a float64 / int64 sum or product does not matter,
    so this is the exact result, rounded once into the dtype."""
    dt = x3.dtype
    r = x3.shape[1]
    with np.errstate(all="ignore"):
        if dt.kind == "f":
            xd = x3.astype(np.float64)
            if op == "Sum":
                return xd.sum(1).astype(dt)
            if op == "Mean":
                return (xd.sum(1) / np.float64(r)).astype(dt)
            if op == "Prod":
                return xd.prod(1).astype(dt)
            return (xd.min(1) if op == "Min" else xd.max(1)).astype(dt)  # numpy propagates NaN
        if dt.kind == "b":
            return x3.all(1) if op == "All" else x3.any(1)
        xi = x3.astype(np.int64)
        if op == "Sum":
            return xi.sum(1).astype(dt)                                  # wraps into the dtype
        if op == "Mean":
            s = xi.sum(1)
            return (np.sign(s) * (np.abs(s) // r)).astype(dt)            # truncates toward zero
        if op == "Prod":
            return xi.prod(1).astype(dt)
        return x3.min(1) if op == "Min" else x3.max(1)


def exact_data(rng, case):
    """Nonzero integers, |x| <= 1000, in the dtype."""
    outer, r, inner, _ = rc.canonical(case.shape, case.axes)
    x = rng.integers(1, 1001, (outer, r, inner)) * rng.choice([-1, 1], (outer, r, inner))
    return x.astype(NP[case.dtype])


def prod_data(rng, case, wrap=False):
    """Factors 1, -1, 2 and (floats) 0.5 in random order: every partial product
    is a power of two within 2^+-103, so any order gives the same exact result.
    wrap (int32): thirty factors of 3, whose product wraps."""
    outer, r, inner, _ = rc.canonical(case.shape, case.axes)
    isf = case.dtype.startswith("float")
    pat = np.ones(r, np.float64)
    k = min(r // 3, 100) if isf else 0
    pat[:k] = 2
    pat[k:2 * k] = 0.5
    extra = min(3 if isf else 12, r - 2 * k)      # the result is +-8 (floats), +-4096 (integers)
    pat[2 * k:2 * k + extra] = 2
    if wrap:
        pat[extra:extra + 30] = 3
    x = np.broadcast_to(pat[None, :, None], (outer, r, inner)).copy()
    x = rng.permuted(x, axis=1)
    x *= rng.choice([-1, 1], x.shape)
    return x.astype(NP[case.dtype])


def probe_positions(case):
    """Indices along r where a kernel changes what it does."""
    outer, r, inner, _ = rc.canonical(case.shape, case.axes)
    info = _C.reduce_route_info(case.dtype, outer, r, inner)
    S, rps = info["S"], info["rows_per_split"]
    vec = 16 // rc.WIDTH[case.dtype]
    pos = {0, r - 1}
    for s in range(1, S):                       # each side of every slice boundary
        pos |= {s * rps - 1, s * rps}
    route = case.route
    if route.startswith("row_wave"):
        nv = r // vec * vec
        pos |= {vec - 1, nv - 1, nv, 63, 64, 64 * vec - 1, 64 * vec}   # last vector lane, scalar tail, lane 63 / next trip
    elif route == "row_block":
        pos |= {u * 1024 for u in range(9)} | {u * 1024 + 1023 for u in range(8)}  # the 8 unrolled loads
        pos |= {r // 8192 * 8192 - 1, r // 8192 * 8192}                               # last full trip / tail
    elif route.startswith("row_split"):
        pos |= {255, 256, rps - 1, (S - 1) * rps + 255}
    else:                                       # column kernels: 4 chains per slice, then the leftover rows
        for s in {0, S - 1}:
            r0, r1 = s * rps, min(r, (s + 1) * rps)
            pos |= {r0, r0 + 1, r0 + 2, r0 + 3, r0 + (r1 - r0) // 4 * 4 - 1, r0 + (r1 - r0) // 4 * 4, r1 - 1}
    return sorted(p for p in pos if 0 <= p < r)


def few_positions(case):
    """A smaller set for values that only pass through + and *."""
    outer, r, inner, _ = rc.canonical(case.shape, case.axes)
    info = _C.reduce_route_info(case.dtype, outer, r, inner)
    rps = info["rows_per_split"]
    vec = 16 // rc.WIDTH[case.dtype]
    pos = {0, r - 1, vec - 1, r // vec * vec, r // 2}
    if info["S"] > 1:
        pos |= {rps - 1, rps}
    return sorted(p for p in pos if 0 <= p < r)


def run_probes(op, case, base, probes):
    """Each probe (position, value) goes into an output element of its own
    (several runs when there are more probes than outputs); the whole result
    of every run is compared with the reference."""
    outer, r, inner = base.shape
    m = outer * inner
    for start in range(0, len(probes), m):
        x3 = base.copy()
        flat = x3.reshape(outer, r, inner)
        for k, (p, v) in enumerate(probes[start:start + m]):
            flat[k // inner, p, k % inner] = v
        assert_same(device_reduce(op, case, x3), ref_reduce(op, x3), "%s %s probes %d.." % (op, case.id, start))


# ------------------------------------------------------------------ Sum / Mean / Min / Max / Prod
@pytest.mark.parametrize("case", NUMERIC, ids=[c.id for c in NUMERIC])
def test_reduce_exact(case):
    rng = np.random.default_rng(seed_of("exact", case.id))
    x3 = exact_data(rng, case)
    for op in ("Sum", "Mean", "Min", "Max"):
        assert_same(device_reduce(op, case, x3), ref_reduce(op, x3), op)
    p3 = prod_data(rng, case)
    want = ref_reduce("Prod", p3)
    assert np.all(np.isfinite(want.astype(np.float64))) and np.all(want != 0)
    assert_same(device_reduce("Prod", case, p3), want, "Prod")
    if case.dtype == "int32" and x3.shape[1] >= 45:
        w3 = prod_data(rng, case, wrap=True)
        assert abs(int(w3[0, :, 0].astype(object).prod())) > 2 ** 31  # it does wrap
        assert_same(device_reduce("Prod", case, w3), ref_reduce("Prod", w3), "Prod (wrapping)")


@pytest.mark.parametrize("case", NUMERIC, ids=[c.id for c in NUMERIC])
def test_reduce_min_max_unique_extreme_everywhere(case):
    rng = np.random.default_rng(seed_of("extreme", case.id))
    base = exact_data(rng, case)
    pos = probe_positions(case)
    run_probes("Max", case, base, [(p, 5000) for p in pos])
    run_probes("Min", case, base, [(p, -5000) for p in pos])
    if case.dtype == "int64":
        # neighbours that a pass through float64 cannot tell apart
        big = (np.int64(1) << 62) - 4096
        hi = base.astype(np.int64) + big
        run_probes("Max", case, hi, [(p, big + 1001) for p in pos])
        run_probes("Min", case, -hi, [(p, -big - 1001) for p in pos])


@pytest.mark.parametrize("case", FLOAT, ids=[c.id for c in FLOAT])
def test_reduce_special_values(case):
    """NaN, +inf and -inf at the adversarial positions. Sum / Mean / Prod
    follow IEEE; Min / Max return NaN whenever one is present (numpy's and the
    host executor's rule)."""
    rng = np.random.default_rng(seed_of("special", case.id))
    base = exact_data(rng, case)
    pos, few = probe_positions(case), few_positions(case)
    nan, inf = np.nan, np.inf
    for op in ("Min", "Max"):
        run_probes(op, case, base, [(p, nan) for p in pos] + [(p, v) for p in few for v in (inf, -inf)])
    specials = [(p, v) for p in few for v in (nan, inf, -inf)]
    for op in ("Sum", "Mean"):
        run_probes(op, case, base, specials)
    run_probes("Prod", case, prod_data(rng, case), specials)
    # a NaN and an infinity in the same slice: NaN wins in Min / Max
    outer, r, inner = base.shape
    if r >= 2:
        x3 = base.copy()
        x3[:, 0, :] = inf
        x3[:, r - 1, :] = nan
        if r > 2:
            x3[:, r // 2, :] = -inf
        for op in ("Min", "Max"):
            got = device_reduce(op, case, x3)
            assert np.all(np.isnan(got)), op


@pytest.mark.parametrize("case", FLOAT, ids=[c.id for c in FLOAT])
def test_reduce_sum_mean_rounding_bound(case):
    """Random normals scaled by 1e6 mixed with 1e-3. The kernels accumulate in
    f64 and round once into T: |got - ref| <= eps_T/2 |ref| + r 2^-52 sum|x|
    (the second term bounds any order of r f64 additions), ref from math.fsum."""
    rng = np.random.default_rng(seed_of("bound", case.id))
    outer, r, inner, _ = rc.canonical(case.shape, case.axes)
    x3 = (rng.standard_normal((outer, r, inner)) * np.where(rng.random((outer, r, inner)) < 0.5, 1e6, 1e-3))
    x3 = x3.astype(NP[case.dtype])
    xd = x3.astype(np.float64)
    ref = np.array([[math.fsum(xd[o, :, c]) for c in range(inner)] for o in range(outer)])
    mag = np.abs(xd).sum(1)
    eps = np.finfo(NP[case.dtype]).eps
    for op, div in (("Sum", 1.0), ("Mean", float(r))):
        got = device_reduce(op, case, x3).astype(np.float64)
        bound = eps / 2 * np.abs(ref / div) + r * 2.0 ** -52 * mag / div
        err = np.abs(got - ref / div)
        worst = np.argmax(err - bound)
        assert np.all(err <= bound), (op, err.flat[worst], bound.flat[worst])


# ------------------------------------------------------------------ All / Any
@pytest.mark.parametrize("case", BOOL, ids=[c.id for c in BOOL])
def test_reduce_all_any(case):
    outer, r, inner, _ = rc.canonical(case.shape, case.axes)
    pos = probe_positions(case)
    for op, fill in (("All", True), ("Any", False)):
        base = np.full((outer, r, inner), fill, np.bool_)
        assert_same(device_reduce(op, case, base), ref_reduce(op, base), op + " uniform")
        assert_same(device_reduce(op, case, ~base), ref_reduce(op, ~base), op + " uniform, negated")
        run_probes(op, case, base, [(p, not fill) for p in pos])   # a single dissenting element
        run_probes(op, case, ~base, [(p, fill) for p in pos])      # a single agreeing element


# ------------------------------------------------------------------ empty reduced axis (defect 7)
@pytest.mark.parametrize("device", [DEV, CPU], ids=["device", "host"])
@pytest.mark.parametrize("dtype", ["float32", "float64", "int32", "int64"])
def test_reduce_over_an_empty_axis(dtype, device):
    x = np.zeros((3, 0, 2), NP[dtype])
    for op, want in (("Sum", 0), ("Prod", 1)):
        (y,) = run(reduce_program(op, dtype, 3, (1,), False), [x], device)
        assert_same(y, np.full((3, 2), want, NP[dtype]), op)
    bad = ["Min", "Max"] + (["Mean"] if dtype.startswith("int") else [])
    for op in bad:
        with pytest.raises(_C.GraphError, match="empty axis"):
            run(reduce_program(op, dtype, 3, (1,), False), [x], device)
    if dtype.startswith("float"):
        (y,) = run(reduce_program("Mean", dtype, 3, (1,), False), [x], device)
        assert y.shape == (3, 2) and y.dtype == NP[dtype] and np.all(np.isnan(y))
    # an empty kept axis is no error: the result is empty
    (y,) = run(reduce_program("Max", dtype, 3, (1,), False), [np.zeros((0, 4, 2), NP[dtype])], device)
    assert y.shape == (0, 2)


@pytest.mark.parametrize("device", [DEV, CPU], ids=["device", "host"])
def test_all_any_over_an_empty_axis(device):
    x = np.zeros((3, 0, 2), np.bool_)
    (y,) = run(reduce_program("All", "bool", 3, (1,), False), [x], device)
    assert_same(y, np.ones((3, 2), np.bool_), "All")
    (y,) = run(reduce_program("Any", "bool", 3, (1,), False), [x], device)
    assert_same(y, np.zeros((3, 2), np.bool_), "Any")


# ------------------------------------------------------------------ ArgMin / ArgMax
ARG_SHAPES = [  # (shape, axis): rows (inner == 1) and columns (inner > 1)
    ((37, 1), 1), ((37, 63), 1), ((37, 64), 1), ((37, 65), 1), ((37, 1000), 1), ((16389, 5), 1),
    ((1000, 3), 0), ((65, 257), 0), ((4, 130, 33), 1), ((2, 600, 2), 1),
]


@functools.lru_cache(maxsize=None)
def arg_program(is_min, dtype, rank, axis, out_dtype):
    def build():
        x = tf.placeholder(NP[dtype], [None] * rank, name="x")
        (tf.argmin if is_min else tf.argmax)(x, axis, output_type=NP[out_dtype], name="y")
    return make_program(build, ["y"], ["x"], "ArgMin" if is_min else "ArgMax", [np.zeros((1,) * rank, NP[dtype])])


def check_arg(x, axis, out_dtype="int64", what=""):
    for is_min in (False, True):
        (got,) = run(arg_program(is_min, x.dtype.name, x.ndim, axis, out_dtype), [x])
        want = (np.argmin if is_min else np.argmax)(x, axis=axis).astype(NP[out_dtype])  # first extreme, first NaN
        assert_same(got, want, "%s %s" % ("ArgMin" if is_min else "ArgMax", what))


@pytest.mark.parametrize("dtype", ["float32", "float64", "int32", "int64"])
@pytest.mark.parametrize("shape,axis", ARG_SHAPES, ids=["x".join(map(str, s)) + "-ax%d" % a for s, a in ARG_SHAPES])
def test_argminmax(shape, axis, dtype):
    rng = np.random.default_rng(seed_of("arg", shape, axis, dtype))
    out_dtype = "int32" if (shape[0] + axis) % 2 else "int64"
    r = shape[axis]
    x = rng.integers(-3, 4, shape).astype(NP[dtype])          # heavy ties: the lowest index wins
    check_arg(x, axis, out_dtype, "ties")
    check_arg(np.full(shape, 7, NP[dtype]), axis, out_dtype, "all equal")
    u = np.moveaxis(rng.integers(-1000, 1000, shape).astype(NP[dtype]), axis, -1).copy()
    flat = u.reshape(-1, r)                                    # one reduced slice per row of `flat`
    rows = np.arange(len(flat))
    flat[rows, rows % r] = 5000                                # unique extremes, at every position in turn
    flat[rows, (rows * 7 + 3) % r] = -5000 if r > 1 else flat[rows, 0]
    check_arg(np.ascontiguousarray(np.moveaxis(u, -1, axis)), axis, out_dtype, "unique extreme")
    if r > 2:                                                  # the extreme twice
        flat[rows, (rows % r + r // 2) % r] = 5000
        check_arg(np.ascontiguousarray(np.moveaxis(u, -1, axis)), axis, out_dtype, "duplicated extreme")
    if dtype == "int64":
        big = np.int64(1) << 60
        check_arg(np.ascontiguousarray(np.moveaxis(u, -1, axis)) + big, axis, out_dtype, "beyond 2^53")
        check_arg(-(np.ascontiguousarray(np.moveaxis(u, -1, axis)) + big), axis, out_dtype, "beyond -2^53")
    if dtype.startswith("float") and r > 1:
        v = rng.integers(-1000, 1000, (len(flat), r)).astype(NP[dtype])
        p = 1 + rows % (r - 1)                                 # a NaN at p > 0
        v[rows, p] = np.nan
        v[::3, r - 1] = np.nan                                 # every third slice: a second NaN at the end
        v[::5, 0] = np.inf
        v[1::5, 0] = -np.inf
        xn = np.ascontiguousarray(np.moveaxis(v.reshape(u.shape), -1, axis))
        check_arg(xn, axis, out_dtype, "NaN")


def test_argminmax_column_grid_stride():
    """More outputs than the column kernel's grid has threads (2048 blocks of
    256): with r == 1 every index is 0, and every output must be written."""
    x = np.arange(600000, dtype=np.float32).reshape(1, 600000)
    check_arg(x, 0, "int32", "grid stride")


# ------------------------------------------------------------------ TopK
@functools.lru_cache(maxsize=None)
def topk_program(dtype, k):
    def build():
        x = tf.placeholder(NP[dtype], [None, None], name="x")
        v, i = tf.nn.top_k(x, k, name="top")
        tf.identity(v, name="tv")
        tf.identity(i, name="ti")
    return make_program(build, ["tv", "ti"], ["x"], "TopKV2", [np.zeros((1, k), NP[dtype])])


def ref_topk(x, k):
    """Sorted by (NaN first, value descending, index ascending)."""
    rows, cols = x.shape
    idx = np.broadcast_to(np.arange(cols), x.shape)
    if x.dtype.kind == "f":
        notnan = ~np.isnan(x)
        desc = np.where(notnan, -x, 0)
    else:
        notnan = np.ones(x.shape, bool)
        desc = ~x                                              # -x - 1: descending, no overflow
    order = np.lexsort((idx, desc, notnan), axis=-1)[:, :k]
    return np.take_along_axis(x, order, 1), order.astype(np.int32)


def check_topk(x, k, what):
    vals, idx = run(topk_program(x.dtype.name, k), [x])
    cols = x.shape[1]
    assert idx.dtype == np.int32 and idx.shape == (len(x), k)
    assert idx.min() >= 0 and idx.max() < cols, (what, idx.min(), idx.max())
    srt = np.sort(idx, axis=1)
    assert np.all(srt[:, 1:] != srt[:, :-1]), what + ": an index twice in a row"
    wv, wi = ref_topk(x, k)
    assert_same(idx, wi, what + " indices")
    assert_same(vals, wv, what + " values")


@pytest.mark.parametrize("dtype", ["float32", "float64", "int32", "int64"])
@pytest.mark.parametrize("cols", [1, 5, 63, 64, 65, 1000])
def test_topk(cols, dtype):
    rng = np.random.default_rng(seed_of("topk", cols, dtype))
    rows = 9
    for k in sorted({1, min(5, cols), cols}):
        check_topk(rng.integers(-1000, 1000, (rows, cols)).astype(NP[dtype]), k, "random k=%d" % k)
        check_topk(rng.integers(-2, 3, (rows, cols)).astype(NP[dtype]), k, "ties k=%d" % k)
        check_topk(np.full((rows, cols), 3, NP[dtype]), k, "all equal k=%d" % k)      # indices 0..k-1
        if dtype == "int64":
            big = np.int64(1) << 60
            check_topk(rng.integers(-50, 50, (rows, cols)) + big, k, "beyond 2^53 k=%d" % k)
            check_topk(-(rng.integers(-50, 50, (rows, cols)) + big), k, "beyond -2^53 k=%d" % k)
        if dtype.startswith("float"):
            x = rng.integers(-5, 6, (rows, cols)).astype(NP[dtype])
            r_ = np.arange(rows)
            x[r_, r_ % cols] = np.inf
            x[r_, (r_ * 3 + 1) % cols] = -np.inf
            check_topk(x, k, "infinities k=%d" % k)
            x[r_, (r_ * 5 + 2) % cols] = np.nan                                           # one NaN per row
            check_topk(x, k, "one NaN k=%d" % k)
            x[:, ::7] = np.nan                                                            # several
            x[0, :] = np.nan                                                              # a row of nothing else
            check_topk(x, k, "several NaNs k=%d" % k)


def test_topk_row_grid_stride():
    """32769 rows: one more than the grid's 8192 blocks x 4 waves."""
    rng = np.random.default_rng(5)
    x = rng.integers(-4, 5, (32769, 3)).astype(np.float32)
    x[::11, 1] = np.nan
    check_topk(x, 2, "grid stride")


# ------------------------------------------------------------------ Softmax / LogSoftmax
@functools.lru_cache(maxsize=None)
def softmax_program(log, dtype):
    def build():
        x = tf.placeholder(NP[dtype], [None, None], name="x")
        (tf.nn.log_softmax if log else tf.nn.softmax)(x, name="y")
    return make_program(build, ["y"], ["x"], "LogSoftmax" if log else "Softmax", [np.zeros((1, 1), NP[dtype])])


def ref_softmax(x, log):
    hp = np.float64 if x.dtype == np.float32 else np.longdouble
    xh = x.astype(hp)
    with np.errstate(all="ignore"):
        z = xh - xh.max(1, keepdims=True)
        s = np.exp(z).sum(1, keepdims=True)
        return z - np.log(s) if log else np.exp(z) / s


def softmax_error(got, ref):
    """Largest |got - ref| / max(1, |ref|) over the finite entries of ref; the
    others (-inf, NaN) must match exactly."""
    fin = np.isfinite(ref)
    other_ok = np.all((got[~fin] == ref[~fin].astype(got.dtype)) | (np.isnan(got[~fin]) & np.isnan(ref[~fin])))
    if not fin.any():
        return 0.0, bool(other_ok)
    err = np.abs(got[fin].astype(ref.dtype) - ref[fin]) / np.maximum(1, np.abs(ref[fin]))
    return float(err.max()), bool(other_ok)


def softmax_input(rng, rows, cols, dtype):
    x = (rng.standard_normal((rows, cols)) * 3).astype(NP[dtype])
    off = np.where(np.arange(rows) % 3 == 0, 1e4, np.where(np.arange(rows) % 3 == 1, -1e4, 0.0))
    x = (x + off[:, None].astype(NP[dtype])).astype(NP[dtype])       # the max must be subtracted
    if cols > 1:
        r_ = np.arange(rows)
        x[r_[::4], (r_[::4] * 7) % cols] = -np.inf                   # probability 0, log -inf
    if rows > 2:
        x[2, :] = -np.inf                                            # a row of nothing else: NaN
    return x


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("rows,cols", [(37, 1), (37, 63), (37, 64), (37, 65), (37, 1000), (32769, 2)])
def test_softmax(rows, cols, dtype):
    """The tolerance is not fixed in advance: the device may err 4x what the
    host executor (ATen) errs against the same float64 / longdouble reference
    on the same input, floored at 4 eps (1 + log2 cols); the margin covers the
    different summation order of 64 lanes. Error: |got - ref| / max(1, |ref|).

    Measured on an MI355X, in units of eps of the dtype (device / host), also
    in docs/PERFORMANCE.md:

        cols (rows)   softmax f32   log f32       softmax f64   log f64
        1 (37)        0 / 0         0 / 0         0 / 0         0 / 0
        63 (37)       1.04 / 1.23   1.11 / 1.63   0.63 / 0.61   1.06 / 1.30
        64 (37)       1.20 / 0.96   1.67 / 1.07   1.19 / 1.19   1.33 / 1.37
        65 (37)       0.80 / 0.57   1.34 / 1.31   0.78 / 1.43   1.09 / 1.54
        1000 (37)     0.77 / 1.25   2.47 / 1.97   0.51 / 1.69   1.18 / 2.73
        2 (32769)     0.75 / 0.75   1.21 / 1.03   0.75 / 0.75   1.05 / 1.05
    """
    rng = np.random.default_rng(seed_of("softmax", rows, cols, dtype))
    x = softmax_input(rng, rows, cols, dtype)
    eps = float(np.finfo(NP[dtype]).eps)
    for log in (False, True):
        ref = ref_softmax(x, log)
        (dev,) = run(softmax_program(log, dtype), [x])
        (host,) = run(softmax_program(log, dtype), [x], CPU)
        derr, dok = softmax_error(dev, ref)
        herr, hok = softmax_error(host, ref)
        allowed = max(4 * herr, 4 * eps * (1 + math.log2(cols)))
        print("softmax figures: log=%d dtype=%s rows=%d cols=%d device=%.3f eps host=%.3f eps allowed=%.3f eps"
              % (log, dtype, rows, cols, derr / eps, herr / eps, allowed / eps))
        assert dok, "-inf / NaN entries differ from the reference"
        assert derr <= allowed, (log, derr, herr, allowed)
        if not log:
            fin = np.isfinite(ref).all(1)
            sums = dev[fin].astype(np.float64).sum(1)
            assert np.all(np.abs(sums - 1) <= cols * eps), np.abs(sums - 1).max()
            assert np.all(dev[fin] >= 0)


# ------------------------------------------------------------------ unsorted segment Sum / Min / Max / Prod
USEG_FN = {"Sum": tf.unsorted_segment_sum, "Min": tf.unsorted_segment_min, "Max": tf.unsorted_segment_max,
           "Prod": tf.unsorted_segment_prod}


@functools.lru_cache(maxsize=None)
def useg_program(op, dtype, ids_dtype, inner, nseg):
    def build():
        x = tf.placeholder(NP[dtype], [None, inner], name="x")
        ids = tf.placeholder(NP[ids_dtype], [None], name="ids")
        USEG_FN[op](x, ids, nseg, name="y")
    return make_program(build, ["y"], ["x", "ids"], "UnsortedSegment" + op,
                        [np.zeros((1, inner), NP[dtype]), np.zeros(1, NP[ids_dtype])])


def useg_identity(op, dtype):
    """TF's value of an empty segment: 0, 1, or the dtype's max() / lowest()."""
    lim = np.finfo(NP[dtype]) if dtype.startswith("float") else np.iinfo(NP[dtype])
    return {"Sum": 0, "Prod": 1, "Min": lim.max, "Max": lim.min}[op]


def ref_useg(op, x, ids, nseg):
    dt = x.dtype
    acc_t = np.float64 if dt.kind == "f" else np.int64
    out = np.full((nseg,) + x.shape[1:], useg_identity(op, dt.name), acc_t)
    ok = (ids >= 0) & (ids < nseg)
    ufunc = {"Sum": np.add, "Prod": np.multiply, "Min": np.minimum, "Max": np.maximum}[op]   # minimum / maximum propagate NaN
    with np.errstate(all="ignore"):
        ufunc.at(out, ids[ok].astype(np.int64), x[ok].astype(acc_t))
        return out.astype(dt)


def useg_data(rng, op, dtype, n, inner):
    if op == "Prod":
        # at most 40 factors of 2 (and of 0.5 in floats) per column: exact in any order
        x = rng.choice([-1.0, 1.0], (n, inner))
        for c in range(inner):
            k = min(n // 3, 40 if dtype.startswith("float") else 20)
            rows = rng.permutation(n)
            x[rows[:k], c] *= 2
            if dtype.startswith("float"):
                x[rows[k:2 * k], c] *= 0.5
        return x.astype(NP[dtype])
    x = rng.integers(1, 1001, (n, inner)) * rng.choice([-1, 1], (n, inner))
    return x.astype(NP[dtype])


def device_useg(case, x, ids, nseg=None):
    nseg = case.nseg if nseg is None else nseg
    (y,) = run(useg_program(case.op, case.dtype, case.ids_dtype, case.inner, nseg), [x, ids])
    return y


@pytest.mark.parametrize("case", rc.USEG_CASES, ids=[c.id for c in rc.USEG_CASES])
def test_unsorted_segment_exact(case):
    rng = np.random.default_rng(seed_of("useg", case.id))
    x = useg_data(rng, case.op, case.dtype, case.n, case.inner)
    ids = rng.integers(-2, case.nseg + 3, case.n).astype(NP[case.ids_dtype])   # some out of range, some segments empty
    assert_same(device_useg(case, x, ids), ref_useg(case.op, x, ids, case.nseg), "random ids")
    one = np.full(case.n, case.nseg - 1, NP[case.ids_dtype])                    # one segment owns every row
    assert_same(device_useg(case, x, one), ref_useg(case.op, x, one, case.nseg), "one segment")
    out = np.where(np.arange(case.n) % 2 == 0, -1, case.nseg).astype(NP[case.ids_dtype])
    assert_same(device_useg(case, x, out), ref_useg(case.op, x, out, case.nseg), "all ids out of range")
    # the same through the binding, which the aggregate path uses
    xd, idd = torch.as_tensor(x).to(DEV), torch.as_tensor(ids).to(DEV)
    got = _C.unsorted_segment_reduce(case.op, xd, idd, case.nseg).cpu().numpy()
    assert_same(got, ref_useg(case.op, x, ids, case.nseg), "binding")


SMALL_USEG = [("int32", 1, 16), ("int64", 1, 17), ("int64", 1, 200), ("float32", 3, 5), ("float64", 3, 200),
              ("float32", 65, 70), ("int32", 3, 5)]


@pytest.mark.parametrize("op", ["Sum", "Min", "Max", "Prod"])
@pytest.mark.parametrize("dtype,inner,nseg", SMALL_USEG, ids=["%s-i%d-s%d" % t for t in SMALL_USEG])
def test_unsorted_segment_one_row_and_no_rows(dtype, inner, nseg, op):
    """n == 1 and n == 0 (a partition that a filter emptied): every segment of
    an empty input gets the identity of the op and dtype, from the op and from
    the binding."""
    case = rc.UsegCase("", op, dtype, "int64", 1, inner, nseg, "", None)
    x = np.full((1, inner), 7, NP[dtype])
    for seg in (0, nseg - 1, nseg, -1):
        ids = np.array([seg], np.int64)
        assert_same(device_useg(case, x, ids), ref_useg(op, x, ids, nseg), "n=1 id=%d" % seg)
    want = np.full((nseg, inner), useg_identity(op, dtype), NP[dtype])
    x0, ids0 = np.zeros((0, inner), NP[dtype]), np.zeros(0, np.int64)
    assert_same(device_useg(case, x0, ids0), want, "n=0, op")
    got = _C.unsorted_segment_reduce(op, torch.as_tensor(x0).to(DEV), torch.as_tensor(ids0).to(DEV), nseg)
    assert_same(got.cpu().numpy(), want, "n=0, binding")
    (host,) = run(useg_program(op, dtype, "int64", inner, nseg), [x0, ids0], CPU)
    assert_same(host, want, "n=0, host executor")


@pytest.mark.parametrize("op", ["Sum", "Min", "Max", "Prod"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("inner,below,above", [(3, 128, 129), (64, 128, 129), (65, 64, 65), (257, 32, 33)])
def test_unsorted_segment_routes_agree(inner, below, above, dtype, op):
    """The same data and ids with nseg just below and just above the boundary
    between the LDS route and the sorted route (nseg padded with empty
    segments): the common segments match bit for bit, and match the reference.
    Includes a segment that holds only -inf (Max) / +inf (Min), NaN-holding
    segments and empty ones."""
    assert _C.unsorted_segment_route(op, dtype, 2000, inner, below).startswith("private")
    assert _C.unsorted_segment_route(op, dtype, 2000, inner, above).startswith("sorted_perm")
    rng = np.random.default_rng(seed_of("agree", inner, dtype, op))
    used = below - 3                                            # the last segments stay empty on both routes
    n = 2000
    x = useg_data(rng, op, dtype, n, inner)
    ids = rng.integers(0, used, n).astype(np.int64)
    ids[ids == 5] = 6                                           # segment 5: empty in the middle
    ids[:40] = 2                                                # segment 2: nothing but one infinity
    ids[40:80] = 3
    keep = (ids != 2) & (ids != 3)
    keep[:80] = True
    x, ids = x[keep], ids[keep]
    x[:40] = -np.inf
    x[40:80] = np.inf
    nanrows = np.flatnonzero(ids == 7)[:2]
    x[nanrows, 0] = np.nan                                      # segment 7 holds NaN in column 0
    case = rc.UsegCase("", op, dtype, "int64", len(x), inner, below, "", None)
    lo = device_useg(case, x, ids, below)
    hi = device_useg(case, x, ids, above)
    assert lo.tobytes() == hi[:below].tobytes(), "the two routes differ"
    assert_same(hi[below:], np.full((above - below, inner), useg_identity(op, dtype), NP[dtype]), "padding segments")
    assert_same(lo, ref_useg(op, x, ids, below), "reference")
    if op == "Max":
        assert np.all(lo[2] == np.finfo(NP[dtype]).min) and np.all(lo[3] == np.inf)
    if op == "Min":
        assert np.all(lo[3] == np.finfo(NP[dtype]).max) and np.all(lo[2] == -np.inf)
    if op in ("Min", "Max") and len(nanrows):
        assert np.isnan(lo[7, 0])


# ------------------------------------------------------------------ CSR segment reduce
@pytest.mark.parametrize("dtype", ["float32", "float64", "int32", "int64"])
@pytest.mark.parametrize("inner", [1, 3, 257])
def test_segment_reduce_csr(inner, dtype):
    """Segments of 1, 2 and 1000 rows."""
    rng = np.random.default_rng(seed_of("csr", inner, dtype))
    offs = np.array([0, 1, 3, 1003], np.int64)
    n = int(offs[-1])
    for op in ("Sum", "Mean", "Min", "Max", "Prod"):
        x = useg_data(rng, op, dtype, n, inner)
        got = _C.segment_reduce(op, torch.as_tensor(x).to(DEV), torch.as_tensor(offs).to(DEV)).cpu().numpy()
        want = np.stack([ref_reduce(op, x[a:b][None])[0] for a, b in zip(offs[:-1], offs[1:])])
        assert_same(got, want, op)
        if dtype.startswith("float") and op in ("Min", "Max"):
            x[1, 0] = np.nan
            x[500, inner - 1] = np.nan
            x[0, 0] = np.inf
            got = _C.segment_reduce(op, torch.as_tensor(x).to(DEV), torch.as_tensor(offs).to(DEV)).cpu().numpy()
            want = np.stack([ref_reduce(op, x[a:b][None])[0] for a, b in zip(offs[:-1], offs[1:])])
            assert_same(got, want, op + " with NaN")
