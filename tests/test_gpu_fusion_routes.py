"""Every route of the kernels csrc/runtime/fusion.cpp generates, on the device,
against exact references. The cases are the table of tests/fusion_cases.py;
tests/test_fusion_routes.py proves on the host that the table covers every op
x dtype of `_C.fusible_ops()` and every route, and that each case plans onto
the route it names.

Each case goes through three checks:

1. Fused equals op by op, bit for bit. The same graph is evaluated on the
   device one node per program, each node's device output feeding the next; a
   single elementwise node is never fused, so this runs elementwise.hip /
   extra.hip / reduce.hip. NaNs must be in the same places (payload and sign
   of a NaN are not compared); everything else must have the same bits. For
   float Sum / Mean / Prod of a row the two routes add in different orders:
   those are compared with the bound of check 2 instead.
2. Against a reference. Exactly rounded ops (add, sub, mul, div, sqrt, min /
   max, abs, neg, floor / ceil / rint, sign, casts, integer ops with
   wrap-around) are bit-equal to numpy in the op's own dtype. Transcendental
   ops are compared with numpy.longdouble (float64) or float64 (float32;
   math.erf for Erf) in ulps of the result: the limit is twice the largest
   error of the host executor (ATen, an independent implementation) on the
   same inputs, and not below 2 ulp; results below the smallest normal are
   compared by absolute error in units of the smallest subnormal. float64 Erf
   has no such reference here and is checked by 1 only. Row Min / Max / ArgMin
   / ArgMax and integer reductions are exact; float Sum / Mean / Prod are
   within gamma_n * sum|x_i| (gamma_n relative for Prod) of a longdouble
   reference, n the row length: the bound of any summation order.
3. The stated rules, as tests of their own at the end of the file.

Measured on an MI355X the largest errors are in docs/PERFORMANCE.md."""
import functools

import numpy as np
import pytest
import torch

import fusion_cases as fc
from tensorframes_amd import engine, tf
from tensorframes_amd._native import _C
from tensorframes_amd.graph import proto as P

pytestmark = pytest.mark.gpu

CASES = fc.build_cases(_C.fusible_ops())
IDS = [c.id for c in CASES]
BY_ID = {c.id: c for c in CASES}
TORCH_NAME = {torch.float32: "float32", torch.float64: "float64", torch.int32: "int32", torch.int64: "int64",
              torch.uint8: "uint8"}


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


# ------------------------------------------------------------------ running a case
def _program(case):
    g, fetches, feeds = case.build()
    values = case.feeds()
    return g, engine.program(g.serialize(), fetches, feeds), fetches, feeds, values


def run_fused(case, dev):
    g, prog, fetches, feeds, values = _program(case)
    ins = [torch.from_numpy(values[k].copy()).to(dev) for k in feeds]
    _C.set_fusion_index64(True if case.idx == 64 else None)
    try:
        plan = prog.describe(ins)
        assert "FUSED" in plan, plan
        assert " idx%d" % case.idx in plan, plan
        out = engine.run_program(prog, ins, dev)
    finally:
        _C.set_fusion_index64(None)
    return [t.cpu().numpy() for t in out]


def run_host(case):
    g, prog, fetches, feeds, values = _program(case)
    ins = [torch.from_numpy(values[k].copy()) for k in feeds]
    return [t.numpy() for t in engine.run_program(prog, ins, torch.device("cpu"))]


def run_op_by_op(case, dev):
    """The case's graph on the device, one node per program."""
    g, _, fetches, feeds, values = _program(case)
    vals = {}
    for op in g.get_operations():
        nd = op.node_def
        if nd.op == "Placeholder":
            vals[op.name] = torch.from_numpy(values[op.name].copy()).to(dev)
            continue
        if nd.op == "Const":
            continue
        g1 = tf.Graph()
        names, ins, feed_names = [], [], []
        with g1.as_default():
            for k, t in enumerate(op.inputs):
                if t.op.type == "Const":
                    if t.op.name not in g1._ops:
                        g1._add(t.op.node_def, 1, [t.dtype])
                    names.append(t.op.name)
                else:
                    v = vals[t.op.name]
                    tf.placeholder(fc.TF_DT[TORCH_NAME[v.dtype]], list(v.shape), name="in%d" % k)
                    names.append("in%d" % k)
                    feed_names.append("in%d" % k)
                    ins.append(v)
            g1._add(P.NodeDef._make("node", nd.op, names, dict(nd.attr)), 1, [op.outputs[0].dtype])
        prog = engine.program(g1.serialize(), ["node"], feed_names)
        assert "FUSED" not in prog.describe(ins), nd.op
        vals[op.name] = engine.run_program(prog, ins, dev)[0]
    return [vals[f].cpu().numpy() for f in fetches]


@functools.lru_cache(maxsize=None)
def results(case_id):
    """(fused, op by op) outputs of a case, computed once for all its checks."""
    dev = _gpu()
    case = BY_ID[case_id]
    return run_fused(case, dev), run_op_by_op(case, dev)


# ------------------------------------------------------------------ comparisons
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def assert_same_bits(got, want, what, zero_sign=True):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype.kind != "f":
        bad = got != want
    else:
        gn, wn = np.isnan(got), np.isnan(want)
        bad = (gn != wn) | (~gn & ~wn & ((bits(got) != bits(want)) if zero_sign else (got != want)))
    if bad.any():
        i = np.flatnonzero(bad.ravel())[:5]
        raise AssertionError("%s: %d of %d differ, first at %s: got %s want %s" %
                             (what, int(bad.sum()), bad.size, i, got.ravel()[i], want.ravel()[i]))


def ulp_error(got, ref):
    """Largest error of `got` in ulps of its dtype against the higher-precision
    `ref`; where the correctly rounded reference is not finite, `got` must be
    the same infinity or a NaN too. Below the smallest normal the unit is the
    smallest subnormal."""
    T = got.dtype.type
    fi = np.finfo(T)
    with np.errstate(all="ignore"):
        want = ref.astype(T)
    fin = np.isfinite(want)
    assert_same_bits(np.where(fin, T(0), got), np.where(fin, T(0), want), "non-finite results", zero_sign=False)
    assert np.isfinite(got[fin]).all(), "finite reference, non-finite result: %s" % got[fin][~np.isfinite(got[fin])][:5]
    if not fin.any():
        return 0.0
    with np.errstate(all="ignore"):  # the spacing of the largest finite value overflows; it is not used as a divisor alone
        unit = np.maximum(np.spacing(np.abs(want[fin])), T(fi.tiny) * T(fi.eps)).astype(ref.dtype)
        unit = np.where(np.isfinite(unit), unit, ref.dtype.type(np.spacing(T(fi.max) / 2)) * 2)
    return float(np.max(np.abs(got[fin].astype(ref.dtype) - ref[fin]) / unit))


ULPS = {}  # (op, dtype) -> (host max, device max), printed by the last test


def gamma(n, dtype):
    u = np.finfo(dtype).eps / 2
    return n * u / (1 - n * u)


def check_rowred(case, fetch, got, ref, x_abs_sum, x_n, what):
    op = fetch[1:]
    if ref.dtype != np.longdouble:
        assert_same_bits(got, ref.astype(got.dtype) if op.startswith("Arg") else ref, what,
                         zero_sign=op not in ("Min", "Max"))
        return
    T = got.dtype.type
    with np.errstate(all="ignore"):
        want = ref.astype(T)
    fin = np.isfinite(want)
    assert_same_bits(np.where(fin, T(0), got), np.where(fin, T(0), want), what + " non-finite rows", zero_sign=False)
    g = gamma(x_n, T)
    if op == "Prod":
        bound = g * np.abs(ref)
    else:
        bound = g * x_abs_sum / (x_n if op == "Mean" else 1)
    with np.errstate(all="ignore"):
        err = np.abs(got.astype(np.longdouble) - ref)
    bad = fin & ~(err <= bound)
    assert not bad.any(), "%s: rows %s err %s bound %s" % (what, np.flatnonzero(bad.ravel())[:5], err[bad][:5], bound[bad][:5])


def rowred_inputs(case):
    """sum|x| per row and the row length of the tensor a row-reduction case reduces."""
    f = case.feeds()
    with np.errstate(all="ignore"):
        v = f["x"] + f["c"] if "c" in f else f["x"]
    first = case.ref(f)[0]
    rows = v.reshape(int(np.prod(first.shape)), -1)
    with np.errstate(all="ignore"):
        return np.abs(rows.astype(np.longdouble)).sum(1).reshape(first.shape), rows.shape[1]


# ------------------------------------------------------------------ checks 1 and 2
@pytest.mark.parametrize("cid", IDS)
def test_fused_equals_op_by_op(cid):
    case = BY_ID[cid]
    fused, single = results(cid)
    _, _, fetches, _, _ = _program(case)
    for name, a, b in zip(fetches, fused, single):
        if case.check == "rowred" and a.dtype.kind == "f" and name[1:] in ("Sum", "Mean", "Prod"):
            x_abs_sum, n = rowred_inputs(case)
            ref = case.ref(case.feeds())[fetches.index(name)]
            check_rowred(case, name, b, ref, x_abs_sum, n, "%s op by op" % name)  # the other order of the same sum
            continue
        assert_same_bits(a, b, "%s fused vs op by op" % name)


@pytest.mark.parametrize("cid", IDS)
def test_fused_matches_reference(cid):
    case = BY_ID[cid]
    fused, _ = results(cid)
    refs = case.ref(case.feeds())
    _, _, fetches, _, _ = _program(case)
    assert len(fused) == len(refs)
    for name, got, ref in zip(fetches, fused, refs):
        if case.check == "device":
            continue
        if case.check == "rowred":
            x_abs_sum, n = rowred_inputs(case)
            check_rowred(case, name, got, ref, x_abs_sum, n, name)
        elif case.check == "ulp":
            host = ulp_error(run_host(case)[0], ref)
            dev = ulp_error(got, ref)
            key = (case.op, case.dtype)
            ULPS[key] = (max(host, ULPS.get(key, (0, 0))[0]), max(dev, ULPS.get(key, (0, 0))[1]))
            print("ULP %-10s %-8s host %.3f device %.3f" % (case.op, case.dtype, host, dev))
            assert dev <= max(2.0, 2.0 * host), "%s %s: device %.3f ulp, host %.3f ulp" % (case.op, case.dtype, dev, host)
        else:
            assert got.shape == ref.shape, (got.shape, ref.shape)
            assert_same_bits(got, ref.astype(got.dtype) if ref.dtype != got.dtype else ref, name,
                             zero_sign=case.check == "exact")


# ------------------------------------------------------------------ check 3: the stated rules
def _run(body, feeds, values, fetches, dev, fused):
    g = tf.Graph()
    with g.as_default():
        body()
    prog = engine.program(g.serialize(), fetches, feeds)
    ins = [torch.from_numpy(np.asarray(values[k])).to(dev) for k in feeds]
    plan = prog.describe(ins) if dev.type == "cuda" else ""
    if dev.type == "cuda":
        assert ("FUSED" in plan) == fused, plan
    return [t.cpu().numpy() for t in engine.run_program(prog, ins, dev)], plan


NAN_OPS = {"Relu": tf.nn.relu, "Relu6": tf.nn.relu6, "LeakyRelu": tf.nn.leaky_relu,
           "Maximum": lambda x: tf.maximum(x, 1.0), "Minimum": lambda x: tf.minimum(x, 1.0)}


@pytest.mark.parametrize("dtype", fc.FLOATS)
@pytest.mark.parametrize("op", sorted(NAN_OPS))
def test_nan_stays_nan_through_clamping_ops(op, dtype):
    """Relu / Relu6 / LeakyRelu / Maximum / Minimum of NaN is NaN: alone, inside
    a generated kernel, and on the host executor."""
    dev = _gpu()
    x = np.array([np.nan, -1.0, 0.0, 2.0, 7.0, -np.nan], dtype)
    want_nan = np.isnan(x)
    for fused in (False, True):
        def body():
            y = NAN_OPS[op](fc._ph(dtype, [None], "x"))
            if fused:
                y = tf.multiply(y, fc._ph(dtype, [], "one"))
            tf.identity(y, name="y")
        feeds = ["x", "one"] if fused else ["x"]
        for d in (dev, torch.device("cpu")):
            got = _run(body, feeds, {"x": x, "one": np.ones((), dtype)}, ["y"], d, fused)[0][0]
            assert np.array_equal(np.isnan(got), want_nan), (op, fused, d, got)


@pytest.mark.parametrize("inner", [5, 16, 17, 130])
@pytest.mark.parametrize("dtype", fc.FLOATS)
def test_row_min_max_argmin_argmax_of_nan(dtype, inner):
    """A NaN in a row: Min and Max give NaN, ArgMax and ArgMin return the index
    of the first NaN (NaN counts as the largest value, and ArgMin returns the
    first NaN too, as numpy does), wherever in the row it stands, on the
    thread-per-row and the wave-per-row kernel."""
    dev = _gpu()
    x = np.tile(np.arange(inner, dtype=dtype) % 7, (256, 1))
    where = {}
    for r, j in enumerate([0, 1, inner // 2, inner - 1, min(64, inner - 1), min(65, inner - 1)]):
        x[r, j] = np.nan
        where[r] = j
    x[6, inner - 1] = np.nan
    x[6, 2] = np.nan
    where[6] = 2            # two NaNs: the first
    x[7, :] = np.nan
    where[7] = 0            # all NaN
    x[8, 1] = np.inf        # an infinity does not hide a later NaN
    x[8, 3] = np.nan
    where[8] = 3

    def body():
        v = tf.multiply(fc._ph(dtype, [None, inner], "x"), fc._ph(dtype, [], "one"))
        for op in ("Min", "Max", "ArgMin", "ArgMax"):
            fc.RED_FN[op](v, 1, name="y" + op)
    got, plan = _run(body, ["x", "one"], {"x": x, "one": np.ones((), dtype)}, ["yMin", "yMax", "yArgMin", "yArgMax"],
                     dev, True)
    assert "FUSED-ROWRED" in plan and (" wave " in plan) == (inner > 16), plan
    rows = sorted(where)
    for k, name in enumerate(("Min", "Max")):
        assert np.isnan(got[k][rows]).all(), (name, got[k][rows])
        assert not np.isnan(got[k][9:]).any()
    for k, name in ((2, "ArgMin"), (3, "ArgMax")):
        assert [int(got[k][r]) for r in rows] == [where[r] for r in rows], (name, got[k][rows], where)
    assert (got[3][9:] == int(np.argmax(x[9]))).all() and (got[2][9:] == 0).all()


@pytest.mark.parametrize("dtype", fc.FLOATS)
def test_abs_of_negative_zero_is_positive_zero(dtype):
    """abs(-0.0) is +0.0, as at::abs and numpy give it: in the stand-alone
    kernel, in a generated kernel, in a GEMM epilogue chain and on the host."""
    dev = _gpu()
    x = np.array([-0.0, 0.0, -1.5, 2.0], dtype)
    want = np.abs(x)
    for fused in (False, True):
        def body():
            y = tf.abs(fc._ph(dtype, [None], "x"))
            if fused:
                y = tf.multiply(y, fc._ph(dtype, [], "one"))
            tf.identity(y, name="y")
        for d in (dev, torch.device("cpu")):
            got = _run(body, ["x", "one"] if fused else ["x"], {"x": x, "one": np.ones((), dtype)}, ["y"], d, fused)[0][0]
            assert_same_bits(got, want, "abs fused=%s on %s" % (fused, d))
    # MatMul -> Neg -> Abs runs in the GEMM epilogue: the product of zeros is +0.0, Neg makes it -0.0
    a = np.zeros((64, 32), dtype)
    a[1, :] = 1.0
    w = np.ones((32, 48), dtype)

    def gemm():
        tf.abs(tf.negative(tf.matmul(fc._ph(dtype, [None, 32], "a"), tf.constant(w))), name="y")
    for d in (dev, torch.device("cpu")):
        got, plan = _run(gemm, ["a"], {"a": a}, ["y"], d, False)
        if d.type == "cuda":
            assert "+epi[neg,abs]" in plan, plan
        want = np.zeros((64, 48), dtype)
        want[1, :] = 32.0
        assert_same_bits(got[0], want, "abs in the GEMM epilogue on %s" % d)


def test_softplus_float64_above_twenty():
    """softplus(x) = x + log1p(exp(-x)) is not x for 20 < x <= 36.7 in float64
    (at 21 the difference is 7.6e-10, 2e5 ulp): alone, fused, and on the host
    the error stays within the limit of check 2."""
    dev = _gpu()
    x = np.concatenate([np.linspace(20.0, 40.0, 4001), np.nextafter(20.0, [0.0, 100.0])])
    h = x.astype(np.longdouble)
    ref = h + np.log1p(np.exp(-h))
    errs = {}
    for fused in (False, True):
        def body():
            y = tf.nn.softplus(fc._ph("float64", [None], "x"))
            if fused:
                y = tf.multiply(y, fc._ph("float64", [], "one"))
            tf.identity(y, name="y")
        for d in (dev, torch.device("cpu")):
            got = _run(body, ["x", "one"] if fused else ["x"], {"x": x, "one": np.ones((), "float64")}, ["y"], d, fused)[0][0]
            errs[(fused, d.type)] = ulp_error(got, ref)
    print("ULP Softplus(20,40] float64", errs)
    host = max(errs[(False, "cpu")], errs[(True, "cpu")])
    assert host <= 2.0, errs
    assert max(errs[(False, "cuda")], errs[(True, "cuda")]) <= max(2.0, 2.0 * host), errs


@pytest.mark.parametrize("dtype", fc.FLOATS)
def test_sign_of_nan_is_zero(dtype):
    """Sign(NaN) is 0 on every route: `(x > 0) - (x < 0)`, what ATen's sign
    gives on the host (numpy and TensorFlow give NaN)."""
    dev = _gpu()
    x = np.array([np.nan, -np.nan, -2.0, -0.0, 0.0, 3.0, np.inf, -np.inf], dtype)
    want = np.array([0, 0, -1, 0, 0, 1, 1, -1], dtype)
    for fused in (False, True):
        def body():
            y = tf.sign(fc._ph(dtype, [None], "x"))
            if fused:
                y = tf.multiply(y, fc._ph(dtype, [], "one"))
            tf.identity(y, name="y")
        for d in (dev, torch.device("cpu")):
            got = _run(body, ["x", "one"] if fused else ["x"], {"x": x, "one": np.ones((), dtype)}, ["y"], d, fused)[0][0]
            assert np.array_equal(got, want), (fused, d, got)


def test_zz_ulp_report():
    """Prints the largest host and device error per transcendental op and dtype
    (run with -s): the figures of docs/PERFORMANCE.md."""
    _gpu()
    for (op, dtype), (host, dev) in sorted(ULPS.items()):
        print("ULPMAX %-10s %-8s host %.3f device %.3f" % (op, dtype, host, dev))
    print("JIT", _C.jit_stats())
