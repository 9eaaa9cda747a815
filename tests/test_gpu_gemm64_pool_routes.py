"""Every dispatch route of csrc/kernels/gemm_f64.hip on the device against exact
references: the float64 MFMA GEMM, the integer GEMM and NHWC pooling
(tests/gemm64_pool_cases.py is the case table; tests/test_gemm64_pool_routes.py
proves on the host that it covers every route).

The data is chosen so that the reference is exact and the assertion is equality
(NaN matching NaN): integer-valued GEMM operands in [-8, 8] with K <= 48 (every
product and partial sum is an exact double in any order), int64 arithmetic for
the integer GEMM, unique values per channel for max pooling and integers of
magnitude <= 1024 for avg pooling (the window sum is exact in f32, the one
division is correctly rounded). A dropped, repeated or misplaced element
changes the result.

Where exactness is not to be had the bound is derived: a GEMM of uniform(-1, 1)
reals lies within gamma_K (|A| @ |B|), gamma_K = K u / (1 - K u), u = 2^-53, of
a long double reference, whatever the order of the FMAs. Only the fused tanh
has a measured bound: its pre-activation is exact (integers / 512), numpy's
float64 tanh of it is the reference, and the largest distance measured on an
MI355X over the cases here is 1.000 ulp on every tile (TANH_ULP_MEASURED; the
host executor's tanh lies 1.000 ulp from numpy's as well); the test allows
twice that, and at least 2 ulp.
"""
import functools
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import gemm64_pool_cases as gc  # noqa: E402
from tensorframes_amd import engine, tf  # noqa: E402
from tensorframes_amd._native import _C  # noqa: E402

DEV = torch.device("cuda", 0)
CPU = torch.device("cpu")
TANH_ULP_MEASURED = 1.0
TANH_ULP_BOUND = max(2.0, 2 * TANH_ULP_MEASURED)


def seed_of(*parts):
    return zlib.crc32("/".join(map(str, parts)).encode())


def run(prog, arrays, device=None):
    outs = engine.run_program(prog, [torch.as_tensor(np.ascontiguousarray(a)) for a in arrays], device or DEV)
    return [o.cpu().numpy() for o in outs]


def assert_same(got, want, what):
    """== plus isnan: NaN matches NaN, the sign of a zero is not pinned."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = ~((got == want) | ((got != got) & (want != want))) if got.dtype.kind == "f" else got != want
    if bad.any():
        idx = np.argwhere(bad)
        first = tuple(idx[0])
        raise AssertionError("%s: %d of %d differ, first at %s: got %r, want %r"
                             % (what, len(idx), got.size, first, got[first], want[first]))


@pytest.fixture(autouse=True)
def automatic_pool_route():
    _C.set_pool_route(None)
    yield
    _C.set_pool_route(None)


# ================================================================== float64 / integer GEMM
ACT_FN = {"relu": tf.nn.relu, "relu6": tf.nn.relu6, "tanh": tf.tanh}


def bias_of(n, dtype=np.float64):
    """Integer-valued, different in every column."""
    return ((np.arange(n) * 7) % 13 - 6).astype(dtype)


@functools.lru_cache(maxsize=None)
def gemm_program(dtype, ta, tb, rank_a, rank_b, epi, n):
    """One MatMul / BatchMatMul step over placeholders of unknown size, its
    epilogue fused; the plan is checked to say so."""
    names = ["a", "b"]
    g = tf.Graph()
    with g.as_default():
        a = tf.placeholder(dtype, [None] * rank_a, name="a")
        b = tf.placeholder(dtype, [None] * rank_b, name="b")
        y = tf.matmul(a, b, transpose_a=ta, transpose_b=tb)
        if epi == "chain":    # as tests/test_epilogue_act.py builds it; every step is exact on the data used
            z = tf.placeholder(dtype, [None, n], name="z")
            r = tf.placeholder(dtype, [None, 1], name="r")
            names += ["z", "r"]
            h = tf.nn.relu(tf.nn.bias_add(y, tf.constant(bias_of(n, dtype))))
            h = (h * 0.5 + tf.constant(bias_of(n, dtype)[::-1].copy())) - z
            h = tf.maximum(h, r)
            y = tf.multiply(h, h)
        elif epi != "none":
            y = tf.nn.bias_add(y, tf.constant(bias_of(n, dtype)))
            if epi != "bias":
                y = ACT_FN[epi[5:]](y)
        tf.identity(y, name="y")
    prog = engine.program(g.serialize(), ["y"], names)
    tdt = torch.as_tensor(np.zeros(1, dtype)).dtype
    sample = [torch.zeros([2] * rank_a, dtype=tdt), torch.zeros([2] * (rank_b - 2) + ([n, 2] if tb else [2, n]), dtype=tdt)]
    if epi == "chain":
        sample += [torch.zeros([2, n], dtype=tdt), torch.zeros([2, 1], dtype=tdt)]
    plan = prog.describe(sample, as_gpu=True)
    want = {"none": "MatMul", "bias": "+bias", "chain": "+bias +relu +epi[mul:scalar,add:col,sub:full,max:row,square]"}
    if np.dtype(dtype).kind == "f":     # the planner fuses epilogues into float GEMMs only: integer ones run BiasAdd / Relu as ops
        assert want.get(epi, "+bias +" + epi[5:]) in plan, plan
        assert "FUSED" not in plan, plan
    return prog


def stored(x, transposed):
    return np.ascontiguousarray(np.swapaxes(x, -1, -2)) if transposed else np.ascontiguousarray(x)


def int_operands(seed, batch, M, N, K, bcast_b=False, lo=-8, hi=8, nonzero=False, dtype=np.float64):
    """Logical A [batch, M, K] and B [batch | 1, K, N]: random integers plus a
    term that differs along every row and column, so a transposed, shifted or
    repeated tile cannot match."""
    rng = np.random.default_rng(seed)
    half = (hi - lo) // 4

    def make(b, r, c):
        x = rng.integers(-half, half + 1, (b, r, c))
        x += ((np.arange(r)[:, None] + 2 * np.arange(c)[None, :] + 3 * np.arange(b)[:, None, None]) % (2 * half + 1)) - half
        if nonzero:
            x[x == 0] = hi
        return x.astype(dtype)
    return make(batch, M, K), make(1 if bcast_b else batch, K, N)


def exact_product(A, B):
    """The exact product of integer-valued operands. In float64 every partial
    sum is an integer far below 2^53, so any summation order (numpy's BLAS, the
    device's MFMA chain) gives the int64 product; the smaller cases say so."""
    if A.dtype.kind != "f":
        return np.matmul(A.astype(np.int64), B.astype(np.int64))
    P = np.matmul(A, B)
    if P.size * A.shape[-1] <= 1 << 22:
        assert np.array_equal(P, np.matmul(A.astype(np.int64), B.astype(np.int64)).astype(np.float64))
    return P


def apply_epi_ref(P, epi, N, z=None, r=None):
    if epi == "none":
        return P
    P = P + bias_of(N, P.dtype)
    if epi == "bias_relu":
        return np.maximum(P, 0)
    if epi == "bias_relu6":
        return np.clip(P, 0, 6)
    if epi == "chain":
        h = (np.maximum(P, 0) * 0.5 + bias_of(N, P.dtype)[::-1]) - z
        return np.maximum(h, r) ** 2
    return P


def device_gemm(dtype, c, A, B, extra=()):
    batched = c.batch > 1
    a_, b_ = stored(A, c.ta), stored(B, c.tb)
    if not batched:
        a_, b_ = a_[0], b_[0]
    elif getattr(c, "bcast_b", False):
        b_ = b_[0]
    prog = gemm_program(dtype, c.ta, c.tb, a_.ndim, b_.ndim, c.epi, c.N)
    (y,) = run(prog, [a_, b_] + list(extra))
    return y if batched else y[None]


NOT_TANH = [c for c in gc.F64_CASES if c.epi != "bias_tanh"]
TANH = [c for c in gc.F64_CASES if c.epi == "bias_tanh"]


@pytest.mark.parametrize("case", NOT_TANH, ids=[c.id for c in NOT_TANH])
def test_f64_gemm_exact(case):
    c = case
    A, B = int_operands(seed_of("f64", c.id), c.batch, c.M, c.N, c.K, c.bcast_b)
    P = exact_product(A, B).astype(np.float64)
    extra, z, r = (), None, None
    if c.epi == "chain":
        rng = np.random.default_rng(seed_of("chain", c.id))
        z = rng.integers(-40, 41, (c.M, c.N)).astype(np.float64)
        r = rng.integers(-20, 21, (c.M, 1)).astype(np.float64)
        extra = (z, r)
    want = apply_epi_ref(P, c.epi, c.N, z, r)
    assert_same(device_gemm(np.float64, c, A, B, extra), want, c.id)


def test_f64_gemm_fused_tanh_within_measured_ulps(capsys):
    """The pre-activation is exact (integers / 512, a few units wide), so the
    difference is the device tanh's alone."""
    worst = 0.0
    for c in TANH:
        A, B = int_operands(seed_of("tanh", c.id), c.batch, c.M, c.N, c.K, c.bcast_b)
        A = A / 512.0
        pre = exact_product(A * 512, B).astype(np.float64) / 512.0 + bias_of(c.N)
        want = np.tanh(pre)
        got = device_gemm(np.float64, c, A, B)
        assert got.shape == want.shape
        assert (np.abs(pre) < 4).mean() > 0.3                                # most of the data is off the saturated range
        ulps = float((np.abs(got - want) / np.spacing(np.abs(want))).max())
        with capsys.disabled():
            print("\n  tanh epilogue %s: max %.3f ulp" % (c.id, ulps))
        worst = max(worst, ulps)
    assert len(TANH) >= 5
    assert worst <= TANH_ULP_BOUND, worst


def _special_positions(M, K, BM):
    pos = [(0, 0), (0, 15), (M - 1, K - 1), (BM - 1, K - 1), (BM, 15), (BM, K - 1)]
    if K > 16:
        pos.append((M - 1, 16))
    return [p for p in dict.fromkeys(pos) if p[0] < M and p[1] < K]


@pytest.mark.parametrize("grid", gc.F64_SPECIAL_GRIDS, ids=["%s-%s%s-%dx%dx%d" % (g[0], "NT"[g[1]], "NT"[g[2]], *g[3:])
                                                           for g in gc.F64_SPECIAL_GRIDS])
def test_f64_gemm_special_values_stay_in_their_row_and_column(grid):
    """One NaN, +inf or -inf in A poisons one output row, in B one column; every
    other output stays bit-exact (a zero-filled tail that leaks would not)."""
    tile, ta, tb, M, N, K = grid
    BM, BN = gc._TILE_DIMS[tile]
    c = gc._f64(tile, ta, tb, 1, M, N, K)
    assert _C.gemm_f64_route(M, N, K, 1, ta, tb)["tile"] == tile
    A0, B0 = int_operands(seed_of("special", *grid), 1, M, N, K, nonzero=True)
    clean = exact_product(A0, B0).astype(np.float64)
    for value in (np.nan, np.inf, -np.inf):
        for (i, k) in _special_positions(M, K, BM):
            A = A0.copy()
            A[0, i, k] = value
            with np.errstate(all="ignore"):
                want = np.matmul(A, B0)
            assert np.array_equal(np.delete(want[0], i, 0), np.delete(clean[0], i, 0)) and not np.isfinite(want[0, i]).any()
            assert_same(device_gemm(np.float64, c, A, B0), want, "A[%d,%d] = %r" % (i, k, value))
        for (j, k) in _special_positions(N, K, BN):
            B = B0.copy()
            B[0, k, j] = value
            with np.errstate(all="ignore"):
                want = np.matmul(A0, B)
            assert np.array_equal(np.delete(want[0], j, 1), np.delete(clean[0], j, 1)) and not np.isfinite(want[0, :, j]).any()
            assert_same(device_gemm(np.float64, c, A0, B), want, "B[%d,%d] = %r" % (k, j, value))


def gamma(K):
    u = 2.0 ** -53
    return K * u / (1 - K * u)


@pytest.mark.parametrize("tile,ta,tb,batch,M,N,K", [("64x16", False, True, 1, 200, 10, 33), ("64x64", True, False, 1, 130, 78, 48),
                                                     ("128x128", False, False, 52, 514, 130, 17)])
def test_f64_gemm_random_reals_within_gamma_k(tile, ta, tb, batch, M, N, K):
    assert _C.gemm_f64_route(M, N, K, batch, ta, tb)["tile"] == tile
    rng = np.random.default_rng(seed_of("real", tile))
    A, B = rng.uniform(-1, 1, (batch, M, K)), rng.uniform(-1, 1, (batch, K, N))
    c = gc._f64(tile, ta, tb, batch, M, N, K)
    got = device_gemm(np.float64, c, A, B)
    want = np.matmul(A.astype(np.longdouble), B.astype(np.longdouble))
    bound = gamma(K) * np.matmul(np.abs(A), np.abs(B))
    err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
    assert (err <= bound).all(), float((err / bound).max())


def test_f64_gemm_more_batches_than_one_grid_dimension():
    """65536 batches: the second launch slice holds the last one."""
    for M, N, K in ((1, 1, 1), (2, 2, 3)):
        assert _C.gemm_f64_route(M, N, K, 65536)["launches"] == 2
        A, B = int_operands(seed_of("batch", M), 65536, M, N, K)
        c = gc._f64("64x16", False, False, 65536, M, N, K)
        assert_same(device_gemm(np.float64, c, A, B), exact_product(A, B).astype(np.float64), "batch 65536 %dx%dx%d" % (M, N, K))


# ------------------------------------------------------------------ integer GEMM
def int_ref(A, B, c, dtype):
    """numpy int64 arithmetic (wrapping), cast to the output type, then the epilogue in that type."""
    with np.errstate(over="ignore"):
        v = np.matmul(A.astype(np.int64), B.astype(np.int64)).astype(dtype)
        if c.epi != "none":
            v = v + bias_of(c.N, dtype)
        if c.epi == "bias_relu":
            v = np.maximum(v, 0)
        elif c.epi == "bias_relu6":
            v = np.clip(v, 0, 6)
    return v.astype(dtype)


@pytest.mark.parametrize("case", gc.INT_CASES, ids=[c.id for c in gc.INT_CASES])
def test_int_gemm_exact(case):
    c = case
    dtype = np.dtype(c.dtype).type
    big = c.epi == "none"       # with an activation keep the sums near its range, else spread them wide
    A, B = int_operands(seed_of("int", c.id), c.batch, c.M, c.N, c.K, lo=-1000 if big else -2, hi=1000 if big else 2, dtype=dtype)
    assert_same(device_gemm(dtype, c, A, B), int_ref(A, B, c, dtype), c.id)


def test_int32_gemm_wraps_mod_2_32():
    c = gc._int("int32", False, True, 1, 17, 33, 40, "bias")
    A, B = int_operands(7, 1, c.M, c.N, c.K, lo=-(1 << 20), hi=1 << 20, dtype=np.int32)
    full = np.matmul(A.astype(np.int64), B.astype(np.int64))
    assert (np.abs(full) >= 1 << 31).mean() > 0.5
    assert_same(device_gemm(np.int32, c, A, B), int_ref(A, B, c, np.int32), c.id)


def test_int64_gemm_and_its_bias_wrap_mod_2_64():
    M, N, K = 5, 4, 17
    rng = np.random.default_rng(11)
    A = rng.integers(-(1 << 40), 1 << 40, (M, K), dtype=np.int64)
    B = rng.integers(-(1 << 40), 1 << 40, (K, N), dtype=np.int64)
    bias = np.array([(1 << 63) - 1, -(1 << 63), 12345, -(1 << 62)], np.int64)
    g = tf.Graph()
    with g.as_default():
        a = tf.placeholder(tf.int64, [None, K], name="a")
        b = tf.placeholder(tf.int64, [K, N], name="b")
        tf.nn.bias_add(tf.matmul(a, b), tf.constant(bias), name="y")
    prog = engine.program(g.serialize(), ["y"], ["a", "b"])
    want = np.empty((M, N), np.int64)
    for i in range(M):
        for j in range(N):
            v = (sum(int(A[i, k]) * int(B[k, j]) for k in range(K)) + int(bias[j])) % (1 << 64)
            want[i, j] = v - (1 << 64) if v >= 1 << 63 else v
    prod = [[sum(int(A[i, k]) * int(B[k, j]) for k in range(K)) for j in range(N)] for i in range(M)]
    assert all(abs(v) >= 1 << 64 for row in prod for v in row)                   # the product wraps

    def signed(v):
        v %= 1 << 64
        return v - (1 << 64) if v >= 1 << 63 else v
    assert any(not -(1 << 63) <= signed(prod[i][j]) + int(bias[j]) < 1 << 63 for i in range(M) for j in range(N))   # so does the bias add
    (got,) = run(prog, [A, B])
    assert_same(got, want, "int64 wrap")


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_int_gemm_past_the_old_launch_limits(dtype):
    """M = 1,048,561 needs 65536 row tiles and 65536 batches two grid.z slices:
    both raised before (`int gemm: M too large`, an unchecked grid.z)."""
    M = gc.INT_LIMIT_M
    assert _C.gemm_int_route(M, 1, 2)["grid"][0] == 65536
    c = gc._int(np.dtype(dtype).name, False, False, 1, M, 1, 2)
    A, B = int_operands(3, 1, M, 1, 2, lo=-1000, hi=1000, dtype=dtype)
    A[0, -1] = (977, -5)                                     # the row only the last tile holds
    assert_same(device_gemm(dtype, c, A, B), int_ref(A, B, c, dtype), "M = %d" % M)
    nb = gc.INT_LIMIT_BATCH
    assert _C.gemm_int_route(2, 2, 3, nb)["launches"] == 2
    c = gc._int(np.dtype(dtype).name, False, True, nb, 2, 2, 3)
    A, B = int_operands(4, nb, 2, 2, 3, lo=-1000, hi=1000, dtype=dtype)
    assert_same(device_gemm(dtype, c, A, B), int_ref(A, B, c, dtype), "batch = %d" % nb)


# ------------------------------------------------------------------ NaN through the fused activations, K = 0
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("act", ["relu", "relu6"])
def test_fused_relu_keeps_nan(dtype, act):
    """A NaN pre-activation stays NaN, as clamp_min / clamp of the host executor
    keep it; +inf clamps to 6 under ReLU6 and -inf to 0."""
    M, N, K = 70, 20, 17
    A, B = int_operands(5, 1, M, N, K, nonzero=True, dtype=dtype)
    A[0, 3, K - 1] = np.nan
    A[0, 64, 0] = np.inf
    A[0, 69, 16] = -np.inf
    c = gc._f64("64x64", False, False, 1, M, N, K, "bias_" + act)
    with np.errstate(all="ignore"):
        pre = np.matmul(A.astype(np.float64), B.astype(np.float64)) + bias_of(N)
        want = (np.maximum(pre, 0) if act == "relu" else np.clip(pre, 0, 6)).astype(dtype)   # numpy keeps NaN
    assert np.isnan(want[0, 3]).all() and not np.isnan(np.delete(want[0], 3, 0)).any()
    assert_same(device_gemm(dtype, c, A, B), want, "device")
    prog = gemm_program(dtype, False, False, 2, 2, "bias_" + act, N)
    assert_same(run(prog, [A[0], B[0]], CPU)[0][None], want, "host executor")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_relu_kernels_keep_nan(dtype):
    x = np.array([np.nan, -np.inf, -1.0, -0.0, 0.0, 2.5, 6.0, 7.0, np.inf] * 37, dtype)
    for fn, ref in ((tf.nn.relu, lambda v: np.maximum(v, 0)), (tf.nn.relu6, lambda v: np.clip(v, 0, 6))):
        g = tf.Graph()
        with g.as_default():
            fn(tf.placeholder(dtype, [None], name="x"), name="y")
        prog = engine.program(g.serialize(), ["y"], ["x"])
        assert_same(run(prog, [x])[0], ref(x), fn.__name__)
        assert_same(run(prog, [x], CPU)[0], ref(x), fn.__name__ + " on the host")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_matmul_k0_applies_the_fused_epilogue(dtype):
    """An empty sum is 0: the output is act(bias) in every row, not zeros."""
    b = np.array([-2.0, 3.0, 9.0], dtype)
    g = tf.Graph()
    with g.as_default():
        xi = tf.placeholder(dtype, [None, 0], name="x")
        tf.nn.relu6(tf.nn.bias_add(tf.matmul(xi, tf.constant(np.zeros((0, 3), dtype))), tf.constant(b)), name="y")
    prog = engine.program(g.serialize(), ["y"], ["x"])
    x = np.zeros((70, 0), dtype)
    assert "+bias +relu6" in prog.describe([torch.as_tensor(x)], as_gpu=True)
    want = np.tile(np.array([0.0, 3.0, 6.0], dtype), (70, 1))
    assert_same(run(prog, [x])[0], want, "device")
    assert_same(run(prog, [x], CPU)[0], want, "host")


# ================================================================== pooling
def pool_ref(x, c, is_max=None):
    """Window maximum (NaN kept) or float32(sum) / float32(taps inside the image)."""
    is_max = c.is_max if is_max is None else is_max
    n, h, w, ch = x.shape
    (oh, pt), (ow, pl) = gc.pool_out(h, c.KH, c.sh, c.pad), gc.pool_out(w, c.KW, c.sw, c.pad)
    y = np.zeros((n, oh, ow, ch), np.float32)
    for i in range(oh):
        for j in range(ow):
            h0, w0 = i * c.sh - pt, j * c.sw - pl
            win = x[:, max(h0, 0):min(h0 + c.KH, h), max(w0, 0):min(w0 + c.KW, w)]
            cnt = win.shape[1] * win.shape[2]
            assert cnt > 0
            if is_max:
                y[:, i, j] = win.max(axis=(1, 2))                 # numpy's max keeps NaN
            else:
                with np.errstate(invalid="ignore"):
                    s = win.astype(np.float64).sum(axis=(1, 2))       # exact: integers, |sum| < 2^24
                    y[:, i, j] = s.astype(np.float32) / np.float32(cnt)
    return y


def pool_epi_ref(y, epi):
    if epi == "none":
        return y
    y = y + bias_of(y.shape[-1], np.float32)                           # one f32 add, correctly rounded on both sides
    return np.maximum(y, 0) if epi == "bias_relu" else np.clip(y, 0, 6) if epi == "bias_relu6" else y


def pool_data(seed, is_max, N, H, W, C):
    rng = np.random.default_rng(seed)
    if is_max:      # unique values per (image, channel): the winning tap is identifiable
        x = np.stack([rng.permutation(H * W * N).reshape(N, H, W) for _ in range(C)], -1) - (H * W * N) // 2
        return x.astype(np.float32)
    return rng.integers(-1024, 1025, (N, H, W, C)).astype(np.float32)


def pool_pieces(c):
    """Channel counts of the pools concatenated: the case's own and the ones that fill its slice's row."""
    if not c.slice:
        return [c.C], 0
    off, ldc = c.slice
    before, after = ([off] if off else []), ([ldc - off - c.C] if ldc - off - c.C else [])
    return before + [c.C] + after, len(before)


def pool_program(c, is_max_of=None):
    chans, own = pool_pieces(c)
    g = tf.Graph()
    with g.as_default():
        outs = []
        for i, ch in enumerate(chans):
            x = tf.placeholder(tf.float32, [None, c.H, c.W, ch], name="x%d" % i)
            is_max = c.is_max if i == own else not c.is_max
            y = (tf.nn.max_pool if is_max else tf.nn.avg_pool)(x, [1, c.KH, c.KW, 1], [1, c.sh, c.sw, 1], c.pad)
            if c.epi != "none":
                y = tf.nn.bias_add(y, tf.constant(bias_of(ch, np.float32)))
                y = {"bias": tf.identity, "bias_relu": tf.nn.relu, "bias_relu6": tf.nn.relu6}[c.epi](y)
            outs.append(y)
        tf.identity(outs[0], name="y") if len(outs) == 1 else tf.concat(outs, 3, name="y")
    names = ["x%d" % i for i in range(len(chans))]
    prog = engine.program(g.serialize(), ["y"], names)
    plan = prog.describe([torch.zeros([c.N, c.H, c.W, ch]) for ch in chans], as_gpu=True)
    if c.epi != "none":
        assert "+bias" in plan and ("relu" not in c.epi or "+" + c.epi[5:] in plan), plan
    if c.slice:
        assert "(%d inputs written in place)" % len(chans) in plan, plan
    assert "FUSED" not in plan, plan
    return prog, chans, own


@pytest.mark.parametrize("case", gc.POOL_CASES, ids=[c.id for c in gc.POOL_CASES])
def test_pool_exact(case):
    c = case
    prog, chans, own = pool_program(c)
    xs = [pool_data(seed_of("pool", c.id, i), c.is_max if i == own else not c.is_max, c.N, c.H, c.W, ch)
          for i, ch in enumerate(chans)]
    want = np.concatenate([pool_epi_ref(pool_ref(x, c, c.is_max if i == own else not c.is_max), c.epi)
                           for i, x in enumerate(xs)], 3)
    _C.set_pool_route(c.force)
    (got,) = run(prog, xs)
    assert_same(got, want, c.id)


POOL_NAN_ROUTES = [None, "pool3x3_v4", "generic_v4_u32", "generic_v4_i64", "generic_v1_i64"]


@pytest.mark.parametrize("force", POOL_NAN_ROUTES, ids=[r or "auto" for r in POOL_NAN_ROUTES])
@pytest.mark.parametrize("is_max", [True, False], ids=["max", "avg"])
def test_pool_nan_reaches_exactly_its_windows(is_max, force):
    """A NaN at a corner, an edge and an interior pixel of a 3x3 SAME pool: with
    stride 1 and 2 the pixel sits in 4 / 6 / 9 and in 1 / 2 / 4 windows, and
    exactly those outputs are NaN. On the border the clamped address of a
    masked tap holds the NaN itself: it must not leak into a window that does
    not contain the pixel."""
    for stride in (1, 2):
        for (i, j) in ((0, 0), (6, 6), (0, 3), (3, 6), (3, 3), (2, 2), (6, 0)):
            c = gc._pool(is_max, 2, 7, 7, 8, 3, 3, stride, stride, "SAME", "none", None, force)
            x = pool_data(seed_of("nan", is_max), is_max, 2, 7, 7, 8)
            x[1, i, j, 5] = np.nan
            want = pool_ref(x, c)
            oh, pt = gc.pool_out(7, 3, stride, "SAME")
            inside = [(a, b) for a in range(oh) for b in range(oh)
                      if a * stride - pt <= i < a * stride - pt + 3 and b * stride - pt <= j < b * stride - pt + 3]
            assert np.isnan(want).sum() == len(inside) and all(np.isnan(want[1, a, b, 5]) for a, b in inside)
            per_dim = {1: {0: 2, 6: 2}, 2: {0: 1, 2: 1, 6: 1}}[stride]
            assert len(inside) == per_dim.get(i, 4 - stride) * per_dim.get(j, 4 - stride)   # 1, 2, 4 and 4, 6, 9 windows
            prog, _, _ = pool_program(c)
            _C.set_pool_route(force)
            assert_same(run(prog, [x])[0], want, "NaN at (%d, %d), stride %d" % (i, j, stride))
            _C.set_pool_route(None)
            if is_max:
                assert_same(run(prog, [x], CPU)[0], want, "host executor, NaN at (%d, %d), stride %d" % (i, j, stride))


@pytest.mark.parametrize("force", [None, "generic_v1_u32"], ids=["auto", "generic_v1_u32"])
def test_pool_nan_with_two_window_overlap_and_fused_relu(force):
    """Stride (1, 2) puts an interior pixel in 3 x 2 windows; the fused bias +
    ReLU6 after the pool keeps the NaN."""
    for is_max in (True, False):
        c = gc._pool(is_max, 1, 5, 8, 4, 3, 3, 1, 2, "SAME", "bias_relu6", None, force)
        x = pool_data(9, is_max, 1, 5, 8, 4)
        x[0, 2, 2, 1] = np.nan
        want = pool_epi_ref(pool_ref(x, c), c.epi)
        assert np.isnan(want).sum() == 6
        prog, _, _ = pool_program(c)
        _C.set_pool_route(force)
        assert_same(run(prog, [x])[0], want, "max" if is_max else "avg")


@pytest.mark.parametrize("force", [None, "generic_v4_u32", "generic_v1_i64"], ids=["auto", "generic_v4_u32", "generic_v1_i64"])
def test_max_pool_of_infinities(force):
    """An all -inf image pools to -inf (the accumulator's start value is a valid
    input), +inf wins its windows, and padding never shows."""
    for k, s, pad in ((3, 1, "SAME"), (3, 2, "VALID"), (2, 2, "SAME")):
        c = gc._pool(True, 3, 5, 5, 4, k, k, s, s, pad, "none", None, force)
        x = pool_data(13, True, 3, 5, 5, 4)
        x[0] = -np.inf
        x[1, 2, 2, :] = np.inf
        x[2, 0, 0, 1] = -np.inf
        want = pool_ref(x, c)
        assert np.isneginf(want[0]).all() and np.isposinf(want[1]).any()
        prog, _, _ = pool_program(c)
        _C.set_pool_route(c.force)
        assert_same(run(prog, [x])[0], want, "%dx%d/%d %s" % (k, k, s, pad))
        _C.set_pool_route(None)
