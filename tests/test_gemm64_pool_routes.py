"""The case table of tests/gemm64_pool_cases.py against the host-side routing of
csrc/kernels/gemm_f64.hip: every case lands on the kernel route it was written
for, and every route the three dispatch functions can return is named by a
case. No device is needed: `_C.gemm_f64_route`, `_C.gemm_int_route` and
`_C.pool_route` are the functions the launch code itself switches on."""
import numpy as np
import pytest
import torch

import gemm64_pool_cases as gc
from tensorframes_amd import engine, tf
from tensorframes_amd._native import _C


@pytest.fixture(autouse=True)
def automatic_pool_route():
    _C.set_pool_route(None)
    yield
    _C.set_pool_route(None)


# ------------------------------------------------------------------ f64 GEMM
def f64_info(c):
    lda, ldb = (c.M if c.ta else c.K), (c.K if c.tb else c.N)
    return _C.gemm_f64_route(c.M, c.N, c.K, c.batch, c.ta, c.tb, lda, ldb)


@pytest.mark.parametrize("case", gc.F64_CASES, ids=[c.id for c in gc.F64_CASES])
def test_f64_case_lands_on_its_route(case):
    info = f64_info(case)
    assert info["tile"] == case.tile and info["kernel"] == gc.f64_kernel(case)
    assert (info["BM"], info["BN"]) == gc._TILE_DIMS[case.tile]
    assert info["grid"] == (-(-case.M // info["BM"]) * -(-case.N // info["BN"]), 1, case.batch)
    assert info["launches"] == 1
    assert info["k_mult16"] == (case.K % 16 == 0)
    # the block kinds the case names are the ones its grid holds
    lda, ldb = (case.M if case.ta else case.K), (case.K if case.tb else case.N)
    assert info["a_pairs"] == (lda % 2 == 0) and info["b_pairs"] == (ldb % 2 == 0)
    assert case.kinds == gc.f64_block_kinds(case.M, case.N, case.K, case.batch, case.ta, case.tb, info["BM"],
                                            info["BN"], case.bcast_b)
    assert case.fast == ("I" in case.kinds and info["k_mult16"])


def _f64_hit(cases):
    hit = {}
    for c in cases:
        hit.setdefault(gc.f64_kernel(c), []).append(c)
    return hit


def test_every_f64_kernel_has_its_cases():
    names = set(_C.gemm_f64_kernel_names())
    assert len(names) == 12                      # tile x transpose_a x transpose_b
    hit = _f64_hit(gc.F64_CASES)
    assert set(hit) == names, sorted(names ^ set(hit))
    for kernel, cases in hit.items():
        kinds = set("".join(c.kinds for c in cases))
        assert kinds == set("IMNC"), (kernel, kinds)
        ks = {c.K for c in cases}
        assert {16, 17, 48} <= ks, (kernel, ks)
        # the FAST loop with one k-tile and with the pipelined tiles before the peeled last one
        assert {c.K for c in cases if c.fast} >= {16, 48}, kernel
        # a checked K tail behind full k-tiles, in a block that loads in pairs
        assert {c.K for c in cases if "I" in c.kinds} >= {18, 34}, kernel
    for tile in gc._TILE_DIMS:
        on_tile = [c for c in gc.F64_CASES if c.tile == tile]
        assert {c.K for c in on_tile} >= set(gc.KS), tile
        # every epilogue on a grid with interior and edge blocks (the 64x16 grid is one tile wide: I and M)
        assert {c.epi for c in on_tile if "I" in c.kinds and len(c.kinds) > 1} >= set(gc.EPILOGUES), tile
    assert {c.batch for c in gc.F64_CASES} >= {1, 3} and any(c.bcast_b for c in gc.F64_CASES)
    blocks = {f64_info(c)["grid"][0] for c in gc.F64_CASES if c.tile == "64x64"}
    assert {1, 3, 13} <= blocks                  # no multiple of 8: the XCD remap's remainder path


def test_f64_completeness_check_notices_a_deleted_case():
    names = set(_C.gemm_f64_kernel_names())
    fewer = [c for c in gc.F64_CASES if not (c.tile == "128x128" and c.ta and not c.tb)]
    assert len(fewer) < len(gc.F64_CASES) and set(_f64_hit(fewer)) != names


def test_f64_tile_thresholds():
    r = _C.gemm_f64_route
    assert r(100000, 16, 8)["tile"] == "64x16" and r(100000, 17, 8)["tile"] == "64x64"
    assert r(32768, 64, 8)["tile"] == "64x64"                    # N <= 64 never takes the big tile
    assert r(511 * 128, 65, 8)["tile"] == "64x64" and r(511 * 128 + 1, 65, 8)["tile"] == "128x128"   # 512 blocks of 128 rows
    assert r(128 * 255, 256, 8)["tile"] == "64x64" and r(128 * 256, 256, 8)["tile"] == "128x128"
    assert r(513, 129, 8, 51)["tile"] == "64x64" and r(513, 129, 8, 52)["tile"] == "128x128"
    # operands off the 16-byte pairs: the kernel is the same, every block checks that operand
    info = r(130, 78, 32, 1, False, False, 32, 78, False, True)
    assert (info["a_pairs"], info["b_pairs"]) == (False, True)
    assert r(130, 78, 32, 1, False, False, 33, 78)["a_pairs"] is False


def test_f64_batches_run_in_grid_z_slices():
    """Up to 65535 batches fit grid.z; more run as further launches (the launch
    refused them before: `gemm: batch too large`)."""
    r = _C.gemm_f64_route
    assert r(1, 1, 1, 65535)["launches"] == 1 and r(1, 1, 1, 65535)["grid"] == (1, 1, 65535)
    info = r(1, 1, 1, 65536)
    assert info["launches"] == 2 and info["max_batch_per_launch"] == 65535 and info["grid"][2] == 65535
    assert r(2, 2, 3, 3 * 65535 + 1)["launches"] == 4


# ------------------------------------------------------------------ integer GEMM
@pytest.mark.parametrize("case", gc.INT_CASES, ids=[c.id for c in gc.INT_CASES])
def test_int_case_grid(case):
    info = _C.gemm_int_route(case.M, case.N, case.K, case.batch)
    assert info["grid"] == (-(-case.M // 16) * -(-case.N // 16), 1, case.batch) and info["launches"] == 1


def test_int_cases_cover_the_tile_edges():
    for dtype in ("int32", "int64"):
        cs = [c for c in gc.INT_CASES if c.dtype == dtype]
        assert {(c.ta, c.tb) for c in cs} == set(gc.TRANS)
        assert {c.M for c in cs} >= {1, 15, 16, 17, 33} and {c.N for c in cs} >= {1, 15, 16, 17, 33}
        assert {c.K for c in cs} >= {1, 16, 17, 40} and {c.batch for c in cs} >= {1, 3}
        assert {c.epi for c in cs} >= {"none", "bias", "bias_relu", "bias_relu6"}


def test_int_gemm_limits():
    """Row tiles run along grid.x (2^31 - 1 blocks), not grid.y (65535: M <=
    1,048,560, which the 2.5 M-row frames exceed), and batches in grid.z slices."""
    r = _C.gemm_int_route
    info = r(gc.INT_LIMIT_M, 1, 2)
    assert info["grid"] == (65536, 1, 1) and info["launches"] == 1
    assert info["grid"][0] > 65535               # what grid.y could not hold
    assert r(2500000, 33, 5)["grid"] == (156250 * 3, 1, 1)
    assert r(1, 1, 1, gc.INT_LIMIT_BATCH)["launches"] == 2
    assert r(1, 1, 1, gc.INT_LIMIT_BATCH)["max_batch_per_launch"] == 65535
    with pytest.raises(_C.GraphError, match="grid too large"):
        r(16 << 31, 1, 1)


# ------------------------------------------------------------------ pooling
def pool_route_of(c, name_only=True):
    OH, _ = gc.pool_out(c.H, c.KH, c.sh, c.pad)
    OW, _ = gc.pool_out(c.W, c.KW, c.sw, c.pad)
    ldc = c.slice[1] if c.slice else 0
    y_aligned = c.slice is None or c.slice[0] % 4 == 0
    f = _C.pool_route if name_only else _C.pool_route_info
    return f(c.N, c.H, c.W, c.C, OH, OW, c.KH, c.KW, ldc, True, y_aligned)


@pytest.mark.parametrize("case", gc.POOL_CASES, ids=[c.id for c in gc.POOL_CASES])
def test_pool_case_lands_on_its_route(case):
    assert pool_route_of(case) == gc.pool_auto_route(case.C, case.KH, case.KW, case.slice)
    _C.set_pool_route(case.force)
    info = pool_route_of(case, name_only=False)
    assert info["route"] == case.route
    assert info["V"] == (4 if "v4" in case.route else 1)
    OH, OW = gc.pool_out(case.H, case.KH, case.sh, case.pad)[0], gc.pool_out(case.W, case.KW, case.sw, case.pad)[0]
    assert info["items"] == case.N * OH * OW * case.C // info["V"]
    assert info["blocks"] == min(-(-info["items"] // 256), 1 << 30 if case.route == "pool3x3_v4_xcd" else 2048)


def test_every_pool_route_has_its_cases():
    names = _C.pool_route_names()
    assert tuple(names) == gc.POOL_ROUTES
    for is_max in (True, False):
        cs = [c for c in gc.POOL_CASES if c.is_max == is_max]
        assert {c.route for c in cs} == set(names), sorted(set(names) - {c.route for c in cs})
        for route in names:
            on = [c for c in cs if c.route == route]
            assert {c.epi for c in on} >= ({"none", "bias_relu6"} if route != "generic_v1_u32" else {"none", "bias"}), route
            assert any(c.slice for c in on), route
            assert {c.N for c in on} >= {1, 3}, route
        assert {(c.H, c.W) for c in cs} >= set(gc.IMAGES) and {(c.KH, c.KW) for c in cs} >= set(gc.WINDOWS) | {(8, 8)}
        assert {(c.sh, c.sw) for c in cs} >= set(gc.STRIDES) and {c.C for c in cs} >= set(gc.CHANNELS)
        assert {c.pad for c in cs} == {"SAME", "VALID"}
        # a concat slice whose offset keeps float4 stores and one that loses them with C % 4 == 0
        assert any(c.slice and c.slice[0] % 4 == 0 and c.slice[0] and "v4" in c.route for c in cs)
        assert any(c.slice and c.slice[0] % 4 and c.C % 4 == 0 and c.slice[1] % 4 == 0 and c.route == "generic_v1_u32"
                   for c in cs)
        # above 256 items with a block count that is no multiple of 8, on the XCD-remapped grid
        xcd = [pool_route_of(c, False)["blocks"] for c in cs if c.route == "pool3x3_v4_xcd"]
        assert any(b > 1 and b % 8 for b in xcd), xcd


def test_pool_completeness_check_notices_a_deleted_case():
    fewer = [c for c in gc.POOL_CASES if c.route != "generic_v4_i64"]
    assert len(fewer) < len(gc.POOL_CASES)
    assert {c.route for c in fewer} != set(_C.pool_route_names())


def test_pool_route_thresholds():
    r = _C.pool_route
    assert r(1, 8, 8, 8, 8, 8, 3, 3) == "pool3x3_v4_xcd"
    assert r(1, 8, 8, 8, 8, 8, 3, 2) == "generic_v4_u32" and r(1, 8, 8, 6, 8, 8, 3, 3) == "generic_v1_u32"
    assert r(1, 8, 8, 8, 8, 8, 3, 3, 0, False, True) == "generic_v1_u32"      # x off 16 bytes
    assert r(1, 8, 8, 8, 8, 8, 3, 3, 0, True, False) == "generic_v1_u32"      # the slice offset is no multiple of 4
    assert r(1, 8, 8, 8, 8, 8, 3, 3, 12) == "pool3x3_v4_xcd" and r(1, 8, 8, 8, 8, 8, 3, 3, 10) == "generic_v1_u32"
    # 2^31 input or output elements: 64-bit indices, and no 3x3 kernel
    assert r(2, 32768, 32768, 4, 16384, 16384, 3, 3) == "generic_v4_i64"
    assert r(2, 32768, 32768, 1, 16384, 16384, 3, 3) == "generic_v1_i64"
    assert r(1, 32768, 32768, 1, 32768, 32768, 3, 3) == "generic_v1_u32"
    assert r(1, 16384, 16384, 4, 16384, 16384, 3, 3) == "pool3x3_v4_xcd"
    # the output span of a wide concat row alone passes 2^31: generic kernel, still 32-bit items
    assert r(1, 16384, 16384, 4, 16384, 16384, 3, 3, 8) == "generic_v4_u32"


def test_set_pool_route_only_forces_a_less_specialised_route():
    order = _C.pool_route_names()
    args3 = (3, 13, 11, 8, 13, 11, 3, 3)           # automatic: pool3x3_v4_xcd
    for name in order:
        _C.set_pool_route(name)
        assert _C.pool_route(*args3) == name
    _C.set_pool_route(order.index("generic_v1_i64"))
    assert _C.pool_route(*args3) == "generic_v1_i64"
    _C.set_pool_route(-1)
    assert _C.pool_route(*args3) == "pool3x3_v4_xcd"
    # more specialised than the shape allows: an error, never another kernel
    for name, args in (("pool3x3_v4_xcd", (3, 13, 11, 8, 13, 11, 3, 2)), ("pool3x3_v4", (3, 13, 11, 8, 13, 11, 2, 2)),
                       ("generic_v4_u32", (3, 13, 11, 7, 13, 11, 3, 3)), ("generic_v4_i64", (3, 13, 11, 7, 13, 11, 2, 2)),
                       ("generic_v1_u32", (2, 32768, 32768, 1, 16384, 16384, 3, 3)),
                       ("pool3x3_v4", (2, 32768, 32768, 4, 16384, 16384, 3, 3))):
        _C.set_pool_route(name)
        with pytest.raises(_C.GraphError, match="more specialised"):
            _C.pool_route(*args)
    _C.set_pool_route("generic_v1_i64")             # the least specialised route serves everything
    for args in ((3, 13, 11, 7, 13, 11, 2, 2), (2, 32768, 32768, 1, 16384, 16384, 3, 3)):
        assert _C.pool_route(*args) == "generic_v1_i64"
    with pytest.raises(_C.GraphError):
        _C.set_pool_route("pool7x7")
    with pytest.raises(_C.GraphError):
        _C.set_pool_route(6)


# ------------------------------------------------------------------ host executor: the contract the device follows
def _host(build, feeds):
    g = tf.Graph()
    with g.as_default():
        build()
    names = list(feeds)
    prog = engine.program(g.serialize(), ["y"], names)
    return engine.run_program(prog, [torch.as_tensor(feeds[n]) for n in names], torch.device("cpu"))[0].numpy()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_host_relu_keeps_nan_fused_and_alone(dtype):
    x = np.array([[np.nan, -1.0], [7.0, 3.0]], dtype)

    def fused(act):
        def build():
            xi = tf.placeholder(dtype, [None, 2], name="x")
            act(tf.nn.bias_add(tf.matmul(xi, tf.constant(np.eye(2, dtype=dtype))), tf.constant(np.zeros(2, dtype))), name="y")
        return build
    for act, hi in ((tf.nn.relu, np.inf), (tf.nn.relu6, 6.0)):
        want = np.array([[np.nan, np.nan], [min(7.0, hi), 3.0]], dtype)   # NaN * 0 of the identity: row 0 is NaN
        got = _host(fused(act), {"x": x})
        assert np.array_equal(got, want, equal_nan=True), (got, want)
        got = _host(lambda: act(tf.placeholder(dtype, [None, 2], name="x"), name="y"), {"x": x})
        assert np.array_equal(got, np.array([[np.nan, 0.0], [min(7.0, hi), 3.0]], dtype), equal_nan=True), got


def test_host_max_pool_keeps_nan():
    x = np.arange(25, dtype=np.float32).reshape(1, 5, 5, 1)
    x[0, 2, 2, 0] = np.nan
    got = _host(lambda: tf.nn.max_pool(tf.placeholder(np.float32, [None, 5, 5, 1], name="x"), [1, 3, 3, 1], [1, 2, 2, 1],
                                       "VALID", name="y"), {"x": x})
    assert got.shape == (1, 2, 2, 1) and np.isnan(got).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_host_matmul_k0_applies_the_fused_epilogue(dtype):
    b = np.array([-2.0, 3.0, 9.0], dtype)

    def build():
        xi = tf.placeholder(dtype, [None, 0], name="x")
        tf.nn.relu6(tf.nn.bias_add(tf.matmul(xi, tf.constant(np.zeros((0, 3), dtype))), tf.constant(b)), name="y")
    got = _host(build, {"x": np.zeros((4, 0), dtype)})
    assert np.array_equal(got, np.tile(np.array([0.0, 3.0, 6.0], dtype), (4, 1)))
