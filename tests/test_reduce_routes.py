"""The case table of tests/reduce_cases.py against the host-side routing of
csrc/kernels/reduce.hip: every case lands on the kernel route it was written
for, and every route the dispatch can take is named by a case of each element
width. No device is needed: `_C.reduce_route` and `_C.unsorted_segment_route`
are the functions the launch code itself switches on."""
import collections

import numpy as np
import pytest
import torch

import reduce_cases as rc
from tensorframes_amd import engine, tf
from tensorframes_amd._native import _C


@pytest.mark.parametrize("case", rc.REDUCE_CASES, ids=[c.id for c in rc.REDUCE_CASES])
def test_reduce_case_lands_on_its_route(case):
    outer, r, inner, _ = rc.canonical(case.shape, case.axes)
    assert _C.reduce_route(case.dtype, outer, r, inner) == case.route


def _routes_hit(cases):
    hit = collections.defaultdict(set)
    for c in cases:
        hit[rc.WIDTH[c.dtype]].add(c.route)
    return hit


def test_every_reduce_route_has_a_case_per_width():
    names = set(_C.reduce_route_names())
    assert len(names) == 11
    hit = _routes_hit(rc.REDUCE_CASES)
    for width in (4, 8, 1):
        assert hit[width] == names, "width %d: no case for %s" % (width, sorted(names - hit[width]))
    for dtype in rc.WIDTH:
        assert {c.route for c in rc.REDUCE_CASES if c.dtype == dtype} == names, dtype


def test_completeness_check_notices_a_deleted_case():
    """Dropping the only row-split-with-fold case of a width must be noticed."""
    names = set(_C.reduce_route_names())
    fewer = [c for c in rc.REDUCE_CASES if not (c.route == "row_split_fold" and rc.WIDTH[c.dtype] == 8)]
    assert len(fewer) < len(rc.REDUCE_CASES)
    assert _routes_hit(fewer)[8] != names


def test_unaligned_input_takes_the_scalar_kernels():
    for dtype, vec in (("float32", 4), ("float64", 2), ("int32", 4), ("int64", 2), ("bool", 16)):
        assert _C.reduce_route(dtype, 1024, 4 * vec, 1, True) == "row_wave_vec"
        assert _C.reduce_route(dtype, 1024, 4 * vec, 1, False) == "row_wave"
        assert _C.reduce_route(dtype, 2048, 3, vec, True) == "col_vec"
        assert _C.reduce_route(dtype, 2048, 3, vec, False) == "col"
        # the number of slices and the workspace do not depend on the alignment
        a = _C.reduce_route_info(dtype, 4, 130, 2 * vec, True)
        b = _C.reduce_route_info(dtype, 4, 130, 2 * vec, False)
        assert (a["route"], b["route"]) == ("col_vec_split", "col_split")
        assert (a["S"], a["rows_per_split"], a["workspace_bytes"]) == (b["S"], b["rows_per_split"], b["workspace_bytes"])


def test_split_rows_always_have_two_slices():
    """inner == 1 off the wave route means outer < 1024 and r > 4096, where the
    plan gives at least two slices: the split kernels never run with S == 1."""
    for dtype in rc.WIDTH:
        for outer in (1, 2, 64, 65, 512, 1023):
            for r in (4097, 4100, 8191, 65536, 65537, 262144, 262145, 1 << 20):
                info = _C.reduce_route_info(dtype, outer, r, 1)
                assert info["route"] in ("row_block", "row_split", "row_split_fold")
                if info["route"] != "row_block":
                    assert info["S"] >= 2 and info["workspace_bytes"] >= info["S"] * outer * 8
                    assert (info["S"] - 1) * info["rows_per_split"] < r <= info["S"] * info["rows_per_split"]


def test_route_plans_are_consistent():
    for c in rc.REDUCE_CASES:
        outer, r, inner, _ = rc.canonical(c.shape, c.axes)
        info = _C.reduce_route_info(c.dtype, outer, r, inner)
        S, rps = info["S"], info["rows_per_split"]
        assert (S - 1) * rps < r <= S * rps            # every slice holds at least one row
        assert (info["fold"] > 0) == c.route.endswith("_fold") == (S > 64)
        assert (S > 1) == ("split" in c.route)
        assert (info["workspace_bytes"] > 0) == (S > 1)
        if c.route.startswith("col"):
            assert info["col_blocks"] == (inner // info["vec"] + 255) // 256
            assert (info["vec"] > 1) == ("vec" in c.route)


def test_reduce_route_rejects_bad_arguments():
    with pytest.raises(ValueError):
        _C.reduce_route("float16", 1, 1, 1)
    with pytest.raises(ValueError):
        _C.reduce_route("float32", 0, 1, 1)
    with pytest.raises(ValueError):
        _C.unsorted_segment_route("Mean", "float32", 1, 1, 1)


# ------------------------------------------------------------------ unsorted segment routes
@pytest.mark.parametrize("case", rc.USEG_CASES, ids=[c.id for c in rc.USEG_CASES])
def test_useg_case_lands_on_its_route(case):
    assert _C.unsorted_segment_route(case.op, case.dtype, case.n, case.inner, case.nseg) == case.route
    if case.blocks is not None:
        info = _C.unsorted_segment_route_info(case.op, case.dtype, case.n, case.inner, case.nseg)
        assert info["B"] == case.blocks
        assert info["G"] == min(64, 1 << (case.blocks - 1).bit_length())


def test_every_useg_route_has_a_case_per_width():
    names = set(_C.unsorted_segment_route_names())
    int_only = {"tiny_int", "small_int"}
    for dtype in ("float32", "float64", "int32", "int64"):
        hit = {c.route for c in rc.USEG_CASES if c.dtype == dtype}
        if dtype.startswith("float"):
            assert hit == names - int_only, "%s: no case for %s" % (dtype, sorted(names - int_only - hit))
        else:
            # the slab and sorted kernels do not depend on the element type beyond
            # its width: the float cases of the same width cover their other classes
            assert int_only <= hit and {"private_g64", "sorted_perm_p1", "sorted_perm_p4", "private_g16"} <= hit
    blocks = {c.blocks for c in rc.USEG_CASES if c.blocks}
    assert {1, 2, 63, 64, 65} <= blocks
    assert {c.ids_dtype for c in rc.USEG_CASES} == {"int32", "int64"}


def test_small_int_route_ends_where_the_lds_table_ends():
    """The LDS test comes first in the dispatch, so at inner == 1 the one-block
    integer route serves 17..128 segments and the sorted route takes over above
    (its 4096-entry table is never filled)."""
    for nseg, want in ((16, "tiny_int"), (17, "small_int"), (128, "small_int"), (129, "sorted_perm_p1"),
                       (4096, "sorted_perm_p1"), (4097, "sorted_perm_p1")):
        assert _C.unsorted_segment_route("Sum", "int64", 1000, 1, nseg) == want
    assert _C.unsorted_segment_route("Sum", "int64", 262145, 1, 128) == "private_g64"
    assert _C.unsorted_segment_route("Sum", "float64", 1000, 1, 16) == "private_g16"  # 16 blocks of 64 rows


# ------------------------------------------------------------------ host executor: empty inputs
RED_FN = {"Sum": tf.reduce_sum, "Mean": tf.reduce_mean, "Min": tf.reduce_min, "Max": tf.reduce_max,
          "Prod": tf.reduce_prod, "All": tf.reduce_all, "Any": tf.reduce_any}


def host_reduce(op, x, axes):
    g = tf.Graph()
    with g.as_default():
        RED_FN[op](tf.placeholder(x.dtype.type, [None] * x.ndim, name="x"), axes, name="y")
    prog = engine.program(g.serialize(), ["y"], ["x"])
    return engine.run_program(prog, [torch.as_tensor(x)], torch.device("cpu"))[0].numpy()


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32, np.int64])
def test_host_reduce_over_an_empty_axis(dtype):
    """Sum 0, Prod 1, float Mean NaN; Min, Max and an integer Mean have no value
    and raise the typed error (the device does the same, test_gpu_reduce_routes.py)."""
    x = np.zeros((3, 0, 2), dtype)
    assert np.array_equal(host_reduce("Sum", x, [1]), np.zeros((3, 2), dtype))
    assert np.array_equal(host_reduce("Prod", x, [1]), np.ones((3, 2), dtype))
    is_float = np.issubdtype(dtype, np.floating)
    for op in ["Min", "Max"] + ([] if is_float else ["Mean"]):
        with pytest.raises(_C.GraphError, match="empty axis"):
            host_reduce(op, x, [1])
    if is_float:
        y = host_reduce("Mean", x, [1])
        assert y.shape == (3, 2) and y.dtype == dtype and np.all(np.isnan(y))
    assert host_reduce("Max", np.zeros((0, 4, 2), dtype), [1]).shape == (0, 2)   # an empty kept axis is no error


def test_host_all_any_over_an_empty_axis():
    x = np.zeros((3, 0, 2), np.bool_)
    assert host_reduce("All", x, [1]).all() and not host_reduce("Any", x, [1]).any()


@pytest.mark.parametrize("op,ident", [("Sum", lambda i: 0), ("Prod", lambda i: 1), ("Min", lambda i: i.max),
                                      ("Max", lambda i: i.min)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32, np.int64])
def test_host_unsorted_segment_of_no_rows(dtype, op, ident):
    """No input rows: every segment gets the identity of the op and dtype, from
    the op and from the binding."""
    lim = np.finfo(dtype) if np.issubdtype(dtype, np.floating) else np.iinfo(dtype)
    want = np.full((4, 3), ident(lim), dtype)
    g = tf.Graph()
    with g.as_default():
        x = tf.placeholder(dtype, [None, 3], name="x")
        ids = tf.placeholder(np.int64, [None], name="ids")
        getattr(tf, "unsorted_segment_" + op.lower())(x, ids, 4, name="y")
    prog = engine.program(g.serialize(), ["y"], ["x", "ids"])
    x0, i0 = torch.zeros((0, 3), dtype=torch.as_tensor(np.zeros(1, dtype)).dtype), torch.zeros(0, dtype=torch.int64)
    got = engine.run_program(prog, [x0, i0], torch.device("cpu"))[0].numpy()
    assert got.dtype == dtype and np.array_equal(got, want)
    got = _C.unsorted_segment_reduce(op, x0, i0, 4).numpy()
    assert got.dtype == dtype and np.array_equal(got, want)
    # out-of-range ids are dropped and an empty segment keeps the identity, as on the device
    x1 = torch.full((2, 3), 7, dtype=x0.dtype)
    got = _C.unsorted_segment_reduce(op, x1, torch.tensor([1, 9]), 4).numpy()
    want[1] = 7
    assert np.array_equal(got, want)
