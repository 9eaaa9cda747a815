"""The case table of tests/fusion_cases.py against the planner and the code
generator of csrc/runtime/fusion.cpp. No device is needed: `describe(inputs,
as_gpu=True)` plans as for a GPU and prints the route of every generated
kernel, and `_C.jit_compile` compiles a generated source for gfx950.

The table holds several hundred cases but few distinct kernels, because the
element count, the row count and the row length are kernel arguments: the
compile test builds each distinct source once (282 sources for 516 cases)."""
import collections
import re

import pytest
import torch

import fusion_cases as fc
from tensorframes_amd import engine
from tensorframes_amd._native import _C

FUSIBLE = _C.fusible_ops()
CASES = fc.build_cases(FUSIBLE)
IDS = [c.id for c in CASES]


def plan_of(case):
    """(program, inputs, plan text) of a case as a GPU would plan it."""
    g, fetches, feeds = case.build()
    prog = engine.program(g.serialize(), fetches, feeds)
    values = case.feeds()
    inputs = [torch.from_numpy(values[k].copy()) for k in feeds]
    _C.set_fusion_index64(True if case.idx == 64 else None)
    try:
        return prog, inputs, prog.describe(inputs, True), prog.fused_sources(inputs)
    finally:
        _C.set_fusion_index64(None)


def fused_lines(plan):
    return [ln for ln in plan.splitlines() if ln.startswith("  FUSED")]


def test_case_ids_are_unique():
    assert len(set(IDS)) == len(IDS)


def test_fusible_ops_lists_the_generator_table():
    assert len(FUSIBLE) == 50
    assert {f["kind"] for f in FUSIBLE.values()} == {"unary", "binary", "cast", "view", "broadcast"}
    assert FUSIBLE["Cast"] == {"kind": "cast", "float_only": False}
    assert FUSIBLE["Tile"]["kind"] == FUSIBLE["BroadcastTo"]["kind"] == "broadcast"
    assert FUSIBLE["Pow"] == {"kind": "binary", "float_only": True}
    assert FUSIBLE["Abs"] == {"kind": "unary", "float_only": False}
    # every unary and binary op has a reference in the table's module
    for op, f in FUSIBLE.items():
        if f["kind"] == "unary":
            assert op in fc.UNARY_REF, op
        if f["kind"] == "binary":
            assert op in fc.BINARY_REF, op


def _op_dtype_pairs(cases):
    return {(c.op, c.dtype) for c in cases if c.op and c.idx == 32}


def _wanted_pairs():
    return {(op, dt) for op, f in FUSIBLE.items() for dt in fc.DTYPES if dt in fc.FLOATS or not f["float_only"]}


def test_every_op_and_dtype_is_in_the_table():
    missing = _wanted_pairs() - _op_dtype_pairs(CASES)
    assert not missing, sorted(missing)
    casts = {c.id for c in CASES if c.op == "Cast"}
    for dst in fc.DTYPES:
        for src in fc.DTYPES + ("uint8",):
            if src != dst:
                assert "sweep-Cast-%s-to-%s" % (src, dst) in casts
    # and the 64-bit index variant runs one op of each kind per dtype
    wide = {(FUSIBLE[c.op]["kind"], c.dtype) for c in CASES if c.op and c.idx == 64}
    assert wide == {(k, dt) for k in ("unary", "binary", "cast", "broadcast") for dt in fc.DTYPES}


def _routes(cases):
    r = set()
    for c in cases:
        for leaf in c.leaves:
            r.add((c.kind, c.idx, c.row, leaf))
    return r


ALL_ROUTES = {(kind, idx, row, leaf)
              for kind, rows in (("FUSED", (None,)), ("FUSED-ROWRED", ("thread", "wave")))
              for idx in (32, 64) for row in rows for leaf in ("contiguous", "scalar", "strided")}


def test_every_route_is_in_the_table():
    assert _routes(CASES) == ALL_ROUTES, sorted(ALL_ROUTES - _routes(CASES), key=str)
    assert len(ALL_ROUTES) == 18
    # every row reduction on every dtype, with and without a prologue, on both row routes and index widths
    seen = collections.Counter()
    for c in CASES:
        if c.kind == "FUSED-ROWRED" and c.id.startswith("rowred-") and "-nd-" not in c.id:
            seen[(c.id.split("-")[1], c.row, c.idx, "->" in c.ops)] += 1
    for dt in fc.DTYPES:
        for row in ("thread", "wave"):
            for idx in (32, 64):
                for prologue in (True, False):
                    assert seen[(dt, row, idx, prologue)] >= 3, (dt, row, idx, prologue)
    assert {i for _, i in fc.ROWRED_SHAPES} == {1, 3, 16, 17, 63, 64, 65, 129, 1000}
    assert {o for o, _ in fc.ROWRED_SHAPES} == {256, 257, 302}
    assert set(fc.GEOMETRY_N) >= {1, 255, 256, 257, 1023, 1024, 1025} and max(fc.GEOMETRY_N) > 2048


def test_completeness_checks_notice_a_deleted_entry():
    """One entry of each kind taken out of the table must be noticed: an op of
    one dtype, a cast pair's dtype, and the only cases of a route."""
    fewer = [c for c in CASES if not (c.op == "Relu6" and c.dtype == "int64")]
    assert len(fewer) < len(CASES) and _wanted_pairs() - _op_dtype_pairs(fewer) == {("Relu6", "int64")}
    fewer = [c for c in CASES if not (c.op == "Cast" and c.dtype == "float32")]
    assert ("Cast", "float32") in _wanted_pairs() - _op_dtype_pairs(fewer)
    fewer = [c for c in CASES if not (c.kind == "FUSED-ROWRED" and c.idx == 64 and c.row == "thread"
                                      and "strided" in c.leaves)]
    assert _routes(fewer) == ALL_ROUTES - {("FUSED-ROWRED", 64, "thread", "strided")}
    fewer = [c for c in CASES if not (c.kind == "FUSED" and c.idx == 64)]
    assert len(ALL_ROUTES - _routes(fewer)) == 3


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_plans_onto_its_route(case):
    """Exactly one generated kernel, with the ops, index width, row route and
    leaf kinds the table names: a case that stops fusing, or fuses less, fails."""
    _, _, plan, sources = plan_of(case)
    lines = fused_lines(plan)
    assert len(lines) == 1 and len(sources) == 1, plan
    head, tail = fc.line_of(case)
    m = re.match(r"  (FUSED(?:-ROWRED)?) (\S+) (\[[^\]]*\] )(\d+) inputs (\d+) outputs \[[^\]]*\]( idx.*)$", lines[0])
    assert m, lines[0]
    assert m.group(1) == case.kind, lines[0]
    assert m.group(3) == head, lines[0]
    assert m.group(6) == tail, lines[0]
    assert int(m.group(4)) == len(case.leaves)
    assert ("typedef unsigned long long idx_t;" in sources[0]) == (case.idx == 64)


def test_index_width_is_part_of_the_plan_key():
    """A plan cached under the automatic index width is not served once 64-bit
    indices are forced, and the other way round (plan_for caches per program)."""
    case = next(c for c in CASES if c.id == "geometry-n257-float32")
    g, fetches, feeds = case.build()
    prog = engine.program(g.serialize(), fetches, feeds)
    values = case.feeds()
    inputs = [torch.from_numpy(values[k]) for k in feeds]
    before = prog.stats()["plans_built"]
    try:
        prog.describe(inputs)            # host plan, cached
        prog.describe(inputs)
        assert prog.stats()["plans_built"] == before + 1
        _C.set_fusion_index64(True)
        prog.describe(inputs)
        assert prog.stats()["plans_built"] == before + 2
        _C.set_fusion_index64(None)
        prog.describe(inputs)
        assert prog.stats()["plans_built"] == before + 2
        assert "idx32" in prog.describe(inputs, True)
        _C.set_fusion_index64(True)
        assert "idx64" in prog.describe(inputs, True)
        _C.set_fusion_index64(False)
        assert "idx32" in prog.describe(inputs, True)
    finally:
        _C.set_fusion_index64(None)


def test_every_generated_source_compiles_for_gfx950():
    sources = {}
    for case in CASES:
        src = plan_of(case)[3][0]
        # the first line is a comment naming the ops; the kernel below it is what is compiled and cached
        sources.setdefault(src, case.id)
    assert 150 < len(sources) < 400, len(sources)
    for src, cid in sources.items():
        assert _C.jit_compile(src) > 1000, cid
