"""`tfs.Window` / `.over()` on host frames (frame/window.py): the API with its
typed errors, ranking semantics, the three frames, the defined row order, and
that the result does not depend on the partitioning or the number of ranks.

Expected values are brute force written here: the rows are sorted with
`np.lexsort` on the ordering table (`spec_words`, copied from
tests/test_gpu_group_agg.py), the groups are walked as Python lists, ranks come
from plain loops, integer sums are Python ints masked to 64 bits, float sums
are `fractions.Fraction` sums rounded once.

Ranks, counts, integer sums, min and max are exact. Float sums and avg of the
positive 1e4 + N(0, 1) data are held to (terms) * 2^-53 * 10 relative. On the
host path a partition adds its rows of a group one after the other
(`np.add.accumulate`) and the partitions' partials are folded in order, so the
terms of a value are the rows it covers + the partitions, + 1 for avg's
division."""
import json
import os
import socket
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import tensorframes_amd as tfs
from tensorframes_amd import Window, functions as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK = (1 << 64) - 1
DTYPES = [np.uint8, np.int8, np.int16, np.int32, np.int64, np.float32, np.float64]
UP, UF, CR = Window.unboundedPreceding, Window.unboundedFollowing, Window.currentRow


# ------------------------------------------------------------------ the specification
def spec_words(a: np.ndarray, descending: bool = False) -> np.ndarray:
    a = np.asarray(a)
    if a.dtype.kind == "f":
        bits, ubits = (32, np.uint32) if a.dtype == np.float32 else (64, np.uint64)
        b = a.view(ubits).astype(np.uint64)
        sign = np.uint64(1 << (bits - 1))
        full = np.uint64((1 << bits) - 1)
        qnan = np.uint64(0x7FC00000 if bits == 32 else 0x7FF8000000000000)
        b = np.where(np.isnan(a), qnan, b)
        b = np.where(b == sign, np.uint64(0), b)            # -0.0 -> +0.0
        w = np.where(b & sign != 0, ~b & full, b | sign)
        return (~w & full) if descending else w
    if a.dtype.kind in "bu":
        w = a.astype(np.uint64)
    else:
        w = a.astype(np.int64).view(np.uint64) ^ np.uint64(1 << 63)
    return ~w if descending else w


def float_total(vals):
    """The sum of f64 values, exact and rounded once; NaN / inf as IEEE adds them."""
    vals = [float(v) for v in vals]
    if any(np.isnan(v) for v in vals) or (np.inf in vals and -np.inf in vals):
        return float("nan")
    if np.inf in vals or -np.inf in vals:
        return np.inf if np.inf in vals else -np.inf
    return float(sum(Fraction(v) for v in vals))


def brute(cols, pkeys, okeys, exprs):
    """(perm, {name: list of expected values in output order}). okeys:
    [(column, descending)], exprs: [(name, fn, column, frame)] with frame one
    of rows / range / whole. min / max come back as the winning row's index
    into the sorted rows (the caller compares canonical values)."""
    words = [spec_words(cols[k]) for k in pkeys] + [spec_words(cols[k], d) for k, d in okeys]
    n = len(next(iter(cols.values())))
    perm = np.lexsort(words[::-1]) if words else np.arange(n)
    sw = [w[perm] for w in words]
    P = len(pkeys)
    gkey = [tuple(int(w[i]) for w in sw[:P]) for i in range(n)]
    okey = [tuple(int(w[i]) for w in sw[P:]) for i in range(n)]
    groups, start = [], 0
    for i in range(1, n + 1):
        if i == n or gkey[i] != gkey[start]:
            groups.append(list(range(start, i)))
            start = i
    out = {name: [None] * n for name, *_ in exprs}
    for g in groups:
        m = len(g)
        peer_first, peer_last, dense = [0] * m, [0] * m, [0] * m
        for j in range(m):
            peer_first[j] = j if j == 0 or okey[g[j]] != okey[g[j - 1]] else peer_first[j - 1]
            dense[j] = 1 if j == 0 else dense[j - 1] + (okey[g[j]] != okey[g[j - 1]])
        for j in range(m - 1, -1, -1):
            peer_last[j] = j if j == m - 1 or okey[g[j]] != okey[g[j + 1]] else peer_last[j + 1]
        for name, fn, col, frame in exprs:
            x = cols[col][perm][g] if col is not None else None
            for j in range(m):
                if fn == "row_number":
                    v = j + 1
                elif fn == "rank":
                    v = peer_first[j] + 1
                elif fn == "dense_rank":
                    v = dense[j]
                else:
                    e = j if frame == "rows" else (peer_last[j] if frame == "range" else m - 1)
                    if fn == "count":
                        v = e + 1
                    elif fn == "sum" and x.dtype.kind != "f":
                        s = sum(int(t) for t in x[:e + 1]) & MASK
                        v = s - (1 << 64) if s >> 63 else s
                    elif fn == "sum":
                        v = float_total(x[:e + 1])
                    elif fn == "avg":
                        t = [float(q) for q in x[:e + 1]]
                        bad = any(not np.isfinite(q) for q in t)
                        v = float_total(t) / (e + 1) if bad else float(sum(Fraction(q) for q in t) / (e + 1))
                    else:
                        w = spec_words(x[:e + 1])
                        v = x[int(np.argmin(w) if fn == "min" else np.argmax(w))]
                out[name][g[j]] = v
    return perm, out


def canonical(v):
    v = np.asarray(v)
    if v.dtype.kind != "f":
        return v
    return np.where(np.isnan(v), np.array(np.nan, dtype=v.dtype), v + v.dtype.type(0.0)).astype(v.dtype)


def check(out, cols, perm, want, exprs, float_terms=None):
    """The frame `out` against the brute force: row order, every column."""
    for k, v in cols.items():
        if k in out.columns:
            np.testing.assert_array_equal(out.to_numpy(k), v[perm], err_msg=k)
    for name, fn, col, frame in exprs:
        got = out.to_numpy(name)
        exp = want[name]
        if fn in ("row_number", "rank", "dense_rank"):
            assert got.dtype == np.int32
            assert got.tolist() == exp, name
        elif fn == "count" or (fn == "sum" and cols[col].dtype.kind != "f"):
            assert got.dtype == np.int64
            assert got.tolist() == exp, name
        elif fn in ("min", "max"):
            assert got.dtype == cols[col].dtype
            e = canonical(np.array(exp, dtype=cols[col].dtype))
            assert got.tobytes() == e.tobytes(), name
        else:
            assert got.dtype == np.float64
            for i, (a, b) in enumerate(zip(got.tolist(), exp)):
                if not np.isfinite(b):
                    assert (np.isnan(a) and np.isnan(b)) or a == b, (name, i, a, b)
                else:
                    bound = float_terms(i) * 2.0 ** -53 * 10
                    assert abs(a - b) <= bound * abs(b), (name, i, a, b, bound)


def base_columns(n=160, seed=0, nkeys=6):
    rng = np.random.default_rng(seed)
    return {
        "id": rng.integers(0, nkeys, n).astype(np.int32),
        "g": rng.integers(-2, 2, n).astype(np.int64),
        "t": rng.integers(0, 12, n).astype(np.int32),            # many ties
        "score": (1e4 + rng.standard_normal(n)).astype(np.float32),
        "x": (1e4 + rng.standard_normal(n)),
        "q": np.rint(100 * rng.standard_normal(n)).astype(np.int64),
        "i": np.arange(n, dtype=np.int64),
    }


def frame_of(cols, nparts=3):
    return tfs.from_columns(cols, num_partitions=nparts)


def terms_all(n, nparts):
    return lambda i: n + nparts + 1


# ------------------------------------------------------------------ API and typed errors
def test_exports_and_constants():
    assert tfs.Window is Window and isinstance(Window.partitionBy("id"), tfs.WindowSpec)
    assert Window.unboundedPreceding < 0 < Window.unboundedFollowing and Window.currentRow == 0
    w = Window.partitionBy("id").orderBy("t").rowsBetween(UP, CR)
    assert isinstance(w.partitionBy("g").orderBy(tfs.desc("t")).rangeBetween(UP, UF), tfs.WindowSpec)
    assert isinstance(F.sum("x").over(w), tfs.WindowExpression)


def test_ranking_needs_order_and_takes_no_frame():
    for fn in (F.row_number, F.rank, F.dense_rank):
        with pytest.raises(ValueError, match="orderBy"):
            fn().over(Window.partitionBy("id"))
        with pytest.raises(ValueError, match="frame"):
            fn().over(Window.partitionBy("id").orderBy("t").rowsBetween(UP, CR))


@pytest.mark.parametrize("bounds", [(-1, 0), (UP, 1), (CR, UF), (0, 0), (-3, 3)])
@pytest.mark.parametrize("kind", ["rowsBetween", "rangeBetween"])
def test_unsupported_frames_name_their_bounds(kind, bounds):
    w = getattr(Window.partitionBy("id").orderBy("t"), kind)(*bounds)
    with pytest.raises(NotImplementedError) as e:
        F.sum("x").over(w)
    assert kind in str(e.value)
    for b in bounds:
        assert ("unboundedPreceding" if b == UP else "unboundedFollowing" if b == UF else
                "currentRow" if b == 0 else str(b)) in str(e.value)


@pytest.mark.parametrize("fn", ["stddev", "stddev_samp", "stddev_pop", "variance", "var_samp", "var_pop"])
def test_stddev_family_is_refused_by_name(fn):
    with pytest.raises(NotImplementedError) as e:
        getattr(F, fn)("x").over(Window.partitionBy("id"))
    assert F.FUNCTIONS[fn] in str(e.value)


def test_functions_that_are_not_added():
    for name in ("lag", "lead", "ntile", "percent_rank", "cume_dist"):
        assert not hasattr(F, name)


def test_window_expression_only_in_with_column_and_select():
    df = frame_of(base_columns())
    w = Window.partitionBy("id").orderBy("t")
    e = F.row_number().over(w)
    with pytest.raises(TypeError, match="withColumn"):
        df.filter(e)
    with pytest.raises(TypeError, match="withColumn"):
        df.orderBy(e)
    with pytest.raises(TypeError, match="withColumn"):
        df.groupBy("id").agg(e)
    with pytest.raises(TypeError, match="withColumn"):
        df.agg(e)
    with pytest.raises(TypeError, match="withColumn"):
        e + 1
    with pytest.raises(TypeError, match="withColumn"):
        df.x * e
    with pytest.raises(TypeError, match="withColumn"):
        e <= 3


def test_select_rules():
    df = frame_of(base_columns())
    w = Window.partitionBy("id").orderBy("t")
    with pytest.raises(ValueError, match="alias"):
        df.select("id", F.rank().over(w))
    with pytest.raises(TypeError, match="split"):
        df.select("id", (df.x + 1).alias("y"), F.rank().over(w).alias("r"))
    with pytest.raises(ValueError, match="duplicate"):
        df.select("id", F.rank().over(w).alias("id"))
    with pytest.raises(ValueError, match="not found"):
        df.select("nope", F.rank().over(w).alias("r"))


def test_key_refusals():
    cols = base_columns()
    cols["s"] = np.array([f"s{i % 3}" for i in range(len(cols["i"]))])
    df = frame_of(cols)                                          # (no frame source makes a half / bfloat16 column)
    with pytest.raises(tfs.InvalidTypeException, match="string"):
        df.withColumn("r", F.rank().over(Window.partitionBy("s").orderBy("t")))
    with pytest.raises(tfs.InvalidTypeException, match="string"):
        df.withColumn("r", F.rank().over(Window.partitionBy("id").orderBy("s")))
    with pytest.raises(tfs.InvalidTypeException, match="binary|string"):
        df.withColumn("r", F.min("q").over(Window.partitionBy("id", "s")))
    with pytest.raises(ValueError, match="at most 8"):
        df.withColumn("r", F.rank().over(Window.partitionBy("id", "g", "t", "q").orderBy("i", "x", "score", "t", "q")))
    with pytest.raises(ValueError, match="not found"):
        df.withColumn("r", F.rank().over(Window.partitionBy("nope").orderBy("t")))
    with pytest.raises(ValueError, match="not found"):
        df.withColumn("r", F.sum("nope").over(Window.partitionBy("id")))
    with pytest.raises(tfs.InvalidTypeException):
        df.withColumn("r", F.sum("s").over(Window.partitionBy("id")))
    with pytest.raises(TypeError, match="computed"):
        Window.partitionBy(df.x + 1)
    with pytest.raises(TypeError):
        F.sum("x").over("id")


# ------------------------------------------------------------------ ranking semantics
RANKS = [("rn", "row_number", None, "rows"), ("r", "rank", None, "rows"), ("d", "dense_rank", None, "rows")]


def rank_exprs(w):
    return [F.row_number().over(w).alias("rn"), F.rank().over(w).alias("r"), F.dense_rank().over(w).alias("d")]


def test_ties_the_three_ranking_functions_differ_as_spark_defines():
    cols = {"id": np.zeros(7, dtype=np.int32), "t": np.array([5, 5, 7, 7, 7, 9, 11], dtype=np.int32),
            "i": np.arange(7, dtype=np.int64)}
    out = frame_of(cols, 2).select("id", "t", "i", *rank_exprs(Window.partitionBy("id").orderBy("t")))
    assert out.to_numpy("rn").tolist() == [1, 2, 3, 4, 5, 6, 7]
    assert out.to_numpy("r").tolist() == [1, 1, 3, 3, 3, 6, 7]
    assert out.to_numpy("d").tolist() == [1, 1, 2, 2, 2, 3, 4]
    assert out.to_numpy("i").tolist() == list(range(7))         # ties keep the input's order


@pytest.mark.parametrize("order", [[("t", True)], [("t", False), ("score", True)], [("g", True), ("t", False)]])
def test_descending_and_mixed_directions(order):
    cols = base_columns(seed=1)
    df = frame_of(cols)
    w = Window.partitionBy("id").orderBy(*[tfs.desc(k) if d else tfs.col(k).asc() for k, d in order])
    out = df.select(*cols, *rank_exprs(w))
    perm, want = brute(cols, ["id"], order, RANKS)
    check(out, cols, perm, want, RANKS)


def test_nan_and_negative_zero_keys():
    n = 60
    rng = np.random.default_rng(2)
    k = rng.choice(np.array([0.0, -0.0, np.nan, 1.5, -np.inf, np.inf], dtype=np.float32), n)
    o = rng.choice(np.array([0.0, -0.0, np.nan, 2.0, -1.0]), n)
    cols = {"k": k, "o": o, "i": np.arange(n, dtype=np.int64)}
    out = frame_of(cols).select("k", "o", "i", *rank_exprs(Window.partitionBy("k").orderBy("o")),
                                F.count("*").over(Window.partitionBy("k").orderBy("o")).alias("c"))
    exprs = RANKS + [("c", "count", None, "range")]
    perm, want = brute(cols, ["k"], [("o", False)], exprs)
    got_i = out.to_numpy("i")
    assert got_i.tolist() == cols["i"][perm].tolist()
    for name, *_ in exprs:
        assert out.to_numpy(name).tolist() == want[name], name
    ks = out.to_numpy("k")
    assert np.isnan(ks[-1]) and not np.isnan(ks[0])                              # NaN is a group, sorted last
    zero = np.nonzero(ks == 0)[0]
    signs = np.signbit(ks[zero])
    assert signs.any() and not signs.all()                                       # -0.0 groups with 0.0 ...
    assert (out.to_numpy("rn")[zero] == 1).sum() == 1                            # ... in one group


def test_two_partition_keys():
    cols = base_columns(seed=3)
    w = Window.partitionBy("id", "g").orderBy("t")
    exprs = RANKS + [("s", "sum", "q", "range")]
    out = frame_of(cols).select(*cols, *rank_exprs(w), F.sum("q").over(w).alias("s"))
    perm, want = brute(cols, ["id", "g"], [("t", False)], exprs)
    check(out, cols, perm, want, exprs)


def test_computed_order_key():
    cols = base_columns(seed=4)
    df = frame_of(cols)
    out = df.withColumn("rn", F.row_number().over(Window.partitionBy("id").orderBy((-df.q).desc())))
    assert out.columns == list(cols) + ["rn"]
    perm, want = brute(cols, ["id"], [("q", False)], RANKS[:1])
    check(out, cols, perm, want, RANKS[:1])


# ------------------------------------------------------------------ frames
def value_column(dtype, n, seed):
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return (1e4 + rng.standard_normal(n)).astype(dt)
    ii = np.iinfo(dt)
    return rng.integers(max(ii.min, -1000), min(ii.max, 1000), n, dtype=dt, endpoint=True)


class HostPartition:
    """The host scan and finish of frame/window.py over one partition sorted
    by (id, t), shaped like a frame for `check`: exprs of column v only."""

    def __init__(self, cols, perm, exprs):
        from tensorframes_amd.frame import window as W
        self.columns = [name for name, *_ in exprs]
        v = torch.from_numpy(np.ascontiguousarray(cols["v"][perm]))
        words = np.stack([spec_words(cols["id"][perm]), spec_words(cols["t"][perm])], 0)
        kinds = ["group_head", "peer_head", "sum_i64" if v.dtype not in (torch.float32, torch.float64) else "sum_f64",
                 "sum_f64", "min_word", "max_word"]
        chan = {"sum": 2, "avg": 3, "min": 4, "max": 5, "count": 0}
        fwd, rev = W._host_scan(words, 1, kinds, [v] * 4)
        outs = W._host_finish(fwd, rev, kinds, [0] * 6, [0] * 6, False, False, 0, 0, [fn for _, fn, _, _ in exprs],
                              [fr for *_, fr in exprs], [chan[fn] for _, fn, _, _ in exprs], [v.dtype] * len(exprs))
        self.data = {name: o.numpy() for name, o in zip(self.columns, outs)}

    def to_numpy(self, name):
        return self.data[name]


@pytest.mark.parametrize("dtype", DTYPES)
def test_three_frames_for_every_aggregate_and_value_dtype(dtype):
    n = 120
    cols = base_columns(n=n, seed=5, nkeys=4)
    cols["v"] = value_column(dtype, n, 6)
    base = Window.partitionBy("id").orderBy("t")
    specs = {"rows": base.rowsBetween(UP, CR), "range": base.rangeBetween(UP, CR), "whole": base.rowsBetween(UP, UF)}
    exprs, items = [], []
    for frame, w in specs.items():
        for fn in ("sum", "count", "avg", "min", "max"):
            exprs.append((f"{fn}_{frame}", fn, "v", frame))
            items.append(getattr(F, fn)("v").over(w).alias(f"{fn}_{frame}"))
    perm, want = brute(cols, ["id"], [("t", False)], exprs)
    if np.dtype(dtype).itemsize * 8 in (8, 16) and np.dtype(dtype) != np.uint8:
        # no frame source makes an int8 / int16 column: these two dtypes meet
        # the host scan and finish where a sorted partition would
        out = HostPartition(cols, perm, exprs)
    else:
        out = frame_of(cols).select(*cols, *items)
    check(out, cols, perm, want, exprs, terms_all(n, 3))


def test_default_frames():
    cols = base_columns(seed=7)
    df = frame_of(cols)
    ordered, unordered = Window.partitionBy("id").orderBy("t"), Window.partitionBy("id")
    out = df.select(*cols, F.sum("q").over(ordered).alias("a"), F.sum("q").over(ordered.rangeBetween(UP, CR)).alias("b"))
    assert out.to_numpy("a").tolist() == out.to_numpy("b").tolist()
    out = df.select(*cols, F.sum("q").over(unordered).alias("a"), F.sum("q").over(unordered.rangeBetween(UP, UF)).alias("b"),
                    F.sum("q").over(unordered.rangeBetween(UP, CR)).alias("c"))
    exprs = [("a", "sum", "q", "whole"), ("b", "sum", "q", "whole"), ("c", "sum", "q", "whole")]
    perm, want = brute(cols, ["id"], [], exprs)
    check(out, cols, perm, want, exprs)


def test_int64_sums_wrap():
    n = 40
    cols = {"id": (np.arange(n) % 2).astype(np.int32), "t": np.arange(n, dtype=np.int32),
            "v": np.full(n, (1 << 62) + 12345, dtype=np.int64)}
    w = Window.partitionBy("id").orderBy("t")
    exprs = [("s", "sum", "v", "rows"), ("w", "sum", "v", "whole")]
    out = frame_of(cols, 3).select("id", "t", "v", F.sum("v").over(w.rowsBetween(UP, CR)).alias("s"),
                                   F.sum("v").over(w.rowsBetween(UP, UF)).alias("w"))
    perm, want = brute(cols, ["id"], [("t", False)], exprs)
    check(out, cols, perm, want, exprs)
    assert min(want["s"]) < 0 < max(want["s"])                   # it did wrap


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_float_sums_with_an_inf_and_a_nan_in_one_group(dtype):
    n = 30
    v = value_column(dtype, n, 8)
    v[7], v[19], v[22] = np.inf, np.nan, -np.inf                 # rows 7 and 19 in group 1, 22 in group 0
    cols = {"id": (np.arange(n) % 2).astype(np.int32), "t": np.arange(n, dtype=np.int32), "v": v}
    w = Window.partitionBy("id").orderBy("t")
    exprs = [("s", "sum", "v", "rows"), ("a", "avg", "v", "rows"), ("w", "sum", "v", "whole"),
             ("lo", "min", "v", "rows"), ("hi", "max", "v", "whole")]
    out = frame_of(cols, 3).select("id", "t", "v", F.sum("v").over(w.rowsBetween(UP, CR)).alias("s"),
                                   F.avg("v").over(w.rowsBetween(UP, CR)).alias("a"),
                                   F.sum("v").over(w.rowsBetween(UP, UF)).alias("w"),
                                   F.min("v").over(w.rowsBetween(UP, CR)).alias("lo"),
                                   F.max("v").over(w.rowsBetween(UP, UF)).alias("hi"))
    perm, want = brute(cols, ["id"], [("t", False)], exprs)
    check(out, cols, perm, want, exprs, terms_all(n, 3))
    s = out.to_numpy("s")[out.to_numpy("id") == 1]
    assert np.isfinite(s[0]) and np.isinf(s[5]) and np.isnan(s[-1])
    assert np.isnan(out.to_numpy("hi")[out.to_numpy("id") == 1]).all()            # NaN is the largest


# ------------------------------------------------------------------ schema and row order
def test_output_schema_names_and_dtypes():
    cols = base_columns()
    df = frame_of(cols, 4)
    w = Window.partitionBy("id").orderBy(tfs.desc("score"))
    out = df.withColumn("rn", F.row_number().over(w))
    assert out.columns == list(cols) + ["rn"] and out.num_partitions == 4
    assert dict(out.dtypes)["rn"] == "int"
    out = df.withColumn("t", F.count("*").over(w))                               # replaced in place
    assert out.columns == list(cols) and out.to_numpy("t").dtype == np.int64
    out = df.select("id", F.sum("score").over(w).alias("fs"), F.sum("q").over(w).alias("is"),
                    F.mean("q").over(w).alias("m"), F.min("score").over(w).alias("lo"), F.max("t").over(w).alias("hi"),
                    F.count("x").over(w).alias("c"), F.dense_rank().over(w).alias("d"))
    assert out.columns == ["id", "fs", "is", "m", "lo", "hi", "c", "d"]
    assert [out.to_numpy(c).dtype for c in out.columns[1:]] == \
        [np.float64, np.int64, np.float64, np.float32, np.int32, np.int64, np.int32]


def test_readme_example_top3_and_share():
    cols = base_columns(seed=9)
    scored = frame_of(cols, 3)
    w = Window.partitionBy("id").orderBy(tfs.desc("score"))
    top3 = scored.withColumn("rn", F.row_number().over(w)).filter(tfs.col("rn") <= 3)
    perm, want = brute(cols, ["id"], [("score", True)], RANKS[:1])
    keep = np.array(want["rn"]) <= 3
    assert top3.to_numpy("i").tolist() == cols["i"][perm][keep].tolist()
    both = scored.select("id", "score", F.rank().over(w).alias("r"), F.sum("score").over(w).alias("running"))
    assert both.columns == ["id", "score", "r", "running"]
    tot = scored.withColumn("total", F.sum("x").over(Window.partitionBy("id")))
    share = tot.withColumn("share", tot.x / tfs.col("total"))
    sums = {k: share.to_numpy("share")[share.to_numpy("id") == k].sum() for k in set(cols["id"].tolist())}
    assert all(abs(s - 1.0) < 1e-12 for s in sums.values())


def test_defined_row_order_is_stable():
    cols = base_columns(seed=10)
    out = frame_of(cols, 5).withColumn("rn", F.row_number().over(Window.partitionBy("g").orderBy("t")))
    want = sorted(range(len(cols["i"])), key=lambda i: (cols["g"][i], cols["t"][i], i))
    assert out.to_numpy("i").tolist() == want
    local = out.local_blocks()
    assert sorted(local) == list(range(5))
    assert [i for p in range(5) for i in local[p].columns["i"].tolist()] == want


# ------------------------------------------------------------------ partitioning
ALL = RANKS + [("c", "count", None, "range"), ("si", "sum", "q", "rows"), ("sw", "sum", "q", "whole"),
               ("lo", "min", "x", "range"), ("hi", "max", "score", "whole"), ("fs", "sum", "x", "rows"),
               ("fr", "sum", "score", "range"), ("fw", "sum", "x", "whole"), ("av", "avg", "score", "rows")]
EXACT = ["rn", "r", "d", "c", "si", "sw", "lo", "hi"]


def all_items(w):
    ws = {"rows": w.rowsBetween(UP, CR), "range": w.rangeBetween(UP, CR), "whole": w.rowsBetween(UP, UF)}
    items = rank_exprs(w)
    for name, fn, col, frame in ALL[3:]:
        items.append((F.count("*") if col is None else getattr(F, fn)(col)).over(ws[frame]).alias(name))
    return items


def uneven(cols, nparts, empty, one_row):
    """A frame of nparts partitions: partition `empty` loses all of its rows,
    `one_row` all but one (rows are dropped with filter). -> (frame, kept columns)"""
    n = len(cols["i"])
    edges = [(p * n) // nparts for p in range(nparts + 1)]
    keep = np.ones(n, dtype=bool)
    keep[edges[empty]:edges[empty + 1]] = False
    keep[edges[one_row] + 1:edges[one_row + 1]] = False
    df = tfs.from_columns(dict(cols, keep=keep.astype(np.int32)), num_partitions=nparts)
    df = df.filter(df.keep > 0).select(*cols)
    sizes = {p: b.nrows for p, b in df.local_blocks().items()}   # (this rank's partitions)
    assert sizes.get(empty, 0) == 0 and sizes.get(one_row, 1) == 1
    return df, {k: v[keep] for k, v in cols.items()}


def heavy_columns(n=210, seed=11):
    """One key owns more than half of the rows."""
    cols = base_columns(n=n, seed=seed)
    rng = np.random.default_rng(seed)
    cols["id"] = np.where(rng.random(n) < 0.6, 2, cols["id"]).astype(np.int32)
    cols["t"] = rng.integers(0, 40, n).astype(np.int32)
    return cols


_BRUTE = {}


def brute_all(tag, cols):
    if tag not in _BRUTE:
        _BRUTE[tag] = brute(cols, ["id"], [("t", False)], ALL)
    return _BRUTE[tag]


def run_all(df, cols):
    return df.select(*cols, *all_items(Window.partitionBy("id").orderBy("t")))


@pytest.mark.parametrize("nparts", [1, 3, 7])
def test_same_frame_in_1_3_7_partitions(nparts):
    cols = base_columns(seed=12)
    out = run_all(frame_of(cols, nparts), cols)
    assert out.num_partitions == nparts
    perm, want = brute_all("base", cols)
    check(out, cols, perm, want, ALL, terms_all(len(cols["i"]), nparts))


def test_seven_partitions_with_an_empty_and_a_one_row_partition():
    df, cols = uneven(base_columns(seed=13), 7, empty=3, one_row=5)
    out = run_all(df, cols)
    perm, want = brute(cols, ["id"], [("t", False)], ALL)
    check(out, cols, perm, want, ALL, terms_all(len(cols["i"]), 7))


def test_a_group_spans_at_least_three_partitions():
    cols = heavy_columns()
    out = run_all(frame_of(cols, 7), cols)
    perm, want = brute_all("heavy", cols)
    check(out, cols, perm, want, ALL, terms_all(len(cols["i"]), 7))
    ids = [set(b.columns["id"].tolist()) for _, b in sorted(out.local_blocks().items())]
    assert sum(2 in s for s in ids) >= 3                                         # it does span them
    sizes = [b.nrows for _, b in sorted(out.local_blocks().items())]
    assert max(sizes) <= 2 * len(cols["i"]) // 7                                 # and the partitions stay balanced


def test_integer_valued_outputs_do_not_depend_on_the_partitioning():
    cols = heavy_columns()
    outs = [run_all(frame_of(cols, p), cols) for p in (1, 3, 7)]
    for name in EXACT + ["i"]:
        first = outs[0].to_numpy(name).tobytes()
        assert all(o.to_numpy(name).tobytes() == first for o in outs[1:]), name


def test_same_bits_from_run_to_run():
    cols = heavy_columns()
    a, b = run_all(frame_of(cols, 7), cols), run_all(frame_of(cols, 7), cols)
    for name, *_ in ALL:
        assert a.to_numpy(name).tobytes() == b.to_numpy(name).tobytes(), name


# ------------------------------------------------------------------ misc
def test_order_without_partition_keys_is_a_global_running_sum():
    cols = base_columns(seed=14)
    df = frame_of(cols, 4)
    out = df.withColumn("cum", F.sum("x").over(Window.orderBy("t").rowsBetween(UP, CR))) \
            .withColumn("ci", F.sum("q").over(Window.orderBy("t").rowsBetween(UP, CR)))
    exprs = [("cum", "sum", "x", "rows"), ("ci", "sum", "q", "rows")]
    perm, want = brute(cols, [], [("t", False)], exprs)
    check(out, cols, perm, want, exprs, terms_all(len(cols["i"]), 4))
    assert len([b for b in out.local_blocks().values() if b.nrows]) >= 3


def test_no_keys_at_all_is_the_whole_frame():
    cols = base_columns(seed=15)
    out = frame_of(cols, 3).withColumn("n", F.count("*").over(Window.partitionBy())) \
                           .withColumn("s", F.sum("q").over(Window.partitionBy()))
    assert out.to_numpy("i").tolist() == cols["i"].tolist()
    assert set(out.to_numpy("n").tolist()) == {len(cols["i"])}
    assert set(out.to_numpy("s").tolist()) == {int(cols["q"].sum())}


def test_expressions_over_one_spec_sort_once():
    cols = base_columns(seed=16)
    df = frame_of(cols, 3).cache()
    df.count()
    before = tfs.metrics.snapshot().get("sort_rows", 0)
    df.orderBy("id", "t").count()
    one_sort = tfs.metrics.snapshot().get("sort_rows", 0) - before
    assert one_sort > 0
    before = tfs.metrics.snapshot().get("sort_rows", 0)
    rows0 = tfs.metrics.snapshot().get("window_rows", 0)
    w = Window.partitionBy("id").orderBy("t")
    df.select("id", F.row_number().over(w).alias("rn"), F.rank().over(w).alias("r"),
              F.sum("x").over(w.rowsBetween(UP, CR)).alias("s"), F.max("q").over(w.rowsBetween(UP, UF)).alias("m")).count()
    assert tfs.metrics.snapshot().get("sort_rows", 0) - before == one_sort
    assert tfs.metrics.snapshot().get("window_rows", 0) - rows0 == len(cols["i"])
    assert tfs.metrics.snapshot().get("window_scan_passes", 0) > 0
    # two different specs: one after the other, two sorts
    before = tfs.metrics.snapshot().get("sort_rows", 0)
    df.select("id", F.row_number().over(w).alias("rn"),
              F.row_number().over(Window.partitionBy("id").orderBy(tfs.desc("t"))).alias("rd")).count()
    assert tfs.metrics.snapshot().get("sort_rows", 0) - before == 2 * one_sort


# ------------------------------------------------------------------ ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _bytes_of(out, names):
    return {c: out.to_numpy(c).tobytes().hex() for c in names}


def _spmd_results():
    cols = heavy_columns(n=180, seed=17)
    df, kept = uneven(cols, 5, empty=1, one_row=3)
    out = run_all(df, kept)
    res = {"all": _bytes_of(out, list(kept) + [n for n, *_ in ALL])}
    g = df.withColumn("cum", F.sum("x").over(Window.orderBy("t", "i").rowsBetween(UP, CR)))
    res["global"] = _bytes_of(g, ["i", "cum"])
    return res


def _worker(rank, world, port, outdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), OMP_NUM_THREADS="1", TFA_SHM_COLLECTIVES="1", TFA_DEVICE="cpu")
    torch.set_num_threads(1)
    sys.path.insert(0, REPO)
    from tensorframes_amd.parallel import dist

    assert dist.init(backend="gloo")
    res = _spmd_results()
    with open(os.path.join(outdir, f"r{rank}.json"), "w") as f:
        json.dump(res, f)
    dist.shutdown()


def test_world_two_gives_the_bytes_of_world_one(tmp_path):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    outs = [json.load(open(tmp_path / f"r{r}.json")) for r in range(2)]
    single = _spmd_results()
    assert outs[0] == single and outs[1] == single
