"""median / percentile / percentile_approx / mode / countDistinct in
`groupBy().agg` and `DataFrame.agg` on host frames (frame/order_agg.py): the
API with its typed errors, the values, and that no output bit depends on the
partitioning or the number of ranks.

Expected values come from tests/order_agg_cases.py: plain Python over the
collected rows. The host path and the specification perform the same IEEE
operations (one rounded product for a rank or a position, two rounded products
and one rounded sum for the interpolation), so everything is compared bit for
bit.

`percentile` is also held against the exact interpolation in
`fractions.Fraction`, to a relative 3 * 2^-53 on positive data: for the dyadic
p in (0.25, 0.5, 0.75) and N < 2^53 the position and both weights are exact,
which leaves the two rounded products and the rounded sum. `np.percentile` is
a sanity check with numpy's own three roundings on top: 6 * 2^-53."""
import json
import os
import socket
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import order_agg_cases as oc
import tensorframes_amd as tfs
from tensorframes_amd import InvalidDimensionException, InvalidTypeException, functions as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUE_DTYPES = [np.int32, np.int64, np.float32, np.float64]
PS = [0.0, 0.1, 0.25, 0.5, 0.75, 1.0]

# (output name, fn, value columns, percentages, is_list) as order_agg_cases.spec takes them
CASES = [("med", "percentile", ("x",), [0.5], False),
         ("pct", "percentile", ("x",), PS, True),
         ("apx", "percentile_approx", ("x",), [0.3], False),
         ("apxs", "percentile_approx", ("x",), PS, True),
         ("mode", "mode", ("x",), [], False),
         ("dx", "count_distinct", ("x",), [], False),
         ("dxy", "count_distinct", ("y", "x"), [], False)]


def expressions():
    return [F.median("x").alias("med"), F.percentile("x", PS).alias("pct"),
            F.percentile_approx("x", 0.3).alias("apx"), F.percentile_approx("x", PS, 100).alias("apxs"),
            F.mode("x").alias("mode"), F.countDistinct("x").alias("dx"), F.countDistinct("y", "x").alias("dxy")]


def columns(n=160, seed=3, vdtype=np.float32, kdtype=np.int32, heavy=False):
    rng = np.random.default_rng(seed)
    ids = rng.integers(-3, 5, n)
    if heavy:
        ids = np.where(rng.random(n) < 0.6, 2, ids)     # one key holds 60 % of the rows
    ids[n - 1] = 77                                      # a group of one row
    x = rng.integers(-6, 7, n) if np.dtype(vdtype).kind == "i" else np.round(rng.standard_normal(n) * 3, 0) / 2
    return {"id": ids.astype(kdtype), "x": x.astype(vdtype), "y": rng.integers(0, 3, n).astype(np.int32),
            "i": np.arange(n, dtype=np.int64)}


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


def frame(cols, nparts):
    if nparts == 1:
        return tfs.from_columns(cols, num_partitions=1), cols
    return uneven(cols, nparts, empty=1, one_row=2)


def check(out, cols, keys, cases):
    """Every column of `out` against the specification, bit for bit."""
    order, want = oc.spec(cols, keys, cases)
    for j, k in enumerate(keys):
        got = [int(w) for w in oc.spec_words(out.to_numpy(k))]
        assert got == [g[j] for g in order], k                   # one row per group, ascending
    for name, *_ in cases:
        got = out.to_numpy(name)
        assert got.dtype == want[name].dtype and got.shape == want[name].shape, name
        assert got.tobytes() == want[name].tobytes(), (name, got, want[name])


def bits(out):
    return {c: out.to_numpy(c).tobytes().hex() for c in out.columns}


# ------------------------------------------------------------------ API and typed errors
def test_exports_names_dtypes_and_alias():
    for name in ("OrderAggregateExpression", "median", "percentile", "percentile_approx", "mode", "countDistinct",
                 "count_distinct", "approx_count_distinct"):
        assert name in F.__all__ and hasattr(F, name), name
    assert F.count_distinct is F.countDistinct
    assert all(isinstance(e, F.OrderAggregateExpression) for e in expressions())
    cols = {"id": np.array([1, 1, 2], dtype=np.int32), "x": np.array([1.5, 2.5, 4.0], dtype=np.float32),
            "y": np.array([7, 7, 9], dtype=np.int64)}
    out = tfs.from_columns(cols).groupBy("id").agg(
        F.median("x"), F.percentile(tfs.col("x"), 0.5), F.percentile("x", [0.25, 0.75]), F.percentile_approx("x", 0.5),
        F.percentile_approx("x", (0.5,), 7), F.mode("x"), F.countDistinct("x"), F.countDistinct("x", "y"),
        F.approx_count_distinct("y"), F.mode("y").alias("my"), F.median("y").name("medy"))
    assert out.columns == ["id", "median(x)", "percentile(x, 0.5)", "percentile(x, array(0.25, 0.75))",
                           "percentile_approx(x, 0.5, 10000)", "percentile_approx(x, array(0.5), 7)", "mode(x)",
                           "count(DISTINCT x)", "count(DISTINCT x, y)", "approx_count_distinct(y)", "my", "medy"]
    got = {c: out.to_numpy(c) for c in out.columns}
    assert [got[c].dtype for c in out.columns] == [np.int32, np.float64, np.float64, np.float64, np.float32,
                                                   np.float32, np.float32, np.int64, np.int64, np.int64, np.int64,
                                                   np.float64]
    assert got["percentile(x, array(0.25, 0.75))"].shape == (2, 2)
    assert got["percentile_approx(x, array(0.5), 7)"].shape == (2, 1)
    assert got["median(x)"].tolist() == [2.0, 4.0] and got["percentile_approx(x, 0.5, 10000)"].tolist() == [1.5, 4.0]
    assert got["my"].tolist() == [7, 9] and got["medy"].tolist() == [7.0, 9.0]
    assert got["count(DISTINCT x)"].tolist() == [2, 1] and got["approx_count_distinct(y)"].tolist() == [1, 1]
    assert "median(x)" in repr(F.median("x"))


def test_refusals():
    n = 6
    df = tfs.from_columns({"k": np.arange(n, dtype=np.int32), "s": np.array([f"s{i}" for i in range(n)]),
                           "v": np.zeros((n, 3)), "x": np.arange(n, dtype=np.float64)})
    g = df.groupBy("k")
    w = tfs.Window.partitionBy("k")
    for e in (F.median("x"), F.percentile("x", 0.5), F.percentile_approx("x", 0.5), F.mode("x"),
              F.countDistinct("x"), F.approx_count_distinct("x")):
        with pytest.raises(NotImplementedError, match="over a window"):
            e.over(w)
        with pytest.raises(TypeError):
            df.filter(e)
        with pytest.raises(TypeError):
            df.orderBy(e)
        with pytest.raises((TypeError, ValueError)):           # (as select refuses F.avg("x"))
            df.select(e)
    for fn in (F.median, F.mode, F.countDistinct, F.approx_count_distinct, lambda c: F.percentile(c, 0.5),
               lambda c: F.percentile_approx(c, 0.5)):
        with pytest.raises(InvalidTypeException, match="string"):
            g.agg(fn("s"))
        with pytest.raises(InvalidDimensionException, match="scalar"):
            g.agg(fn("v"))
        with pytest.raises(ValueError, match="nope"):
            g.agg(fn("nope"))
        with pytest.raises(TypeError, match="computed"):
            fn(tfs.col("x") + 1)
    rows = tfs.create_dataframe([(True, 1, 1.0), (False, 2, 2.0), (True, 1, 4.5)], ["b", "k", "x"])
    with pytest.raises(InvalidTypeException, match="bool"):
        rows.groupBy("k").agg(F.median("b"))
    with pytest.raises(InvalidTypeException, match="string"):
        df.groupBy("s").agg(F.median("x"))                       # the keys follow groupBy().agg
    for fn in (F.percentile, F.percentile_approx):
        for bad in (-0.1, 1.5, float("nan"), [0.5, 2.0]):
            with pytest.raises(ValueError, match=r"\[0, 1\]"):
                fn("x", bad)
        with pytest.raises(ValueError, match="1..16"):
            fn("x", [])
        with pytest.raises(ValueError, match="1..16"):
            fn("x", [0.5] * 17)
        with pytest.raises(TypeError):
            fn("x", "half")
        assert len(fn("x", [0.5] * 16).percentages) == 16
    for bad in (0, -5):
        with pytest.raises(ValueError, match="accuracy"):
            F.percentile_approx("x", 0.5, bad)
    with pytest.raises(TypeError, match="accuracy"):
        F.percentile_approx("x", 0.5, 10.5)
    for bad in (0, -0.05, float("nan")):
        with pytest.raises(ValueError, match="rsd"):
            F.approx_count_distinct("x", bad)
    # group keys + value columns must fit the 8 sort words
    wide = tfs.from_columns({f"c{j}": np.arange(4, dtype=np.int32) for j in range(10)})
    with pytest.raises(ValueError, match=r"7 group keys and 2 value\s+columns, 9 sort words"):
        wide.groupBy(*[f"c{j}" for j in range(7)]).agg(F.countDistinct("c7", "c8"))
    assert wide.groupBy(*[f"c{j}" for j in range(7)]).agg(F.median("c7")).count() == 4
    with pytest.raises(ValueError, match="appears twice"):
        g.agg(F.median("x"), F.percentile("x", 0.5).alias("median(x)"))
    with pytest.raises(ValueError, match="appears twice"):
        g.agg(F.avg("x").alias("k"), F.median("x"))
    # the dict form is not extended
    with pytest.raises(ValueError, match="median"):
        g.agg({"x": "median"})
    with pytest.raises(ValueError, match="not an aggregate function"):
        g.agg({"x": "mode"})
    assert "median" not in F.FUNCTIONS and "mode" not in F.FUNCTIONS
    for absent in ("lag", "lead", "ntile", "percent_rank", "cume_dist"):
        assert not hasattr(F, absent)


# ------------------------------------------------------------------ values
@pytest.mark.parametrize("vdtype", VALUE_DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("nparts", [1, 3, 7])
def test_values_int_keys(nparts, vdtype):
    df, cols = frame(columns(vdtype=vdtype, heavy=(nparts == 7)), nparts)
    out = df.groupBy("id").agg(*expressions())
    assert out.num_partitions == nparts
    check(out, cols, ["id"], CASES)


@pytest.mark.parametrize("nparts", [1, 3, 7])
def test_values_float_keys_and_two_keys(nparts):
    cols = columns(vdtype=np.float64, kdtype=np.float32, seed=5)
    cols["id"][:9] = [np.nan, -0.0, 0.0, np.nan, np.inf, -np.inf, 0.0, -0.0, np.nan]
    df, kept = frame(cols, nparts)
    check(df.groupBy("id").agg(*expressions()), kept, ["id"], CASES)
    check(df.groupBy("y", "id").agg(*expressions()[:6]), kept, ["y", "id"], CASES[:6])


@pytest.mark.parametrize("vdtype", VALUE_DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("nparts", [1, 3, 7])
def test_values_no_keys(nparts, vdtype):
    df, cols = frame(columns(vdtype=vdtype, seed=9), nparts)
    out = df.agg(*expressions())
    assert out.num_partitions == 1 and out.count() == 1
    check(out, cols, [], CASES)


def test_percentile_against_exact_fractions_and_numpy():
    rng = np.random.default_rng(21)
    n = 400
    cols = {"id": rng.integers(0, 6, n).astype(np.int32), "x": 1e4 + rng.standard_normal(n)}
    ps = [0.25, 0.5, 0.75]
    out = tfs.from_columns(cols, num_partitions=3).groupBy("id").agg(F.percentile("x", ps).alias("p"))
    ids, got = out.to_numpy("id"), out.to_numpy("p")
    eps = 2.0 ** -53
    for g, row in zip(ids.tolist(), got):
        v = np.sort(cols["x"][cols["id"] == g])
        for p, have in zip(ps, row.tolist()):
            pos = Fraction(p) * (len(v) - 1)
            lo, hi = pos.numerator // pos.denominator, -((-pos.numerator) // pos.denominator)
            exact = Fraction(float(v[lo])) if lo == hi else (hi - pos) * Fraction(float(v[lo])) + \
                (pos - lo) * Fraction(float(v[hi]))
            assert abs(Fraction(have) - exact) <= 3 * eps * abs(exact), (g, p, have, float(exact))
            assert abs(have - np.percentile(v, 100 * p)) <= 6 * eps * abs(have), (g, p)


def test_special_values():
    nan, inf = np.nan, np.inf
    groups = {1: [nan, 1.0, nan, 2.0, nan],            # NaNs count, sort last, and are one value
              2: [-inf, inf, 1.0, -inf],               # inf - inf cases are the formula's
              3: [-0.0, 0.0, 0.0, -0.0, 1.0],          # one value, decoded as +0.0
              4: [2.5, 2.5, 2.5, 2.5],                 # all equal
              5: [inf, inf],
              6: [-inf, inf],
              7: [nan],
              8: [3.0, 1.0, 3.0, 1.0, 2.0]}            # two longest runs: the smaller value wins
    for dt in (np.float32, np.float64):
        cols = {"id": np.concatenate([[g] * len(v) for g, v in groups.items()]).astype(np.int32),
                "x": np.concatenate(list(groups.values())).astype(dt)}
        cols["y"] = np.zeros(len(cols["x"]), dtype=np.int32)
        for nparts in (1, 4):
            out = tfs.from_columns(cols, num_partitions=nparts).groupBy("id").agg(*expressions())
            check(out, cols, ["id"], CASES)
        got = {c: out.to_numpy(c) for c in out.columns}
        assert got["dx"].tolist() == [3, 3, 2, 1, 1, 2, 1, 3]
        assert got["mode"][:4].tobytes() == np.array([nan, -inf, 0.0, 2.5], dtype=dt).tobytes()
        assert got["mode"][7] == 1.0
        assert np.isnan(got["med"][0]) and got["med"][2] == 0.0 and not np.signbit(got["med"][2])
        assert np.isnan(got["med"][5])                             # 0.5 * -inf + 0.5 * inf
        assert got["med"][4] == inf and np.isnan(got["med"][6])


def test_boundary_groups_and_spanning_bits():
    cols = columns(n=200, vdtype=np.float64, heavy=True, seed=13)
    exprs = [F.percentile("x", [0.0, 1.0]).alias("ends"), F.percentile_approx("x", [0.0, 1.0]).alias("aends")] + \
        expressions()
    one = tfs.from_columns(cols, num_partitions=1).groupBy("id").agg(*exprs)
    ids = one.to_numpy("id").tolist()
    ends, aends = one.to_numpy("ends"), one.to_numpy("aends")
    for j, g in enumerate(ids):
        v = cols["x"][cols["id"] == g]
        assert ends[j].tolist() == [v.min(), v.max()] and aends[j].tolist() == [v.min(), v.max()]
    j = ids.index(77)                                            # a group of one row
    v = float(cols["x"][cols["id"] == 77][0])
    assert one.to_numpy("med")[j] == v and one.to_numpy("pct")[j].tolist() == [v] * len(PS)
    assert one.to_numpy("dx")[j] == 1 and one.to_numpy("mode")[j] == v
    # the heavy key spans at least three partitions of the sorted frame
    many = tfs.from_columns(cols, num_partitions=7)
    srt = many.select("id", "x").orderBy("id", "x")
    holds = [p for p, b in sorted(srt.local_blocks().items()) if b.nrows and (b.columns["id"] == 2).any()]
    assert len(holds) >= 3
    out = many.groupBy("id").agg(*exprs)
    assert bits(out) == bits(one)
    # its row sits in the partition that holds the group's first sorted row
    where = [p for p, b in sorted(out.local_blocks().items()) if b.nrows and (b.columns["id"] == 2).any()]
    assert where == holds[:1]
    check(out, cols, ["id"], CASES)


@pytest.mark.parametrize("keys", [["id"], []], ids=["keyed", "whole"])
def test_same_bits_for_every_partitioning(keys):
    cols = columns(n=230, vdtype=np.float32, heavy=True, seed=8)
    outs = []
    for nparts in (1, 3, 7):
        df = tfs.from_columns(cols, num_partitions=nparts)
        outs.append(bits(df.groupBy(*keys).agg(*expressions()) if keys else df.agg(*expressions())))
    assert outs[0] == outs[1] == outs[2]


def test_mixed_with_moment_aggregates_and_result_order():
    df, cols = frame(columns(vdtype=np.float32, heavy=True, seed=6), 7)
    mixed = df.groupBy("id").agg(F.avg("x"), F.median("x").alias("med"), F.count("*"), F.countDistinct("y", "x"),
                                 F.max("x"), F.mode("x"))
    assert mixed.columns == ["id", "avg(x)", "med", "count(1)", "count(DISTINCT y, x)", "max(x)", "mode(x)"]
    a = df.groupBy("id").agg(F.avg("x"), F.count("*"), F.max("x"))
    b = df.groupBy("id").agg(F.median("x").alias("med"), F.countDistinct("y", "x"), F.mode("x"))
    ids = b.to_numpy("id")
    assert ids.tolist() == sorted(set(cols["id"].tolist()))       # only order aggregates: ascending keys
    assert b.num_partitions == 7
    at = {k: j for j, k in enumerate(mixed.to_numpy("id").tolist())}
    assert sorted(at) == ids.tolist()
    for src in (a, b):
        sel = [at[k] for k in src.to_numpy("id").tolist()]
        for c in src.columns[1:]:
            assert mixed.to_numpy(c)[sel].tobytes() == src.to_numpy(c).tobytes(), c
    # no keys: one row, the columns side by side in call order
    whole = df.agg(F.avg("x"), F.median("x"), F.count("*"), F.approx_count_distinct("id"))
    assert whole.columns == ["avg(x)", "median(x)", "count(1)", "approx_count_distinct(id)"] and whole.count() == 1
    assert whole.to_numpy("avg(x)").tobytes() == df.agg(F.avg("x")).to_numpy("avg(x)").tobytes()
    assert whole.to_numpy("median(x)").tobytes() == df.agg(F.median("x")).to_numpy("median(x)").tobytes()
    assert whole.to_numpy("count(1)").tolist() == [len(cols["i"])]
    assert whole.to_numpy("approx_count_distinct(id)").tolist() == [len(set(cols["id"].tolist()))]


def test_one_sort_per_value_tuple_and_metrics():
    cols = columns(seed=2)
    df = tfs.from_columns(cols, num_partitions=3)
    before = tfs.metrics.snapshot()
    df.groupBy("id").agg(F.median("x"), F.mode("x"), F.percentile_approx("x", 0.5), F.countDistinct("x")).count()
    mid = tfs.metrics.snapshot()
    assert mid.get("order_agg_sorts", 0) - before.get("order_agg_sorts", 0) == 1
    assert mid.get("order_agg_rows", 0) - before.get("order_agg_rows", 0) == len(cols["i"])
    assert mid.get("order_agg_host_partitions", 0) - before.get("order_agg_host_partitions", 0) == 3
    df.groupBy("id").agg(F.median("x"), F.countDistinct("x", "y")).count()
    assert tfs.metrics.snapshot().get("order_agg_sorts", 0) - mid.get("order_agg_sorts", 0) == 2


def test_fold_refuses_equal_tuples_across_partitions():
    from tensorframes_amd.frame.order_agg import _fold
    W, P = 2, 1
    rec = lambda n, single, fw, lw, first, last: [n, single] + fw + lw + first + last  # noqa: E731
    ok = np.array([rec(3, 1, [5, 1], [5, 2], [3, 2, 2, 1], [3, 2, 2, 1]),
                   rec(0, 0, [0, 0], [0, 0], [0] * 4, [0] * 4),
                   rec(4, 0, [5, 3], [6, 9], [2, 1, 2, 3], [2, 2, 1, 8])], dtype=np.int64)
    continues, spans = _fold(ok, W, P)
    assert continues == [False, False, True] and len(spans) == 1
    assert spans[0]["pieces"] == [(0, 0, 3), (2, 0, 2)] and spans[0]["rows"] == 5 and spans[0]["distinct"] == 3
    assert spans[0]["mode_len"] == 2 and spans[0]["mode_word"] == 1   # a tie: the earlier piece
    bad = ok.copy()
    bad[2, 2:4] = [5, 2]                                         # the first tuple of partition 2 = the last of 0
    with pytest.raises(RuntimeError, match="equal"):
        _fold(bad, W, P)


# ------------------------------------------------------------------ ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _spmd_results():
    df, _ = uneven(columns(n=180, vdtype=np.float32, heavy=True, seed=17), 5, empty=1, one_row=3)
    res = {"keyed": bits(df.groupBy("id").agg(*expressions())),
           "whole": bits(df.agg(*expressions())),
           "mixed": bits(df.groupBy("id").agg(F.avg("y"), F.median("x"), F.countDistinct("y")).orderBy("id"))}
    return res


def _worker(rank, world, port, outdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), OMP_NUM_THREADS="1", TFA_SHM_COLLECTIVES="1", TFA_DEVICE="cpu")
    torch.set_num_threads(1)
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
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
