"""`groupBy(...).pivot(...).agg(...)` and `df.stat.crosstab` on the host path (the
CPU oracle of the device path), also under gloo SPMD.

Expected cells are written here, never taken from the package: a dict keyed by
(key tuple, pivot value) over the input rows, the statistics by their textbook
two-pass formulas. The inputs are small integers and multiples of 0.25, so
every sum is exact in float64: count, sum, min and max are compared exactly,
the quotients within the bound that `stat` works out.
A second check holds every cell to the bits of `groupBy(keys, p).agg(...)` on
the same frame and partitioning, and every other cell to the documented fill
(0 where the output is int64, NaN where it is floating)."""
import json
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import tensorframes_amd as tfs
from tensorframes_amd import functions as F
from tensorframes_amd.frame.window import Window

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def columns(n=240, seed=1):
    rng = np.random.default_rng(seed)
    k, p = rng.integers(-2, 4, n), rng.integers(0, 5, n)
    p = np.where((k + p) % 4 == 0, (p + 1) % 5, p)                      # no key has all five values
    return {"k": k.astype(np.int32),
            "d": rng.integers(0, 3, n).astype(np.int64),
            "p": p.astype(np.int32),
            "i": rng.integers(-9, 10, n).astype(np.int64),
            "x": (rng.integers(-8, 9, n) * 0.25).astype(np.float32),
            "y": rng.integers(-8, 9, n) * 0.25}


def frame(cols, nparts):
    return tfs.from_columns(cols, num_partitions=nparts)


def rows_of(df, keys):
    """{key tuple: {column: numpy scalar}} of a result frame."""
    got = {c: df.to_numpy(c) for c in df.columns}
    n = len(got[df.columns[0]]) if df.columns else 0
    out = {}
    for r in range(n):
        key = tuple(got[k][r].item() for k in keys)
        assert key not in out
        out[key] = {c: got[c][r] for c in df.columns if c not in keys}
    return out


# ------------------------------------------------------------------ the specification
def cells_of(cols, keys, p):
    """{(key tuple, pivot value): row indices}, by a plain loop."""
    out = {}
    for r in range(len(cols[p])):
        out.setdefault((tuple(cols[k][r].item() for k in keys), cols[p][r].item()), []).append(r)
    return out


T = 1e-13  # see stat()


def stat(fn, cols, rows, a, b=None):
    """(the statistic of the rows, the absolute error allowed).

    count, sum, min and max of these inputs are exact in float64: the bound is
    0. The sums behind a mean, an M2 and a co-moment are exact too, but a
    quotient by n is not, and the package merges per-partition means and M2s
    with Chan's formula: some tens of float64 roundings (2^-53 each), every one
    relative to a quantity no larger than max|x| (a mean), n (2 max|x|)^2 (an
    M2) or n (2 max|x|)(2 max|y|) (a co-moment). T = 1e-13 of those scales is
    about a thousand roundings, and seven orders of magnitude below the
    change a misplaced row makes (0.25 / n). stddev is compared through its
    square, corr by first-order propagation of the three errors."""
    v = [float(cols[a][r]) for r in rows]
    n = len(v)
    if fn == "count":
        return n, 0.0
    if fn == "sum":
        return (sum(int(cols[a][r]) for r in rows) if cols[a].dtype.kind == "i" else math.fsum(v)), 0.0
    if fn == "min":
        return min(v), 0.0
    if fn == "max":
        return max(v), 0.0
    top = max(abs(t) for t in v)
    if fn == "avg":
        return math.fsum(v) / n, T * top
    mean = math.fsum(v) / n
    m2 = math.fsum((t - mean) ** 2 for t in v)
    if fn == "stddev_samp":  # (the variance: the caller squares the cell)
        return (m2 / (n - 1), T * 8 * top * top) if n >= 2 else (math.nan, 0.0)
    if fn == "var_pop":
        return m2 / n, T * 4 * top * top
    assert fn == "corr"
    w = [float(cols[b][r]) for r in rows]
    wtop = max(abs(t) for t in w)
    mw = math.fsum(w) / n
    m2w = math.fsum((t - mw) ** 2 for t in w)
    c = math.fsum((s - mean) * (t - mw) for s, t in zip(v, w))
    if not (m2 > 0 and m2w > 0):
        return math.nan, 0.0
    r = c / math.sqrt(m2 * m2w)
    return r, T * 4 * n * (top * wtop / math.sqrt(m2 * m2w) + abs(r) * (top * top / m2 + wtop * wtop / m2w) / 2)


EXPRS = [("count", None, None, F.count("*")), ("sum", "i", None, F.sum("i")), ("sum", "x", None, F.sum("x")),
         ("avg", "y", None, F.avg("y")), ("min", "x", None, F.min("x")), ("max", "y", None, F.max("y")),
         ("stddev_samp", "y", None, F.stddev_samp("y")), ("var_pop", "x", None, F.var_pop("x")),
         ("corr", "x", "y", F.corr("x", "y"))]


@pytest.mark.parametrize("nparts", [1, 2, 5])
@pytest.mark.parametrize("keys", [["k"], ["k", "d"], []])
def test_every_cell_is_the_statistic_of_its_rows(keys, nparts):
    cols = columns()
    df = frame(cols, nparts)
    out = df.groupBy(*keys).pivot("p").agg(*[e[3] for e in EXPRS])
    values = sorted(set(cols["p"].tolist()))
    names = [f"{v}_{e[3].output_name}" for v in values for e in EXPRS]
    assert out.columns == keys + names
    cells = cells_of(cols, keys, "p")
    got = rows_of(out, keys)
    assert sorted(got) == sorted({k for k, _ in cells})
    checked = fills = 0
    for key, row in got.items():
        for v in values:
            rows = cells.get((key, v))
            for fn, a, b, e in EXPRS:
                cell = row[f"{v}_{e.output_name}"]
                if rows is None:
                    fills += 1
                    if fn == "count" or (fn == "sum" and a == "i"):
                        assert cell.dtype == np.int64 and cell == 0
                    else:
                        assert cell.dtype.kind == "f" and np.isnan(cell)
                    continue
                want, bound = stat(fn, cols, rows, a if a is not None else "i", b)
                checked += 1
                got_value = float(cell) ** 2 if fn == "stddev_samp" else float(cell)
                if isinstance(want, float) and math.isnan(want):
                    assert np.isnan(cell), (key, v, fn)
                else:
                    assert float(cell) >= 0 or fn != "stddev_samp"
                    assert abs(got_value - want) <= bound, (key, v, fn, cell, want, bound)
    assert checked and (fills or not keys)
    assert out.schema["0_count(1)"].dataType == tfs.LongType() and out.schema["0_sum(i)"].dataType == tfs.LongType()
    assert out.schema["0_min(x)"].dataType == tfs.FloatType() and out.schema["0_max(y)"].dataType == tfs.DoubleType()
    assert out.schema["0_sum(x)"].dataType == tfs.DoubleType()


@pytest.mark.parametrize("nparts", [1, 3])
@pytest.mark.parametrize("keys", [["k"], ["d", "k"], []])
def test_cells_have_the_bits_of_the_composite_key_agg(keys, nparts):
    cols = columns(seed=2)
    cols["p"] = np.array([0.5, -0.0, np.nan, -1.25, 0.0, 3.0], dtype=np.float64)[np.arange(len(cols["k"])) % 6]
    cols["p"][cols["k"] == 3] = 3.0                                     # a key that has one value only
    df = frame(cols, nparts)
    exprs = [e[3] for e in EXPRS]
    listed = [3.0, np.nan, 7.5, 0.0, -1.25]                              # 0.5 is not listed, 7.5 has no rows
    out = df.groupBy(*keys).pivot("p", listed).agg(*exprs)
    long = df.groupBy(*keys, "p").agg(*exprs)
    want = rows_of(long, keys + ["p"])
    want = {tuple("nan" if isinstance(t, float) and math.isnan(t) else t for t in k): v for k, v in want.items()}
    got = rows_of(out, keys)
    assert sorted(got) == sorted({k[:-1] for k in want})
    texts = ["3.0", "NaN", "7.5", "0.0", "-1.25"]
    hits = 0
    for key, row in got.items():
        for v, t in zip(listed, texts):
            cell = want.get(key + (("nan" if math.isnan(v) else v),))
            for e in exprs:
                g = row[f"{t}_{e.output_name}"]
                if cell is not None:
                    hits += 1
                    w = cell[e.output_name]
                else:
                    w = np.zeros((), np.int64) if g.dtype == np.int64 else np.array(np.nan, dtype=g.dtype)
                assert g.dtype == w.dtype
                np.testing.assert_array_equal(np.asarray(g).view(f"u{g.dtype.itemsize}"),
                                              np.asarray(w).view(f"u{w.dtype.itemsize}"), err_msg=f"{key} {t} {e}")
    assert hits
    assert all(np.all(out.to_numpy(f"7.5_{e.output_name}") == 0) or np.all(np.isnan(out.to_numpy(f"7.5_{e.output_name}")))
               for e in exprs)                                           # a listed value without rows: all fill


# ------------------------------------------------------------------ values
def test_discovered_values_ascend_with_nan_last_and_one_zero():
    p = np.array([2.5, -0.0, np.nan, -3.0, 0.0, np.inf, np.nan, -np.inf], dtype=np.float32)
    df = frame({"k": np.arange(8, dtype=np.int32) % 2, "p": p, "x": np.ones(8)}, 3)
    pv = df.groupBy("k").pivot("p")
    assert isinstance(pv, tfs.PivotedData)
    assert [str(v) for v in pv.values] == ["-inf", "-3.0", "0.0", "2.5", "inf", "nan"]
    assert not np.signbit(pv.values[2])
    out = pv.count()
    assert out.columns == ["k", "-Infinity", "-3.0", "0.0", "2.5", "Infinity", "NaN"]
    assert out.to_numpy("0.0").tolist() == [1, 1] and out.to_numpy("NaN").tolist() == [2, 0]
    both = frame({"p": p, "x": np.ones(8)}, 2).groupBy().pivot("p").count()
    assert both.to_numpy("0.0").tolist() == [2] and both.to_numpy("NaN").tolist() == [2]


def test_explicit_values_keep_their_order_and_unlisted_rows_count_for_nothing_else():
    cols = columns(seed=3)
    df = frame(cols, 2)
    out = df.groupBy("k").pivot("p", [2, 0, 1]).agg(F.sum("i"))
    assert out.columns == ["k", "2", "0", "1"]
    full = df.groupBy("k").pivot("p").agg(F.sum("i"))
    for v in ("0", "1", "2"):
        np.testing.assert_array_equal(out.to_numpy(v), full.to_numpy(v))
    np.testing.assert_array_equal(out.to_numpy("k"), full.to_numpy("k"))
    only = frame({"k": np.array([1, 1, 2, 3], np.int32), "p": np.array([0, 1, 5, 5], np.int32),
                  "x": np.array([1.0, 2.0, 4.0, 8.0])}, 2)
    got = only.groupBy("k").pivot("p", [1, 9]).agg(F.sum("x"), F.count("*"))
    assert got.to_numpy("k").tolist() == [1, 2, 3]                       # keys 2 and 3 have no listed value: a row still
    np.testing.assert_array_equal(got.to_numpy("1_sum(x)"), [2.0, np.nan, np.nan])
    assert got.to_numpy("1_count(1)").tolist() == [1, 0, 0] and got.to_numpy("9_count(1)").tolist() == [0, 0, 0]
    assert np.isnan(got.to_numpy("9_sum(x)")).all()
    ints = only.groupBy("k").pivot("p", [np.int64(1), 5.0]).count()      # numpy numbers, and a float that is whole
    assert ints.columns == ["k", "1", "5"] and ints.to_numpy("5").tolist() == [0, 1, 1]


# ------------------------------------------------------------------ names
def test_names():
    df = frame({"k": np.array([1, 1, 2], np.int32), "p": np.array([0.1, np.nan, np.inf], np.float32),
                "q": np.array([0.1, 0.25, 1e300]), "x": np.array([1.0, 2.0, 3.0])}, 1)
    assert df.groupBy("k").pivot("p").agg(F.sum("x")).columns == ["k", "0.1", "Infinity", "NaN"]
    assert df.groupBy("k").pivot("q").count().columns == ["k", "0.1", "0.25", "1e+300"]
    two = df.groupBy("k").pivot(tfs.col("p"), [np.float32(0.1)]).agg(F.sum("x"), F.avg("x").alias("ax"))
    assert two.columns == ["k", "0.1_sum(x)", "0.1_ax"]
    assert df.groupBy("k").pivot("p", [np.float32(0.1)]).agg({"x": "max"}).columns == ["k", "0.1"]
    assert df.groupBy("k").pivot("p", [np.float32(0.1)]).sum("x").columns == ["k", "0.1"]
    assert df.groupBy("k").pivot("p", [np.nan]).mean().columns == ["k", "NaN_avg(q)", "NaN_avg(x)"]
    with pytest.raises(ValueError, match="appears twice"):
        df.groupBy("k").pivot("p").agg(F.sum("x").alias("a"), F.avg("x").alias("a"))
    clash = frame({"1": np.array([1, 2], np.int32), "p": np.array([1, 2], np.int32), "x": np.array([1.0, 2.0])}, 1)
    with pytest.raises(ValueError, match="appears twice"):
        clash.groupBy("1").pivot("p").count()


# ------------------------------------------------------------------ typed errors
def test_typed_errors():
    cols = columns(40)
    df = frame(cols, 2)
    strs = tfs.create_dataframe([tfs.Row(k=1, s="a", x=1.0), tfs.Row(k=2, s="b", x=2.0)])
    with pytest.raises(tfs.InvalidTypeException, match="string column"):
        strs.groupBy("k").pivot("s")
    with pytest.raises(ValueError, match="one of the grouping keys"):
        df.groupBy("k", "p").pivot("p")
    with pytest.raises(TypeError, match="computed column"):
        df.groupBy("k").pivot(tfs.col("p") + 1)
    with pytest.raises(ValueError, match="must not be empty"):
        df.groupBy("k").pivot("p", [])
    with pytest.raises(ValueError, match="not a number"):
        df.groupBy("k").pivot("p", [True])
    with pytest.raises(ValueError, match="without change"):
        df.groupBy("k").pivot("p", [1, 1.5])
    with pytest.raises(ValueError, match="without change"):
        df.groupBy("k").pivot("p", [2 ** 31])
    with pytest.raises(ValueError, match="without change"):
        df.groupBy("k").pivot("x", [0.1])                                # not a float32
    with pytest.raises(ValueError, match="are the same value"):
        df.groupBy("k").pivot("p", [1, 2, 1])
    with pytest.raises(ValueError, match="are the same value"):
        df.groupBy("k").pivot("y", [0.0, 1.0, -0.0])
    with pytest.raises(ValueError, match="1025 pivot values; at most 1024"):
        df.groupBy("k").pivot("p", list(range(1025)))
    with pytest.raises(ValueError, match="5000 output columns; at most 4096"):
        df.groupBy("k").pivot("p", list(range(1000))).agg(*[F.sum("i").alias(f"s{j}") for j in range(5)])
    with pytest.raises(NotImplementedError, match="pivot"):
        df.groupBy("k").pivot("p").agg(F.median("x"))
    with pytest.raises(TypeError, match="window expression"):
        df.groupBy("k").pivot("p").agg(F.sum("x").over(Window.partitionBy("k")))
    with pytest.raises(ValueError, match=r"min\(i\) of an integer column.*cast"):
        df.groupBy("k").pivot("p").agg(F.min("i"))
    with pytest.raises(ValueError, match=r"max\(i\) of an integer column.*cast"):
        df.groupBy("k").pivot("p").max("i")
    with pytest.raises(ValueError, match="Column nope not found"):
        df.groupBy("k").pivot("nope")
    with pytest.raises(ValueError, match="Column nope not found"):
        df.groupBy("k").pivot("p").agg(F.sum("nope"))
    many = frame({"k": np.zeros(1100, np.int32), "p": np.arange(1100, dtype=np.int64)}, 1)
    with pytest.raises(ValueError, match="1100 pivot values; at most 1024"):
        many.groupBy("k").pivot("p")


# ------------------------------------------------------------------ empty results
def test_a_frame_without_rows_gives_the_keys_only():
    df = frame(columns(20), 2)
    none = df.filter(df["k"] > 100)
    out = none.groupBy("k", "d").pivot("p").agg(F.sum("x"), F.count("*"))
    assert out.columns == ["k", "d"] and out.count() == 0
    listed = none.groupBy("k").pivot("p", [1, 2]).agg(F.sum("x"), F.count("*"))
    assert listed.columns == ["k", "1_sum(x)", "1_count(1)", "2_sum(x)", "2_count(1)"] and listed.count() == 0
    assert listed.to_numpy("k").dtype == np.int32 or listed.to_numpy("k").size == 0
    blocks = listed.local_blocks()
    assert all(list(b.columns) == listed.columns and b.nrows == 0 for b in blocks.values()) and blocks


# ------------------------------------------------------------------ crosstab
def test_crosstab():
    a = np.array([3, 1, 3, 2, 1, 3], np.int32)
    b = np.array([7, 7, 8, 9, 7, 8], np.int64)
    df = frame({"a": a, "b": b}, 2)
    ct = df.stat.crosstab("a", "b")
    assert ct.columns == ["a_b", "7", "8", "9"]
    assert ct.to_numpy("a_b").tolist() == [1, 2, 3] and ct.to_numpy("a_b").dtype == np.int32
    table = np.stack([ct.to_numpy(c) for c in ("7", "8", "9")], 1)
    assert table.dtype == np.int64 and table.tolist() == [[2, 0, 0], [0, 0, 1], [1, 2, 0]]
    pv = df.groupBy("a").pivot("b").count()
    for c in ("7", "8", "9"):
        np.testing.assert_array_equal(ct.to_numpy(c), pv.to_numpy(c))
    np.testing.assert_array_equal(ct.to_numpy("a_b"), pv.to_numpy("a"))
    other = df.crosstab("a", "b")
    assert other.columns == ct.columns
    assert all(other.to_numpy(c).tolist() == ct.to_numpy(c).tolist() for c in ct.columns)
    with pytest.raises(ValueError, match="not found"):
        df.stat.crosstab("a", "z")


# ------------------------------------------------------------------ several ranks
def _spmd_results(df):
    exprs = [F.count("*"), F.sum("i"), F.sum("x"), F.avg("y"), F.min("x"), F.stddev_samp("y"), F.corr("x", "y")]
    out = {"two": (df.groupBy("k", "d").pivot("p", [3, 0, 9, 1]).agg(*exprs), ["k", "d"]),
           "found": (df.groupBy("k").pivot("p").agg(F.sum("x")), ["k"]),
           "none": (df.groupBy().pivot("p").agg(F.avg("y"), F.count("*")), []),
           "cross": (df.crosstab("k", "p"), ["k_p"])}
    res = {}
    for name, (o, keys) in out.items():
        rows = {repr(key): {n: np.asarray(v).tobytes().hex() for n, v in vals.items()}
                for key, vals in rows_of(o, keys).items()}
        local = {repr(tuple(b.columns[k][r].item() for k in keys))
                 for b in o.local_blocks().values() for r in range(b.nrows)}
        res[name] = {"rows": rows, "columns": o.columns, "owners": sorted(o.local_blocks()),
                     "nparts": o.num_partitions, "local": sorted(local)}
    return res


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _frame_of(cols, nparts):
    """The rows of `cols` in `nparts` even partitions, this rank's partitions only."""
    from tensorframes_amd.frame.block import Block
    from tensorframes_amd.frame.dataframe import DataFrame, _Materialized
    from tensorframes_amd.parallel import dist
    n = len(cols["k"])
    schema = tfs.from_columns({k: v[:1] for k, v in cols.items()}, num_partitions=1).schema
    blocks = {}
    for p in dist.local_partitions(nparts):
        a, b = (p * n) // nparts, ((p + 1) * n) // nparts
        blocks[p] = Block(b - a, {k: torch.from_numpy(np.ascontiguousarray(v[a:b])) for k, v in cols.items()})
    return DataFrame(schema, _Materialized(blocks), nparts)


def _worker(rank, world, port, outdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), OMP_NUM_THREADS="1", TFA_SHM_COLLECTIVES="1", TFA_DEVICE="cpu")
    torch.set_num_threads(1)
    sys.path.insert(0, REPO)
    from tensorframes_amd.parallel import dist

    assert dist.init(backend="gloo")
    res = _spmd_results(_frame_of(columns(seed=5), 5))
    with open(os.path.join(outdir, f"r{rank}.json"), "w") as f:
        json.dump(res, f)
    dist.shutdown()


def test_two_ranks_have_the_bits_of_one_process(tmp_path):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    outs = [json.load(open(tmp_path / f"r{r}.json")) for r in range(world)]
    single = _spmd_results(_frame_of(columns(seed=5), 5))
    for name, want in single.items():
        assert want["owners"] == [0] and want["nparts"] == 1 and want["rows"]
        seen = []
        for r, o in enumerate(outs):
            got = o[name]
            assert got["columns"] == want["columns"]
            assert got["owners"] == [r] and got["nparts"] == world       # one output partition per rank
            assert got["rows"] == want["rows"]                           # (to_numpy gathers: the union of the ranks)
            seen += got["local"]
        assert sorted(seen) == sorted(want["local"])                     # every key on exactly one rank
        assert len(seen) == len(set(seen))
    assert outs[0]["none"]["local"] == ["()"] and outs[1]["none"]["local"] == []   # no keys: rank 0
    assert all(o["two"]["local"] for o in outs)                          # the keys do spread over ranks
