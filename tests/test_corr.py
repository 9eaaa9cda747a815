"""`F.corr` / `F.covar_samp` / `F.covar_pop`, `df.stat.corr` / `df.stat.cov` and
their shortcuts on the host path (the CPU oracle of the device kernels), also
under gloo SPMD.

Expected values are written here, never taken from the package: the groups
are row lists built from the keys, `fractions.Fraction` over the
f64-converted data gives the exact co-moment C = sum (x - mean_x)(y - mean_y)
and both M2, each rounded once, Python ints give n and the count of
non-finite rows.

Tolerances (derived, not measured). The float data is x = 1e4 + z,
y = 1e4 + 0.6 z + 0.8 w with z, w standard normal (kappa = 1e4 on both sides,
r near 0.6), cast to the column dtype; the integer columns have a smaller
kappa (mean 100, sigma 5 for uint8; mean 1e4, sigma 100 otherwise), so the
same bounds hold with more room.
  * C: |C_got - C_exact| <= 1e-11 * sqrt(M2x_exact * M2y_exact). The scale is
    the Cauchy-Schwarz one, because C itself can be near zero; 1e-11 is the
    BOUND of tests/test_describe.py (log2(n) * eps * kappa).
  * M2_x, M2_y: 1e-11 relative.
  * corr: 2e-11 absolute (dC / scale + r / 2 * (dM2x / M2x + dM2y / M2y)).
  * covar_pop / covar_samp: the C bound divided by n / n - 1.
  * n and the non-finite count: exact.
`test_textbook_shortcut_is_rejected` shows that the bound rejects
sum(xy) - n mean_x mean_y."""
import json
import math
import os
import socket
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import tensorframes_amd as tfs
from tensorframes_amd import InvalidDimensionException, InvalidTypeException
from tensorframes_amd import functions as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-11
CORR_BOUND = 2e-11
FRAME_DTYPES = [np.uint8, np.int32, np.int64, np.float32, np.float64]  # (the types a frame column can have)
WORD_DTYPES = [np.uint8, np.int8, np.int16, np.int32, np.int64, np.float32, np.float64]
ROWS = [0, 1, 2, 65, 1000]
PAIR_FNS = [("corr", F.corr), ("covar_samp", F.covar_samp), ("covar_pop", F.covar_pop)]


# ------------------------------------------------------------------ the specification
def pair_data(dx, dy, n, seed=0):
    """x = 1e4 + z, y = 1e4 + 0.6 z + 0.8 w, cast to the column dtypes (integers: a scaled, rounded form)."""
    rng = np.random.default_rng(seed)
    z, w = rng.standard_normal(n), rng.standard_normal(n)

    def cast(v, dt):
        dt = np.dtype(dt)
        if dt.kind == "f":
            return (1e4 + v).astype(dt)
        if dt.itemsize == 1:
            return np.clip(np.rint(100 + 5 * v), 0 if dt.kind == "u" else -128, 127).astype(dt)
        return np.rint(10000 + 100 * v).astype(dt)
    return cast(z, dx), cast(0.6 * z + 0.8 * w, dy)


_EXACT = {}


def exact(x: np.ndarray, y: np.ndarray):
    """(C, M2x, M2y) of the f64-converted data in exact rational arithmetic, each rounded once."""
    key = (x.dtype.str, x.tobytes(), y.dtype.str, y.tobytes())
    if key not in _EXACT:
        fx = [Fraction(float(v)) for v in x.astype(np.float64)]
        fy = [Fraction(float(v)) for v in y.astype(np.float64)]
        n = len(fx)
        sx, sy = sum(fx), sum(fy)
        # sum (x - mx)(y - my) = sum xy - sx sy / n, exactly
        c = sum(a * b for a, b in zip(fx, fy)) - sx * sy / n
        m2x = sum(a * a for a in fx) - sx * sx / n
        m2y = sum(b * b for b in fy) - sy * sy / n
        _EXACT[key] = (float(c), float(m2x), float(m2y))
    return _EXACT[key]


def spec(fn: str, x: np.ndarray, y: np.ndarray):
    """(expected value, absolute bound) of pair statistic `fn` over the group's rows."""
    n = len(x)
    bad = int((~(np.isfinite(x.astype(np.float64)) & np.isfinite(y.astype(np.float64)))).sum())
    if n == 0 or bad:
        return math.nan, 0.0
    c, m2x, m2y = exact(x, y)
    scale = math.sqrt(m2x * m2y)
    if fn == "covar_pop":
        return c / n, BOUND * scale / n
    if fn == "covar_samp":
        return (c / (n - 1), BOUND * scale / (n - 1)) if n >= 2 else (math.nan, 0.0)
    if m2x == 0 or m2y == 0:
        return math.nan, 0.0
    return c / scale, CORR_BOUND


def check_value(got, fn, x, y, where=""):
    got = np.asarray(got)[()]
    assert got.dtype == np.float64, (where, fn, got.dtype)
    want, bound = spec(fn, x, y)
    if math.isnan(want):
        assert math.isnan(got), (where, fn, got)
    else:
        assert abs(float(got) - want) <= bound, (where, fn, got, want, abs(float(got) - want), bound)


def check_record(r: np.ndarray, x: np.ndarray, y: np.ndarray, where=""):
    """One pair record [7] against the rows it stands for (finite data)."""
    f = r[:6].view(np.float64)
    assert f[0] == float(len(x)) and int(r[6]) == 0, (where, f[0], r[6])
    if len(x) == 0:
        assert not r.any()
        return
    c, m2x, m2y = exact(x, y)
    scale = math.sqrt(m2x * m2y)
    assert abs(f[5] - c) <= BOUND * scale, (where, f[5], c, abs(f[5] - c) / max(scale, 1e-300))
    for got, want in ((f[3], m2x), (f[4], m2y)):
        assert abs(got - want) <= BOUND * want, (where, got, want)


def same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), (got, want)


def keyed_rows(out, key="k"):
    """{key value: {output column: numpy scalar}} over this process's partitions."""
    res = {}
    for b in out.local_blocks().values():
        cols = {n: b.columns[n].cpu().numpy() for n in out.columns}
        for r in range(b.nrows):
            assert cols[key][r].item() not in res
            res[cols[key][r].item()] = {n: cols[n][r] for n in out.columns if n != key}
    return res


# ------------------------------------------------------------------ interface
def test_functions_names_aliases_and_errors():
    for stat, fn in PAIR_FNS:
        e = fn("a", "b")
        assert isinstance(e, F.PairAggregateExpression) and not isinstance(e, F.AggregateExpression)
        assert e.output_name == f"{stat}(a, b)" and (e.fn, e.x, e.y) == (stat, "a", "b")
        assert fn(tfs.col("a"), "b").output_name == f"{stat}(a, b)" == fn("a", tfs.col("b")).output_name
        assert e.alias("q").output_name == "q" == e.name("q").output_name
        assert stat in F.__all__ and getattr(F, stat) is fn
        assert not isinstance(e, tfs.Column)
        with pytest.raises(TypeError, match="withColumn"):
            fn(tfs.col("a") + 1, "b")
        with pytest.raises(TypeError, match="withColumn"):
            fn("a", tfs.col("b") * 2)
        with pytest.raises(TypeError, match="sort order"):
            fn("a", tfs.col("b").desc())
        with pytest.raises(TypeError):
            fn("a", 3)
        with pytest.raises(TypeError):
            e.alias("")
    assert "PairAggregateExpression" in F.__all__


def _small():
    x, y = pair_data(np.float64, np.float32, 200, seed=3)
    k = (np.arange(200) % 3).astype(np.int32)
    return {"k": k, "x": x, "y": y, "i": np.arange(200, dtype=np.int32), "u": (np.arange(200) % 7).astype(np.uint8)}


def test_output_names_types_and_mixing_with_one_column_expressions():
    cols = _small()
    df = tfs.from_columns(cols, num_partitions=3)
    out = df.groupBy("k").agg(F.avg("x"), F.corr("x", "y"), F.count("*"), F.covar_samp("y", "x"), F.max("u"),
                              F.covar_pop("x", "i").alias("cp"), F.corr("u", "i"))
    assert out.columns == ["k", "avg(x)", "corr(x, y)", "count(1)", "covar_samp(y, x)", "max(u)", "cp", "corr(u, i)"]
    dts = [out.to_numpy(c).dtype for c in out.columns]
    assert dts == [np.int32, np.float64, np.float64, np.int64, np.float64, np.uint8, np.float64, np.float64]
    rows = keyed_rows(out)
    alone = keyed_rows(df.groupBy("k").agg(F.avg("x"), F.count("*"), F.max("u")))
    pairs_alone = keyed_rows(df.groupBy("k").agg(F.corr("x", "y"), F.covar_samp("y", "x")))
    for g in range(3):
        at = cols["k"] == g
        check_value(rows[g]["corr(x, y)"], "corr", cols["x"][at], cols["y"][at])
        check_value(rows[g]["covar_samp(y, x)"], "covar_samp", cols["y"][at], cols["x"][at])
        check_value(rows[g]["cp"], "covar_pop", cols["x"][at], cols["i"][at])
        check_value(rows[g]["corr(u, i)"], "corr", cols["u"][at], cols["i"][at])
        for c in ("avg(x)", "count(1)", "max(u)"):                      # the one-column results do not change
            same_bits(rows[g][c], alone[g][c])
        for c in ("corr(x, y)", "covar_samp(y, x)"):                    # nor do the pair results in other company
            same_bits(rows[g][c], pairs_alone[g][c])
    whole = df.agg(F.corr("x", "y"), F.sum("i"), F.covar_pop("x", "y"))
    assert whole.columns == ["corr(x, y)", "sum(i)", "covar_pop(x, y)"] and whole.count() == 1
    assert [whole.to_numpy(c).dtype for c in whole.columns] == [np.float64, np.int64, np.float64]
    check_value(whole.to_numpy("corr(x, y)")[0], "corr", cols["x"], cols["y"])
    check_value(whole.to_numpy("covar_pop(x, y)")[0], "covar_pop", cols["x"], cols["y"])
    assert int(whole.to_numpy("sum(i)")[0]) == int(cols["i"].sum())
    via_group = df.groupBy().agg(F.corr("x", "y"))
    same_bits(via_group.to_numpy("corr(x, y)"), whole.to_numpy("corr(x, y)"))
    # the dict form stays as it is: one-column functions only
    with pytest.raises(ValueError, match="not an aggregate function"):
        df.groupBy("k").agg({"x": "corr"})
    with pytest.raises(ValueError, match="appears twice"):
        df.groupBy("k").agg(F.corr("x", "y"), F.corr("x", "y"))
    with pytest.raises(ValueError, match="appears twice"):
        df.agg(F.corr("x", "y"), F.covar_pop("x", "i").alias("corr(x, y)"))
    with pytest.raises(ValueError, match="appears twice"):
        df.groupBy("k").agg(F.corr("x", "y").alias("k"))


def _pair_rows(fn):
    before = tfs.metrics.snapshot().get("pair_agg_rows", 0)
    fn()
    return tfs.metrics.snapshot().get("pair_agg_rows", 0) - before


def test_expressions_of_one_pair_share_its_record():
    cols = _small()
    df = tfs.from_columns(cols, num_partitions=2)
    n = len(cols["k"])
    for run in (lambda e: df.groupBy("k").agg(*e).local_blocks(), lambda e: df.agg(*e)):
        assert _pair_rows(lambda: run([F.corr("x", "y")])) == n
        three = [F.corr("x", "y"), F.covar_samp("x", "y"), F.covar_pop("x", "y").alias("c")]
        assert _pair_rows(lambda: run(three)) == n
        assert _pair_rows(lambda: run([F.corr("x", "y"), F.corr("y", "x")])) == 2 * n      # ordered pairs
        assert _pair_rows(lambda: run([F.avg("x")])) == 0
    before = tfs.metrics.snapshot()
    df.agg(F.corr("x", "y"))
    after = tfs.metrics.snapshot()
    assert after.get("pair_agg_host_partitions", 0) - before.get("pair_agg_host_partitions", 0) == 2
    assert after.get("pair_agg_device_partitions", 0) == before.get("pair_agg_device_partitions", 0)


def test_sixteen_pairs_per_call():
    rng = np.random.default_rng(1)
    cols = {f"c{j}": rng.standard_normal(40) for j in range(6)}
    cols["k"] = (np.arange(40) % 2).astype(np.int32)
    df = tfs.from_columns(cols, num_partitions=2)
    names = [f"c{j}" for j in range(6)]
    pairs = [(a, b) for a in names for b in names if a != b][:17]
    exprs = [F.corr(a, b) for a, b in pairs[:16]] + [F.covar_samp(a, b) for a, b in pairs[:16]]
    out = df.groupBy("k").agg(*exprs)                                    # 32 outputs of 16 pairs
    assert len(out.columns) == 33
    for a, b in pairs[:16]:
        for g in range(2):
            at = cols["k"] == g
            check_value(keyed_rows(out)[g][f"corr({a}, {b})"], "corr", cols[a][at], cols[b][at])
    assert df.agg(*exprs).count() == 1
    for run in (df.groupBy("k").agg, df.agg):
        with pytest.raises(ValueError, match="at most 16 distinct column pairs per call, got 17"):
            run(*[F.corr(a, b) for a, b in pairs])


def test_typed_errors():
    n = 6
    df = tfs.from_columns({"k": np.arange(n, dtype=np.int32), "s": np.array([f"s{i}" for i in range(n)]),
                           "v": np.zeros((n, 3)), "x": np.arange(n, dtype=np.float64),
                           "y": np.arange(n, dtype=np.float64) ** 2})
    rows = tfs.create_dataframe([(True, 1, 1.0), (False, 2, 2.0), (True, 1, 4.5)], ["b", "k", "x"])
    for fn in (F.corr, F.covar_samp, F.covar_pop):
        for run in (df.groupBy("k").agg, df.agg):
            with pytest.raises(InvalidTypeException, match="string"):
                run(fn("x", "s"))
            with pytest.raises(InvalidTypeException, match="string"):
                run(fn("s", "x"))
            with pytest.raises(InvalidDimensionException, match="scalar"):
                run(fn("v", "x"))
            with pytest.raises(ValueError, match="nope"):
                run(fn("x", "nope"))
        with pytest.raises(InvalidTypeException, match="bool"):
            rows.groupBy("k").agg(fn("x", "b"))
    with pytest.raises(InvalidTypeException, match="string"):
        df.corr("x", "s")
    with pytest.raises(InvalidDimensionException, match="scalar"):
        df.stat.cov("v", "x")
    with pytest.raises(ValueError, match="nope"):
        df.cov("nope", "x")
    with pytest.raises(TypeError):
        df.corr(df["x"] * 2, "y")
    # keys follow groupBy().agg's rules
    with pytest.raises(InvalidTypeException, match="aggregate"):
        df.groupBy("s").agg(F.corr("x", "y"))
    # not a window function, not a Column
    from tensorframes_amd import Window
    e = F.corr("x", "y")
    with pytest.raises(NotImplementedError, match="pair aggregates are not supported over a window"):
        e.over(Window.partitionBy("k"))
    with pytest.raises(TypeError):
        e + 1
    with pytest.raises(TypeError):
        e * e
    with pytest.raises(TypeError):
        df.filter(e)
    with pytest.raises(TypeError):
        df.withColumn("c", e)
    for method in ("spearman", "kendall", "", None):
        with pytest.raises(ValueError, match="pearson"):
            df.corr("x", "y", method)
        with pytest.raises(ValueError, match="pearson"):
            df.stat.corr("x", "y", method=method)
    assert df.corr("x", "y", "pearson") == df.corr("x", "y", method="pearson")


def test_stat_corr_is_df_corr_is_agg():
    cols = _small()
    df = tfs.from_columns(cols, num_partitions=3)
    a = df.stat.corr("x", "y")
    assert isinstance(a, float) and isinstance(df.cov("x", "y"), float)
    want = df.agg(F.corr("x", "y")).to_numpy("corr(x, y)")
    same_bits(np.array([a]), want)
    same_bits(np.array([df.corr("x", "y")]), want)
    cov = df.agg(F.covar_samp("x", "y"), F.covar_pop("x", "y"))
    same_bits(np.array([df.stat.cov("x", "y")]), cov.to_numpy("covar_samp(x, y)"))
    same_bits(np.array([df.cov("x", "y")]), cov.to_numpy("covar_samp(x, y)"))
    assert df.cov("x", "y") != float(cov.to_numpy("covar_pop(x, y)")[0])   # cov is the sample covariance
    check_value(np.float64(a), "corr", cols["x"], cols["y"])
    check_value(np.float64(df.cov("x", "y")), "covar_samp", cols["x"], cols["y"])


# ------------------------------------------------------------------ values
@pytest.mark.parametrize("dy", FRAME_DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("dx", FRAME_DTYPES, ids=lambda d: np.dtype(d).name)
def test_every_pair_of_frame_dtypes(dx, dy):
    for n in ROWS:
        x, y = pair_data(dx, dy, n, seed=n)
        sizes = [1, 2] + [n - 3] if n > 3 else [n]                      # group sizes 1, 2 and many
        k = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
        np.random.default_rng(n + 1).shuffle(k)
        df = tfs.from_columns({"k": k, "x": x, "y": y}, num_partitions=3)
        exprs = [fn("x", "y") for _, fn in PAIR_FNS]
        whole = df.agg(*exprs)
        assert whole.count() == 1
        for stat, _ in PAIR_FNS:
            check_value(whole.to_numpy(f"{stat}(x, y)")[0], stat, x, y, (n, stat))
        out = df.groupBy("k").agg(*exprs)
        rows = keyed_rows(out)
        assert set(rows) == set(np.unique(k).tolist()) and out.count() == (len(sizes) if n else 0)
        for g in rows:
            for stat, _ in PAIR_FNS:
                check_value(rows[g][f"{stat}(x, y)"], stat, x[k == g], y[k == g], (n, g, stat))
        if n == 1:
            assert math.isnan(df.corr("x", "y")) and math.isnan(df.cov("x", "y"))
            assert whole.to_numpy("covar_pop(x, y)")[0] == 0.0
        if n == 0:
            assert math.isnan(df.corr("x", "y")) and math.isnan(df.cov("x", "y"))
            assert math.isnan(whole.to_numpy("covar_pop(x, y)")[0])


def test_host_records_of_all_seven_dtypes_and_their_merge():
    from tensorframes_amd.frame import group_agg as GA
    rng = np.random.default_rng(3)
    n = 700
    ids = rng.integers(0, 5, n)
    for j, dx in enumerate(WORD_DTYPES):
        dy = WORD_DTYPES[(j + 3) % 7]
        x, y = pair_data(dx, dy, n, seed=10 + j)
        rec = GA._host_pair_records([torch.from_numpy(x), torch.from_numpy(y)],
                                    [torch.from_numpy(y), torch.from_numpy(y)], ids, 5)
        assert rec.shape == (5, 2, 7) and rec.dtype == np.int64
        halves = [GA._host_pair_records([torch.from_numpy(x[a:b])], [torch.from_numpy(y[a:b])], ids[a:b], 5)
                  for a, b in ((0, 300), (300, n))]
        both = np.stack(halves, 1).reshape(10, 1, 7)                    # ordered by (group, partition)
        merged = GA._merge_pair_records(both, np.arange(0, 11, 2))
        for g in range(5):
            at = ids == g
            check_record(rec[g, 0], x[at], y[at], (dx, dy, g))
            check_record(rec[g, 1], y[at], y[at], (dy, dy, g))
            check_record(merged[g, 0], x[at], y[at], (dx, dy, g, "merged"))
        outs = GA._pair_results(merged, [0, 0, 0], ["corr", "covar_samp", "covar_pop"])
        for (stat, _), o in zip(PAIR_FNS, outs):
            for g in range(5):
                check_value(o[g], stat, x[ids == g], y[ids == g], (dx, dy, g, stat))
    # the empty record is all zeros, merges away on either side, and has no statistics
    empty = np.zeros((1, 1, 7), dtype=np.int64)
    one = rec[:1, :1]
    same_bits(GA._pair_chan(empty, one), one)
    same_bits(GA._pair_chan(one, empty), one)
    same_bits(GA._pair_chan(empty, empty), empty)
    assert all(math.isnan(o[0]) for o in GA._pair_results(empty, [0, 0, 0], ["corr", "covar_samp", "covar_pop"]))


def test_constant_equal_and_opposite_columns():
    rng = np.random.default_rng(5)
    n = 1000
    x = 1e4 + rng.standard_normal(n)
    k = (np.arange(n) % 4).astype(np.int64)
    cols = {"k": k, "x": x, "same": x.copy(), "neg": -x, "c": np.full(n, 7.25), "ci": np.full(n, 3, dtype=np.int32),
            "x32": x.astype(np.float32)}
    df = tfs.from_columns(cols, num_partitions=3)
    out = df.groupBy("k").agg(F.corr("x", "c"), F.covar_samp("x", "c"), F.covar_pop("c", "x"), F.corr("ci", "x"),
                              F.covar_pop("ci", "c"), F.corr("x", "same"), F.corr("x", "neg"), F.corr("x32", "x32"),
                              F.corr("c", "c"))
    rows = keyed_rows(out)
    for g in range(4):
        r = rows[g]
        assert math.isnan(r["corr(x, c)"]) and math.isnan(r["corr(ci, x)"]) and math.isnan(r["corr(c, c)"])
        assert r["covar_samp(x, c)"] == 0.0 and r["covar_pop(c, x)"] == 0.0 and r["covar_pop(ci, c)"] == 0.0
        assert abs(r["corr(x, same)"] - 1.0) <= CORR_BOUND and abs(r["corr(x32, x32)"] - 1.0) <= CORR_BOUND
        assert abs(r["corr(x, neg)"] + 1.0) <= CORR_BOUND
    assert math.isnan(df.corr("x", "c")) and df.cov("x", "c") == 0.0
    assert abs(df.corr("x", "same") - 1.0) <= CORR_BOUND and abs(df.corr("neg", "x") + 1.0) <= CORR_BOUND
    # a variance: cov(x, x) is var_samp(x)
    var = float(df.agg(F.var_samp("x")).to_numpy("var_samp(x)")[0])
    assert abs(df.cov("x", "x") - var) <= 2 * BOUND * var


@pytest.mark.parametrize("side", ["x", "y"])
@pytest.mark.parametrize("where", ["first", "last", "middle"])
@pytest.mark.parametrize("special", [(math.nan,), (math.inf,), (math.inf, -math.inf)], ids=["nan", "inf", "both"])
def test_non_finite_rows_make_their_group_nan(special, where, side):
    from tensorframes_amd.frame import group_agg as GA
    n, parts = 300, 5
    x, y = pair_data(np.float64, np.float32, n, seed=8)
    k = (np.arange(n) % 3).astype(np.int32)
    clean = {"k": k, "x": x, "y": y}
    rows_of_1 = np.nonzero(k == 1)[0]
    at = {"first": rows_of_1[:len(special)], "last": rows_of_1[-len(special):],
          "middle": rows_of_1[len(rows_of_1) // 2:][:len(special)]}[where]
    if where == "middle":
        assert n // parts * 2 <= at[0] < n // parts * 3                  # a row of partition 2 of 5
    dirty = {c: v.copy() for c, v in clean.items()}
    dirty[side][at] = np.array(special, dtype=dirty[side].dtype)
    exprs = [fn("x", "y") for _, fn in PAIR_FNS]
    got = keyed_rows(tfs.from_columns(dirty, num_partitions=parts).groupBy("k").agg(*exprs))
    ref = keyed_rows(tfs.from_columns(clean, num_partitions=parts).groupBy("k").agg(*exprs))
    for stat, _ in PAIR_FNS:
        name = f"{stat}(x, y)"
        assert math.isnan(got[1][name]), (name, got[1][name])
        for g in (0, 2):                                                 # the other groups are untouched
            same_bits(got[g][name], ref[g][name])
            check_value(got[g][name], stat, clean["x"][k == g], clean["y"][k == g])
    whole = tfs.from_columns(dirty, num_partitions=parts).agg(*exprs)
    assert all(math.isnan(whole.to_numpy(c)[0]) for c in whole.columns)
    assert math.isnan(tfs.from_columns(dirty, num_partitions=parts).corr("x", "y"))
    # the count is exact, and n counts every row
    rec = GA._host_pair_records([torch.from_numpy(dirty["x"])], [torch.from_numpy(dirty["y"])], k.astype(np.int64), 3)
    assert rec[:, 0, 6].tolist() == [0, len(special), 0]
    assert rec[:, 0, 0].view(np.float64).tolist() == [100.0, 100.0, 100.0]
    halves = [GA._host_pair_records([torch.from_numpy(dirty["x"][a:b])], [torch.from_numpy(dirty["y"][a:b])],
                                    k[a:b].astype(np.int64), 3) for a, b in ((0, 150), (150, n))]
    merged = GA._merge_pair_records(np.stack(halves, 1).reshape(6, 1, 7), np.arange(0, 7, 2))
    assert merged[:, 0, 6].tolist() == [0, len(special), 0]


def test_a_non_finite_row_in_each_column_counts_rows_not_values():
    from tensorframes_amd.frame import group_agg as GA
    x = np.array([1.0, math.nan, 3.0, math.inf, 5.0])
    y = np.array([2.0, math.inf, 1.0, 4.0, -math.inf], dtype=np.float32)
    rec = GA._host_pair_records([torch.from_numpy(x)], [torch.from_numpy(y)], np.zeros(5, dtype=np.int64), 1)
    assert int(rec[0, 0, 6]) == 3 and rec[0, 0, :1].view(np.float64)[0] == 5.0
    df = tfs.from_columns({"x": x, "y": y})
    assert math.isnan(df.corr("x", "y")) and math.isnan(df.cov("x", "y"))


def test_textbook_shortcut_is_rejected():
    """sum(xy) - n mean_x mean_y on the f64 data of seed 0 at n = 65, 1000 and 40000 is off by more than 1e-9 of
    the Cauchy-Schwarz scale (8.6e-9, 2.4e-8 and 2.7e-8 when this was written), the host path within 1e-11."""
    from tensorframes_amd.frame import group_agg as GA
    for n in (65, 1000, 40000):
        x, y = pair_data(np.float64, np.float64, n, seed=0)
        c, m2x, m2y = exact(x, y)
        scale = math.sqrt(m2x * m2y)
        shortcut = float((x * y).sum() - n * x.mean() * y.mean())
        rec = GA._host_pair_records([torch.from_numpy(x)], [torch.from_numpy(y)], np.zeros(n, dtype=np.int64), 1)
        got = float(rec[0, 0, 5:6].view(np.float64)[0])
        print(f"n = {n}: host path {abs(got - c) / scale:.2e}, shortcut {abs(shortcut - c) / scale:.2e}")
        assert abs(got - c) <= BOUND * scale
        assert abs(shortcut - c) > 1e-9 * scale
        df = tfs.from_columns({"x": x, "y": y}, num_partitions=4)
        check_value(np.float64(df.corr("x", "y")), "corr", x, y)
        check_value(np.float64(df.cov("x", "y")), "covar_samp", x, y)


@pytest.mark.parametrize("parts", [1, 3, 7])
def test_any_partitioning_within_the_tolerance(parts):
    n = 5000
    x, y = pair_data(np.float32, np.float64, n, seed=2)
    k = np.random.default_rng(3).integers(0, 6, n).astype(np.int64)
    df = tfs.from_columns({"k": k, "x": x, "y": y}, num_partitions=parts)
    rows = keyed_rows(df.groupBy("k").agg(*[fn("x", "y") for _, fn in PAIR_FNS]))
    for g in range(6):
        for stat, _ in PAIR_FNS:
            check_value(rows[g][f"{stat}(x, y)"], stat, x[k == g], y[k == g], (parts, g, stat))
    check_value(np.float64(df.corr("x", "y")), "corr", x, y)


# ------------------------------------------------------------------ several ranks
def frame_of(cols, sizes):
    """A frame whose partition p holds sizes[p] rows (zero allowed), this rank's partitions only."""
    from tensorframes_amd.frame.block import Block
    from tensorframes_amd.frame.dataframe import DataFrame, _Materialized
    from tensorframes_amd.parallel import dist
    n = len(next(iter(cols.values())))
    assert sum(sizes) == n
    schema = tfs.from_columns({k: v[:1] for k, v in cols.items()}, num_partitions=1).schema
    starts = np.concatenate([[0], np.cumsum(sizes)])
    blocks = {}
    for p in dist.local_partitions(len(sizes)):
        a, b = int(starts[p]), int(starts[p + 1])
        blocks[p] = Block(b - a, {k: torch.from_numpy(np.ascontiguousarray(v[a:b])) for k, v in cols.items()})
    return DataFrame(schema, _Materialized(blocks), len(sizes))


SPMD_SIZES = [400, 0, 731, 1, 250, 513, 105]                             # 7 partitions, one empty, one of one row


def _spmd_columns():
    n = sum(SPMD_SIZES)
    x, y = pair_data(np.float64, np.float32, n, seed=4)
    rng = np.random.default_rng(5)
    k = rng.integers(0, 9, n).astype(np.int32)
    z = rng.standard_normal(n)
    z[k == 3] = np.where(np.arange((k == 3).sum()) % 50 == 0, np.nan, z[k == 3])  # a group with NaNs
    return {"k": k, "x": x, "y": y, "z": z, "i": np.rint(100 * rng.standard_normal(n)).astype(np.int64)}


def _spmd_exprs():
    return [F.corr("x", "y"), F.covar_samp("x", "y"), F.covar_pop("y", "x"), F.avg("x"), F.corr("x", "z"),
            F.covar_samp("i", "y"), F.count("*"), F.corr("i", "x")]


def _spmd_results(df):
    out = df.groupBy("k").agg(*_spmd_exprs())
    rows = {str(key): {n: np.asarray(v).tobytes().hex() for n, v in vals.items()}
            for key, vals in keyed_rows(out).items()}
    whole = df.agg(*_spmd_exprs())
    return {"rows": rows, "owners": sorted(out.local_blocks()),
            "whole": {c: whole.to_numpy(c).tobytes().hex() for c in whole.columns},
            "scalars": [np.float64(v).tobytes().hex() for v in (df.corr("x", "y"), df.stat.cov("i", "y"))]}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, outdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), OMP_NUM_THREADS="1", TFA_SHM_COLLECTIVES="1", TFA_DEVICE="cpu")
    torch.set_num_threads(1)
    sys.path.insert(0, REPO)
    from tensorframes_amd.parallel import dist

    assert dist.init(backend="gloo", force=True)                         # (a world of one builds a group too)
    res = _spmd_results(frame_of(_spmd_columns(), SPMD_SIZES))
    with open(os.path.join(outdir, f"r{rank}.json"), "w") as f:
        json.dump(res, f)
    dist.shutdown()


@pytest.mark.parametrize("world", [1, 2, 4])
def test_pair_agg_spmd_has_the_bits_of_one_process(world, tmp_path):
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    outs = [json.load(open(tmp_path / f"r{r}.json")) for r in range(world)]
    cols = _spmd_columns()
    single = _spmd_results(frame_of(cols, SPMD_SIZES))                   # this process, the same partitioning
    rows = {}
    for r, o in enumerate(outs):
        assert o["owners"] == [r]
        assert not set(o["rows"]) & set(rows)                            # a key lives on one rank
        rows.update(o["rows"])
        assert o["whole"] == single["whole"]                             # DataFrame.agg: the same row on every rank
        assert o["scalars"] == single["scalars"]
    assert rows == single["rows"] and len(rows) == 9
    if world > 1:
        assert sum(1 for o in outs if o["rows"]) >= 2                    # the keys do spread over ranks
    # and the values are right: the NaN group is NaN only where z is read
    k = cols["k"]
    for g in range(9):
        got = {n: np.frombuffer(bytes.fromhex(v), dtype=np.float64 if n != "count(1)" else np.int64)[0]
               for n, v in rows[str(g)].items()}
        at = k == g
        check_value(got["corr(x, y)"], "corr", cols["x"][at], cols["y"][at])
        check_value(got["covar_pop(y, x)"], "covar_pop", cols["y"][at], cols["x"][at])
        check_value(got["covar_samp(i, y)"], "covar_samp", cols["i"][at], cols["y"][at])
        check_value(got["corr(x, z)"], "corr", cols["x"][at], cols["z"][at])
        assert math.isnan(got["corr(x, z)"]) == (g == 3)
        assert int(got["count(1)"]) == int(at.sum())
