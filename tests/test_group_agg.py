"""`GroupedData.agg` / `DataFrame.agg` and `tfs.functions` on the host path (the
CPU oracle of the device kernels), also under gloo SPMD.

Expected values are written here, never taken from the package: a dict from
key tuple to the group's values (in row order) gives the groups,
`fractions.Fraction` gives exact mean and M2, Python ints masked to 64 bits
give integer sums, and the ordering table (`spec_words`, copied from
tests/test_gpu_sort.py) gives min and max.

Tolerances. Counts, integer sums, min and max are exact. Mean, stddev and
variance keep the 1e-11 relative bound derived in tests/test_describe.py: the
data are the same 1e4 + N(0, 1) columns (kappa = 1e4) with fewer rows per
group, so the room only grows; the textbook shortcut sum(x^2) - n * mean^2 is
rejected by the same bound (`test_textbook_shortcut_is_rejected`). Float sums
of that positive data are held to (terms of the summation) * 2^-53 * 10
relative to the exact rational sum. On the device the terms are rows per lane
(8) + 6 butterfly steps + chunks + partitions (25 terms, 2.8e-14 for the
largest group: tests/test_gpu_group_agg.py). The host path measured here sums
a group's rows of one partition sequentially (`np.add.reduceat`), so its term
count is the rows of the group + partitions: 1543 + 7 = 1550 terms for the
largest group, a bound of 1.72e-12 (`sum_bound`), computed per group from its
own row count.

Frames hold five numeric dtypes (uint8, int32, int64, float32, float64); the
record code is checked for all seven statistics dtypes directly
(`test_host_records_of_all_seven_dtypes`)."""
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
MASK = (1 << 64) - 1
CHUNK = 512
SIZES = [1, 2, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 7]
WORD_DTYPES = [np.uint8, np.int8, np.int16, np.int32, np.int64, np.float32, np.float64]


def sum_bound(rows: int, partitions: int) -> float:
    return (rows + partitions) * 2.0 ** -53 * 10


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


def canonical(v):
    """What a word decodes to: -0.0 as 0.0, every NaN as the quiet NaN."""
    v = np.asarray(v)
    if v.dtype.kind != "f":
        return v
    return np.where(np.isnan(v), np.array(np.nan, dtype=v.dtype), v + v.dtype.type(0.0)).astype(v.dtype)


def same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), (got, want)


_EXACT = {}


def exact(x: np.ndarray):
    """(mean, M2, sum) of the f64-converted finite data in exact rational arithmetic, rounded once."""
    key = (x.dtype.str, x.tobytes())
    if key not in _EXACT:
        fx = [Fraction(float(v)) for v in x.astype(np.float64)]
        total = sum(fx)
        mean = total / len(fx)
        _EXACT[key] = (float(mean), float(sum((v - mean) ** 2 for v in fx)), float(total))
    return _EXACT[key]


def int_sum(x: np.ndarray) -> int:
    s = sum(int(v) for v in x) & MASK
    return s - (1 << 64) if s >> 63 else s


def spec(fn: str, x: np.ndarray):
    """The expected value of statistic `fn` over the group's values x (row order)."""
    n = len(x)
    if fn == "count":
        return np.int64(n)
    if fn in ("min", "max"):
        w = spec_words(x)
        return canonical(x[np.argmin(w) if fn == "min" else np.argmax(w)])[()]
    fl = x.dtype.kind == "f"
    if fn == "sum" and not fl:
        return np.int64(int_sum(x))
    special = None
    if fl:
        nan, pinf, ninf = np.isnan(x).any(), (x == np.inf).any(), (x == -np.inf).any()
        if nan or (pinf and ninf):
            special = (math.nan, math.nan)
        elif pinf or ninf:
            special = (math.inf if pinf else -math.inf, math.nan)
    if special is not None:
        mean, m2, total = special[0], special[1], special[0]
    else:
        mean, m2, total = exact(x)
    if fn == "sum":
        return np.float64(total)
    if fn == "avg":
        return np.float64(mean)
    if fn in ("var_samp", "stddev_samp"):
        v = m2 / (n - 1) if n >= 2 else math.nan
    else:
        v = m2 / n
    return np.float64(math.sqrt(v) if fn.startswith("stddev") and not math.isnan(v) else v)


def rel(got: float, want: float) -> float:
    return abs(got - want) / abs(want)


def check_value(got, want, fn: str, rows: int, partitions: int, where=""):
    got, want = np.asarray(got)[()], np.asarray(want)[()]
    assert got.dtype == want.dtype, (where, fn, got.dtype, want.dtype)
    if fn in ("count", "min", "max") or want.dtype.kind != "f" or not np.isfinite(want):
        assert got.tobytes() == want.tobytes(), (where, fn, got, want)
        return
    if want == 0.0:                                                    # (a sum of -0.0 alone may keep its sign)
        assert got == 0.0, (where, fn, got, want)
        return
    bound = sum_bound(rows, partitions) if fn == "sum" else BOUND
    assert rel(float(got), float(want)) <= bound, (where, fn, got, want, rel(float(got), float(want)), bound)


def groups_of(cols, keys):
    """{key tuple (canonical Python values): row indices in row order}"""
    out = {}
    kc = [canonical(cols[k]) for k in keys]
    for r in range(len(kc[0])):
        out.setdefault(tuple(c[r].item() for c in kc), []).append(r)
    return {k: np.array(v) for k, v in out.items()}


def frame_rows(out, keys):
    """{key tuple: {output column: numpy scalar}} over this process's partitions."""
    res = {}
    for b in out.local_blocks().values():
        cols = {n: (b.columns[n].cpu().numpy() if isinstance(b.columns[n], torch.Tensor) else None)
                for n in out.columns}
        for r in range(b.nrows):
            key = tuple(canonical(cols[k][r:r + 1])[0].item() for k in keys)
            assert key not in res, key
            res[key] = {n: cols[n][r] for n in out.columns if n not in keys}
    return res


def check_frame(out, cols, keys, exprs, partitions):
    """Every output of `out` against the specification."""
    groups = groups_of(cols, keys)
    got = frame_rows(out, keys)
    assert out.columns == list(keys) + [name for name, _, _ in exprs]
    assert set(got) == set(groups), (sorted(got)[:5], sorted(groups)[:5])
    for key, rows in groups.items():
        for name, fn, col in exprs:
            x = cols[col][rows] if col is not None else np.zeros(len(rows))
            check_value(got[key][name], spec(fn, x), fn, len(rows), partitions, (key, name))
    # each partition holds its keys in ascending order
    for b in out.local_blocks().values():
        w = [spec_words(b.columns[k].numpy()) for k in keys]
        order = np.lexsort(w[::-1])
        assert (order == np.arange(b.nrows)).all()


ALL_FNS = [("count", F.count), ("sum", F.sum), ("avg", F.avg), ("avg", F.mean), ("min", F.min), ("max", F.max),
           ("stddev_samp", F.stddev), ("stddev_samp", F.stddev_samp), ("stddev_pop", F.stddev_pop),
           ("var_samp", F.variance), ("var_samp", F.var_samp), ("var_pop", F.var_pop)]


def _columns(seed=0):
    ids = np.repeat(np.arange(len(SIZES)), SIZES)
    rng = np.random.default_rng(seed)
    rng.shuffle(ids)
    n = len(ids)
    z = rng.standard_normal(n)
    z[ids == 3] = np.where(np.arange((ids == 3).sum()) % 9 == 0, np.nan, z[ids == 3])      # a NaN group
    z[np.nonzero(ids == 4)[0][::7]] = np.inf                                                # +inf
    z[np.nonzero(ids == 5)[0][::11]] = -np.inf                                              # -inf
    at = np.nonzero(ids == 6)[0]
    z[at[::13]], z[at[1::13]] = np.inf, -np.inf                                             # both
    z[np.nonzero(ids == 7)[0][::5]] = -0.0
    z[np.nonzero(ids == 1)[0]] = -0.0                                                       # a group of -0.0 alone
    return {"k": np.array([7, -2, 0, 11, 5, 2 ** 31 - 1, -2 ** 31, 3, 4], dtype=np.int32)[ids],
            "f": (rng.integers(0, 3, n) * 0.5 - 0.5),
            "j": rng.integers(0, 2, n).astype(np.int64) * (2 ** 40) - 5,
            "x": (1e4 + rng.standard_normal(n)).astype(np.float32), "h": 1e4 + rng.standard_normal(n), "z": z,
            "g": rng.integers(2 ** 53, 2 ** 62, n).astype(np.int64) * rng.choice([-1, 1], n),
            "i": np.rint(10000 + 100 * rng.standard_normal(n)).astype(np.int32),
            "u": rng.integers(0, 256, n).astype(np.uint8)}


VALUES = ["x", "h", "z", "g", "i", "u"]


# ------------------------------------------------------------------ functions, names, types
def test_functions_names_aliases_and_errors():
    for stat, fn in ALL_FNS:
        e = fn("x")
        assert isinstance(e, F.AggregateExpression) and e.output_name == f"{stat}(x)"
        assert fn(tfs.col("x")).output_name == f"{stat}(x)" and e.alias("q").output_name == "q"
    assert F.count("*").output_name == "count(1)" == F.count(1).output_name
    assert not isinstance(F.sum("x"), tfs.Column)
    with pytest.raises(TypeError, match="withColumn"):
        F.sum(tfs.col("x") + 1)
    with pytest.raises(TypeError, match="sort order"):
        F.max(tfs.col("x").desc())
    with pytest.raises(TypeError):
        F.avg(3)
    with pytest.raises(TypeError):
        F.avg("x").alias("")
    assert tfs.functions is F


def test_every_function_and_alias_against_the_specification():
    cols = _columns()
    df = tfs.from_columns(cols, num_partitions=3)
    exprs, todo = [], []
    for v in VALUES:
        for j, (stat, fn) in enumerate(ALL_FNS):
            name = f"{fn.__name__}_{v}"
            todo.append(fn(v).alias(name))
            exprs.append((name, stat, v))
    out = df.groupBy("k").agg(*todo)
    check_frame(out, cols, ["k"], exprs, 3)
    # Spark's names and types
    named = df.groupBy("k").agg(F.count("*"), F.count("x"), F.sum("i"), F.sum("x"), F.mean("u"), F.stddev("h"),
                                F.variance("h"), F.stddev_pop("h"), F.var_pop("h"), F.min("u"), F.max("x"),
                                F.max("h").alias("top"))
    assert named.columns == ["k", "count(1)", "count(x)", "sum(i)", "sum(x)", "avg(u)", "stddev_samp(h)",
                             "var_samp(h)", "stddev_pop(h)", "var_pop(h)", "min(u)", "max(x)", "top"]
    dts = [named.to_numpy(c).dtype for c in named.columns]
    assert dts == [np.int32, np.int64, np.int64, np.int64, np.float64, np.float64, np.float64, np.float64,
                   np.float64, np.float64, np.uint8, np.float32, np.float64]
    same_bits(named.to_numpy("count(1)"), named.to_numpy("count(x)"))
    with pytest.raises(ValueError, match="appears twice"):
        df.groupBy("k").agg(F.sum("x"), F.sum("x"))
    with pytest.raises(ValueError, match="appears twice"):
        df.groupBy("k").agg(F.sum("x").alias("k"))
    with pytest.raises(ValueError, match="at least one"):
        df.groupBy("k").agg()


@pytest.mark.parametrize("name,dtype", [("u", np.uint8), ("i", np.int32), ("g", np.int64), ("x", np.float32),
                                        ("h", np.float64)])
def test_output_dtypes(name, dtype):
    df = tfs.from_columns(_columns(), num_partitions=2)
    out = df.groupBy("k").agg(F.count(name), F.sum(name), F.avg(name), F.stddev(name), F.stddev_pop(name),
                              F.variance(name), F.var_pop(name), F.min(name), F.max(name))
    fl = np.dtype(dtype).kind == "f"
    want = [np.int64, np.float64 if fl else np.int64] + [np.float64] * 5 + [dtype, dtype]
    assert [out.to_numpy(c).dtype for c in out.columns[1:]] == [np.dtype(t) for t in want]
    whole = df.agg(F.count(name), F.sum(name), F.avg(name), F.min(name))
    assert [whole.to_numpy(c).dtype for c in whole.columns] == [np.dtype(t) for t in (want[0], want[1], np.float64,
                                                                                       dtype)]


def test_host_records_of_all_seven_dtypes():
    from tensorframes_amd.frame import group_agg as GA
    rng = np.random.default_rng(3)
    ids = rng.integers(0, 5, 700)
    for dt in WORD_DTYPES:
        dt = np.dtype(dt)
        if dt.kind == "f":
            x = (1e4 + rng.standard_normal(700)).astype(dt)
        else:
            ii = np.iinfo(dt)
            x = rng.integers(ii.min, ii.max, 700, dtype=dt, endpoint=True)
        rec = GA._host_group_records([torch.from_numpy(x)], ids, 5)
        halves = [GA._host_group_records([torch.from_numpy(x[a:b])], ids[a:b], 5) for a, b in ((0, 300), (300, 700))]
        both = np.stack(halves, 1).reshape(10, 1, 6)                  # ordered by (group, partition)
        merged = GA._merge_records(both, np.arange(0, 11, 2), [dt.kind == "f"])
        stats = ["count", "sum", "avg", "stddev_samp", "min", "max"]
        for r, parts in ((rec, 1), (merged, 2)):
            outs = GA._host_results(r, [0] * 6, stats, [dt] * 6)
            for g in range(5):
                for s, o in zip(stats, outs):
                    check_value(o[g], spec(s, x[ids == g]), s, int((ids == g).sum()), parts, (dt, g, s))


# ------------------------------------------------------------------ forms of the call
def test_dict_form_and_shortcuts():
    cols = _columns()
    df = tfs.from_columns(cols, num_partitions=2)
    out = df.groupBy("k").agg({"h": "mean", "i": "SUM", "u": "max", "*": "count"})
    check_frame(out, cols, ["k"], [("avg(h)", "avg", "h"), ("sum(i)", "sum", "i"), ("max(u)", "max", "u"),
                                   ("count(1)", "count", None)], 2)
    with pytest.raises(ValueError, match="median"):
        df.groupBy("k").agg({"h": "median"})
    with pytest.raises(ValueError, match="nope"):
        df.groupBy("k").agg({"nope": "sum"})
    for fn, stat in (("sum", "sum"), ("avg", "avg"), ("mean", "avg"), ("min", "min"), ("max", "max")):
        named = getattr(df.groupBy("k"), fn)("h", "u")
        check_frame(named, cols, ["k"], [(f"{stat}(h)", stat, "h"), (f"{stat}(u)", stat, "u")], 2)
        every = getattr(df.groupBy("k", "f"), fn)()
        others = [c for c in df.columns if c not in ("k", "f")]
        assert every.columns == ["k", "f"] + [f"{stat}({c})" for c in others]
    check_frame(df.groupBy("k", "f").max(), cols, ["k", "f"], [(f"max({c})", "max", c) for c in
                                                               ("j", "x", "h", "z", "g", "i", "u")], 2)
    with pytest.raises(ValueError, match="nope"):
        df.groupBy("k").sum("nope")


@pytest.mark.parametrize("keys", [["k"], ["f", "k"], ["j", "f", "k"]])
def test_one_two_and_three_keys(keys):
    cols = _columns(seed=2)
    df = tfs.from_columns(cols, num_partitions=3)
    exprs = [("count(1)", "count", None), ("avg(h)", "avg", "h"), ("stddev_samp(x)", "stddev_samp", "x"),
             ("sum(g)", "sum", "g"), ("min(z)", "min", "z"), ("max(z)", "max", "z"), ("sum(h)", "sum", "h")]
    out = df.groupBy(*keys).agg(F.count("*"), F.avg("h"), F.stddev("x"), F.sum("g"), F.min("z"), F.max("z"),
                                F.sum("h"))
    check_frame(out, cols, keys, exprs, 3)
    assert [out.to_numpy(k).dtype for k in keys] == [cols[k].dtype for k in keys]


def test_frame_agg_without_keys():
    cols = _columns(seed=5)
    cols["z"] = np.where(np.isfinite(cols["z"]), cols["z"], 0.25)
    df = tfs.from_columns(cols, num_partitions=3)
    todo = [F.count("*")] + [fn(v) for v in VALUES for fn in (F.sum, F.avg, F.stddev, F.var_pop, F.min, F.max)]
    out = df.agg(*todo)
    assert out.num_partitions == 1 and out.count() == 1
    assert out.columns == [e.output_name for e in todo]
    n = len(cols["k"])
    for e in todo:
        x = cols[e.column] if e.column is not None else np.zeros(n)
        check_value(out.to_numpy(e.output_name)[0], spec(e.fn, x), e.fn, n, 3, e.output_name)
    via_group = df.groupBy().agg(*todo)
    for c in out.columns:
        same_bits(via_group.to_numpy(c), out.to_numpy(c))
    same_bits(df.agg({"h": "max"}).to_numpy("max(h)"), out.to_numpy("max(h)"))


def test_frames_without_rows():
    df = tfs.from_columns({"k": np.zeros(0, dtype=np.int32), "x": np.zeros(0), "i": np.zeros(0, dtype=np.int32)},
                          num_partitions=2)
    out = df.agg(F.count("*"), F.sum("x"), F.sum("i"), F.avg("x"), F.stddev("x"), F.var_pop("i"))
    same_bits(out.to_numpy("count(1)"), np.array([0], dtype=np.int64))
    same_bits(out.to_numpy("sum(x)"), np.array([0.0]))
    same_bits(out.to_numpy("sum(i)"), np.array([0], dtype=np.int64))
    for c in ("avg(x)", "stddev_samp(x)", "var_pop(i)"):
        assert out.to_numpy(c).dtype == np.float64 and np.isnan(out.to_numpy(c)[0])
    with pytest.raises(ValueError, match=r"min\(x\)"):
        df.agg(F.count("*"), F.min("x"))
    with pytest.raises(ValueError, match=r"max\(i\)"):
        df.agg(F.max("i"))
    keyed = df.groupBy("k").agg(F.count("*"), F.avg("x"), F.max("i"))
    assert keyed.columns == ["k", "count(1)", "avg(x)", "max(i)"] and keyed.count() == 0
    full = tfs.from_columns({"k": np.ones(1, dtype=np.int32), "x": np.ones(1), "i": np.ones(1, dtype=np.int32)})
    assert str(keyed.schema) == str(full.groupBy("k").agg(F.count("*"), F.avg("x"), F.max("i")).schema)
    assert keyed.explain_tensors() == full.groupBy("k").agg(F.count("*"), F.avg("x"), F.max("i")).explain_tensors()
    for b in keyed.local_blocks().values():
        assert b.nrows == 0 and [b.columns[c].dtype for c in keyed.columns] == [torch.int32, torch.int64,
                                                                                 torch.float64, torch.int32]


def test_one_row_groups_and_float_specials():
    cols = _columns()
    df = tfs.from_columns(cols, num_partitions=3)
    out = df.groupBy("k").agg(F.count("*"), F.sum("z"), F.avg("z"), F.stddev("z"), F.variance("z"), F.min("z"),
                              F.max("z"), F.stddev("h"), F.stddev_pop("h"))
    rows = frame_rows(out, ["k"])
    nan, inf = math.nan, math.inf
    one = rows[(7,)]                                                   # the one-row group
    assert one["count(1)"] == 1 and math.isnan(one["stddev_samp(h)"]) and one["stddev_pop(h)"] == 0.0
    assert math.isnan(one["stddev_samp(z)"]) and math.isnan(one["var_samp(z)"])
    for key, want in (((11,), (nan, nan, nan)), ((5,), (inf, inf, nan)), ((2 ** 31 - 1,), (-inf, -inf, nan)),
                      ((-2 ** 31,), (nan, nan, nan))):
        got = (rows[key]["sum(z)"], rows[key]["avg(z)"], rows[key]["stddev_samp(z)"])
        same_bits(np.array(got), np.array(want))
    same_bits(rows[(11,)]["max(z)"], np.float64(nan))                  # NaN is the largest
    same_bits(rows[(5,)]["max(z)"], np.float64(inf))
    same_bits(rows[(-2,)]["min(z)"], np.float64(0.0))                  # -0.0 comes back as 0.0
    same_bits(rows[(-2,)]["max(z)"], np.float64(0.0))
    check_frame(out, cols, ["k"], [(e, e.split("(")[0], e.split("(")[1][:-1] if e != "count(1)" else None)
                                   for e in out.columns[1:]], 3)


def test_int64_sums_wrap_and_large_values_stay_exact():
    base = 2 ** 62
    g = np.array([base - 1, base - 2, base - 3, base - 4, -base, -base + 1, -base - 7, -base + 5,
                  2 ** 53 + 1, 2 ** 53 + 3, 2 ** 60 + 1, -(2 ** 53) - 1], dtype=np.int64)
    k = np.array([0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2], dtype=np.int64)
    for parts in (1, 2, 4):
        out = tfs.from_columns({"k": k, "g": g}, num_partitions=parts).groupBy("k").agg(F.sum("g"), F.min("g"),
                                                                                        F.max("g"))
        want = [int_sum(g[k == j]) for j in range(3)]
        assert want[0] == (4 * base - 10) - 2 ** 64 and want[1] == 2 ** 64 - 4 * base - 1   # both wrapped
        same_bits(out.to_numpy("sum(g)"), np.array(want, dtype=np.int64))
        same_bits(out.to_numpy("min(g)"), np.array([g[k == j].min() for j in range(3)]))
        same_bits(out.to_numpy("max(g)"), np.array([g[k == j].max() for j in range(3)]))
    whole = tfs.from_columns({"k": k, "g": g}, num_partitions=3).agg(F.sum("g"), F.max("g"))
    same_bits(whole.to_numpy("sum(g)"), np.array([int_sum(g)], dtype=np.int64))
    same_bits(whole.to_numpy("max(g)"), np.array([g.max()]))


def test_typed_errors():
    n = 6
    df = tfs.from_columns({"k": np.arange(n, dtype=np.int32), "s": np.array([f"s{i}" for i in range(n)]),
                           "v": np.zeros((n, 3)), "x": np.arange(n, dtype=np.float64)})
    g = df.groupBy("k")
    with pytest.raises(InvalidTypeException, match="string"):
        g.agg(F.sum("s"))
    # a bool column (only row data can hold one)
    rows = tfs.create_dataframe([(True, 1, 1.0), (False, 2, 2.0), (True, 1, 4.5)], ["b", "k", "x"])
    with pytest.raises(InvalidTypeException, match="bool"):
        rows.groupBy("k").agg(F.avg("b"))
    assert rows.groupBy("k").sum().columns == ["k", "sum(x)"]
    with pytest.raises(InvalidDimensionException, match="scalar"):
        g.agg(F.max("v"))
    with pytest.raises(InvalidTypeException, match="aggregate"):
        df.groupBy("s").agg(F.sum("x"))
    with pytest.raises(InvalidTypeException, match="numeric scalar"):
        df.groupBy("v").agg(F.sum("x"))
    with pytest.raises(TypeError, match="withColumn"):
        g.agg(F.sum(df["x"] * 2))
    with pytest.raises(TypeError, match="tfs.functions"):
        g.agg(df["v"].sum())
    with pytest.raises(ValueError, match="nope"):
        g.agg(F.sum("nope"))
    with pytest.raises(ValueError, match="not an aggregate function"):
        g.agg({"x": "mode"})
    with pytest.raises(InvalidTypeException, match="string"):
        df.agg(F.min("s"))
    same_bits(g.agg(F.count("s")).to_numpy("count(s)"), np.ones(n, dtype=np.int64))   # rows, whatever s holds


def test_grouping_is_that_of_count():
    rng = np.random.default_rng(9)
    n = 500
    f = rng.integers(-2, 3, n).astype(np.float32)
    f[::7] = np.nan
    f[3::11] = -0.0
    f[5::13] = 0.0
    d = f.astype(np.float64)
    d[1::17] = np.float64(np.frombuffer(np.uint64(0x7FF8000000000001).tobytes(), dtype=np.float64)[0])  # another NaN
    cols = {"f": f, "d": d, "k": rng.integers(0, 4, n).astype(np.int32), "x": rng.standard_normal(n)}
    for keys in (["f"], ["d"], ["k", "f"], ["d", "k"]):
        for parts in (1, 3):
            df = tfs.from_columns(cols, num_partitions=parts)
            cnt = df.groupBy(*keys).count()
            out = df.groupBy(*keys).agg(F.count("*"), F.count("x"))
            for k in keys:
                same_bits(out.to_numpy(k), cnt.to_numpy(k))
            same_bits(out.to_numpy("count(1)"), cnt.to_numpy("count"))
            same_bits(out.to_numpy("count(x)"), cnt.to_numpy("count"))
            assert int(out.to_numpy("count(1)").sum()) == n


@pytest.mark.parametrize("parts", [1, 3, 7])
def test_any_partitioning_within_the_tolerance(parts):
    cols = _columns(seed=1)
    df = tfs.from_columns(cols, num_partitions=parts)
    before = tfs.metrics.snapshot()
    out = df.groupBy("k").agg(F.sum("h"), F.avg("h"), F.stddev("h"), F.sum("x"), F.avg("x"), F.var_pop("x"),
                              F.sum("i"), F.avg("i"), F.stddev("u"))
    check_frame(out, cols, ["k"], [(c, c.split("(")[0], c.split("(")[1][:-1]) for c in out.columns[1:]], parts)
    after = tfs.metrics.snapshot()
    assert after.get("group_agg_host_partitions", 0) - before.get("group_agg_host_partitions", 0) >= parts
    assert after.get("group_agg_device_partitions", 0) == before.get("group_agg_device_partitions", 0)


def test_textbook_shortcut_is_rejected():
    cols = _columns()
    rows = np.nonzero(cols["k"] == 4)[0]                               # the 3 * 512 + 7 row group
    assert len(rows) >= 65
    x = cols["h"][rows]
    _, m2, _ = exact(x)
    want = math.sqrt(m2 / (len(x) - 1))
    out = tfs.from_columns(cols, num_partitions=2).groupBy("k").agg(F.stddev("h"))
    got = float(out.to_numpy("stddev_samp(h)")[list(out.to_numpy("k")).index(4)])
    assert rel(got, want) <= BOUND
    n = len(x)
    shortcut = math.sqrt(((x * x).sum() - n * x.mean() ** 2) / (n - 1))
    print(f"host path {rel(got, want):.2e}, shortcut {rel(shortcut, want):.2e}")
    assert rel(shortcut, want) > BOUND


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


def sizes_with_gaps(n, nparts):
    """Uneven partition sizes, one of them empty."""
    cuts = sorted({(n * (2 * p + 1)) // (2 * nparts + 1) for p in range(1, nparts)})
    cuts = ([0] + cuts + [n] * nparts)[:nparts] + [n]
    sizes = [b - a for a, b in zip(cuts[:-1], cuts[1:])]
    sizes[2] += sizes[1]                                               # partition 1 gives its rows to partition 2
    sizes[1] = 0
    assert sum(sizes) == n and len(sizes) == nparts
    return sizes


def _spmd_exprs():
    out = [F.count("*")]
    for v in VALUES:
        out += [F.sum(v), F.avg(v), F.stddev(v), F.var_pop(v), F.min(v), F.max(v)]
    return out


def _spmd_results(df):
    out = df.groupBy("k", "f").agg(*_spmd_exprs())
    rows = {repr(key): {n: np.asarray(v).tobytes().hex() for n, v in vals.items()}
            for key, vals in frame_rows(out, ["k", "f"]).items()}
    whole = df.agg(*_spmd_exprs())
    empty = df.filter(df["k"] > 2 ** 31 - 2).filter(df["k"] < 0).groupBy("k").agg(F.avg("x"))
    return {"rows": rows, "owners": sorted(out.local_blocks()), "nparts": out.num_partitions,
            "whole": {c: whole.to_numpy(c).tobytes().hex() for c in whole.columns},
            "whole_owner": sorted(whole.local_blocks()), "empty": [empty.count(), empty.columns]}


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

    assert dist.init(backend="gloo")
    cols = _columns(seed=4)
    res = _spmd_results(frame_of(cols, sizes_with_gaps(len(cols["k"]), 5)))
    with open(os.path.join(outdir, f"r{rank}.json"), "w") as f:
        json.dump(res, f)
    dist.shutdown()


@pytest.mark.parametrize("world", [2, 4])
def test_agg_spmd_has_the_bits_of_one_process(world, tmp_path):
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    outs = [json.load(open(tmp_path / f"r{r}.json")) for r in range(world)]
    cols = _columns(seed=4)
    sizes = sizes_with_gaps(len(cols["k"]), 5)
    assert 0 in sizes and len(set(sizes)) > 2
    single = _spmd_results(frame_of(cols, sizes))                      # one process, the same partitioning
    assert single["owners"] == [0] and single["nparts"] == 1
    rows = {}
    for r, o in enumerate(outs):
        assert o["owners"] == [r] and o["nparts"] == world             # one output partition per rank
        assert not set(o["rows"]) & set(rows)                          # a key lives on one rank
        rows.update(o["rows"])
        assert o["whole"] == single["whole"]                           # the same row on every rank
        assert o["whole_owner"] == ([0] if r == 0 else [])
        assert o["empty"] == [0, ["k", "avg(x)"]]
    assert rows == single["rows"] and len(rows) == len(groups_of(cols, ["k", "f"]))
    assert sum(1 for o in outs if o["rows"]) >= 2                      # the keys do spread over ranks
