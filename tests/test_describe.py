"""`DataFrame.describe` / `summary` / `approxQuantile` on the host path (the
CPU oracle of the device kernels), also under gloo SPMD.

Expected values come from numpy and Python written here, never from the
package: the ordering table of docs/MIGRATION.md (`spec_words`, copied from
tests/test_order_by.py) and exact rational arithmetic (`fractions.Fraction`).

The mean / stddev bound, 1e-11 relative, is derived, not tuned. Columns are
1e4 + N(0, 1), so the condition number of the variance is kappa = mean / std =
1e4. Welford per lane with Chan's pairwise merge above it (the device kernel)
and the two-pass form (the host path) have error about log2(n) * eps * kappa =
14 * 1.1e-16 * 1e4 = 1.5e-11 at worst and far less in practice: a host
prototype of the lane-Welford + pairwise merge stays <= 3.5e-13 on exactly
these inputs. The textbook shortcut, sum(x^2) - n * mean^2, loses kappa^2 =
1e8: on the f64 columns with n >= 65 it is >= 1.7e-9 off. So 1e-11 passes the
intended algorithms with about 30x room and rejects the shortcut by about
100x; `test_mean_and_stddev_against_exact_arithmetic` repeats both checks
(host path: <= 1.3e-13 here; the shortcut: 4.2e-9 .. 8.7e-9)."""
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

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-11
FRAME_DTYPES = [np.uint8, np.int32, np.int64, np.float32, np.float64]  # (the types a frame column can have)
WORD_DTYPES = [np.uint8, np.int8, np.int16, np.int32, np.int64, np.float32, np.float64]
PROBS = [0.0, 0.1, 0.25, 0.5, 0.75, 0.9, 1.0]


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


def spec_order(words) -> np.ndarray:
    """words: [uint64 [n]], most significant first -> stable permutation."""
    return np.lexsort(list(words)[::-1])


def canonical(v):
    """What a word decodes to: -0.0 as 0.0, every NaN as the quiet NaN."""
    v = np.asarray(v)
    if v.dtype.kind != "f":
        return v
    out = np.where(np.isnan(v), np.array(np.nan, dtype=v.dtype), v + v.dtype.type(0.0))
    return out.astype(v.dtype)


def spec_quantiles(x: np.ndarray, probs) -> np.ndarray:
    """The rows at 0-based positions max(ceil(p N) - 1, 0) of orderBy's order, canonical."""
    s = x[spec_order([spec_words(x)])]
    return canonical(s[[max(math.ceil(p * len(x)) - 1, 0) for p in probs]])


def same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), (got, want)


def as_doubles(v) -> np.ndarray:
    return np.array([float(t) for t in np.asarray(v).reshape(-1)], dtype=np.float64)


_EXACT = {}


def exact_mean_std(x: np.ndarray):
    """(mean, sample stddev) of the f64-converted data in exact rational arithmetic."""
    key = (x.dtype.str, x.tobytes())
    if key not in _EXACT:
        fx = [Fraction(float(v)) for v in x.astype(np.float64)]
        n = len(fx)
        mean = sum(fx) / n
        m2 = sum((v - mean) ** 2 for v in fx)
        _EXACT[key] = (float(mean), math.sqrt(float(m2 / (n - 1))) if n > 1 else math.nan)
    return _EXACT[key]


def rel(got: float, want: float) -> float:
    return abs(got - want) / abs(want)


def frame_of(cols, sizes):
    """A frame whose partition p holds sizes[p] rows (zero allowed), this rank's partitions only."""
    from tensorframes_amd.frame.block import Block, StringColumn
    from tensorframes_amd.frame.dataframe import DataFrame, _Materialized
    from tensorframes_amd.parallel import dist
    n = len(next(iter(cols.values())))
    assert sum(sizes) == n
    schema = tfs.from_columns({k: v[:1] for k, v in cols.items()}, num_partitions=1).schema
    starts = np.concatenate([[0], np.cumsum(sizes)])
    blocks = {}
    for p in dist.local_partitions(len(sizes)):
        a, b = int(starts[p]), int(starts[p + 1])
        blocks[p] = Block(b - a, {k: StringColumn.from_numpy(v[a:b]) if v.dtype.kind == "U"
                                  else torch.from_numpy(np.ascontiguousarray(v[a:b])) for k, v in cols.items()})
    return DataFrame(schema, _Materialized(blocks), len(sizes))


def sizes_with_gaps(n, nparts):
    """Uneven partition sizes, one of them empty when there are three or more."""
    if nparts == 1:
        return [n]
    cuts = sorted({(n * (2 * p + 1)) // (2 * nparts + 1) for p in range(1, nparts)})
    cuts = ([0] + cuts + [n] * nparts)[:nparts] + [n]
    sizes = [b - a for a, b in zip(cuts[:-1], cuts[1:])]
    if nparts >= 3:                                       # partition 1 gives its rows to partition 2
        sizes[2] += sizes[1]
        sizes[1] = 0
    assert sum(sizes) == n and len(sizes) == nparts
    return sizes


def table(out):
    """{label: {column: double}} of a describe / summary frame."""
    labels = out.to_numpy("summary").tolist()
    return labels, {c: dict(zip(labels, out.to_numpy(c).tolist())) for c in out.columns if c != "summary"}


def values(dtype, n, seed):
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    if dt.kind == "f":
        x = rng.standard_normal(n).astype(dt)
        fi = np.finfo(dt)
        special = [np.nan, np.inf, -np.inf, 0.0, -0.0, fi.tiny / 4, -fi.tiny / 4, fi.max, -np.nan]
        if n >= 4:
            for j, s in enumerate(special[:max(n // 2, 1)]):
                x[(j * 7) % n] = s
        return x
    ii = np.iinfo(dt)
    x = rng.integers(ii.min, ii.max, n, dtype=dt, endpoint=True)
    if n >= 4:
        x[0], x[n // 2] = ii.max, ii.min
    return x


def passes_of(fn):
    before = tfs.metrics.snapshot().get("quantile_passes", 0)
    res = fn()
    return res, tfs.metrics.snapshot().get("quantile_passes", 0) - before


# ------------------------------------------------------------------ call forms
def mixed_frame(n=40, nparts=3):
    rng = np.random.default_rng(3)
    cols = {"a": rng.standard_normal(n).astype(np.float32), "k": rng.integers(-9, 9, n).astype(np.int32),
            "s": np.array([f"s{i}" for i in range(n)]),
            "v": rng.standard_normal((n, 3)).astype(np.float32), "d": rng.standard_normal(n)}
    return tfs.from_columns(cols, num_partitions=nparts), cols


def test_describe_call_forms_and_schema():
    df, cols = mixed_frame()
    out = df.describe()
    assert out.num_partitions == 1
    assert out.dtypes == [("summary", "string"), ("a", "double"), ("k", "double"), ("d", "double")]
    labels, t = table(out)
    assert labels == ["count", "mean", "stddev", "min", "max"]
    for c in ("a", "k", "d"):
        x = cols[c].astype(np.float64)
        assert t[c]["count"] == 40.0 and t[c]["min"] == x.min() and t[c]["max"] == x.max()
        assert t[c]["mean"] == pytest.approx(x.mean(), rel=1e-12)
        assert t[c]["stddev"] == pytest.approx(x.std(ddof=1), rel=1e-12)
    one = df.describe("a")
    assert one.dtypes == [("summary", "string"), ("a", "double")]
    same_bits(one.to_numpy("a"), out.to_numpy("a"))
    two = df.describe(["d", "a"])
    assert two.columns == ["summary", "d", "a"]
    rows = out.collect()
    assert [r.summary for r in rows] == labels and rows[0].k == 40.0


def test_summary_call_forms():
    df, cols = mixed_frame()
    out = df.summary()
    assert out.dtypes == [("summary", "string"), ("a", "double"), ("k", "double"), ("d", "double")]
    labels, t = table(out)
    assert labels == ["count", "mean", "stddev", "min", "25%", "50%", "75%", "max"]
    for c in ("a", "k", "d"):
        q = spec_quantiles(cols[c], [0.25, 0.5, 0.75])
        same_bits(np.array([t[c]["25%"], t[c]["50%"], t[c]["75%"]]), as_doubles(q))
    few = df.summary("count", "5%", "max")
    labels, t = table(few)
    assert labels == ["count", "5%", "max"]
    assert t["k"]["5%"] == float(spec_quantiles(cols["k"], [0.05])[0]) and t["k"]["max"] == float(cols["k"].max())
    labels, t = table(df.summary("12.5%", "100%", "0%"))
    assert labels == ["12.5%", "100%", "0%"]
    assert t["d"]["12.5%"] == float(spec_quantiles(cols["d"], [0.125])[0])
    assert t["d"]["100%"] == cols["d"].max() and t["d"]["0%"] == cols["d"].min()
    for bad in ("median", "101%", "-1%", "%", "x%"):
        with pytest.raises(ValueError, match="not a statistic"):
            df.summary(bad)


def test_approx_quantile_call_forms():
    df, cols = mixed_frame()
    want_a = as_doubles(spec_quantiles(cols["a"], [0.25, 0.5, 0.75])).tolist()
    want_k = as_doubles(spec_quantiles(cols["k"], [0.25, 0.5, 0.75])).tolist()
    got = df.approxQuantile("a", [0.25, 0.5, 0.75], 0.0)
    assert isinstance(got, list) and all(type(v) is float for v in got) and got == want_a
    assert df.approxQuantile(["a", "k"], [0.25, 0.5, 0.75], 0.01) == [want_a, want_k]
    assert df.approxQuantile(("k",), [0.25, 0.5, 0.75], 0.5) == [want_k]
    assert df.stat.approxQuantile("a", [0.25, 0.5, 0.75], 0.0) == want_a
    assert df.stat.approx_quantile("k", [0.25, 0.5, 0.75], 0.0) == want_k
    assert df.approx_quantile("a", [0.25, 0.5, 0.75], 1.0) == want_a
    assert df.approxQuantile("a", [], 0.0) == []


def test_ineligible_columns_are_skipped_by_default_and_refused_by_name():
    df, _ = mixed_frame()
    assert df.describe().columns == ["summary", "a", "k", "d"]
    assert df.summary("count").columns == ["summary", "a", "k", "d"]
    for call in (df.describe, lambda c: df.approxQuantile(c, [0.5], 0.0),
                 lambda c: df.approxQuantile(["a", c], [0.5], 0.0)):
        with pytest.raises(InvalidTypeException, match="string column"):
            call("s")
        with pytest.raises(InvalidDimensionException, match=r"reduce the cell first \(\.sum\(\)"):
            call("v")
        with pytest.raises(ValueError, match="nope"):
            call("nope")
    # a bool column (only row data can hold one) next to a string and a double
    rows = tfs.create_dataframe([(True, "p", 1.0), (False, "q", 2.0), (True, "r", 4.5)], ["b", "s", "x"])
    assert rows.describe().columns == ["summary", "x"]
    assert rows.approxQuantile("x", [0.5], 0.0) == [2.0]
    for call in (rows.describe, lambda c: rows.approxQuantile(c, [0.5], 0.0)):
        with pytest.raises(InvalidTypeException, match="bool"):
            call("b")
        with pytest.raises(InvalidTypeException, match="string column"):
            call("s")
    # a reduced cell is a scalar column
    red = df.select(df.v.sum().alias("vs"))
    assert red.describe().columns == ["summary", "vs"]


# ------------------------------------------------------------------ mean / stddev
def centred(dtype, n):
    return (1e4 + np.random.default_rng(n).standard_normal(n)).astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [2, 65, 4097, 3 * 4096 + 7])
def test_mean_and_stddev_against_exact_arithmetic(dtype, n):
    x = centred(dtype, n)
    mean, std = exact_mean_std(x)
    for nparts in (1, 4, 7):
        _, t = table(tfs.from_columns({"x": x}, num_partitions=nparts).describe())
        em, es = rel(t["x"]["mean"], mean), rel(t["x"]["stddev"], std)
        print(f"{np.dtype(dtype).name} n={n} nparts={nparts}: mean {em:.2e} stddev {es:.2e}")
        assert em <= BOUND and es <= BOUND
        assert t["x"]["count"] == float(n)
    if dtype == np.float64 and n >= 65:
        # the same bound rejects the textbook shortcut, sum(x^2) - n mean^2 in f64, by two orders
        shortcut = math.sqrt(((x * x).sum() - n * x.mean() ** 2) / (n - 1))
        print(f"n={n}: shortcut stddev {rel(shortcut, std):.2e}")
        assert rel(shortcut, std) > 100 * BOUND


# ------------------------------------------------------------------ exact values
@pytest.mark.parametrize("dtype", WORD_DTYPES)
def test_decode_sort_word_inverts_the_table(dtype):
    from tensorframes_amd.frame._scalar_columns import _decode_sort_word
    dt = np.dtype(dtype)
    if dt.kind == "f":
        fi = np.finfo(dt)
        x = np.array([0.0, 1.5, -1.5, np.inf, -np.inf, fi.tiny, -fi.tiny, fi.tiny / 8, -fi.tiny / 8,
                      fi.smallest_subnormal, -fi.smallest_subnormal, fi.max, fi.min, fi.eps], dtype=dt)
    else:
        ii = np.iinfo(dt)
        x = np.array([ii.min, ii.min + 1, -1 if ii.min < 0 else 1, 0, 1, ii.max - 1, ii.max], dtype=dt)
    v = values(dtype, 50, 1)
    if dt.kind == "f":
        v = v[~np.isnan(v) & ~((v == 0) & np.signbit(v))]          # (NaN and -0.0 canonicalise: below)
    x = np.concatenate([x, v])
    same_bits(_decode_sort_word(spec_words(x), dt), x)
    one = _decode_sort_word(int(spec_words(x[1:2])[0]), dt)
    assert one.dtype == dt and one.tobytes() == x[1:2].tobytes()
    same_bits(_decode_sort_word(spec_words(x), torch.from_numpy(x).dtype), x)          # a torch dtype too
    if dt.kind == "f":
        ubits = np.uint32 if dt == np.float32 else np.uint64
        odd = np.array([-0.0, np.nan, -np.nan], dtype=dt)
        payload = np.array([0x7F800001 if dt == np.float32 else 0x7FF0000000000001], dtype=ubits).view(dt)
        odd = np.concatenate([odd, payload])
        got = _decode_sort_word(spec_words(odd), dt)
        quiet = np.array([0x7FC00000 if dt == np.float32 else 0x7FF8000000000000], dtype=ubits).view(dt)[0]
        same_bits(got, np.array([0.0, quiet, quiet, quiet], dtype=dt))


@pytest.mark.parametrize("dtype", FRAME_DTYPES)
def test_count_min_max_are_exact(dtype):
    from tensorframes_amd.frame import stats
    dt = np.dtype(dtype)
    x = values(dtype, 203, 5)
    s = x[spec_order([spec_words(x)])]
    for nparts in (1, 4):
        df = frame_of({"x": x}, sizes_with_gaps(len(x), nparts))
        # the decoded words, before the double conversion (int64 extremes round as doubles)
        mom = stats._moments(df, df.local_blocks(), ["x"], "test")
        assert mom.n == [203]
        same_bits(np.array(mom.extreme(0, "min")), canonical(s[0]))
        same_bits(np.array(mom.extreme(0, "max")), canonical(s[-1]))
        _, t = table(df.describe())
        same_bits(np.array([t["x"]["count"], t["x"]["min"], t["x"]["max"]]),
                  np.array([203.0, float(canonical(s[0])), float(canonical(s[-1]))]))
    if dt.kind == "f":
        # NaN sorts last, so it is the max; a NaN or an infinity propagates into mean and stddev
        _, t = table(tfs.from_columns({"x": x}, num_partitions=2).describe())
        assert math.isnan(t["x"]["max"]) and t["x"]["min"] == -math.inf
        assert math.isnan(t["x"]["mean"]) and math.isnan(t["x"]["stddev"])
        y = np.array([1.0, np.inf, 2.0, 3.0], dtype=dt)
        for nparts in (1, 2, 4):
            _, t = table(tfs.from_columns({"y": y}, num_partitions=nparts).describe())
            assert t["y"]["mean"] == math.inf and math.isnan(t["y"]["stddev"]) and t["y"]["max"] == math.inf
    if dt == np.int64:
        ii = np.iinfo(np.int64)
        assert x.max() == ii.max and x.min() == ii.min
        assert t["x"]["max"] == float(ii.max) and t["x"]["min"] == float(ii.min)


# ------------------------------------------------------------------ quantiles
@pytest.mark.parametrize("dtype", FRAME_DTYPES)
@pytest.mark.parametrize("n", [1, 4, 5, 100, 12295])
def test_quantiles_match_the_sorted_order(dtype, n):
    x = values(dtype, n, 11 + n)
    want = as_doubles(spec_quantiles(x, PROBS))
    for nparts in (1, 3, 8):
        df = frame_of({"x": x}, sizes_with_gaps(n, nparts))
        same_bits(np.array(df.approxQuantile("x", PROBS, 0.0)), want)
    # every relativeError returns the exact value
    same_bits(np.array(tfs.from_columns({"x": x}, num_partitions=2).approxQuantile("x", PROBS, 0.25)), want)


@pytest.mark.parametrize("dtype", FRAME_DTYPES)
def test_quantiles_inside_runs_of_equal_values(dtype):
    dt = np.dtype(dtype)
    five = np.array([3, 250, 7, 0, 64], dtype=dt) if dt.kind != "f" else np.array([-2.5, 0.0, 1e-3, 7.0, np.inf], dtype=dt)
    x = np.random.default_rng(2).choice(five, 1000)
    want = as_doubles(spec_quantiles(x, PROBS))
    for nparts in (1, 3, 8):
        same_bits(np.array(frame_of({"x": x}, sizes_with_gaps(1000, nparts)).approxQuantile("x", PROBS, 0.0)), want)
    same = np.full(77, five[1], dtype=dt)
    df = tfs.from_columns({"x": same}, num_partitions=3)
    got, passes = passes_of(lambda: df.approxQuantile("x", PROBS, 0.0))
    assert got == [float(five[1])] * len(PROBS) and passes == 0       # an all-equal column: no pass at all


def test_pass_counts():
    rng = np.random.default_rng(8)
    n = 5000
    cols = {"k": rng.integers(0, 1000, n).astype(np.int32), "x": rng.standard_normal(n).astype(np.float32),
            "g": rng.integers(np.iinfo(np.int64).min, np.iinfo(np.int64).max, n, dtype=np.int64, endpoint=True)}
    cols["g"][:2] = [np.iinfo(np.int64).min, np.iinfo(np.int64).max]
    df = tfs.from_columns(cols, num_partitions=4)
    for name, check in (("k", lambda p: p == 2), ("x", lambda p: 1 <= p <= 4), ("g", lambda p: p == 8)):
        got, passes = passes_of(lambda: df.approxQuantile(name, [0.1, 0.5, 0.9], 0.0))
        assert check(passes), (name, passes)                       # per column and pass, not per partition
        same_bits(np.array(got), as_doubles(spec_quantiles(cols[name], [0.1, 0.5, 0.9])))
    before = tfs.metrics.snapshot().get("stats_rows", 0)
    df.describe().count()
    assert tfs.metrics.snapshot().get("stats_rows", 0) - before == 3 * n   # rows read by moments, per column


# ------------------------------------------------------------------ edge cases
def test_empty_frame_and_single_row():
    empty = tfs.from_columns({"x": np.zeros(0, dtype=np.float32), "k": np.zeros(0, dtype=np.int64)}, num_partitions=2)
    labels, t = table(empty.describe())
    for c in ("x", "k"):
        assert t[c]["count"] == 0.0
        assert all(math.isnan(t[c][s]) for s in ("mean", "stddev", "min", "max"))
    assert empty.approxQuantile("x", [0.5], 0.0) == [] and empty.approxQuantile(["x", "k"], [0.1, 0.9], 0.0) == [[], []]
    _, t = table(empty.summary())
    assert t["x"]["count"] == 0.0 and math.isnan(t["x"]["50%"])
    one = tfs.from_columns({"x": np.array([2.5], dtype=np.float64)}, num_partitions=3)
    _, t = table(one.describe())
    assert t["x"] == pytest.approx({"count": 1.0, "mean": 2.5, "stddev": math.nan, "min": 2.5, "max": 2.5}, nan_ok=True)
    assert math.isnan(t["x"]["stddev"])
    assert one.approxQuantile("x", [0.0, 0.5, 1.0], 0.0) == [2.5, 2.5, 2.5]


def test_argument_errors():
    df, _ = mixed_frame()
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        df.approxQuantile("a", [0.5, 1.5], 0.0)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        df.approxQuantile("a", [-0.1], 0.0)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        df.approxQuantile("a", [math.nan], 0.0)
    with pytest.raises(ValueError, match="relativeError"):
        df.approxQuantile("a", [0.5], -1)
    with pytest.raises(ValueError, match="at most 16"):
        df.approxQuantile("a", [i / 16 for i in range(17)], 0.0)
    assert len(df.approxQuantile("a", [i / 15 for i in range(16)], 0.0)) == 16
    with pytest.raises(TypeError):
        df.approxQuantile("a", 0.5, 0.0)
    with pytest.raises(TypeError):
        df.approxQuantile(3, [0.5], 0.0)
    with pytest.raises(ValueError, match="at most 16"):
        df.summary(*[f"{i}%" for i in range(17)])
    with pytest.raises(ValueError, match="summary"):
        tfs.from_columns({"summary": np.arange(3.0)}).describe()


# ------------------------------------------------------------------ several ranks
def _spmd_columns():
    n = 997
    rng = np.random.default_rng(33)
    x = (1e4 + rng.standard_normal(n)).astype(np.float32)
    z = rng.standard_normal(n)
    z[::41] = np.nan
    z[3::97] = -0.0
    return {"x": x, "z": z, "k": rng.integers(0, 1000, n).astype(np.int32),
            "g": rng.integers(-2 ** 62, 2 ** 62, n).astype(np.int64), "u": rng.integers(0, 256, n).astype(np.uint8),
            "s": np.array([f"row-{i}" for i in range(n)])}


def _spmd_results(df):
    d, s = df.describe(), df.summary("count", "mean", "stddev", "min", "1%", "50%", "99.5%", "max")
    res = {"describe": {c: d.to_numpy(c).tobytes().hex() for c in d.columns if c != "summary"},
           "summary": {c: s.to_numpy(c).tobytes().hex() for c in s.columns if c != "summary"},
           "labels": d.to_numpy("summary").tolist() + s.to_numpy("summary").tolist(),
           "owner": sorted(d.local_blocks()),
           "q": np.array(df.approxQuantile(["x", "z", "k", "g", "u"], PROBS, 0.0)).tobytes().hex(),
           "q1": np.array(df.stat.approxQuantile("z", [0.33], 0.1)).tobytes().hex()}
    return res


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
    cols = _spmd_columns()
    res = _spmd_results(frame_of(cols, sizes_with_gaps(len(cols["s"]), 5)))
    with open(os.path.join(outdir, f"r{rank}.json"), "w") as f:
        json.dump(res, f)
    dist.shutdown()


@pytest.mark.parametrize("world", [2, 4])
def test_describe_spmd(world, tmp_path):
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    outs = [json.load(open(tmp_path / f"r{r}.json")) for r in range(world)]
    cols = _spmd_columns()
    sizes = sizes_with_gaps(len(cols["s"]), 5)
    assert 0 in sizes and len(set(sizes)) > 2
    single = _spmd_results(frame_of(cols, sizes))                 # one process, the same partitioning
    for r, o in enumerate(outs):
        assert o["owner"] == ([0] if r == 0 else [])              # one partition, owned as every partition 0 is
        for key in ("describe", "summary", "labels", "q", "q1"):
            assert o[key] == single[key], (r, key)
    want = np.stack([as_doubles(spec_quantiles(cols[c], PROBS)) for c in ("x", "z", "k", "g", "u")])
    assert single["q"] == want.tobytes().hex()
