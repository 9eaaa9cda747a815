"""`DataFrame.sample` / `randomSplit` / `sampleBy` and `F.rand` / `F.randn` on
host frames (frame/sampling.py): the generator, the kept rows, the typed
errors, and that the result does not depend on the partitioning or the number
of ranks.

Every expected value comes from the Philox4x32-10 written here from its
definition, on Python ints: u is an integer x over 2^53, and a comparison with
a float bound f is the integer comparison with ceil(f * 2^53) (exact, through
`Fraction`). Poisson counts are looked up in a table built here with the
documented recurrence. Kept rows, counts and `rand` are compared exactly.
`randn` is held to 2^-48 * max(1, r), r = sqrt(-2 ln u1): r carries a relative
error of a few ulp of log halved by sqrt (at most 2^-51), cos an absolute
error of at most 2^-50 from the rounded argument plus 2^-51 from the function;
the sum is at most r * 2^-49 and the bound doubles it."""
import bisect
import functools
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
from tensorframes_amd import functions as F
from tensorframes_amd.frame import sampling

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = 0xFFFFFFFF
N = 1000
SEEDS = [0, 1, -1, 2 ** 64 - 1]


# ------------------------------------------------------------------ the specification
def philox(counter, key):
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for r in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        if r < 9:
            k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


KNOWN = [(((0, 0, 0, 0), (0, 0)), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
         (((M32,) * 4, (M32,) * 2), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
         (((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)),
          (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]


@functools.lru_cache(maxsize=None)
def words(seed, purpose, n=N):
    """The four words of the global rows 0 .. n under `seed` (any Python int)."""
    seed %= 2 ** 64
    key = (seed & M32, seed >> 32)
    return [philox((i & M32, i >> 32, purpose, 0), key) for i in range(n)]


def x53(a, b):
    return ((a << 32) | b) >> 11


def u_ints(seed, purpose=0, n=N):
    return [x53(w[0], w[1]) for w in words(seed, purpose, n)]


def thr(f):
    """The int t with (u >= f) == (x >= t) and (u < f) == (x < t) for u = x * 2^-53."""
    return math.ceil(Fraction(f) * 2 ** 53)


def poisson_cdf(lam):
    term = math.exp(-lam)
    cdf = [term]
    j = 0
    while cdf[-1] < 1.0 - 2.0 ** -53 and len(cdf) < 64:
        j += 1
        term *= lam / j
        cdf.append(cdf[-1] + term)
    return cdf


def bounds_of(weights):
    total = 0.0
    for w in weights:
        total += float(w)
    run, out = 0.0, [0.0]
    for w in weights:
        run += float(w)
        out.append(run / total)
    out[-1] = 1.0
    return out


# ------------------------------------------------------------------ frames
def base_columns(n=N):
    rng = np.random.default_rng(21)
    return {"i": np.arange(n, dtype=np.int64), "k": rng.integers(-2, 4, n).astype(np.int32),
            "x": rng.standard_normal(n).astype(np.float32)}


def frame_of(cols, nparts, empty=()):
    """The rows of cols in nparts partitions; the partitions `empty` hold no
    rows (their rows are dropped with filter before, so the row sequence of
    the frame is what is left). -> (frame, the columns it holds)"""
    n = len(cols["i"])
    edges = [(p * n) // nparts for p in range(nparts + 1)]
    keep = np.ones(n, dtype=bool)
    for p in empty:
        keep[edges[p]:edges[p + 1]] = False
    df = tfs.from_columns(dict(cols, keep=keep.astype(np.int32)), num_partitions=nparts)
    df = df.filter(df.keep > 0).select(*cols)
    return df, {c: v[keep] for c, v in cols.items()}


def even_frame(cols, nparts):
    return tfs.from_columns(cols, num_partitions=nparts)


def partition_rows(df):
    return [b.nrows for _, b in sorted(df.local_blocks().items())]


def kept_per_partition(sizes, mask):
    out, a = [], 0
    for s in sizes:
        out.append(int(np.sum(mask[a:a + s])))
        a += s
    return out


# ------------------------------------------------------------------ the generator
def test_known_answers():
    for (counter, key), want in KNOWN:
        assert philox(counter, key) == want
        got = sampling.philox4x32_10(*counter, *key)
        assert tuple(int(g) for g in got) == want


def test_numpy_philox_equals_the_specification_on_random_inputs():
    rng = np.random.default_rng(0)
    c = rng.integers(0, 2 ** 32, (1000, 4), dtype=np.uint64)
    k = rng.integers(0, 2 ** 32, (1000, 2), dtype=np.uint64)
    got = np.stack(sampling.philox4x32_10(c[:, 0], c[:, 1], c[:, 2], c[:, 3], k[:, 0], k[:, 1]), 1)
    want = [philox(tuple(int(v) for v in c[j]), tuple(int(v) for v in k[j])) for j in range(1000)]
    assert got.dtype == np.uint64 and got.tolist() == [list(w) for w in want]


def test_poisson_table_follows_the_documented_recurrence():
    for lam in (0.0, 0.3, 1.0, 16.0):
        assert sampling.poisson_cdf(lam) == poisson_cdf(lam)
    assert poisson_cdf(0.0) == [1.0] and len(poisson_cdf(16.0)) == 64
    assert sampling.split_bounds([3, 1, 1]) == bounds_of([3, 1, 1]) == [0.0, 0.6, 0.8, 1.0]


# ------------------------------------------------------------------ sample
PARTITIONINGS = [(1, ()), (3, ()), (7, ()), (3, (0,)), (7, (3,)), (7, (6,)), (7, (0, 3, 6))]


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("fraction", [0.0, 1.0, 0.5, 1e-3])
def test_sample_keeps_exactly_the_rows_below_the_fraction(seed, fraction):
    cols = base_columns()
    for nparts, empty in PARTITIONINGS:
        df, held = frame_of(cols, nparts, empty)
        n = len(held["i"])
        mask = np.array([x < thr(fraction) for x in u_ints(seed)[:n]])
        out = df.sample(fraction, seed)
        assert out.num_partitions == nparts and out.columns == df.columns
        assert partition_rows(out) == kept_per_partition(partition_rows(df), mask)
        for c in held:
            got = out.to_numpy(c)
            assert got.tobytes() == held[c][mask].tobytes() or (not mask.any() and got.size == 0), (nparts, empty, c)
    if fraction == 0.0:
        assert out.count() == 0
    if fraction == 1.0:
        assert out.count() == n


def test_sample_is_the_same_for_the_three_partitionings_and_all_call_forms():
    cols = base_columns()
    want = None
    for nparts in (1, 3, 7):
        df = even_frame(cols, nparts)
        for out in (df.sample(0.5, 3), df.sample(False, 0.5, 3), df.sample(fraction=0.5, seed=3),
                    df.sample(0.5, seed=3),
                    df.sample(withReplacement=False, fraction=0.5, seed=3)):
            got = out.to_numpy("i").tolist()
            want = got if want is None else want
            assert got == want
    assert want == [i for i, x in enumerate(u_ints(3)) if x < thr(0.5)]
    assert 0 < even_frame(cols, 3).sample(0.25).count() < N


# ------------------------------------------------------------------ randomSplit
@pytest.mark.parametrize("seed", SEEDS)
def test_random_split_partitions_the_rows(seed):
    cols = base_columns()
    b = bounds_of([3, 1, 1])
    xs = u_ints(seed)
    for nparts, empty in PARTITIONINGS[1:5]:
        df, held = frame_of(cols, nparts, empty)
        n = len(held["i"])
        splits = df.randomSplit([3, 1, 1], seed)
        assert len(splits) == 3
        got = [s.to_numpy("i").astype(np.int64) for s in splits]
        for j, g in enumerate(got):
            mask = np.array([thr(b[j]) <= x < thr(b[j + 1]) for x in xs[:n]])
            assert g.tolist() == held["i"][mask].tolist()
            assert splits[j].to_numpy("x").tobytes() == held["x"][mask].tobytes() or g.size == 0
        allrows = np.concatenate(got)
        assert len(set(allrows.tolist())) == len(allrows) == n
        assert sorted(allrows.tolist()) == held["i"].tolist()


def test_random_split_single_weight_returns_the_input():
    cols = base_columns()
    df = even_frame(cols, 3)
    (only,) = df.randomSplit([2.5], 11)
    assert partition_rows(only) == partition_rows(df)
    for c in cols:
        assert only.to_numpy(c).tobytes() == cols[c].tobytes()


# ------------------------------------------------------------------ sampleBy
def spec_word(v):
    """What makes two keys one stratum: NaN is NaN, -0.0 is 0.0."""
    v = v.item() if hasattr(v, "item") else v
    if isinstance(v, float):
        return "nan" if math.isnan(v) else (0.0 if v == 0.0 else v)
    return v


def by_cases():
    rng = np.random.default_rng(5)
    f32 = rng.choice(np.array([np.nan, -0.0, 0.0, 1.5, -2.25, 7.0], dtype=np.float32), N)
    f64 = rng.choice(np.array([np.nan, -0.0, 0.0, 1.5, 1e300, -3.0], dtype=np.float64), N)
    return [
        (rng.integers(-2, 4, N).astype(np.int32), {-2: 1.0, 0: 0.5, 3: 0.0, 99: 1.0}),
        (rng.choice(np.array([-2 ** 62, -1, 0, 5, 2 ** 62], dtype=np.int64), N),
         {-2 ** 62: 0.7, 2 ** 62: 1.0, 5: 0.25}),
        (f32, {float("nan"): 0.6, -0.0: 1.0, 1.5: 0.5, -2.25: 0.0}),
        (f32, {0.0: 0.5}),
        (f64, {float("nan"): 1.0, 0.0: 0.3, 1e300: 0.9}),
    ]


@pytest.mark.parametrize("ci", range(5))
def test_sample_by_against_brute_force(ci):
    keys, fractions = by_cases()[ci]
    seed = SEEDS[ci % 4]
    cols = {"i": np.arange(N, dtype=np.int64), "key": keys}
    look = {spec_word(k if not isinstance(k, float) else keys.dtype.type(k)): thr(f) for k, f in fractions.items()}
    want = None
    for nparts, empty in [(1, ()), (3, ()), (7, (0, 3, 6))]:
        df, held = frame_of(cols, nparts, empty)
        xs = u_ints(seed)[:len(held["i"])]
        mask = np.array([x < look.get(spec_word(k), 0) for x, k in zip(xs, held["key"])])
        for out in (df.sampleBy("key", fractions, seed), df.stat.sampleBy("key", fractions, seed)):
            assert out.to_numpy("i").tolist() == held["i"][mask].tolist()
            assert out.to_numpy("key").tobytes() == held["key"][mask].tobytes()
        if not empty:
            want = held["i"][mask].tolist() if want is None else want
            assert held["i"][mask].tolist() == want
    assert 0 < len(want) < N
    listed = {spec_word(keys.dtype.type(k)) for k, f in fractions.items() if f > 0}
    assert {spec_word(k) for k in keys[np.array(want)]} <= listed          # keys not listed are dropped
    full = {spec_word(keys.dtype.type(k)) for k, f in fractions.items() if f == 1.0}
    if full:
        assert sum(spec_word(k) in full for k in keys) == sum(spec_word(k) in full for k in keys[np.array(want)])


def test_sample_by_nothing_listed_keeps_nothing():
    df = even_frame(base_columns(), 3)
    out = df.sampleBy("k", {}, 1)
    assert out.count() == 0 and out.columns == df.columns


# ------------------------------------------------------------------ with replacement
@pytest.mark.parametrize("lam", [0.0, 0.3, 1.0, 16.0])
def test_sample_with_replacement_repeats_rows_by_the_table(lam):
    cols = base_columns()
    ts = [thr(c) for c in poisson_cdf(lam)]  # (c <= u) == (thr(c) <= x)
    for seed in (0, -1):
        counts = np.array([bisect.bisect_right(ts, x) for x in u_ints(seed, 2)], dtype=np.int64)
        want = None
        for nparts, empty in [(1, ()), (3, ()), (7, (0, 3, 6))]:
            df, held = frame_of(cols, nparts, empty)
            n = len(held["i"])
            out = df.sample(True, lam, seed)
            rep = np.repeat(np.arange(n), counts[:n])
            assert out.columns == df.columns and out.num_partitions == nparts
            assert out.to_numpy("i").astype(np.int64).tolist() == held["i"][rep].tolist()   # consecutive, in order
            assert out.to_numpy("x").astype(np.float32).tobytes() == held["x"][rep].tobytes()
            sizes = partition_rows(df)
            assert partition_rows(out) == [int(counts[a:a + s].sum()) for a, s in
                                           zip(np.cumsum([0] + sizes[:-1]).tolist(), sizes)]
    if lam == 0.0:
        assert out.count() == 0 and [f.name for f in out.schema.fields] == ["i", "k", "x"]
        assert out.schema["x"].dataType == df.schema["x"].dataType
    else:
        assert counts.max() >= 1 and (lam < 1 or counts.max() >= 2)


# ------------------------------------------------------------------ rand / randn
def test_rand_is_u_bit_for_bit_and_randn_within_the_bound():
    cols = base_columns()
    for seed in SEEDS:
        u = np.array([x * 2.0 ** -53 for x in u_ints(seed)])
        zs, bound = [], []
        for w in words(seed, 1):
            u1, u2 = (x53(w[0], w[1]) + 1) * 2.0 ** -53, x53(w[2], w[3]) * 2.0 ** -53
            r = math.sqrt(-2.0 * math.log(u1))
            zs.append(r * math.cos(2.0 * math.pi * u2))
            bound.append(2.0 ** -48 * max(1.0, r))
        for nparts in (1, 3, 7):
            df = even_frame(cols, nparts)
            out = df.withColumn("r", F.rand(seed)).withColumn("z", F.randn(seed))
            assert out.columns == ["i", "k", "x", "r", "z"] and partition_rows(out) == partition_rows(df)
            r = out.to_numpy("r")
            assert r.dtype == np.float64 and r.tobytes() == u.tobytes()
            z = out.to_numpy("z")
            assert z.dtype == np.float64 and np.all(np.abs(z - np.array(zs)) <= np.array(bound))
            for c in cols:
                assert out.to_numpy(c).tobytes() == cols[c].tobytes()
    assert u.min() >= 0.0 and u.max() < 1.0


def test_rand_in_select_and_with_column():
    df, held = frame_of(base_columns(), 7, (0, 3, 6))
    out = df.select("i", F.rand(4).alias("a"), F.rand(5).alias("b"), F.rand(4).alias("c"), F.randn(4))
    assert out.columns == ["i", "a", "b", "c", "randn(4)"]
    a, b, c = out.to_numpy("a"), out.to_numpy("b"), out.to_numpy("c")
    assert a.tobytes() == c.tobytes() and not np.array_equal(a, b)      # the same seed, another seed
    assert a.tobytes() == np.array([x * 2.0 ** -53 for x in u_ints(4)[:len(a)]]).tobytes()
    assert out.to_numpy("i").tolist() == held["i"].tolist()
    # an existing column is replaced in place
    rep = df.withColumn("k", F.rand(4))
    assert rep.columns == ["i", "k", "x"] and rep.to_numpy("k").tobytes() == a.tobytes()
    assert rep.schema["k"].dataType == tfs.DoubleType()
    assert "rand" in F.__all__ and "randn" in F.__all__
    assert isinstance(F.rand(), sampling.RandomExpression) and F.rand(3).alias("q").output_name == "q"


# ------------------------------------------------------------------ seed=None
def test_seed_none_is_fixed_per_frame_and_differs_per_call():
    df = even_frame(base_columns(), 3)
    a, b = df.sample(0.5), df.sample(0.5)
    assert a.count() == len(a.collect()) and a.to_numpy("i").tolist() == a.to_numpy("i").tolist()
    assert a.to_numpy("i").tolist() != b.to_numpy("i").tolist()        # (the seeds differ)
    s1, s2 = df.randomSplit([1, 1])
    assert sorted(s1.to_numpy("i").tolist() + s2.to_numpy("i").tolist()) == list(range(N))
    r = df.withColumn("r", F.rand())
    assert r.to_numpy("r").tobytes() == r.to_numpy("r").tobytes()
    assert r.to_numpy("r").tobytes() != df.withColumn("r", F.rand()).to_numpy("r").tobytes()
    by = df.sampleBy("k", {0: 0.5, 1: 0.5})
    assert by.to_numpy("i").tolist() == by.to_numpy("i").tolist()


# ------------------------------------------------------------------ errors
def test_fraction_errors_name_the_value():
    df = even_frame(base_columns(100), 2)
    for bad in (float("nan"), float("inf"), -0.1, 1.5, True):
        with pytest.raises(ValueError, match=f"sample: .*{repr(bad)}"):
            df.sample(bad, 1) if not isinstance(bad, bool) else df.sample(False, bad, 1)
        with pytest.raises(ValueError, match=f"sampleBy: .*{repr(bad)}"):
            df.sampleBy("k", {1: bad}, 1)
    with pytest.raises(ValueError, match="sample: .*16.5"):
        df.sample(True, 16.5, 1)
    with pytest.raises(ValueError, match="sample: .*-1.0"):
        df.sample(True, -1.0, 1)
    assert df.sample(True, 16.0, 1).count() > 100
    with pytest.raises(TypeError, match="sample: a fraction is expected"):
        df.sample()
    with pytest.raises(ValueError, match="sample: .*'a'"):
        df.sample(False, "a")


def test_weight_errors_name_the_value():
    df = even_frame(base_columns(100), 2)
    for bad in (float("nan"), float("inf"), -1.0, 0.0, 0, True):
        with pytest.raises(ValueError, match=f"randomSplit: .*{repr(bad)}"):
            df.randomSplit([1.0, bad], 1)
    with pytest.raises(ValueError, match="randomSplit: the list of weights is empty"):
        df.randomSplit([], 1)
    with pytest.raises(TypeError, match="randomSplit: a list of weights"):
        df.randomSplit(0.5, 1)


def test_seed_errors():
    df = even_frame(base_columns(100), 2)
    for bad in (1.5, "3", True):
        for call in (lambda: df.sample(0.5, bad), lambda: df.sample(False, 0.5, bad),
                     lambda: df.randomSplit([1, 1], bad), lambda: df.sampleBy("k", {1: 0.5}, bad),
                     lambda: F.rand(bad), lambda: F.randn(bad)):
            with pytest.raises(TypeError, match=f"the seed must be an int.*{repr(bad)}"):
                call()
    assert df.sample(0.5, np.int64(3)).to_numpy("i").tolist() == df.sample(0.5, 3).to_numpy("i").tolist()
    assert df.sample(0.5, 3 - 2 ** 64).to_numpy("i").tolist() == df.sample(0.5, 3).to_numpy("i").tolist()


def test_sample_by_errors():
    df = tfs.from_columns({"k": np.arange(6, dtype=np.int32), "f": np.arange(6, dtype=np.float32),
                           "s": [f"s{i}" for i in range(6)], "v": np.zeros((6, 2), dtype=np.float32)}, num_partitions=2)
    with pytest.raises(tfs.InvalidTypeException, match="sampleBy: 's' is a string column"):
        df.sampleBy("s", {"s1": 0.5}, 1)
    with pytest.raises(tfs.InvalidDimensionException, match="sampleBy: the key 'v' holds a cell of rank 1"):
        df.sampleBy("v", {0: 0.5}, 1)
    with pytest.raises(ValueError, match="sampleBy: Column nope not found"):
        df.sampleBy("nope", {0: 0.5}, 1)
    with pytest.raises(ValueError, match="sampleBy: at most 4096 strata are supported, got 4097"):
        df.sampleBy("k", {i: 0.5 for i in range(4097)}, 1)
    assert df.sampleBy("k", {i: 1.0 for i in range(4096)}, 1).count() == 6
    with pytest.raises(ValueError, match=r"sampleBy: the keys nan and nan are the same value"):
        df.sampleBy("f", {float("nan"): 0.5, float("nan"): 0.5}, 1)   # (two objects: two dict keys)
    with pytest.raises(ValueError, match=r"sampleBy: the keys 0.1 and 0.10000000149011612 are the same value"):
        df.sampleBy("f", {0.1: 0.5, float(np.float32(0.1)): 0.5}, 1)  # (one float32)
    with pytest.raises(ValueError, match="sampleBy: the key 1.5 is not a value of the int32 column 'k'"):
        df.sampleBy("k", {1.5: 0.5}, 1)
    with pytest.raises(TypeError, match="sampleBy: the key 'a' is not a value"):
        df.sampleBy("k", {"a": 0.5}, 1)
    with pytest.raises(TypeError, match="sampleBy: fractions must be a dict"):
        df.sampleBy("k", [0.5], 1)


def test_random_expressions_are_refused_outside_select_and_with_column():
    df = even_frame(base_columns(100), 2)
    e = F.rand(3)
    for op in (lambda: e + 1, lambda: 1 + e, lambda: e * 2, lambda: e - e, lambda: e / 2, lambda: -e, lambda: e < 0.5,
               lambda: e >= 0.5, lambda: e == 1, lambda: e != 1, lambda: e & e, lambda: bool(e)):
        with pytest.raises(TypeError, match=r"'rand\(3\)' is a random expression.*add it as a column first"):
            op()
    with pytest.raises(TypeError, match=r"filter: 'rand\(3\)' is a random expression"):
        df.filter(e)
    with pytest.raises(TypeError, match=r"orderBy: 'rand\(3\)' is a random expression"):
        df.orderBy(e)
    with pytest.raises(TypeError, match=r"groupBy: 'randn\(\)' is a random expression"):
        df.groupBy(F.randn())
    with pytest.raises(TypeError, match=r"dropDuplicates: 'rand\(3\)' is a random expression"):
        df.dropDuplicates([e])
    with pytest.raises(TypeError, match="select: the computed Column .* stands next to a random expression"):
        df.select((df.x + 1).alias("y"), e)
    with pytest.raises(ValueError, match="select: duplicate output column name 'i'"):
        df.select("i", e.alias("i"))


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
    cols = base_columns(n=230)
    df, _ = frame_of(cols, 5, (1,))
    names = list(cols)
    res = {"sample": _bytes_of(df.sample(0.4, 17), names), "replace": _bytes_of(df.sample(True, 1.3, 17), names),
           "by": _bytes_of(df.sampleBy("k", {-1: 0.5, 0: 1.0, 2: 0.25}, 17), names),
           "rand": _bytes_of(df.withColumn("r", F.rand(17)).withColumn("z", F.randn(17)), names + ["r", "z"])}
    for j, s in enumerate(df.randomSplit([3, 1, 1], 17)):
        res[f"split{j}"] = _bytes_of(s, names)
    none = df.sample(0.5)  # (one seed for every rank, and for both actions)
    res["none"] = [none.count(), len(none.collect())]
    res["none"] = res["none"][0] == res["none"][1]
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
    assert single["none"] is True and len(single["sample"]["i"]) > 0
