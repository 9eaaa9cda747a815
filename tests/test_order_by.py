"""`DataFrame.orderBy` / `sort` / `sortWithinPartitions` and `Column.asc()` /
`.desc()` on the host path (the CPU oracle of the device sort).

Every comparison is exact. The expected order comes from the few lines of
numpy below, written from the ordering table of docs/MIGRATION.md (one
unsigned 64-bit word per key and row, rows ordered by the tuple of words,
ties in input order), followed by `np.lexsort`; nothing of the package is
used to compute it."""
import json
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import tensorframes_amd as tfs
from tensorframes_amd import InvalidDimensionException, InvalidTypeException

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def spec_order(keys) -> np.ndarray:
    """keys: [(values, descending)], most significant first -> stable permutation."""
    words = [spec_words(a, d) for a, d in keys]
    return np.lexsort(words[::-1])


def same_bits(got: np.ndarray, want: np.ndarray):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert got.tobytes() == want.tobytes()


def check_frame(out, cols, perm, names=None):
    for name in names or cols:
        got = out.to_numpy(name)
        if cols[name].dtype.kind in "US":
            assert got.tolist() == cols[name][perm].tolist(), name
        else:
            same_bits(got, cols[name][perm])


def base_columns(n=57, seed=0):
    rng = np.random.default_rng(seed)
    return {
        "k": rng.integers(-3, 4, n).astype(np.int32),
        "x": rng.standard_normal(n).astype(np.float32),
        "d": rng.standard_normal(n),
        "i": np.arange(n, dtype=np.int64),
    }


# ------------------------------------------------------------------ key forms
KEY_CASES = {
    "name": (lambda f: (("k",), {}), lambda c: [(c["k"], False)]),
    "two_names": (lambda f: (("k", "x"), {}), lambda c: [(c["k"], False), (c["x"], False)]),
    "list_of_names": (lambda f: ((["k", "x"],), {}), lambda c: [(c["k"], False), (c["x"], False)]),
    "column": (lambda f: ((f.k, f["x"]), {}), lambda c: [(c["k"], False), (c["x"], False)]),
    "desc_method": (lambda f: ((f.k.desc(), f.x.asc()), {}), lambda c: [(c["k"], True), (c["x"], False)]),
    "desc_function": (lambda f: ((tfs.desc("k"), tfs.asc("d")), {}), lambda c: [(c["k"], True), (c["d"], False)]),
    "unbound_col": (lambda f: ((tfs.col("d").desc(),), {}), lambda c: [(c["d"], True)]),
    "ascending_false": (lambda f: (("k", "x"), {"ascending": False}), lambda c: [(c["k"], True), (c["x"], True)]),
    "ascending_list": (lambda f: (("k", "x"), {"ascending": [True, False]}),
                       lambda c: [(c["k"], False), (c["x"], True)]),
    "explicit_wins": (lambda f: ((f.k.asc(), "x"), {"ascending": False}), lambda c: [(c["k"], False), (c["x"], True)]),
    "computed": (lambda f: (((f.x + f.x).desc(), "k"), {}), lambda c: [(c["x"] + c["x"], True), (c["k"], False)]),
    "computed_cast": (lambda f: ((f.k.cast("double") * 0.5,), {}),
                      lambda c: [(c["k"].astype(np.float64) * 0.5, False)]),
}


@pytest.mark.parametrize("case", sorted(KEY_CASES))
@pytest.mark.parametrize("method", ["orderBy", "sort", "order_by"])
def test_order_by_key_forms(case, method):
    cols = base_columns()
    df = tfs.from_columns(cols, num_partitions=3)
    make, spec = KEY_CASES[case]
    args, kw = make(df)
    out = getattr(df, method)(*args, **kw)
    assert out.columns == df.columns and out.num_partitions == 3
    check_frame(out, cols, spec_order(spec(cols)))


@pytest.mark.parametrize("case", ["name", "desc_method", "ascending_list", "computed"])
@pytest.mark.parametrize("method", ["sortWithinPartitions", "sort_within_partitions"])
def test_sort_within_partitions(case, method):
    cols = base_columns(n=41)
    nparts = 3
    df = tfs.from_columns(cols, num_partitions=nparts)
    sizes = [b.nrows for _, b in sorted(df.local_blocks().items())]
    make, spec = KEY_CASES[case]
    args, kw = make(df)
    out = getattr(df, method)(*args, **kw)
    assert out.columns == df.columns and out.num_partitions == nparts
    assert [b.nrows for _, b in sorted(out.local_blocks().items())] == sizes
    perm, a = [], 0
    for s in sizes:  # every partition sorted on its own
        part = {k: v[a:a + s] for k, v in cols.items()}
        perm.extend((a + spec_order(spec(part))).tolist())
        a += s
    check_frame(out, cols, np.asarray(perm, dtype=np.int64))


# ------------------------------------------------------------------ partitions
def _even_sizes(n, nparts):
    """Rows per partition of from_columns (n rows sliced evenly)."""
    return [((p + 1) * n) // nparts - (p * n) // nparts for p in range(nparts)]


def _uneven(cols, nparts, drop_partition=None):
    """A frame whose partitions have uneven sizes (one of them empty): rows
    are dropped with filter. Returns (frame, the kept columns)."""
    n = len(cols["i"])
    sizes = _even_sizes(n, nparts)
    keep = (np.arange(n) % 3 != 1)
    keep[:sizes[0]] &= np.arange(sizes[0]) % 4 == 0          # partition 0: a quarter of the others
    if drop_partition is not None and drop_partition < nparts:
        a = sum(sizes[:drop_partition])
        keep[a:a + sizes[drop_partition]] = False
    cols = dict(cols, keep=keep.astype(np.int32))
    df = tfs.from_columns(cols, num_partitions=nparts)
    df = df.filter(df.keep > 0)
    kept = np.concatenate([[0], np.cumsum(sizes)])
    return df, {k: v[keep] for k, v in cols.items()}, [int(keep[a:b].sum()) for a, b in zip(kept[:-1], kept[1:])]


@pytest.mark.parametrize("nparts", [1, 3, 5])
def test_partition_counts_and_empty_partitions(nparts):
    df, cols, _ = _uneven(base_columns(n=64, seed=nparts), nparts, drop_partition=1)
    out = df.orderBy("k", df.x.desc())
    assert out.num_partitions == nparts
    check_frame(out, cols, spec_order([(cols["k"], False), (cols["x"], True)]))
    blocks = out.local_blocks()
    assert sorted(blocks) == list(range(nparts))
    assert sum(b.nrows for b in blocks.values()) == len(cols["i"])
    # all rows of one key tuple sit in one partition: the splitters cut between keys
    dup = df.orderBy("k")
    check_frame(dup, cols, spec_order([(cols["k"], False)]))
    ks = [set(b.columns["k"].tolist()) for _, b in sorted(dup.local_blocks().items())]
    seen = set()
    for s in ks:
        assert not (s & seen)
        seen |= s


def test_more_partitions_than_rows_and_empty_frame():
    cols = {"k": np.array([2, -1, 2], dtype=np.int64), "i": np.arange(3, dtype=np.int64)}
    df = tfs.from_columns(cols, num_partitions=5)
    out = df.orderBy(df.k.desc())
    assert out.num_partitions == 5
    check_frame(out, cols, spec_order([(cols["k"], True)]))
    empty = df.filter(df.k > 100).orderBy("k")
    assert empty.count() == 0 and empty.num_partitions == 5
    assert df.filter(df.k > 100).sortWithinPartitions("k").count() == 0


def test_ties_keep_input_order():
    n = 200
    cols = {"k": (np.arange(n) * 7 % 3).astype(np.int32), "c": np.zeros(n, dtype=np.float32),
            "i": np.arange(n, dtype=np.int64)}
    for nparts in (1, 3, 5):
        df = tfs.from_columns(cols, num_partitions=nparts)
        got = df.orderBy("k").to_numpy("i")
        want = np.concatenate([np.nonzero(cols["k"] == v)[0] for v in range(3)])
        assert got.tolist() == want.tolist()
        assert df.orderBy(df.k.desc()).to_numpy("i").tolist() == \
            np.concatenate([np.nonzero(cols["k"] == v)[0] for v in (2, 1, 0)]).tolist()
        # a constant key: nothing moves, whatever the direction
        assert df.orderBy("c").to_numpy("i").tolist() == list(range(n))
        assert df.orderBy(df.c.desc(), "c").to_numpy("i").tolist() == list(range(n))


# ------------------------------------------------------------------ edge values
def _float_specials(dtype):
    fi = np.finfo(dtype)
    ubits = np.uint32 if dtype == np.float32 else np.uint64
    neg_nan = np.array([0xFFC00001 if dtype == np.float32 else 0xFFF8000000000001], dtype=ubits).view(dtype)[0]
    sig_nan = np.array([0x7F800001 if dtype == np.float32 else 0x7FF0000000000001], dtype=ubits).view(dtype)[0]
    vals = [np.nan, 1.5, -0.0, np.inf, 0.0, -np.inf, fi.tiny, -fi.tiny, fi.smallest_subnormal, -fi.smallest_subnormal,
            neg_nan, fi.max, fi.min, 0.0, -0.0, sig_nan, -1.5, 1.5, np.nan]
    return np.array(vals, dtype=dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("descending", [False, True])
def test_float_edge_cases(dtype, descending):
    x = _float_specials(dtype)
    cols = {"x": x, "i": np.arange(len(x), dtype=np.int64)}
    # the specification itself, on the cases the table names
    w = spec_words(x)
    assert w[0] == w[10] == w[15] == w[18]                      # all NaNs are equal ...
    assert w[0] > w[3] > w[11]                                  # ... and sort after +inf
    assert w[2] == w[4]                                         # -0.0 == 0.0
    assert w[5] < w[12] < w[7] < w[9] < w[4] < w[8] < w[6]      # -inf < min < -tiny < -denormal < 0 < denormal < tiny
    if dtype == np.float32:
        assert int(spec_words(x, True).max()) < 2 ** 32         # descending stays in the low 32 bits
    for nparts in (1, 3):
        df = tfs.from_columns(cols, num_partitions=nparts)
        key = df.x.desc() if descending else df.x
        check_frame(df.orderBy(key), cols, spec_order([(x, descending)]))
    got = tfs.from_columns(cols, num_partitions=2).orderBy("x", ascending=not descending).to_numpy("i").tolist()
    nan_rows = [0, 10, 15, 18]
    assert (got[:4] if descending else got[-4:]) == nan_rows    # NaNs together, in input order


@pytest.mark.parametrize("dtype", [np.int32, np.int64, np.uint8])  # (the integer types a frame column can have)
def test_integer_extremes(dtype):
    ii = np.iinfo(dtype)
    x = np.array([0, ii.max, ii.min, 1, ii.max, ii.min, ii.max - 1, ii.min + 1, 0], dtype=dtype)
    cols = {"x": x, "i": np.arange(len(x), dtype=np.int64)}
    df = tfs.from_columns(cols, num_partitions=2)
    for descending in (False, True):
        out = df.orderBy(df.x.desc() if descending else df.x.asc())
        check_frame(out, cols, spec_order([(x, descending)]))
        got = out.to_numpy("x").astype(object)
        assert all((a >= b) if descending else (a <= b) for a, b in zip(got[:-1], got[1:]))


# ------------------------------------------------------------------ other columns, metadata, composition
def test_vector_and_string_columns_travel_with_the_key():
    n = 37
    cols = base_columns(n=n, seed=3)
    cols["v"] = np.random.default_rng(4).standard_normal((n, 3)).astype(np.float32)
    cols["s"] = np.array([f"name-{i}" * (1 + i % 3) for i in range(n)])
    perm = spec_order([(cols["k"], True), (cols["d"], False)])
    for nparts in (1, 4):
        df = tfs.from_columns(cols, num_partitions=nparts)
        check_frame(df.orderBy(df.k.desc(), "d"), cols, perm)
    # host object columns (a frame made from rows)
    rows = [tfs.Row(k=int(cols["k"][i]), s=str(cols["s"][i]), v=cols["v"][i].tolist()) for i in range(n)]
    out = tfs.create_dataframe(rows, num_partitions=3).orderBy("k")
    p = spec_order([(cols["k"].astype(np.int64), False)])
    got = out.collect()
    assert [r.s for r in got] == cols["s"][p].tolist()
    assert [r.k for r in got] == cols["k"][p].tolist()
    assert [r.v for r in got] == [cols["v"][i].tolist() for i in p]


def test_metadata_survives():
    cols = base_columns(n=20)
    cols["v"] = np.ones((20, 4), dtype=np.float32)
    df = tfs.analyze(tfs.from_columns(cols, num_partitions=2))
    for out in (df.orderBy("k"), df.sortWithinPartitions(df.x.desc()), df.orderBy((df.x * 2.0).desc())):
        assert out.schema.names == df.schema.names
        for f, g in zip(df.schema.fields, out.schema.fields):
            assert f.dataType == g.dataType and f.metadata == g.metadata
        assert tfs.ColumnInformation(out.schema["v"]).stf.shape.dims[-1] == 4


def test_composes_with_limit_and_filter():
    cols = base_columns(n=50, seed=9)
    df = tfs.from_columns(cols, num_partitions=4)
    perm = spec_order([(cols["x"], True)])
    top = df.orderBy(df.x.desc()).limit(7)
    assert top.to_numpy("i").tolist() == perm[:7].tolist()
    flt = df.orderBy(df.x.desc()).filter(tfs.col("k") > 0)
    assert flt.to_numpy("i").tolist() == [i for i in perm.tolist() if cols["k"][i] > 0]
    pre = df.filter(df.k > 0).orderBy("x")
    keep = np.nonzero(cols["k"] > 0)[0]
    assert pre.to_numpy("i").tolist() == keep[spec_order([(cols["x"][keep], False)])].tolist()
    assert [r.i for r in df.sort("x").take(3)] == spec_order([(cols["x"], False)])[:3].tolist()


def test_metrics_count_sorted_rows():
    cols = base_columns(n=30)
    df = tfs.from_columns(cols, num_partitions=3)
    before = tfs.metrics.snapshot().get("sort_rows", 0)
    df.sortWithinPartitions("k").count()
    assert tfs.metrics.snapshot().get("sort_rows", 0) - before == 30


# ------------------------------------------------------------------ errors
def test_typed_errors():
    n = 6
    cols = {"k": np.arange(n, dtype=np.int32), "x": np.arange(n, dtype=np.float32),
            "v": np.ones((n, 3), dtype=np.float32), "s": np.array([f"s{i}" for i in range(n)])}
    df = tfs.from_columns(cols, num_partitions=2)
    for method in (df.orderBy, df.sort, df.sortWithinPartitions):
        with pytest.raises(ValueError, match="nope"):
            method("nope")
        with pytest.raises(ValueError, match="nope"):
            method(tfs.col("nope").desc())
        with pytest.raises(InvalidDimensionException, match=r"\.sum\(\)"):
            method("v")
        with pytest.raises(InvalidDimensionException, match="reduce the cell"):
            method((df.v * 2.0).desc())
        with pytest.raises(InvalidTypeException, match="not supported as sort keys yet"):
            method("s")
        with pytest.raises(InvalidTypeException, match="not supported as sort keys yet"):
            method(df.s.desc())
        with pytest.raises(InvalidTypeException, match="cast it"):
            method(df.k > 2)
        with pytest.raises(ValueError, match="ascending"):
            method("k", "x", ascending=[True])
        with pytest.raises(TypeError, match="ascending"):
            method("k", ascending="yes")
        with pytest.raises(ValueError, match="at least one"):
            method()
        with pytest.raises(TypeError):
            method(3)
    # a reduced vector is a scalar key
    assert df.orderBy(df.v.sum().desc(), df.k.desc()).to_numpy("k").tolist() == list(range(n))[::-1]
    # a sort order is not a value
    with pytest.raises(InvalidTypeException, match="sort order"):
        df.select(df.k.desc())
    with pytest.raises(InvalidTypeException, match="sort order"):
        df.select("x", tfs.asc("k"))
    with pytest.raises(InvalidTypeException, match="sort order"):
        df.filter((df.k > 2).desc())
    with pytest.raises(InvalidTypeException, match="sort order"):
        df.withColumn("y", df.x.asc())
    with pytest.raises(InvalidTypeException, match="sort order"):
        df.k.desc() + 1
    with pytest.raises(InvalidTypeException, match="sort order"):
        1 + df.k.desc()
    with pytest.raises(InvalidTypeException, match="sort order"):
        df.x * df.x.asc()
    with pytest.raises(InvalidTypeException, match="sort order"):
        df.k.desc() > 2
    with pytest.raises(InvalidTypeException, match="sort order"):
        -df.k.desc()
    with pytest.raises(InvalidTypeException, match="sort order"):
        df.v.desc().sum()
    with pytest.raises(InvalidTypeException, match="sort order"):
        df.k.asc().cast("double")
    assert df.k.desc().sort_order == "desc" and df.k.asc().sort_order == "asc" and df.k.sort_order is None
    from tensorframes_amd import scala_dsl
    assert scala_dsl.desc("k").sort_order == "desc" and scala_dsl.asc("k").sort_order == "asc"


# ------------------------------------------------------------------ several ranks
def _spmd_columns():
    n = 83
    rng = np.random.default_rng(21)
    return {
        "k": rng.integers(0, 3, n).astype(np.int32),          # heavy duplicates
        "g": rng.integers(-50, 50, n).astype(np.int64),
        "x": rng.standard_normal(n).astype(np.float32),
        "v": rng.standard_normal((n, 2)),
        "s": np.array([f"row-{i}" for i in range(n)]),
        "i": np.arange(n, dtype=np.int64),
    }


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
    import tensorframes_amd as tfs
    from tensorframes_amd.parallel import dist

    assert dist.init(backend="gloo")
    df, _, _ = _uneven(_spmd_columns(), 5, drop_partition=3)
    res = {}
    for name, keys in (("dup", lambda f: ("k",)), ("two", lambda f: (f.k.desc(), "x")),
                       ("wide", lambda f: (f.g, f.x.desc()))):
        out = df.orderBy(*keys(df))
        rows = out.collect()
        res[name] = {
            "nparts": out.num_partitions,
            "i": [r.i for r in rows], "s": [r.s for r in rows], "v": [r.v for r in rows],
            "local": {str(p): b.columns["i"].tolist() for p, b in out.local_blocks().items()},
        }
    within = df.sortWithinPartitions("g")
    res["within"] = {"i": [r.i for r in within.collect()],
                     "local": {str(p): b.nrows for p, b in within.local_blocks().items()}}
    with open(os.path.join(outdir, f"r{rank}.json"), "w") as f:
        json.dump(res, f)
    dist.shutdown()


@pytest.mark.parametrize("world", [2, 4])
def test_order_by_spmd(world, tmp_path):
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    outs = [json.load(open(tmp_path / f"r{r}.json")) for r in range(world)]
    _, cols, sizes = _uneven(_spmd_columns(), 5, drop_partition=3)
    assert len(set(sizes)) > 2 and 0 in sizes                       # uneven, one empty
    specs = {"dup": [(cols["k"], False)], "two": [(cols["k"], True), (cols["x"], False)],
             "wide": [(cols["g"], False), (cols["x"], True)]}
    for name, spec in specs.items():
        perm = spec_order(spec)
        want_i = cols["i"][perm].tolist()
        parts = {}
        for r, o in enumerate(outs):
            got = o[name]
            assert got["nparts"] == 5
            assert got["i"] == want_i                                # collect() on every rank
            assert got["s"] == cols["s"][perm].tolist()
            assert got["v"] == cols["v"][perm].tolist()
            assert sorted(int(p) for p in got["local"]) == [p for p in range(5) if p % world == r]
            parts.update({int(p): v for p, v in got["local"].items()})
        assert sorted(parts) == list(range(5))
        # reading the partitions in order gives the sorted rows: boundaries never step back
        assert [i for p in range(5) for i in parts[p]] == want_i
    a, want = 0, []
    for s in sizes:
        want.extend((a + spec_order([(cols["g"][a:a + s], False)])).tolist())
        a += s
    for o in outs:
        assert o["within"]["i"] == cols["i"][want].tolist()
    assert [sum(int(o["within"]["local"].get(str(p), 0)) for o in outs) for p in range(5)] == sizes
