"""`DataFrame.union` / `unionByName`, `dropDuplicates` / `distinct`, `intersect`
and `subtract` on host frames (frame/setops.py): the API with its typed errors,
first-occurrence semantics, the defined row order, and that the result does
not depend on the partitioning or the number of ranks.

The specification is written here: the rows are walked in global input order
(partition order, then row order) and a Python dict keeps the first row of
every tuple of ordering words (`spec_words`, copied from
tests/test_gpu_group_agg.py: NaN equals NaN, -0.0 equals 0.0); the kept rows
are then sorted by their word tuples. Outputs are bitwise copies of input
rows, so every comparison is exact."""
import json
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import tensorframes_amd as tfs
from tensorframes_amd import Window, functions as F
from tensorframes_amd import core

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.bool_, np.uint8, np.int8, np.int16, np.int32, np.int64, np.float32, np.float64]
METRICS = ("distinct_rows_in", "distinct_rows_exchanged", "distinct_rows_kept", "distinct_device_partitions",
           "distinct_host_partitions")


# ------------------------------------------------------------------ the specification
def spec_words(a: np.ndarray) -> np.ndarray:
    a = np.asarray(a)
    if a.dtype.kind == "f":
        bits, ubits = (32, np.uint32) if a.dtype == np.float32 else (64, np.uint64)
        b = a.view(ubits).astype(np.uint64)
        sign = np.uint64(1 << (bits - 1))
        full = np.uint64((1 << bits) - 1)
        qnan = np.uint64(0x7FC00000 if bits == 32 else 0x7FF8000000000000)
        b = np.where(np.isnan(a), qnan, b)
        b = np.where(b == sign, np.uint64(0), b)            # -0.0 -> +0.0
        return np.where(b & sign != 0, ~b & full, b | sign)
    if a.dtype.kind in "bu":
        return a.astype(np.uint64)
    return a.astype(np.int64).view(np.uint64) ^ np.uint64(1 << 63)


def first_occurrences(cols, keys):
    """The indices (into the rows in global input order) of the first row of
    every distinct word tuple, sorted by the tuples."""
    words = [spec_words(cols[k]) for k in keys]
    first = {}
    for i in range(len(words[0])):
        first.setdefault(tuple(int(w[i]) for w in words), i)
    return [first[t] for t in sorted(first)]


def column_bytes(col):
    """A column's rows as comparable values: dense rows as bytes, others as they are."""
    if isinstance(col, np.ndarray) and col.dtype != object:
        return [np.ascontiguousarray(r).tobytes() for r in col]
    return list(col)


def frame_rows(df, names=None):
    """The frame's rows in partition order, every cell bitwise."""
    names = list(names or df.columns)
    got = {}
    for n in names:
        f = df.schema[n]
        if f.dataType.simpleString() in ("string", "binary"):
            got[n] = [r[0] for r in df.select(n).collect()]
        else:
            got[n] = column_bytes(df.to_numpy(n))
    return list(zip(*[got[n] for n in names]))


def spec_rows(cols, idx, names=None):
    names = list(names or cols)
    vals = {n: column_bytes(cols[n]) for n in names}
    return [tuple(vals[n][i] for n in names) for i in idx]


_NEAR = {np.dtype(np.int8): np.int32, np.dtype(np.int16): np.int32, np.dtype(np.bool_): np.uint8}


def frame_of(cols, nparts=3):
    """A frame of the columns. A frame made from columns has int32, int64 or
    uint8 integer columns; the key paths also take int8, int16 and bool
    tensors, which only hand-built blocks can hold (their schema then names
    the nearest column type), as in tests/test_join.py."""
    if not any(isinstance(v, np.ndarray) and v.dtype in _NEAR for v in cols.values()):
        return tfs.from_columns(cols, num_partitions=nparts)
    from tensorframes_amd.frame.block import Block
    from tensorframes_amd.frame.dataframe import DataFrame, _Materialized
    df = tfs.from_columns({c: v.astype(_NEAR.get(v.dtype, v.dtype)) for c, v in cols.items()}, num_partitions=nparts)
    n = len(next(iter(cols.values())))
    blocks = {p: Block(b.nrows, {c: torch.from_numpy(cols[c][(p * n) // nparts:((p + 1) * n) // nparts].copy())
                                 for c in cols}) for p, b in df.local_blocks().items()}
    return DataFrame(df.schema, _Materialized(blocks), nparts)


def uneven(cols, nparts, empty, one_row):
    """A frame of nparts partitions: partition `empty` loses all of its rows,
    `one_row` all but one (rows are dropped with filter). -> (frame, kept columns)"""
    n = len(next(iter(cols.values())))
    edges = [(p * n) // nparts for p in range(nparts + 1)]
    keep = np.ones(n, dtype=bool)
    keep[edges[empty]:edges[empty + 1]] = False
    keep[edges[one_row] + 1:edges[one_row + 1]] = False
    df = tfs.from_columns(dict(cols, keep=keep.astype(np.int32)), num_partitions=nparts)
    df = df.filter(df.keep > 0).select(*cols)
    sizes = {p: b.nrows for p, b in df.local_blocks().items()}   # (this rank's partitions)
    assert sizes.get(empty, 0) == 0 and sizes.get(one_row, 1) == 1
    return df, {k: v[keep] for k, v in cols.items()}


def base_columns(n=230, seed=0):
    rng = np.random.default_rng(seed)
    return {
        "id": rng.integers(0, 40, n).astype(np.int32),
        "g": rng.integers(-2, 2, n).astype(np.int64),
        "f": rng.choice(np.array([0.0, -0.0, np.nan, 1.5, -1.5, np.inf], dtype=np.float32), n),
        "v": rng.standard_normal((n, 3)).astype(np.float32),
        "s": np.array([f"row-{i % 17}" for i in range(n)], dtype=object),
        "i": np.arange(n, dtype=np.int64),
    }


def snap():
    s = tfs.metrics.snapshot()
    return {m: s.get(m, 0) for m in METRICS}


# ------------------------------------------------------------------ dropDuplicates / distinct
def values_of(dtype, n, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.bool_:
        return rng.integers(0, 2, n).astype(np.bool_)
    if np.dtype(dtype).kind == "f":
        pool = np.array([0.0, -0.0, np.nan, -np.nan, 1.0, -1.0, np.inf, -np.inf, 2.5, 1e-30], dtype=dtype)
        return rng.choice(pool, n)
    info = np.iinfo(dtype)
    pool = np.array([info.min, info.max, 0, 1, 2, 3, info.max - 1, info.min + 1], dtype=dtype)
    return rng.choice(pool, n)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_every_key_dtype(dtype):
    n = 120
    cols = {"k": values_of(dtype, n, 1), "i": np.arange(n, dtype=np.int64)}
    out = frame_of(cols, 3).dropDuplicates(["k"])
    want = first_occurrences(cols, ["k"])
    assert frame_rows(out) == spec_rows(cols, want)
    assert out.schema == frame_of(cols, 3).schema and out.num_partitions == 3


def test_nan_equals_nan_and_minus_zero_equals_zero():
    nan2 = np.array([0x7FF8000000000001], dtype=np.uint64).view(np.float64)[0]   # another NaN pattern
    x = np.array([np.nan, -0.0, 0.0, nan2, 1.0, -np.nan, 0.0, 1.0], dtype=np.float64)
    cols = {"x": x, "i": np.arange(len(x), dtype=np.int64)}
    out = frame_of(cols, 2).dropDuplicates(["x"])
    assert out.to_numpy("i").tolist() == [1, 4, 0]                 # -0.0 (first zero), 1.0, the first NaN: NaN last
    assert out.to_numpy("x").tobytes() == x[[1, 4, 0]].tobytes()   # the kept rows bit for bit


@pytest.mark.parametrize("nkeys", [1, 2, 8])
def test_1_2_and_8_keys(nkeys):
    n = 300
    rng = np.random.default_rng(nkeys)
    cols = {f"k{j}": values_of(DTYPES[j], n, 10 + j) if j >= nkeys - 1 else np.zeros(n, dtype=DTYPES[j])
            for j in range(nkeys)}
    cols["k0"] = rng.integers(0, 3, n).astype(cols["k0"].dtype)
    cols["i"] = np.arange(n, dtype=np.int64)
    keys = [f"k{j}" for j in range(nkeys)]
    out = frame_of(cols, 3).dropDuplicates(keys)
    want = first_occurrences(cols, keys)
    assert 1 < len(want) < n
    assert frame_rows(out) == spec_rows(cols, want)


def test_a_vector_and_a_string_column_ride_along():
    cols = base_columns()
    out = frame_of(cols, 3).dropDuplicates(["id", "f"])
    want = first_occurrences(cols, ["id", "f"])
    assert frame_rows(out) == spec_rows(cols, want)
    assert out.schema == frame_of(cols, 3).schema
    assert frame_rows(frame_of(cols, 3).drop_duplicates(subset=["id", "f"])) == spec_rows(cols, want)


def test_distinct_equals_drop_duplicates_without_subset():
    cols = {k: v for k, v in base_columns(seed=2).items() if k in ("id", "g", "f")}
    df = frame_of(cols, 3)
    want = spec_rows(cols, first_occurrences(cols, ["id", "g", "f"]))
    assert frame_rows(df.distinct()) == want
    assert frame_rows(df.dropDuplicates()) == want
    assert frame_rows(df.dropDuplicates(["id", "g", "f", "id"])) == want     # a repeated name counts once


def test_the_kept_row_is_the_first_in_partition_then_row_order():
    # key 7 appears in every partition; its first row is row 1 of partition 0
    k = np.array([3, 7, 7, 5, 7, 3, 7, 9, 7], dtype=np.int32)
    cols = {"k": k, "i": np.arange(len(k), dtype=np.int64)}
    out = frame_of(cols, 3).dropDuplicates(["k"])
    assert out.to_numpy("k").tolist() == [3, 5, 7, 9]
    assert out.to_numpy("i").tolist() == [0, 3, 1, 7]


def test_the_result_order_is_order_by_of_the_keys():
    cols = base_columns(seed=3)
    df = frame_of(cols, 3)
    out = df.dropDuplicates(["f", "id"])
    want = first_occurrences(cols, ["f", "id"])
    srt = df.orderBy("f", "id")
    # orderBy is stable: its first row of every run of equal keys is the first occurrence
    words = [spec_words(srt.to_numpy(k)) for k in ("f", "id")]
    head = [j for j in range(len(words[0])) if j == 0 or any(w[j] != w[j - 1] for w in words)]
    assert srt.to_numpy("i")[head].tolist() == out.to_numpy("i").tolist() == [int(cols["i"][j]) for j in want]


_SPEC = {}


def uneven_case():
    if "uneven" not in _SPEC:
        cols = base_columns(n=260, seed=4)
        _SPEC["uneven"] = cols
    return _SPEC["uneven"]


@pytest.mark.parametrize("nparts", [1, 3, 7])
def test_same_rows_in_1_3_7_partitions(nparts):
    cols = uneven_case()
    out = frame_of(cols, nparts).dropDuplicates(["id", "g"])
    assert out.num_partitions == nparts
    assert frame_rows(out) == spec_rows(cols, first_occurrences(cols, ["id", "g"]))


def test_an_empty_and_a_one_row_partition():
    df, kept = uneven(uneven_case(), 7, empty=2, one_row=4)
    out = df.dropDuplicates(["id", "g"])
    assert out.num_partitions == 7
    assert frame_rows(out) == spec_rows(kept, first_occurrences(kept, ["id", "g"]))
    none = df.filter(df.id < 0).dropDuplicates(["id"])
    assert none.num_partitions == 7 and none.count() == 0 and none.columns == df.columns


def test_two_runs_give_the_same_rows():
    df = frame_of(uneven_case(), 3)
    assert frame_rows(df.dropDuplicates(["g", "f"])) == frame_rows(df.dropDuplicates(["g", "f"]))


def test_a_value_that_fills_more_than_one_partition():
    n = 200
    k = np.full(n, 5, dtype=np.int64)
    k[::50] = [1, 9, 1, 9]                                          # a few other keys
    cols = {"k": k, "i": np.arange(n, dtype=np.int64)}
    out = frame_of(cols, 5).dropDuplicates(["k"])
    assert out.to_numpy("k").tolist() == [1, 5, 9] and out.to_numpy("i").tolist() == [0, 1, 50]
    assert sum(b.nrows for b in out.local_blocks().values()) == 3


def test_the_exchange_carries_the_locally_distinct_rows():
    cols = uneven_case()
    nparts = 4
    df = frame_of(cols, nparts)
    local = sum(len(first_occurrences({k: v[(p * 260) // nparts:((p + 1) * 260) // nparts] for k, v in cols.items()},
                                      ["id"])) for p in range(nparts))
    before = snap()
    kept = df.dropDuplicates(["id"]).count()
    after = snap()
    assert after["distinct_rows_in"] - before["distinct_rows_in"] == 260
    assert after["distinct_rows_exchanged"] - before["distinct_rows_exchanged"] == local
    assert after["distinct_rows_kept"] - before["distinct_rows_kept"] == kept == len(set(cols["id"].tolist()))
    assert after["distinct_host_partitions"] - before["distinct_host_partitions"] == nparts
    assert after["distinct_device_partitions"] == before["distinct_device_partitions"]


def test_typed_refusals():
    df = frame_of(base_columns(), 3)
    with pytest.raises(ValueError, match="dropDuplicates.*empty subset"):
        df.dropDuplicates([])
    with pytest.raises(ValueError, match="dropDuplicates: column nope not found"):
        df.dropDuplicates(["id", "nope"])
    with pytest.raises(core.InvalidTypeException, match="dropDuplicates: 's' is a string column"):
        df.dropDuplicates(["s"])
    with pytest.raises(core.InvalidTypeException, match="distinct: 's' is a string column"):
        df.select("id", "s").distinct()
    with pytest.raises(core.InvalidDimensionException, match="dropDuplicates: the key 'v' holds a cell"):
        df.dropDuplicates(["v"])
    with pytest.raises(TypeError, match="subset must be a list"):
        df.dropDuplicates("id")
    nine = frame_of({f"c{j}": np.arange(5, dtype=np.int32) for j in range(9)}, 2)
    with pytest.raises(ValueError, match="dropDuplicates: at most 8 key columns, got 9"):
        nine.dropDuplicates([f"c{j}" for j in range(9)])
    with pytest.raises(ValueError, match="distinct: at most 8 key columns, got 9"):
        nine.distinct()
    # (no column type holds half or bfloat16 values: such a key cannot reach dropDuplicates)
    wexpr = F.row_number().over(Window.partitionBy("id").orderBy("g"))
    with pytest.raises(TypeError, match="dropDuplicates: .* is a window expression"):
        df.dropDuplicates([wexpr])
    with pytest.raises(TypeError, match="union: a DataFrame is expected"):
        df.union(wexpr)


# ------------------------------------------------------------------ union / unionByName
def test_union_puts_the_partitions_side_by_side():
    a = base_columns(n=50, seed=5)
    b = base_columns(n=31, seed=6)
    bcols = {"id2": b["id"], "g2": b["g"], "f2": b["f"], "v2": b["v"], "s2": b["s"], "i2": b["i"] + 1000}
    da, db = frame_of(a, 3), frame_of(bcols, 2)
    u = da.union(db)
    assert u.num_partitions == 5 and u.columns == da.columns and u.schema == da.schema
    both = {k: np.concatenate([a[k], bcols[k2]]) for k, k2 in zip(a, bcols)}
    assert frame_rows(u) == spec_rows(both, range(81))
    blocks, ba, bb = u.local_blocks(), da.local_blocks(), db.local_blocks()
    assert sorted(blocks) == [0, 1, 2, 3, 4]
    for q in range(3):
        assert blocks[q] is ba[q]
    for p in range(2):
        assert blocks[3 + p].nrows == bb[p].nrows
        assert blocks[3 + p].columns["id"] is bb[p].columns["id2"]            # nothing is copied
    assert frame_rows(da.unionAll(db)) == frame_rows(u)
    # a.union(b).dropDuplicates prefers a's rows
    dd = u.dropDuplicates(["id"])
    assert frame_rows(dd) == spec_rows(both, first_occurrences(both, ["id"]))
    firsts = dd.to_numpy("i")
    assert (firsts[np.isin(dd.to_numpy("id"), a["id"])] < 1000).all()


def test_union_by_name_reorders_the_other_frame():
    a = {"x": np.arange(4, dtype=np.int32), "y": np.arange(4, dtype=np.float64) / 2}
    b = {"y": np.array([9.5, 8.5]), "x": np.array([7, 6], dtype=np.int32)}
    u = frame_of(a, 2).unionByName(frame_of(b, 1))
    assert u.columns == ["x", "y"] and u.num_partitions == 3
    assert u.to_numpy("x").tolist() == [0, 1, 2, 3, 7, 6] and u.to_numpy("y").tolist() == [0, .5, 1, 1.5, 9.5, 8.5]
    with pytest.raises(ValueError, match=r"unionByName: .*lacks the columns \['y'\].*unknown columns \['z'\]"):
        frame_of(a, 2).unionByName(frame_of({"x": b["x"], "z": b["y"]}, 1))
    with pytest.raises(ValueError, match="unionByName"):
        frame_of(a, 2).union_by_name(frame_of({"x": b["x"]}, 1))


def test_union_type_arity_and_name_mismatches():
    a = frame_of({"x": np.arange(4, dtype=np.int32), "y": np.arange(4, dtype=np.float64)}, 2)
    with pytest.raises(ValueError, match="union: this frame has 2 columns .* the other 1"):
        a.union(frame_of({"x": np.arange(4, dtype=np.int32)}, 1))
    with pytest.raises(core.InvalidTypeException, match=r"union: column 'y' is double.* and float.*'q'.*\.cast\(\)"):
        a.union(frame_of({"p": np.arange(4, dtype=np.int32), "q": np.arange(4, dtype=np.float32)}, 1))
    with pytest.raises(core.InvalidTypeException, match=r"union: column 'x' is int.* and bigint.*\.cast\(\)"):
        a.union(frame_of({"x": np.arange(4, dtype=np.int64), "y": np.arange(4, dtype=np.float64)}, 1))
    with pytest.raises(core.InvalidTypeException, match="intersect: column 'x'"):
        a.intersect(frame_of({"x": np.arange(4, dtype=np.int64), "y": np.arange(4, dtype=np.float64)}, 1))
    with pytest.raises(ValueError, match="subtract: this frame has 2 columns"):
        a.subtract(frame_of({"x": np.arange(4, dtype=np.int32)}, 1))


def test_union_of_analyzed_frames_keeps_the_cell_shape_and_drops_the_lead_dimension():
    a = tfs.analyze(frame_of({"v": np.zeros((6, 3), dtype=np.float32), "x": np.arange(6, dtype=np.int32)}, 1))
    b = tfs.analyze(frame_of({"w": np.ones((4, 3), dtype=np.float32), "z": np.arange(4, dtype=np.int32)}, 1))
    assert a.explain_tensors() == "DataFrame[FloatType[6,3], IntegerType[6]]"
    u = a.union(b)
    assert u.explain_tensors() == "DataFrame[FloatType[?,3], IntegerType[?]]"
    assert u.columns == ["v", "x"] and u.count() == 10
    c = tfs.analyze(frame_of({"w": np.ones((4, 2), dtype=np.float32), "z": np.arange(4, dtype=np.int32)}, 1))
    with pytest.raises(core.InvalidDimensionException, match=r"union: the cells of column 'v' have shape \[3\] .* \[2\]"):
        a.union(c)


# ------------------------------------------------------------------ intersect / subtract
def row_key(cols, i):
    return tuple(int(spec_words(cols[k])[i]) for k in cols)


def test_intersect_and_subtract_against_python_sets():
    rng = np.random.default_rng(7)
    pool = np.array([0.0, -0.0, np.nan, 1.0, 2.0], dtype=np.float64)
    a = {"k": rng.integers(0, 6, 90).astype(np.int32), "x": rng.choice(pool, 90)}
    b = {"kk": rng.integers(2, 9, 60).astype(np.int32), "xx": rng.choice(pool, 60)}
    bn = {"k": b["kk"], "x": b["xx"]}
    da, db = frame_of(a, 3), frame_of(b, 2)
    in_b = {row_key(bn, i) for i in range(60)}
    firsts = first_occurrences(a, ["k", "x"])
    both = [i for i in firsts if row_key(a, i) in in_b]
    only = [i for i in firsts if row_key(a, i) not in in_b]
    assert both and only and any(np.isnan(a["x"][i]) for i in both)
    inter, sub = da.intersect(db), da.subtract(db)
    assert inter.columns == sub.columns == ["k", "x"] and inter.num_partitions == sub.num_partitions == 3
    assert frame_rows(inter) == spec_rows(a, both)
    assert frame_rows(sub) == spec_rows(a, only)


# ------------------------------------------------------------------ ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _by_partition(out):
    """Every column's bytes and the rows of every partition (all ranks agree on both)."""
    from tensorframes_amd.parallel import frame_comm
    rows = frame_comm.partition_rows({p: b.nrows for p, b in out.local_blocks().items()}, out.num_partitions)
    return {"rows": rows, "cols": {c: out.to_numpy(c).tobytes().hex() for c in out.columns}}


def _spmd_results():
    a = {k: v for k, v in base_columns(n=150, seed=8).items() if k != "s"}
    b = {k: v for k, v in base_columns(n=90, seed=9).items() if k != "s"}
    b["i"] = b["i"] + 1000
    da, _ = uneven(a, 5, empty=1, one_row=3)                      # n1 = 5 is odd: the union exchanges
    db = frame_of(b, 2)
    keys = {k: a[k] for k in ("id", "g", "f")}
    other = {k: b[k] for k in ("id", "g", "f")}
    return {"union": _by_partition(da.union(db).dropDuplicates(["id"])),
            "union_rows": _by_partition(da.union(db)),
            "distinct": _by_partition(frame_of(keys, 3).distinct()),
            "intersect": _by_partition(frame_of(keys, 3).intersect(frame_of(other, 2)))}


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
    assert sum(single["union"]["rows"]) > 0 and sum(single["intersect"]["rows"]) > 0
    assert outs[0] == single and outs[1] == single
