"""DataFrame.join on the host path: inner / left_semi / left_anti broadcast
equi-joins against a specification written here (a dict from the key's word
tuple to the right frame's global rows, walked in left row order). All
comparisons are exact, payload bits included."""
import json
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import tensorframes_amd as tfs
from tensorframes_amd.core import InvalidDimensionException, InvalidTypeException

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SEMI = ("left_semi", "leftsemi", "semi")
ANTI = ("left_anti", "leftanti", "anti")


# ------------------------------------------------------------------ the specification
def spec_words(a: np.ndarray) -> np.ndarray:
    """The ordering table of docs/MIGRATION.md: equal words <=> equal join keys."""
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


def spec_tuples(keys):
    words = [spec_words(k) for k in keys]
    return [tuple(int(w[i]) for w in words) for i in range(len(words[0]))]


def spec_join(lkeys, rkeys, how="inner"):
    """inner: (left rows, right rows) of the output, in order; semi / anti:
    (left rows kept, None). lkeys / rkeys: one array per key, global rows."""
    table = {}
    for r, t in enumerate(spec_tuples(rkeys)):
        table.setdefault(t, []).append(r)
    li, ri = [], []
    for i, t in enumerate(spec_tuples(lkeys)):
        hits = table.get(t, [])
        if how == "inner":
            li += [i] * len(hits)
            ri += hits
        elif (how == "semi") == bool(hits):
            li.append(i)
    return np.array(li, dtype=np.int64), (np.array(ri, dtype=np.int64) if how == "inner" else None)


def same_bits(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    if len(want) == 0:                  # (to_numpy of a frame without rows does not know the column's dtype)
        assert len(got) == 0, what
        return
    if want.dtype.kind in "OUS":
        assert got.tolist() == want.tolist(), what
    else:
        assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape)
        assert np.ascontiguousarray(got).tobytes() == np.ascontiguousarray(want).tobytes(), what


def check_join(left, right, lcols, rcols, on, how="inner"):
    """`left.join(right, on, how)` against the specification, every column."""
    keys = [on] if isinstance(on, str) else list(on)
    kind = "inner" if how == "inner" else ("semi" if how in SEMI else "anti")
    li, ri = spec_join([lcols[k] for k in keys], [rcols[k] for k in keys], kind)
    out = left.join(right, on, how)
    assert out.num_partitions == left.num_partitions
    lrest = [c for c in lcols if c not in keys]
    rrest = [c for c in rcols if c not in keys]
    if kind == "inner":
        assert out.columns == keys + lrest + rrest
    else:
        assert out.columns == list(lcols)
    assert out.count() == len(li)
    for c in out.columns:
        src, idx = (rcols, ri) if kind == "inner" and c in rrest else (lcols, li)
        same_bits(out.to_numpy(c), np.asarray(src[c])[idx], c)
    return out


def _cols(n, seed, lo=0, hi=12):
    rng = np.random.default_rng(seed)
    return {"k": rng.integers(lo, hi, n).astype(np.int64), "i": np.arange(n, dtype=np.int64)}


def _left_right(n=40, m=25):
    lc = _cols(n, 1)
    lc["a"] = np.random.default_rng(5).standard_normal(n).astype(np.float32)
    rc = _cols(m, 2, 3, 16)
    rc = {"k": rc["k"], "j": rc["i"], "b": np.random.default_rng(6).standard_normal(m)}
    return lc, rc


# ------------------------------------------------------------------ interface
@pytest.mark.parametrize("on", ["k", ["k"], ("k",)])
def test_on_forms(on):
    lc, rc = _left_right()
    check_join(tfs.from_columns(lc, num_partitions=2), tfs.from_columns(rc, num_partitions=2), lc, rc, on)


@pytest.mark.parametrize("how", ("inner",) + SEMI + ANTI)
def test_how_aliases(how):
    lc, rc = _left_right()
    out = check_join(tfs.from_columns(lc, num_partitions=3), tfs.from_columns(rc, num_partitions=2), lc, rc, "k", how)
    assert 0 < out.count()


def test_schema_and_column_order():
    lc = {"a": np.arange(4, dtype=np.float32), "k2": np.array([1, 2, 1, 2], np.int32), "z": np.zeros(4),
          "k1": np.array([0, 0, 1, 1], np.int64)}
    rc = {"r": np.arange(3, dtype=np.int64), "k1": np.array([1, 0, 1], np.int64), "k2": np.array([2, 1, 3], np.int32)}
    left, right = tfs.from_columns(lc, num_partitions=2), tfs.from_columns(rc, num_partitions=1)
    inner = check_join(left, right, lc, rc, ["k1", "k2"])
    assert inner.columns == ["k1", "k2", "a", "z", "r"]
    assert [f.name for f in inner.schema.fields[:4]] == ["k1", "k2", "a", "z"]
    assert inner.schema["k1"] == left.schema["k1"] and inner.schema["r"] == right.schema["r"]
    for how in ("semi", "anti"):
        out = check_join(left, right, lc, rc, ["k1", "k2"], how)
        assert out.schema == left.schema


@pytest.mark.parametrize("nparts", [1, 3, 7])
def test_left_partitions_keep_their_rows(nparts):
    lc, rc = _left_right(n=5 if nparts == 7 else 40)       # 7 partitions of 5 rows: some are empty
    left = tfs.from_columns(lc, num_partitions=nparts)
    if nparts == 3:
        left = left.filter(left.i >= 14)                    # partition 0 (rows 0..12) becomes empty
        keep = lc["i"] >= 14
        lc = {c: v[keep] for c, v in lc.items()}
    right = tfs.from_columns(rc, num_partitions=2)
    out = check_join(left, right, lc, rc, "k")
    # output partition p holds the matches of left partition p, in left row order
    lparts = {p: b.columns["i"].tolist() for p, b in left.local_blocks().items()}
    table = {}
    for r, k in enumerate(rc["k"].tolist()):
        table.setdefault(k, []).append(r)
    for p, b in out.local_blocks().items():
        want = [(i, r) for i in lparts[p] for r in table.get(int(lc["k"][lc["i"].tolist().index(i)]), [])]
        assert list(zip(b.columns["i"].tolist(), b.columns["j"].tolist())) == want


@pytest.mark.parametrize("n,m", [(0, 6), (6, 0), (0, 0)])
def test_empty_frames(n, m):
    lc, rc = _left_right(n, m)
    left, right = tfs.from_columns(lc, num_partitions=2), tfs.from_columns(rc, num_partitions=2)
    for how in ("inner", "semi", "anti"):
        out = check_join(left, right, lc, rc, "k", how)
        assert out.count() == (n if how == "anti" else 0)


def test_result_does_not_depend_on_the_right_partitioning():
    lc, rc = _left_right(60, 37)
    left = tfs.from_columns(lc, num_partitions=3)
    one = check_join(left, tfs.from_columns(rc, num_partitions=1), lc, rc, "k")
    five = check_join(left, tfs.from_columns(rc, num_partitions=5), lc, rc, "k")
    assert [tuple(r) for r in one.collect()] == [tuple(r) for r in five.collect()]


def test_duplicates_on_both_sides_follow_right_global_order():
    lc = {"k": np.array([7, 7, 1, 7], np.int32), "i": np.arange(4, dtype=np.int64)}
    rc = {"k": np.array([7, 1, 7, 9, 7, 1], np.int32), "j": np.arange(6, dtype=np.int64)}
    out = check_join(tfs.from_columns(lc, num_partitions=2), tfs.from_columns(rc, num_partitions=4), lc, rc, "k")
    assert out.to_numpy("j").tolist() == [0, 2, 4, 0, 2, 4, 1, 5, 0, 2, 4]
    semi = check_join(tfs.from_columns(lc, num_partitions=2), tfs.from_columns(rc, num_partitions=4), lc, rc, "k",
                      "semi")
    assert semi.to_numpy("i").tolist() == [0, 1, 2, 3]     # duplicates on the right never multiply rows


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_float_keys(dtype):
    nan2 = np.array([0x7FC00001 if dtype == np.float32 else 0x7FF8000000000001],
                    dtype=np.uint32 if dtype == np.float32 else np.uint64).view(dtype)[0]   # another NaN payload
    lk = np.array([np.nan, -0.0, 0.0, np.inf, -np.inf, 1.5, nan2, 2.5], dtype=dtype)
    rk = np.array([0.0, np.nan, np.inf, -0.0, 1.5, -np.inf, 3.5], dtype=dtype)
    lc = {"k": lk, "i": np.arange(len(lk), dtype=np.int64)}
    rc = {"k": rk, "j": np.arange(len(rk), dtype=np.int64)}
    left, right = tfs.from_columns(lc, num_partitions=2), tfs.from_columns(rc, num_partitions=2)
    out = check_join(left, right, lc, rc, "k")
    pairs = list(zip(out.to_numpy("i").tolist(), out.to_numpy("j").tolist()))
    assert pairs == [(0, 1), (1, 0), (1, 3), (2, 0), (2, 3), (3, 2), (4, 5), (5, 4), (6, 1)]
    got = out.to_numpy("k")
    assert np.signbit(got[1]) and np.signbit(got[2]) and not np.signbit(got[3])   # the left side's -0.0 bits stay
    check_join(left, right, lc, rc, "k", "semi")
    anti = check_join(left, right, lc, rc, "k", "anti")
    assert anti.to_numpy("i").tolist() == [7]


def _frame_holding(cols, nparts):
    """A frame whose blocks hold `cols` as they are. A frame made from columns
    has int32, int64 or uint8 integer columns; the key paths also take int8,
    int16 and bool tensors, which only hand-built blocks can hold (their
    schema then names the nearest column type)."""
    from tensorframes_amd.frame.block import Block
    from tensorframes_amd.frame.dataframe import DataFrame, _Materialized
    near = {np.dtype(np.int8): np.int32, np.dtype(np.int16): np.int32, np.dtype(np.bool_): np.uint8}
    df = tfs.from_columns({c: v.astype(near.get(v.dtype, v.dtype)) for c, v in cols.items()}, num_partitions=nparts)
    n = len(next(iter(cols.values())))
    blocks = {p: Block(b.nrows, {c: torch.from_numpy(cols[c][(p * n) // nparts:((p + 1) * n) // nparts].copy())
                                 for c in cols}) for p, b in df.local_blocks().items()}
    return DataFrame(df.schema, _Materialized(blocks), nparts)


@pytest.mark.parametrize("dtype", [np.int8, np.int64, np.bool_, np.uint8, np.int16, np.int32])
def test_integer_and_bool_keys(dtype):
    if dtype == np.bool_:
        lk, rk = np.array([True, False, True]), np.array([False, False, True, True])
    elif dtype == np.uint8:
        lk, rk = np.array([0, 255, 128, 7], np.uint8), np.array([255, 255, 0, 127, 128], np.uint8)
    else:
        lo, hi = np.iinfo(dtype).min, np.iinfo(dtype).max
        lk, rk = np.array([lo, hi, 0, -1, 1, hi], dtype), np.array([hi, lo, lo, -1, 2, 0], dtype)
    lc = {"k": lk, "i": np.arange(len(lk), dtype=np.int64)}
    rc = {"k": rk, "j": np.arange(len(rk), dtype=np.int64)}
    for how in ("inner", "semi", "anti"):
        out = check_join(_frame_holding(lc, 2), _frame_holding(rc, 3), lc, rc, "k", how)
        assert out.count() > 0 or how == "anti"


def test_two_keys_with_many_ties_on_the_first():
    rng = np.random.default_rng(3)
    n, m = 90, 70
    x = rng.integers(0, 6, n).astype(np.float64) / 2
    x[::11] = np.nan
    y = rng.integers(0, 6, m).astype(np.float64) / 2
    y[::7] = np.nan
    lc = {"g": rng.integers(0, 3, n).astype(np.int32), "x": x, "i": np.arange(n, dtype=np.int64)}
    rc = {"g": rng.integers(0, 3, m).astype(np.int32), "x": y, "j": np.arange(m, dtype=np.int64)}
    for how in ("inner", "semi", "anti"):
        check_join(tfs.from_columns(lc, num_partitions=3), tfs.from_columns(rc, num_partitions=2), lc, rc,
                   ["g", "x"], how)


def test_eight_keys_work_and_nine_raise():
    rng = np.random.default_rng(4)
    n, m = 50, 40
    names = [f"k{j}" for j in range(9)]
    lc = {k: rng.integers(0, 2, n).astype(np.int32) for k in names}
    rc = {k: rng.integers(0, 2, m).astype(np.int32) for k in names}
    lc["i"] = np.arange(n, dtype=np.int64)
    rc["j"] = np.arange(m, dtype=np.int64)
    left, right = tfs.from_columns(lc, num_partitions=2), tfs.from_columns(rc, num_partitions=2)
    l8 = {k: v for k, v in lc.items() if k != "k8"}
    r8 = {k: v for k, v in rc.items() if k != "k8"}
    out = check_join(left.drop("k8"), right.drop("k8"), l8, r8, names[:8])
    assert out.count() > 0
    with pytest.raises(ValueError, match="at most 8"):
        left.join(right, names)


def test_vector_and_string_columns_travel_as_payload():
    rng = np.random.default_rng(8)
    n, m = 30, 20
    lc = {"k": rng.integers(0, 8, n).astype(np.int64), "lv": rng.standard_normal((n, 3)).astype(np.float32),
          "ls": np.array([f"left-{i}" * (1 + i % 3) for i in range(n)])}
    rc = {"k": rng.integers(0, 8, m).astype(np.int64), "rv": rng.standard_normal((m, 2, 2)),
          "rs": np.array([f"right-{i}" * (1 + i % 2) for i in range(m)])}
    for how in ("inner", "semi", "anti"):
        check_join(tfs.from_columns(lc, num_partitions=3), tfs.from_columns(rc, num_partitions=2), lc, rc, "k", how)


def test_ragged_and_object_payload_columns():
    left = tfs.create_dataframe([(1, [1.0]), (2, [1.0, 2.0]), (1, [])], schema=["k", "cells"], num_partitions=2)
    right = tfs.create_dataframe([(1, "a", [5, 6]), (3, "b", [7]), (1, "c", [8, 9, 10])], schema=["k", "s", "rc"],
                                 num_partitions=2)
    rows = [tuple(r) for r in left.join(right, "k").collect()]
    assert rows == [(1, [1.0], "a", [5, 6]), (1, [1.0], "c", [8, 9, 10]), (1, [], "a", [5, 6]),
                    (1, [], "c", [8, 9, 10])]


def test_metadata_of_an_analyzed_column_survives():
    lc = {"k": np.arange(6, dtype=np.int64), "v": np.ones((6, 4), dtype=np.float32)}
    rc = {"k": np.array([1, 3, 5], np.int64), "w": np.ones((3, 2))}
    left = tfs.analyze(tfs.from_columns(lc, num_partitions=2))
    right = tfs.analyze(tfs.from_columns(rc, num_partitions=1))
    out = left.join(right, "k")
    for name, src in (("k", left), ("v", left), ("w", right)):
        assert out.schema[name].metadata == src.schema[name].metadata and out.schema[name].metadata
    assert left.join(right, "k", "semi").schema["v"].metadata == left.schema["v"].metadata


def test_composition_with_filter_order_by_and_limit():
    lc, rc = _left_right(80, 50)
    left, right = tfs.from_columns(lc, num_partitions=4), tfs.from_columns(rc, num_partitions=3)
    keep_l, keep_r = lc["a"] > -0.5, rc["j"] < 41
    fl, fr = left.filter(left.a > -0.5), right.filter(right.j < 41)
    lcf = {c: v[keep_l] for c, v in lc.items()}
    rcf = {c: v[keep_r] for c, v in rc.items()}
    out = check_join(fl, fr, lcf, rcf, "k")
    li, ri = spec_join([lcf["k"]], [rcf["k"]])
    j = rcf["j"][ri]
    order = np.lexsort([np.arange(len(j)), spec_words(-j)])           # by j descending, stable
    top = out.orderBy(out.j.desc()).limit(9)
    assert top.to_numpy("j").tolist() == j[order][:9].tolist()
    assert top.to_numpy("i").tolist() == lcf["i"][li][order][:9].tolist()


def test_metrics_count_rows():
    lc, rc = _left_right(40, 25)
    li, _ = spec_join([lc["k"]], [rc["k"]])
    before = tfs.metrics.snapshot()
    tfs.from_columns(lc, num_partitions=3).join(tfs.from_columns(rc, num_partitions=2), "k").count()
    after = tfs.metrics.snapshot()
    assert after.get("join_rows_left", 0) - before.get("join_rows_left", 0) == 40
    assert after.get("join_rows_build", 0) - before.get("join_rows_build", 0) == 25
    assert after.get("join_rows_out", 0) - before.get("join_rows_out", 0) == len(li)


# ------------------------------------------------------------------ typed errors
def test_typed_errors():
    lc, rc = _left_right()
    left, right = tfs.from_columns(lc, num_partitions=2), tfs.from_columns(rc, num_partitions=2)
    with pytest.raises(TypeError, match="withColumnRenamed"):
        left.join(right, None)
    with pytest.raises(TypeError, match="withColumnRenamed"):
        left.join(right, left.k == right.k)
    for how in ("left", "right", "outer", "full", "left_outer", "right_outer", "full_outer", "cross"):
        with pytest.raises(NotImplementedError, match="[Nn]ulls"):
            left.join(right, "k", how)
    with pytest.raises(ValueError, match="left_semi"):
        left.join(right, "k", "sideways")
    with pytest.raises(ValueError, match="not found in the right"):
        left.join(right, "i")
    with pytest.raises(ValueError, match="not found in the left"):
        left.join(right, "j")
    # keys: one scalar per row, a sortable dtype, the same dtype on both sides
    vec = tfs.analyze(tfs.from_columns({"k": np.zeros((4, 2), np.int64)}))
    with pytest.raises(InvalidDimensionException, match="scalar"):
        vec.join(vec, "k", "semi")
    strs = tfs.from_columns({"k": np.array(["a", "b"]), "x": np.zeros(2)})
    with pytest.raises(InvalidTypeException, match="string"):
        strs.join(strs, "k", "semi")
    # (no column type holds half or bfloat16 values: such a key cannot reach join)
    with pytest.raises(TypeError):
        tfs.from_columns({"k": torch.zeros(3, dtype=torch.float16)})
    r32 = tfs.from_columns({"k": rc["k"].astype(np.int32), "j": rc["j"]})
    with pytest.raises(InvalidTypeException, match=r"int64.*int32.*cast"):
        left.join(r32, "k")
    # inner: a shared name that is not a key is refused; semi / anti do not care
    clash = tfs.from_columns({"k": rc["k"], "i": rc["j"]})
    with pytest.raises(ValueError, match=r"\['i'\]"):
        left.join(clash, "k")
    assert left.join(clash, "k", "semi").columns == left.columns


def test_errors_are_raised_when_join_is_called_and_the_result_is_lazy():
    calls = []
    from tensorframes_amd.frame.block import Block
    from tensorframes_amd.frame.types import LongType, StructField, StructType

    def gen(p):
        calls.append(p)
        return Block(2, {"k": torch.tensor([p, p + 1])})
    lazy = tfs.generate(StructType([StructField("k", LongType(), False)]), 2, gen)
    out = lazy.join(lazy, "k", "semi")
    assert calls == []
    assert out.count() == 4


# ------------------------------------------------------------------ SPMD over gloo
def _spmd_frames(tfs_mod, left_parts, right_one_rank, world):
    rng = np.random.default_rng(11)
    n, m = 57, 33
    x = rng.integers(0, 5, n).astype(np.float32)
    x[::9] = np.nan
    y = rng.integers(0, 5, m).astype(np.float32)
    y[::5] = np.nan
    lc = {"g": rng.integers(0, 3, n).astype(np.int64), "x": x, "i": np.arange(n, dtype=np.int64),
          "ls": np.array([f"l{i}" for i in range(n)])}
    rc = {"g": rng.integers(0, 3, m).astype(np.int64), "x": y, "j": np.arange(m, dtype=np.int64),
          "rv": rng.standard_normal((m, 3)), "rs": np.array([f"r{i}" * (i % 3) for i in range(m)])}
    left = tfs_mod.from_columns(lc, num_partitions=left_parts)
    # one partition: every row of the right side sits on rank 0, in every world
    right = tfs_mod.from_columns(rc, num_partitions=1 if right_one_rank else 5)
    return left, right, lc, rc


CASES = {"plain": (5, False), "idle_rank": (1, False), "one_rank": (4, True)}


def _run_case(tfs_mod, name, world):
    left_parts, one_rank = CASES[name]
    left, right, _, _ = _spmd_frames(tfs_mod, left_parts, one_rank, world)
    res = {}
    for how in ("inner", "semi", "anti"):
        out = left.join(right, ["g", "x"], how)
        res[how] = [[v if not isinstance(v, float) or v == v else "nan" for v in r] for r in out.collect()]
        res[how + "_local"] = {str(p): b.columns["i"].tolist() for p, b in out.local_blocks().items()}
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
    import tensorframes_amd as tfs_mod
    from tensorframes_amd.parallel import dist

    assert dist.init(backend="gloo")
    res = {name: _run_case(tfs_mod, name, world) for name in CASES}
    with open(os.path.join(outdir, f"r{rank}.json"), "w") as f:
        json.dump(res, f)
    dist.shutdown()


@pytest.fixture(scope="module")
def world_one():
    return json.loads(json.dumps({name: _run_case(tfs, name, 1) for name in CASES}))


def test_world_one_matches_the_specification(world_one):
    for name, (left_parts, one_rank) in CASES.items():
        _, _, lc, rc = _spmd_frames(tfs, left_parts, one_rank, 1)
        for how in ("inner", "semi", "anti"):
            li, _ = spec_join([lc["g"], lc["x"]], [rc["g"], rc["x"]], how)
            assert [r[2] for r in world_one[name][how]] == li.tolist()
        assert len(world_one[name]["inner"]) > 57                      # duplicates multiply rows


@pytest.mark.parametrize("world", [2, 3])
def test_join_spmd(world, world_one, tmp_path):
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    outs = [json.load(open(tmp_path / f"r{r}.json")) for r in range(world)]
    for name, (left_parts, _) in CASES.items():
        for how in ("inner", "semi", "anti"):
            parts = {}
            for r, o in enumerate(outs):
                assert o[name][how] == world_one[name][how], (name, how, r)       # content and order, every rank
                local = o[name][how + "_local"]
                assert sorted(int(p) for p in local) == [p for p in range(left_parts) if p % world == r]
                parts.update(local)
            assert parts == world_one[name][how + "_local"]
