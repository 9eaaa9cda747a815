"""`F.skewness` / `F.kurtosis` on the host path (the CPU oracle of the device
kernels), also under gloo ranks. Expected values are written here: the
f64-converted values are scaled to Python ints by a power of two, Mk = sum
(x - mean)^k and Sk = sum |x - mean|^k are `fractions.Fraction`s rounded once.

Tolerances (derived, not measured). The data is that of tests/test_gpu_corr.py:
1e4 + N(0, 1) for floats (kappa = |mean| / sigma = 1e4), scaled and rounded for
the integers. With u = 2^-53, a deviation x - mean carries an absolute error
delta <= L u kappa sigma: one rounding of the subtraction at the size of x, and
the error of the running mean, of the same size once per level of the update /
merge tree. For M2 that derivation (tests/test_corr.py) gave 1e-11 relative at
kappa = 1e4. (d + delta)^k = d^k + k d^(k-1) delta + ..., and sigma S(k-1) <= Sk
(power means), so the same delta costs k / 2 times as much relative to Sk:
1.5e-11 for M3, 2e-11 for M4. On top come the roundings of the sums: every
term of a sum, an update or a merge is bounded by Sk and a row passes a
sequential step once, so they add at most n u Sk; groups here have n <= 2^14
rows: OPS = 2e-12. kappa is the group's own: two or three rows that lie close
together have a far larger |mean| / sigma than the column (two rows h apart
and a mean off by e give M3 = 6 h^2 e where 0 is exact), so the bounds scale
with K = kappa_group / 1e4, kappa_group = |mean| / sqrt(M2 / n), exact. Per group:
  * M2 within B2 M2, B2 = 1e-11 K; the mean within 1e-11 relative;
  * M3 within B3 S3, B3 = 1.5e-11 K + OPS; M4 within B4 S4, B4 = 2e-11 K + OPS;
  * skewness g = sqrt(n) M3 / M2^1.5 within B3 sqrt(n) S3 / M2^1.5 + 1.5 |g| B2;
  * kurtosis k = n M4 / M2^2 - 3 within (k + 3) (B4 + 2 B2);
  * n and the non-finite count exact; NaN exactly where the rules say.
A group whose propagated bound exceeds 1 would be skipped; `spec` asserts that
there is none: 0 groups skipped (the constant group is NaN by rule, M2 == 0).
Largest error of the numpy host form over this file, as a fraction of the
bound: M3 0.098, M4 0.031; the largest |M3 err| / S3 itself is 1.03e-11
(float64, a few rows with K = 6.8)."""
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
from tensorframes_amd._native import _C
from tensorframes_amd.frame import group_agg as GA

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = 2e-12
DTYPES = [np.uint8, np.int8, np.int16, np.int32, np.int64, np.float32, np.float64]
FRAME_DTYPES = [np.uint8, np.int32, np.int64, np.float32, np.float64]  # (the types a frame column can have)


def bounds(e):  # (B2, B3, B4) of a group with exact moments `e`: the docstring's derivation
    K = abs(e["mean"]) / math.sqrt(e["m2"] / e["n"]) / 1e4 if e["m2"] > 0 else 0.0
    return 1e-11 * K, 1.5e-11 * K + OPS, 2e-11 * K + OPS


def data(dt, n, seed=0):
    """1e4 + N(0, 1) cast to the dtype (integers: a scaled, rounded form)"""
    v, dt = np.random.default_rng(seed).standard_normal(n), np.dtype(dt)
    if dt.kind == "f":
        return (1e4 + v).astype(dt)
    if dt.itemsize == 1:
        return np.clip(np.rint(100 + 5 * v), 0 if dt.kind == "u" else -128, 127).astype(dt)
    return np.rint(10000 + 100 * v).astype(dt)


_EXACT = {}


def exact(x: np.ndarray):
    """{n, bad, mean, m2, m3, m4, s3} of the f64-converted rows; the moments exact, rounded once (finite rows)."""
    key = (x.dtype.str, x.tobytes())
    if key not in _EXACT:
        xf = x.astype(np.float64)
        n, bad = len(xf), int((~np.isfinite(xf)).sum())
        e = {"n": n, "bad": bad}
        if n and not bad:
            ratios = [float(v).as_integer_ratio() for v in xf]
            D = max(r[1] for r in ratios)
            ix = [r[0] * (D // r[1]) for r in ratios]
            s = sum(ix)
            dev = [n * v - s for v in ix]                               # (x - mean) * n * D, an int
            e["mean"] = float(Fraction(s, n * D))
            for k in (2, 3, 4):
                e[f"m{k}"] = float(Fraction(sum(d ** k for d in dev), (n * D) ** k))
            e["s3"] = float(Fraction(sum(abs(d) ** 3 for d in dev), (n * D) ** 3))
        _EXACT[key] = e
    return _EXACT[key]


def spec(fn: str, x: np.ndarray):
    """(expected value, absolute bound) of skewness / kurtosis over the group's rows."""
    e = exact(x)
    if e["n"] == 0 or e["bad"] or e["m2"] == 0:
        return math.nan, 0.0
    n, m2 = e["n"], e["m2"]
    B2, B3, B4 = bounds(e)
    if fn == "skewness":
        g = math.sqrt(n) * e["m3"] / m2 ** 1.5
        bound = B3 * math.sqrt(n) * e["s3"] / m2 ** 1.5 + 1.5 * abs(g) * B2
    else:
        g = n * e["m4"] / m2 ** 2 - 3.0
        bound = (g + 3.0) * (B4 + 2 * B2)
    assert bound < 1                                                    # (no group is skipped)
    return g, bound


def check_value(got, fn, x, where=""):
    got = np.asarray(got)[()]
    want, bound = spec(fn, x)
    assert got.dtype == np.float64 and (math.isnan(got) if math.isnan(want) else abs(float(got) - want) <= bound), (
        where, fn, got, want, bound)


def check_record(r: np.ndarray, x: np.ndarray, where=""):
    """One high record [6] against the finite rows it stands for."""
    f, e = r[:5].view(np.float64), exact(x)
    assert f[0] == float(len(x)) and int(r[5]) == 0, (where, f[0], r[5])
    if len(x) == 0:
        assert not r.any(), (where, r)
        return
    B2, B3, B4 = bounds(e)
    assert abs(f[1] - e["mean"]) <= 1e-11 * abs(e["mean"]), (where, f[1], e["mean"])
    assert abs(f[2] - e["m2"]) <= B2 * e["m2"], (where, f[2], e["m2"])
    assert abs(f[3] - e["m3"]) <= B3 * e["s3"], (where, f[3], e["m3"])
    assert abs(f[4] - e["m4"]) <= B4 * e["m4"], (where, f[4], e["m4"])


def grouped_columns(dt, seed=0):
    """k, x: groups of 1, 2, 3 and 700 rows, a constant group, and for the float dtypes a group with a NaN
    row and one with an infinity, shuffled."""
    sizes = [1, 2, 3, 700, 5] + ([4, 4] if np.dtype(dt).kind == "f" else [])
    k = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
    x = data(dt, len(k), seed)
    x[k == 4] = x[k == 4][0]
    if len(sizes) > 5:
        x[np.nonzero(k == 5)[0][1]] = np.nan
        x[np.nonzero(k == 6)[0][2]] = -np.inf
    order = np.random.default_rng(seed + 1).permutation(len(k))
    return k[order], x[order]


def keyed_rows(out, key="k"):  # {key value: {output column: numpy scalar}}
    cols = {n: out.to_numpy(n) for n in out.columns}
    return {cols[key][r].item(): {n: cols[n][r] for n in out.columns if n != key} for r in range(len(cols[key]))}


def test_functions_names_and_refusals():
    from tensorframes_amd import Window
    for name, fn in (("skewness", F.skewness), ("kurtosis", F.kurtosis)):
        e = fn("x")
        assert isinstance(e, F.HighAggregateExpression) and not isinstance(e, F.AggregateExpression)
        assert (e.fn, e.column, e.output_name) == (name, "x", f"{name}(x)") and name in F.__all__
        assert fn(tfs.col("x")).alias("s").output_name == "s" and name not in F.FUNCTIONS
        with pytest.raises(TypeError):
            fn(tfs.col("x") * 2)
    n = 6
    df = tfs.from_columns({"k": np.arange(n, dtype=np.int32) % 2, "s": np.array([f"s{i}" for i in range(n)]),
                           "v": np.zeros((n, 3)), "x": np.arange(n, dtype=np.float64), "p": np.arange(n) % 3})
    rows = tfs.create_dataframe([(True, 1, 1.0), (False, 2, 2.0), (True, 1, 4.5)], ["b", "k", "x"])
    for fn in (F.skewness, F.kurtosis):
        for run in (df.groupBy("k").agg, df.agg):
            for col, err, match in (("s", InvalidTypeException, "string"), ("v", InvalidDimensionException, "scalar"),
                                    ("nope", ValueError, "nope")):
                with pytest.raises(err, match=match):
                    run(fn(col))
        for call, err, match in (
                (lambda: rows.groupBy("k").agg(fn("b")), InvalidTypeException, "bool"),
                (lambda: df.agg({"x": fn("x").fn}), ValueError, "not an aggregate function"),
                (lambda: fn("x").over(Window.partitionBy("k")), NotImplementedError, "not supported over a window"),
                (lambda: df.groupBy("k").pivot("p").agg(fn("x")), NotImplementedError, "pivot"),
                (lambda: df.filter(fn("x")), TypeError, ""), (lambda: df.orderBy(fn("x")), TypeError, ""),
                (lambda: df.select(fn("x")), TypeError, "aggregate expression")):
            with pytest.raises(err, match=match or None):
                call()
    # the bindings refuse a host tensor before anything is read (the rest: tests/test_gpu_high_moments.py)
    host, idx = torch.zeros(4, dtype=torch.float64), torch.zeros(5, dtype=torch.int64)
    for call in (lambda: _C.column_high_moments([host]), lambda: _C.group_high_moments([host], idx[:4], idx),
                 lambda: _C.merge_high_records(torch.zeros((1, 1, 6), dtype=torch.int64), idx),
                 lambda: _C.high_results(torch.zeros((1, 1, 6), dtype=torch.int64), [0], ["skewness"])):
        with pytest.raises(ValueError, match="device tensor"):
            call()
    with pytest.raises(ValueError, match="1..16 columns"):
        _C.column_high_moments([host] * 17)
    with pytest.raises(ValueError, match="at most 16 distinct skewness"):
        wide = tfs.from_columns({f"c{i}": np.arange(4.0) for i in range(17)})
        wide.agg(*[F.skewness(f"c{i}") for i in range(17)])


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_host_records_every_dtype(dt):
    k, x = grouped_columns(dt, seed=3)
    ng = int(k.max()) + 1
    whole = GA._host_high_records([torch.from_numpy(x)], k, ng)
    # two partitions (every group in both: ids ascending), merged in (key, partition) order
    halves = [GA._host_high_records([torch.from_numpy(x[h::2])], k[h::2], ng) for h in (0, 1)]
    present = np.stack([np.bincount(k[h::2], minlength=ng) > 0 for h in (0, 1)], 1).reshape(-1)
    both = np.stack(halves, 1).reshape(2 * ng, 1, 6)[present]
    offsets = np.concatenate([[0], np.cumsum(present.reshape(ng, 2).sum(1))]).astype(np.int64)
    merged = GA._merge_high_records(both, offsets)
    for recs_of, tag in ((whole, "whole"), (merged, "merged")):
        assert recs_of.shape == (ng, 1, 6) and recs_of.dtype == np.int64
        outs = GA._high_results(recs_of, [0, 0], ["skewness", "kurtosis"])
        for g in range(ng):
            rows = x[k == g]
            if exact(rows)["bad"]:
                assert int(recs_of[g, 0, 5]) == 1 and recs_of[g, 0, :1].view(np.float64)[0] == len(rows)
            else:
                check_record(recs_of[g, 0], rows, (dt, g, tag))
            check_value(outs[0][g], "skewness", rows, (dt, g, tag))
            check_value(outs[1][g], "kurtosis", rows, (dt, g, tag))
        assert math.isnan(outs[0][0]) and math.isnan(outs[1][4])        # one row; a constant group
    # the empty record is all zeros, merges away on either side without a changed bit, and has no statistics
    empty, one = np.zeros((1, 1, 6), dtype=np.int64), whole[3:4]
    for a, b in ((empty, one), (one, empty), (empty, empty)):
        assert GA._high_pebay(a, b).tobytes() == (one if (a is one or b is one) else empty).tobytes()
    assert all(math.isnan(o[0]) for o in GA._high_results(empty, [0, 0], ["skewness", "kurtosis"]))


@pytest.mark.parametrize("parts", [1, 3])
@pytest.mark.parametrize("dt", FRAME_DTYPES, ids=lambda d: np.dtype(d).name)
def test_frames_against_the_reference(dt, parts):
    k, x = grouped_columns(dt, seed=5)
    df = tfs.from_columns({"k": k, "x": x}, num_partitions=parts)
    exprs = [F.skewness("x"), F.kurtosis("x").alias("ku"), F.avg("x")]
    out = df.groupBy("k").agg(*exprs)
    assert out.columns == ["k", "skewness(x)", "ku", "avg(x)"]
    rows, plain = keyed_rows(out), keyed_rows(df.groupBy("k").agg(F.avg("x")))
    assert set(rows) == set(np.unique(k).tolist())
    for g, got in rows.items():
        check_value(got["skewness(x)"], "skewness", x[k == g], (dt, parts, g))
        check_value(got["ku"], "kurtosis", x[k == g], (dt, parts, g))
        # avg still comes from the six-field record: the bytes of the call without the new expressions
        assert got["avg(x)"].tobytes() == plain[g]["avg(x)"].tobytes()
    finite = x[k < 5]
    dense = tfs.from_columns({"x": finite}, num_partitions=parts)
    whole = dense.agg(*exprs)
    check_value(whole.to_numpy("skewness(x)")[0], "skewness", finite, (dt, parts))
    check_value(whole.to_numpy("ku")[0], "kurtosis", finite, (dt, parts))
    assert whole.to_numpy("avg(x)").tobytes() == dense.agg(F.avg("x")).to_numpy("avg(x)").tobytes()
    # a group of 0 rows, and (the float dtypes) a non-finite row anywhere: NaN
    for nan in [tfs.from_columns({"x": finite[:0]})] + ([df] if np.dtype(dt).kind == "f" else []):
        assert np.isnan(nan.agg(F.skewness("x")).to_numpy("skewness(x)")[0])
        assert np.isnan(nan.agg(F.kurtosis("x")).to_numpy("kurtosis(x)")[0])


def _spmd_results():
    k, x = grouped_columns(np.float64, seed=7)
    df = tfs.from_columns({"k": k, "x": x, "i": data(np.int32, len(k), 8)}, num_partitions=5)
    exprs = [F.skewness("x"), F.kurtosis("i"), F.stddev("x"), F.corr("x", "i"), F.kurtosis("x")]
    keyed = df.groupBy("k").agg(*exprs).orderBy("k")
    whole = df.agg(*exprs)
    return {"keyed": {c: keyed.to_numpy(c).tobytes().hex() for c in keyed.columns},
            "whole": {c: whole.to_numpy(c).tobytes().hex() for c in whole.columns}}


def _worker(rank, world, port, outdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), OMP_NUM_THREADS="1", TFA_SHM_COLLECTIVES="1", TFA_DEVICE="cpu")
    torch.set_num_threads(1)
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from tensorframes_amd.parallel import dist

    assert dist.init(backend="gloo")
    with open(os.path.join(outdir, f"r{rank}.json"), "w") as f:
        json.dump(_spmd_results(), f)
    dist.shutdown()


def test_two_ranks_give_the_bytes_of_one(tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    single = _spmd_results()
    assert all(json.load(open(tmp_path / f"r{r}.json")) == single for r in range(2))
