"""The device kernel under `groupBy().pivot().agg` (csrc/kernels/pivot.hip:
`_C.pivot_spread`) and the frame path that uses it, on the GPU.

Kernel level: the expected cells come from a plain loop over the arrays written
here. Frame level: the device path is compared with the host path
(tests/test_pivot.py holds that one to its specification). The kernel copies
bits, so every comparison is exact. No test hands the kernel offsets out of
range, descending ranges or lengths that do not agree."""
import json
import os
import socket
import sys
import time

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import tensorframes_amd as tfs
from tensorframes_amd import functions as F
from tensorframes_amd._native import _C

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOP = 1 << 63
DTYPES = (np.int64, np.float64, np.float32, np.int32)
# one fill per dtype: a float64 NaN with a payload, a float32 NaN with a payload, plain integers
FILLS = {np.int64: -7, np.float64: 0x7FF8000000000123, np.float32: 0x7FC00456, np.int32: 0x12345678}


def B():
    return int(_C.pivot_block_threads())


def dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------ the specification
def spread_by_loop(offsets, pivot_words, value_words, vals, fills):
    """[V, G] per column, as unsigned bit patterns: the record of group g whose
    word is value_words[j], else the fill's low bytes."""
    G, V = len(offsets) - 1, len(value_words)
    outs = []
    for v, f in zip(vals, fills):
        u = np.dtype(f"u{v.dtype.itemsize}")
        bits = v.view(u)
        o = np.full((V, G), (int(f) & ((1 << (8 * u.itemsize)) - 1)), dtype=u)
        for g in range(G):
            at = {int(pivot_words[r]): r for r in range(int(offsets[g]), int(offsets[g + 1]))}
            for j in range(V):
                r = at.get(int(value_words[j]))
                if r is not None:
                    o[j, g] = bits[r]
        outs.append(o)
    return outs


def case(G, V, nout, seed=0):
    """(offsets, pivot words, value words, columns, fills). The listed words lie
    on both sides of 1 << 63 and are not sorted; group g has, by g % 6, no
    record, one listed record, every listed value, unlisted words only (before,
    between and after the listed ones), a mix of both, one unlisted record."""
    rng = np.random.default_rng(seed)
    half = V // 2
    listed = [16 + 8 * i for i in range(half)] + [TOP - 8 + 8 * i for i in range(V - half)]  # ascending, unsigned
    between = [w + 3 for w in listed[:: max(1, V // 7)]]
    groups = []
    for g in range(G):
        kind = g % 6
        if kind == 0:
            ws = []
        elif kind == 1:
            ws = [listed[g % V]]
        elif kind == 2:
            ws = list(listed)
        elif kind == 3:
            ws = [3] + between + [(1 << 64) - 5]
        elif kind == 4:
            ws = [5] + listed[g % 2::2] + between[:3] + [(1 << 64) - 2]
        else:
            ws = [between[g % len(between)]]
        groups.append(sorted(set(ws)))
    offsets = np.concatenate([[0], np.cumsum([len(w) for w in groups])]).astype(np.int64)
    m = int(offsets[-1])
    pw = np.array([w for ws in groups for w in ws], dtype=np.uint64)
    vw = np.array(listed, dtype=np.uint64)[rng.permutation(V)]
    vals, fills = [], []
    for a in range(nout):
        dt = DTYPES[a % 4]
        raw = rng.integers(0, 1 << 62, m, dtype=np.int64) * 4 + a           # any bits, NaN patterns among them
        vals.append(raw.astype(np.int64).view(np.uint64).astype(f"u{np.dtype(dt).itemsize}").view(dt))
        fills.append(FILLS[dt] + (a // 4 if np.dtype(dt).kind == "i" else 0))
    return offsets, pw, vw, vals, fills


def run_kernel(offsets, pw, vw, vals, fills):
    outs = _C.pivot_spread(dev(offsets), dev(pw.view(np.int64)), dev(vw.view(np.int64)), [dev(v) for v in vals], fills)
    assert len(outs) == len(vals)
    res = []
    for o, v in zip(outs, vals):
        assert o.is_cuda and tuple(o.shape) == (len(vw), len(offsets) - 1) and o.is_contiguous()
        assert o.cpu().numpy().dtype == v.dtype
        res.append(o.cpu().numpy().view(f"u{v.dtype.itemsize}"))
    return res


def sizes():
    b = B()
    gs = [0, 1, 2, 63, 64, 65, b - 1, b, b + 1, 3 * b + 7]
    vs = [1, 2, 63, 64, 65, 1024]
    pairs = [(g, v) for g in gs for v in (1, 65)] + [(g, v) for v in vs for g in (1, b + 1)]
    return sorted(set(pairs))


def test_kernel_equals_the_loop_at_every_size():
    assert B() % 64 == 0
    for i, (G, V) in enumerate(sizes()):
        offsets, pw, vw, vals, fills = case(G, V, 2 if i % 2 else 1, seed=i)
        assert G < 6 or ((pw >= TOP).any() and (pw < TOP).any())            # a signed compare would misorder these
        assert V < 3 or not np.all(vw[:-1] <= vw[1:])                        # the listed words are not sorted
        got = run_kernel(offsets, pw, vw, vals, fills)
        want = spread_by_loop(offsets, pw, vw, vals, fills)
        for a, (g, w) in enumerate(zip(got, want)):
            np.testing.assert_array_equal(g, w, err_msg=f"G={G} V={V} output {a}")


@pytest.mark.parametrize("nout", [1, 2, 16])
def test_outputs_of_mixed_element_types_and_their_fills(nout):
    G, V = B() + 1, 65
    offsets, pw, vw, vals, fills = case(G, V, nout, seed=40 + nout)
    got = run_kernel(offsets, pw, vw, vals, fills)
    want = spread_by_loop(offsets, pw, vw, vals, fills)
    for a, (g, w) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(g, w, err_msg=f"output {a}")
        fill = int(fills[a]) & ((1 << (8 * g.dtype.itemsize)) - 1)
        assert (g[:, 0] == fill).all() and (g == fill).sum() >= V           # group 0 has no record: the fill's bits
        if vals[a].dtype.kind == "f":
            assert np.isnan(g[:, 0].view(vals[a].dtype)).all()              # the NaN payload came back bit for bit
    again = run_kernel(offsets, pw, vw, vals, fills)
    for g, h in zip(got, again):
        np.testing.assert_array_equal(g, h)                                  # the same bits on every run


def test_no_groups_or_no_values_launch_nothing():
    offsets, pw, vw, vals, fills = case(0, 5, 2)
    got = run_kernel(offsets, pw, vw, vals, fills)
    assert [g.shape for g in got] == [(5, 0), (5, 0)]
    offsets, pw, vw, vals, fills = case(7, 3, 1)
    outs = _C.pivot_spread(dev(offsets), dev(pw.view(np.int64)), dev(vw[:0].view(np.int64)), [dev(vals[0])], fills)
    assert tuple(outs[0].shape) == (0, 7) and outs[0].is_cuda


def test_argument_errors():
    offsets, pw, vw, vals, fills = case(9, 4, 2)
    o, p, v = dev(offsets), dev(pw.view(np.int64)), dev(vw.view(np.int64))
    cols = [dev(x) for x in vals]
    with pytest.raises(ValueError, match="pivot_spread: offsets must be a device tensor"):
        _C.pivot_spread(o.cpu(), p, v, cols, fills)
    with pytest.raises(ValueError, match=r"pivot_spread: vals\[1\] must be a device tensor"):
        _C.pivot_spread(o, p, v, [cols[0], cols[1].cpu()], fills)
    with pytest.raises(TypeError, match="pivot_spread: offsets must be int64"):
        _C.pivot_spread(o.to(torch.int32), p, v, cols, fills)
    with pytest.raises(TypeError, match="pivot_spread: pivot_words must be int64"):
        _C.pivot_spread(o, p.to(torch.float64), v, cols, fills)
    with pytest.raises(TypeError, match="pivot_spread: value_words must be int64"):
        _C.pivot_spread(o, p, v.to(torch.int32), cols, fills)
    with pytest.raises(TypeError, match=r"pivot_spread: vals\[0\] has .* 4- or 8-byte"):
        _C.pivot_spread(o, p, v, [cols[0].to(torch.float16), cols[1]], fills)
    with pytest.raises(ValueError, match=r"pivot_spread: offsets \[G \+ 1\] expected"):
        _C.pivot_spread(o[:0], p, v, cols, fills)
    with pytest.raises(ValueError, match="pivot_spread: offsets must be 1-D"):
        _C.pivot_spread(o.reshape(2, 5), p, v, cols, fills)
    with pytest.raises(ValueError, match=r"pivot_spread: vals\[1\] must be contiguous \[\d+\]"):
        _C.pivot_spread(o, p, v, [cols[0], cols[1][:-1]], fills)
    with pytest.raises(ValueError, match="pivot_spread: 1 fills for 2 outputs"):
        _C.pivot_spread(o, p, v, cols, fills[:1])
    with pytest.raises(ValueError, match=r"pivot_spread: 1\.\.16 outputs per call, got 17"):
        _C.pivot_spread(o, p, v, [cols[0]] * 17, [0] * 17)
    with pytest.raises(ValueError, match=r"pivot_spread: 1\.\.16 outputs per call, got 0"):
        _C.pivot_spread(o, p, v, [], [])
    with pytest.raises(ValueError, match="pivot_spread: at most 1024 values per call, got 1025"):
        _C.pivot_spread(o, p, dev(np.arange(1025, dtype=np.int64)), cols, fills)


# ------------------------------------------------------------------ frames
def frame_columns(n=3000, seed=3):
    """f, g and i hold small multiples of 0.25 and small integers: every sum of
    them is exact in float64, in whatever order it is taken."""
    rng = np.random.default_rng(seed)
    p = np.array([1.5, -0.0, np.nan, 0.0, -2.25, np.inf, 7.0], dtype=np.float32)[rng.integers(0, 7, n)]
    k = rng.integers(0, 400, n).astype(np.int32)
    p[k % 5 == 0] = 7.0                                                     # keys with one pivot value only
    return {"k": k, "d": rng.integers(0, 3, n).astype(np.int64), "p": p,
            "f": (rng.integers(-64, 65, n) * 0.25).astype(np.float32), "g": rng.integers(-4000, 4001, n) * 0.25,
            "i": rng.integers(-1000, 1000, n).astype(np.int32)}


def exprs():
    return [F.count("*"), F.sum("f"), F.avg("g"), F.sum("i"), F.min("f"), F.max("g"), F.stddev_samp("g"),
            F.var_pop("i"), F.corr("f", "g")]


def exact_exprs():
    """The statistics whose arithmetic is exact on frame_columns(). Stage 1 of
    the device path (kernels/group_stats.hip) and of the host path (numpy) are
    different algorithms: their means and M2s agree within the bound of
    tests/test_gpu_group_agg.py, not bit for bit, so only these can be held to
    the host path's bits. The others are held to the bits of the device's own
    `groupBy(keys, p).agg(...)` below: the spread copies bits."""
    return [F.count("*"), F.sum("f"), F.sum("g"), F.sum("i"), F.min("f"), F.max("g"), F.min("g"), F.max("f")]


def pivots(df, exact=False):
    return {"found": df.groupBy("k").pivot("p").agg(*(exact_exprs() if exact else exprs())),
            "listed": df.groupBy("k", "d").pivot("p", [np.nan, 0.0, 9.0, -2.25]).agg(F.sum("f"), F.count("*")),
            "whole": df.groupBy().pivot("p").agg(F.sum("g") if exact else F.avg("g"), F.max("f")),
            "cross": df.crosstab("k", "p")}


def materialise(frames):
    return {name: (o.columns, o.local_blocks()) for name, o in frames.items()}


def bits_of(columns, blocks):
    return {c: np.concatenate([blocks[q].columns[c].cpu().numpy() for q in sorted(blocks)]).tobytes().hex()
            for c in columns}


def _delta(fn):
    keys = ("pivot_device_partitions", "pivot_host_partitions", "pivot_cells")
    before = tfs.metrics.snapshot()
    res = fn()
    after = tfs.metrics.snapshot()
    return res, {k: after.get(k, 0) - before.get(k, 0) for k in keys}


def test_device_frames_have_the_bits_of_the_host_path():
    host = tfs.from_columns(frame_columns(), num_partitions=3)
    on_dev = host.cache_on_device(DEV)
    got, d = _delta(lambda: materialise(pivots(on_dev, exact=True)))
    assert d["pivot_device_partitions"] == 3 * len(got) and d["pivot_host_partitions"] == 0 and d["pivot_cells"] > 0
    want, d = _delta(lambda: materialise(pivots(host, exact=True)))
    assert d["pivot_host_partitions"] == 3 * len(want) and d["pivot_device_partitions"] == 0
    assert got["found"][0][:3] == ["k", "-2.25_count(1)", "-2.25_sum(f)"] and got["found"][0][-1] == "NaN_max(f)"
    for name in want:
        assert got[name][0] == want[name][0]
        assert all(c.is_cuda for b in got[name][1].values() for c in b.columns.values()), name
        assert not any(c.is_cuda for b in want[name][1].values() for c in b.columns.values())
        assert bits_of(*got[name]) == bits_of(*want[name]), name
    assert sum(b.nrows for b in got["found"][1].values()) == len(set(frame_columns()["k"].tolist()))


def test_device_cells_have_the_bits_of_the_device_composite_key_agg():
    on_dev = tfs.from_columns(frame_columns(), num_partitions=3).cache_on_device(DEV)
    wide = on_dev.groupBy("k", "d").pivot("p", [7.0, np.nan, 0.0, 9.0, -2.25]).agg(*exprs())
    texts = ["7.0", "NaN", "0.0", "9.0", "-2.25"]
    long = on_dev.groupBy("k", "d", "p").agg(*exprs())
    lcols = {c: long.to_numpy(c) for c in long.columns}
    cells = {}
    for r in range(len(lcols["k"])):
        p = float(lcols["p"][r])
        cells[(int(lcols["k"][r]), int(lcols["d"][r]), "NaN" if p != p else str(p + 0.0))] = r
    blocks = wide.local_blocks()
    assert all(c.is_cuda for b in blocks.values() for c in b.columns.values())
    wcols = {c: wide.to_numpy(c) for c in wide.columns}
    assert len(wcols["k"]) == len({k[:2] for k in cells})                   # a row for every key, listed value or not
    hits = 0
    for r in range(len(wcols["k"])):
        for t in texts:
            at = cells.get((int(wcols["k"][r]), int(wcols["d"][r]), t))
            for e in exprs():
                g = wcols[f"{t}_{e.output_name}"][r]
                if at is not None:
                    hits += 1
                    w = lcols[e.output_name][at]
                else:
                    w = np.zeros((), np.int64) if g.dtype == np.int64 else np.array(np.nan, dtype=g.dtype)
                assert g.dtype == w.dtype and g.tobytes() == np.asarray(w).tobytes(), (r, t, e.output_name, g, w)
    assert hits > 1000 and "9.0" not in {k[2] for k in cells}


def test_a_partition_on_the_host_takes_every_partition_to_the_host_path():
    from tensorframes_amd.frame.dataframe import DataFrame, _Materialized
    host = tfs.from_columns(frame_columns(900, seed=4), num_partitions=3)
    blocks = {q: (b if q == 1 else b.to(torch.device(DEV))) for q, b in host.local_blocks().items()}
    mixed = DataFrame(host.schema, _Materialized(blocks), 3)
    mixed._persist, mixed._cached = True, blocks
    got, d = _delta(lambda: materialise({"found": mixed.groupBy("k").pivot("p").agg(*exprs())}))
    assert d["pivot_host_partitions"] == 3 and d["pivot_device_partitions"] == 0
    want = materialise({"found": host.groupBy("k").pivot("p").agg(*exprs())})
    assert bits_of(*got["found"]) == bits_of(*want["found"])


# ------------------------------------------------------------------ two ranks, one GPU
KEYS = {"found": ["k"], "listed": ["k", "d"], "whole": [], "cross": ["k_p"]}


def _results(df):
    """Every result gathered and put in ascending key order (the ranks'
    partitions interleave the keys), each column as the hex of its bytes."""
    out = {}
    for name, o in pivots(df).items():
        blocks = o.local_blocks()
        cols = {c: o.to_numpy(c) for c in o.columns}
        order = np.lexsort([cols[k] for k in reversed(KEYS[name])]) if KEYS[name] else np.arange(len(cols[o.columns[0]]))
        out[name] = {"cols": {c: np.ascontiguousarray(v[order]).tobytes().hex() for c, v in cols.items()},
                     "rows": int(len(order)),
                     "on_device": all(c.is_cuda for b in blocks.values() if b.nrows for c in b.columns.values())}
    return out


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, outdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), OMP_NUM_THREADS="1", TFA_SHM_COLLECTIVES="1")
    torch.set_num_threads(1)
    sys.path.insert(0, REPO)
    from tensorframes_amd import engine
    from tensorframes_amd.parallel import dist

    assert dist.init(backend="gloo")
    res = _results(tfs.from_columns(frame_columns(), num_partitions=5).cache_on_device(None))
    res["device"] = engine.compute_device().type
    with open(os.path.join(outdir, f"r{rank}.json"), "w") as f:
        json.dump(res, f)
    dist.shutdown()


def test_pivot_two_ranks_share_one_gpu(tmp_path):
    ctx = mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=False)
    deadline = time.monotonic() + 120
    while not ctx.join(timeout=1):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("the ranks did not finish in 120 s")
    outs = [json.load(open(tmp_path / f"r{r}.json")) for r in range(2)]
    single = _results(tfs.from_columns(frame_columns(), num_partitions=5).cache_on_device(DEV))
    for o in outs:
        assert o.pop("device") == "cuda"
        assert o == single                                          # every output column, byte for byte; on the device
    assert all(v["on_device"] and v["rows"] for v in single.values())
