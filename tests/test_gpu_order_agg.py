"""The device kernels under median / percentile / mode / countDistinct
(csrc/kernels/group_order.hip: group_order_summary, group_order_finish) and
the frame paths that use them, on the GPU.

Kernel level: expected values are brute force written here, from a plain loop
over the ordering words (`heads`, in the style of tests/test_gpu_window.py);
all of `group_order_summary` is integers and compared exactly. The outputs of
`group_order_finish` are compared bit for bit with the specification of
tests/order_agg_cases.py: typed results are words decoded back, and the
interpolation of `percentile` is the same two rounded products and one rounded
sum on both sides (a contracted multiply-add would show on the random float64
values at p = 0.1 or 0.3).

Frame level: device-cached frames against the host path of the same frames,
bit for bit. No test hands a kernel an index out of range or lengths that do
not agree."""
import json
import os
import socket
import sys
import time

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import order_agg_cases as oc
import tensorframes_amd as tfs
from tensorframes_amd import functions as F
from tensorframes_amd._native import _C

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.uint8, np.int8, np.int16, np.int32, np.int64, np.float32, np.float64]
Q16 = [0.0, 0.05, 0.1, 0.2, 0.25, 0.3, 0.4, 0.5, 0.6, 0.7, 0.75, 0.8, 0.9, 0.95, 0.99, 1.0]


def C():
    return int(_C.group_order_chunk_rows())


def T():
    return int(_C.window_tile_rows())


def U():
    return int(_C.unique_tile_rows())


def dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def words_of(group_lengths, peer_lengths=None, gw=1, pw=1):
    """uint64 [gw + pw, n]: the first gw words change at every group, the
    others at every peer run (peer_lengths: run lengths over all rows; default
    one run per row)."""
    n = int(sum(group_lengths))
    g = np.repeat(np.arange(len(group_lengths), dtype=np.uint64) * np.uint64(3) + np.uint64(5), group_lengths)
    if peer_lengths is None:
        p = np.arange(n, dtype=np.uint64)
    else:
        assert sum(peer_lengths) == n
        p = np.repeat(np.arange(len(peer_lengths), dtype=np.uint64), peer_lengths)
    # (only the last word of a kind changes; the others are constant)
    rows = [np.full(n, 9, dtype=np.uint64)] * (gw - 1) + [g] * (gw > 0) + [np.full(n, 4, dtype=np.uint64)] * (pw - 1) + \
        [p] * (pw > 0)
    return np.stack(rows, 0)


def heads(words, P):
    """(group head, peer head) flags by a plain loop over the rows."""
    W, n = words.shape
    gh, ph = [False] * n, [False] * n
    for m in range(n):
        if m == 0:
            gh[m] = ph[m] = True
            continue
        ph[m] = any(int(words[w, m]) != int(words[w, m - 1]) for w in range(W))
        gh[m] = any(int(words[w, m]) != int(words[w, m - 1]) for w in range(P))
    return gh, ph


def brute_summary(words, P):
    W, n = words.shape
    gh, ph = heads(words, P)
    starts = [i for i in range(n) if gh[i]] + [n]
    distinct, mode_pos, mode_len = [], [], []
    for a, b in zip(starts[:-1], starts[1:]):
        runs = [i for i in range(a, b) if ph[i]]
        lens = [e - s for s, e in zip(runs, runs[1:] + [b])]
        best = max(range(len(runs)), key=lambda j: (lens[j], -runs[j]))     # the longest, then the first
        distinct.append(len(runs))
        mode_pos.append(runs[best])
        mode_len.append(lens[best])
    return starts, distinct, mode_pos, mode_len


def summary(words, P):
    got = _C.group_order_summary(dev(words.view(np.int64)), P)
    assert all(t.dtype == torch.int64 and t.is_cuda for t in got)
    return [t.cpu().numpy().tolist() for t in got]


def check_summary(words, P):
    got = summary(words, P)
    want = brute_summary(words, P)
    for name, g, w in zip(("starts", "distinct", "mode_pos", "mode_len"), got, want):
        assert g == w, (name, words.shape, P)


def split(n, rng, mean):
    """Random lengths that add up to n."""
    out = []
    while n > 0:
        k = int(min(n, max(1, rng.geometric(1.0 / mean))))
        out.append(k)
        n -= k
    return out


# ------------------------------------------------------------------ group_order_summary
def sizes():
    c = C()
    s = {1, 2, 63, 64, 65, c - 1, c, c + 1, 2 * c + 7, 5 * c + 3}
    for t in (T(), U()):
        s |= {t - 1, t, t + 1, 2 * t + 7}
    return sorted(s)


def test_summary_sizes_around_the_chunk_and_tile_edges():
    rng = np.random.default_rng(1)
    for n in sizes():
        check_summary(words_of([1] * n), 1)                                  # every row its own group
        check_summary(words_of([n], split(n, rng, 3)), 1)                    # one group holding every row
        check_summary(words_of(split(n, rng, 40), split(n, rng, 2)), 1)      # (group heads are peer heads: word 0)


def test_summary_groups_that_end_at_chunk_and_tile_edges():
    c, t = C(), T()
    rng = np.random.default_rng(2)
    lengths = [c, 2 * c, c, t - 4 * c if t > 4 * c else c, t, 3, c - 3, 2 * t, 1]
    n = sum(lengths)
    check_summary(words_of(lengths, split(n, rng, 5)), 1)
    check_summary(words_of(lengths), 1)


def test_summary_peer_runs_and_the_mode_rule():
    c = C()
    runs = [1, 2, 64, c + 1, 5, 2, 1]
    w = words_of([sum(runs)], runs)
    got = summary(w, 1)
    assert got[1] == [len(runs)] and got[2] == [67] and got[3] == [c + 1]
    check_summary(w, 1)
    # two longest runs of equal length: the first wins
    w = words_of([20], [3, 7, 2, 7, 1])
    assert summary(w, 1)[2:] == [[3], [7]]
    w = words_of([4, 20, 6], [4, 3, 7, 2, 7, 1, 2, 2, 2])
    assert summary(w, 1)[1:] == [[1, 5, 3], [0, 7, 24], [4, 7, 2]]
    # the longest run straddles a chunk edge (and its head lies in the chunk before)
    runs = [1] * (c - 20) + [45] + [1] * 30 + [44] + [1] * (c - 7)
    w = words_of([sum(runs)], runs)
    assert summary(w, 1)[2:] == [[c - 20], [45]]
    check_summary(w, 1)
    # ... in a group that starts off the chunk grid, after another group
    w = words_of([37, sum(runs)], [37] + runs)
    assert summary(w, 1)[2:] == [[0, 37 + c - 20], [37, 45]]
    check_summary(w, 1)


def test_summary_without_keys_with_eight_words_and_without_rows():
    rng = np.random.default_rng(3)
    n = 2 * C() + 7
    w = words_of([n], split(n, rng, 4), gw=0, pw=1)                          # P == 0: one group
    got = summary(w, 0)
    assert got[0] == [0, n]
    check_summary(w, 0)
    check_summary(words_of(split(n, rng, 30), split(n, rng, 3), gw=3, pw=5), 3)   # W == 8
    check_summary(words_of(split(n, rng, 30), split(n, rng, 3), gw=7, pw=1), 7)
    w8 = words_of(split(n, rng, 30), gw=8, pw=0)                             # P == W: every group one run
    got = summary(w8, 8)
    assert got[1] == [1] * (len(got[0]) - 1) and got[3] == np.diff(got[0]).tolist()
    empty = _C.group_order_summary(torch.empty((2, 0), dtype=torch.int64, device=DEV), 1)   # nothing is launched
    assert [tuple(t.shape) for t in empty] == [(1,), (0,), (0,), (0,)] and empty[0].tolist() == [0]


def test_summary_heavy_group_and_equal_bytes_on_every_run():
    c = C()
    rng = np.random.default_rng(4)
    lengths = split(3 * c, rng, 20) + [20 * c + 5] + split(2 * c, rng, 20)    # one key holds most of the rows
    n = sum(lengths)
    w = words_of(lengths, split(n, rng, 3))
    check_summary(w, 1)
    d = dev(w.view(np.int64))
    a = [t.cpu().numpy().tobytes() for t in _C.group_order_summary(d, 1)]
    b = [t.cpu().numpy().tobytes() for t in _C.group_order_summary(d, 1)]
    assert a == b


def test_summary_words_one_element_into_their_buffer():
    rng = np.random.default_rng(5)
    n = C() + 9                                                              # (odd: row 1 of the words is 16-byte aligned)
    w = words_of(split(n, rng, 25), split(n, rng, 2))
    buf = torch.zeros(2 * n + 1, dtype=torch.int64, device=DEV)
    buf[1:] = dev(w.view(np.int64)).reshape(-1)
    view = buf[1:].view(2, n)
    assert view.data_ptr() % 16 == 8 and view.is_contiguous()
    got = [t.cpu().numpy().tolist() for t in _C.group_order_summary(view, 1)]
    assert got == [list(x) for x in brute_summary(w, 1)]


# ------------------------------------------------------------------ group_order_finish
def values_of(dt, n, rng):
    dt = np.dtype(dt)
    if dt.kind == "f":
        x = (rng.standard_normal(n) * 3).astype(dt)
        ties = rng.random(n) < 0.3
        x[ties] = np.round(x[ties])
        for v, k in ((np.nan, 5), (-0.0, 3), (0.0, 3), (np.inf, 2), (-np.inf, 1)):
            x[rng.integers(0, n, k)] = v
        return x
    info = np.iinfo(dt)
    x = rng.integers(max(info.min, -9), min(info.max, 9) + 1, n).astype(dt)
    x[rng.integers(0, n, 3)] = info.max
    x[rng.integers(0, n, 3)] = info.min
    return x


FNS = ["count_distinct", "mode", "percentile_approx", "percentile_approx", "percentile", "percentile"]
PCTS = [[], [], [0.3], Q16, [0.5], Q16]
CASES = [("d", "count_distinct", ("x",), [], False), ("m", "mode", ("x",), [], False),
         ("a1", "percentile_approx", ("x",), [0.3], True), ("a16", "percentile_approx", ("x",), Q16, True),
         ("p1", "percentile", ("x",), [0.5], True), ("p16", "percentile", ("x",), Q16, True)]


def sorted_case(dt, seed, lengths):
    """The columns g, x in sorted order."""
    rng = np.random.default_rng(seed)
    g = np.repeat(np.arange(len(lengths), dtype=np.int32), lengths)
    x = values_of(dt, len(g), rng)
    perm = np.lexsort([oc.spec_words(x), g])
    return {"g": g[perm], "x": x[perm]}


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_finish_every_dtype_and_function(dt):
    cols = sorted_case(dt, 11, [1, 2, 3, C() + 1, 5, 64, 2, 1])
    n = len(cols["g"])
    w = np.stack([oc.spec_words(cols["g"]), oc.spec_words(cols["x"])], 0).view(np.int64)
    buf = torch.zeros(2 * n + 1, dtype=torch.int64, device=DEV)              # the words one element into their buffer
    buf[1:] = dev(w).reshape(-1)
    words = buf[1:].view(2, n)
    assert words.data_ptr() % 16 == 8
    if np.dtype(dt) in (np.dtype(np.int32), np.dtype(np.int64), np.dtype(np.float32), np.dtype(np.float64)):
        enc = _C.sort_encode([dev(cols["g"]), dev(cols["x"])], [False, False])   # (what the frame layer hands in)
        assert torch.equal(enc, words)
    summ = _C.group_order_summary(words, 1)
    outs = _C.group_order_finish(words, *summ, FNS, PCTS, torch.from_numpy(np.zeros(0, dtype=dt)).dtype)
    _, want = oc.spec(cols, ["g"], CASES)
    for (name, *_), got in zip(CASES, outs):
        got = got.cpu().numpy()
        assert got.dtype == want[name].dtype and got.shape == want[name].shape, name
        assert got.tobytes() == want[name].tobytes(), (name, got, want[name])


def test_finish_random_float64_is_not_contracted():
    rng = np.random.default_rng(12)
    lengths = split(3000, rng, 12)
    g = np.repeat(np.arange(len(lengths), dtype=np.int32), lengths)
    x = 1e4 + rng.standard_normal(len(g))
    perm = np.lexsort([oc.spec_words(x), g])
    cols = {"g": g[perm], "x": x[perm]}
    words = _C.sort_encode([dev(cols["g"]), dev(cols["x"])], [False, False])
    summ = _C.group_order_summary(words, 1)
    got = _C.group_order_finish(words, *summ, ["percentile"], [Q16], torch.float64)[0].cpu().numpy()
    _, want = oc.spec(cols, ["g"], [("p", "percentile", ("x",), Q16, True)])
    assert got.tobytes() == want["p"].tobytes()


def test_bindings_refuse_what_does_not_fit():
    n = 10
    w = words_of([4, 6], [2, 2, 3, 3]).view(np.int64)
    d = dev(w)
    with pytest.raises(ValueError, match="device"):
        _C.group_order_summary(torch.from_numpy(w), 1)
    with pytest.raises(TypeError, match="int64"):
        _C.group_order_summary(d.to(torch.int32), 1)
    with pytest.raises(ValueError, match="P"):
        _C.group_order_summary(d, 3)                                          # P > W
    with pytest.raises(ValueError, match="P"):
        _C.group_order_summary(d, -1)
    with pytest.raises(ValueError, match="words per row"):
        _C.group_order_summary(dev(np.zeros((9, n), dtype=np.int64)), 1)      # W > 8
    with pytest.raises(ValueError, match="contiguous"):
        _C.group_order_summary(dev(np.zeros((n, 2), dtype=np.int64)).t(), 1)
    starts, distinct, mode_pos, mode_len = _C.group_order_summary(d, 1)
    ok = (["mode"], [[]], torch.float32)
    assert len(_C.group_order_finish(d, starts, distinct, mode_pos, mode_len, *ok)) == 1
    with pytest.raises(ValueError, match="device"):
        _C.group_order_finish(d, starts.cpu(), distinct, mode_pos, mode_len, *ok)
    with pytest.raises(ValueError, match="device"):
        _C.group_order_finish(d.cpu(), starts, distinct, mode_pos, mode_len, *ok)
    with pytest.raises(TypeError, match="int64"):
        _C.group_order_finish(d, starts, distinct.to(torch.int32), mode_pos, mode_len, *ok)
    with pytest.raises(ValueError, match="entries"):                          # lengths that do not agree
        _C.group_order_finish(d, starts, distinct, mode_pos[:1], mode_len, *ok)
    with pytest.raises(ValueError, match="entries"):
        _C.group_order_finish(d, starts, torch.cat([distinct, distinct]), mode_pos, mode_len, *ok)
    with pytest.raises(ValueError, match="groups for"):
        _C.group_order_finish(d[:, :0].contiguous(), starts, distinct, mode_pos, mode_len, *ok)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        _C.group_order_finish(d, starts, distinct, mode_pos, mode_len, ["percentile"], [[0.5, 1.5]], torch.float32)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        _C.group_order_finish(d, starts, distinct, mode_pos, mode_len, ["percentile_approx"], [[float("nan")]],
                              torch.float32)
    with pytest.raises(ValueError, match="percentages"):
        _C.group_order_finish(d, starts, distinct, mode_pos, mode_len, ["percentile"], [[0.5] * 17], torch.float32)
    with pytest.raises(ValueError, match="percentages"):
        _C.group_order_finish(d, starts, distinct, mode_pos, mode_len, ["percentile"], [[]], torch.float32)
    with pytest.raises(ValueError, match="percentages"):
        _C.group_order_finish(d, starts, distinct, mode_pos, mode_len, ["mode"], [[0.5]], torch.float32)
    with pytest.raises(ValueError, match="not an order aggregate"):
        _C.group_order_finish(d, starts, distinct, mode_pos, mode_len, ["avg"], [[]], torch.float32)
    with pytest.raises(ValueError, match="outputs"):
        _C.group_order_finish(d, starts, distinct, mode_pos, mode_len, ["mode"] * 17, [[]] * 17, torch.float32)
    with pytest.raises(TypeError, match="not supported"):
        _C.group_order_finish(d, starts, distinct, mode_pos, mode_len, ["mode"], [[]], torch.float16)


# ------------------------------------------------------------------ frames
def frame_columns(n, seed, heavy=True):
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, 9, n)
    if heavy:
        ids = np.where(rng.random(n) < 0.6, 4, ids)                           # one key holds 60 % of the rows
    return {"id": ids.astype(np.int32), "score": np.round(rng.standard_normal(n) * 4, 0).astype(np.float32) / 2,
            "label": rng.integers(0, 5, n).astype(np.int64), "x": 1e4 + rng.standard_normal(n),
            "i": np.arange(n, dtype=np.int64)}


def uneven(cols, nparts, empty):
    """A frame whose partition `empty` loses all of its rows (dropped with filter)."""
    n = len(cols["i"])
    edges = [(p * n) // nparts for p in range(nparts + 1)]
    keep = np.ones(n, dtype=bool)
    if nparts > 1:
        keep[edges[empty]:edges[empty + 1]] = False
    df = tfs.from_columns(dict(cols, keep=keep.astype(np.int32)), num_partitions=nparts)
    return df.filter(df.keep > 0).select(*cols)


def exprs():
    return [F.median("score"), F.percentile("x", [0.1, 0.5, 0.9]), F.percentile_approx("score", [0.25, 0.75]),
            F.mode("score"), F.mode("label"), F.countDistinct("label"), F.countDistinct("label", "score"),
            F.approx_count_distinct("score"), F.percentile_approx("x", 0.3)]


def bits(out):
    return {c: out.to_numpy(c).tobytes().hex() for c in out.columns}


def on_device(out):
    return all(c.is_cuda for b in out.local_blocks().values() if b.nrows for c in b.columns.values())


@pytest.mark.parametrize("nparts", [1, 3, 7])
def test_device_frames_give_the_bits_of_the_host_path(nparts):
    cols = frame_columns(C() + 700, 20 + nparts)
    host = uneven(cols, nparts, empty=1)
    device = host.cache_on_device(DEV)
    before = tfs.metrics.snapshot().get("order_agg_device_partitions", 0)
    got = device.groupBy("id").agg(*exprs())
    want = host.groupBy("id").agg(*exprs())
    assert on_device(got) and got.num_partitions == nparts
    assert bits(got) == bits(want)
    assert tfs.metrics.snapshot().get("order_agg_device_partitions", 0) > before
    if nparts == 7:                                                           # the heavy key spans partitions
        srt = device.select("id", "score").orderBy("id", "score")
        assert sum(1 for b in srt.local_blocks().values() if b.nrows and bool((b.columns["id"] == 4).any())) >= 3
    assert bits(device.agg(*exprs())) == bits(host.agg(*exprs()))
    mixed = [F.avg("x"), F.median("score"), F.count("*"), F.countDistinct("label")]
    both = bits(device.groupBy("id").agg(*mixed).orderBy("id"))
    # (the moment aggregates of the device path are not the host path's bit for bit: they are held to the device's)
    moments = bits(device.groupBy("id").agg(F.avg("x"), F.count("*")).orderBy("id"))
    order = bits(host.groupBy("id").agg(F.median("score"), F.countDistinct("label")))
    assert list(both) == ["id", "avg(x)", "median(score)", "count(1)", "count(DISTINCT label)"]
    assert {c: both[c] for c in moments} == moments and {c: both[c] for c in order} == order


def test_device_partition_metric_counts_the_partitions():
    cols = frame_columns(900, 31)
    device = tfs.from_columns(cols, num_partitions=3).cache_on_device(DEV)
    before = tfs.metrics.snapshot()
    assert device.groupBy("id").agg(F.median("score"), F.mode("score")).count() == len(set(cols["id"].tolist()))
    after = tfs.metrics.snapshot()
    assert after.get("order_agg_device_partitions", 0) - before.get("order_agg_device_partitions", 0) == 3
    assert after.get("order_agg_host_partitions", 0) == before.get("order_agg_host_partitions", 0)
    assert after.get("order_agg_rows", 0) - before.get("order_agg_rows", 0) == 900
    assert after.get("order_agg_sorts", 0) - before.get("order_agg_sorts", 0) == 1


def test_readme_example_on_a_device_frame():
    cols = frame_columns(500, 12, heavy=False)
    scored = tfs.from_columns(cols, num_partitions=3).cache_on_device(DEV)
    out = scored.groupBy("id").agg(F.median("score"), F.percentile_approx("score", [0.25, 0.75]),
                                   F.countDistinct("label"), F.avg("score"))
    assert out.columns == ["id", "median(score)", "percentile_approx(score, array(0.25, 0.75), 10000)",
                           "count(DISTINCT label)", "avg(score)"]
    ids = out.to_numpy("id")
    med, cd = out.to_numpy("median(score)"), out.to_numpy("count(DISTINCT label)")
    for j, g in enumerate(ids.tolist()):
        sel = cols["id"] == g
        assert med[j] == np.median(cols["score"][sel].astype(np.float64))
        assert cd[j] == len(set(cols["label"][sel].tolist()))
    whole = scored.agg(F.mode("label"), F.approx_count_distinct("id"))
    vals, counts = np.unique(cols["label"], return_counts=True)
    assert whole.to_numpy("mode(label)").tolist() == [int(vals[np.argmax(counts)])]
    assert whole.to_numpy("approx_count_distinct(id)").tolist() == [len(set(cols["id"].tolist()))]


# ------------------------------------------------------------------ two ranks, one GPU
def _results(df):
    # (one sort: the result stays where the frame is cached; several sorts are joined, and a join across ranks
    # gathers its right side through the host)
    one = df.groupBy("id").agg(F.median("score"), F.mode("score"), F.countDistinct("score"))
    return {"cols": bits(df.groupBy("id").agg(*exprs())), "one": bits(one), "on_device": on_device(one),
            "whole": bits(df.agg(*exprs()))}


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
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import tensorframes_amd as tfs
    from tensorframes_amd import engine
    from tensorframes_amd.parallel import dist

    assert dist.init(backend="gloo")
    cols = frame_columns(C() + 700, 13)
    res = _results(tfs.from_columns(cols, num_partitions=5).cache_on_device())
    res["device"] = engine.compute_device().type
    with open(os.path.join(outdir, f"r{rank}.json"), "w") as f:
        json.dump(res, f)
    dist.shutdown()


def test_order_agg_two_ranks_share_one_gpu(tmp_path):
    ctx = mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=False)
    deadline = time.monotonic() + 120
    while not ctx.join(timeout=1):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("the ranks did not finish in 120 s")
    outs = [json.load(open(tmp_path / f"r{r}.json")) for r in range(2)]
    cols = frame_columns(C() + 700, 13)
    single = _results(tfs.from_columns(cols, num_partitions=5).cache_on_device(DEV))
    assert single["on_device"]
    for o in outs:
        assert o["device"] == "cuda" and o["on_device"]
        assert o["cols"] == single["cols"] and o["one"] == single["one"]        # every output column, byte for byte
        assert o["whole"] == single["whole"]
