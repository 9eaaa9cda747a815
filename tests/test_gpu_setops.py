"""The device kernel under `dropDuplicates` / `distinct`
(csrc/kernels/unique.hip: `_C.unique_rows`) and the frame paths that use it,
on the GPU.

Kernel level: the expected row indices come from a plain loop over the words
written here. Frame level: the device path is compared with the host path
(tests/test_setops.py holds that one to its specification). Outputs are row
indices and bitwise row copies, so every comparison is exact.
No test hands the kernel an index out of range or lengths that do not agree."""
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
from tensorframes_amd._native import _C

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANE_ROWS, WAVE_ROWS = 8, 512                       # positions of a lane, of a wave of the kernel


def T():
    return int(_C.unique_tile_rows())


def dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------ the specification
def heads_by_loop(words: np.ndarray, perm=None):
    """perm[i] of every position i whose word tuple differs from position i - 1's."""
    W, n = words.shape
    order = list(range(n)) if perm is None else [int(p) for p in perm]
    kept = []
    for i, r in enumerate(order):
        if i == 0 or any(int(words[w, r]) != int(words[w, order[i - 1]]) for w in range(W)):
            kept.append(r)
    return kept


def words_of_runs(lengths, W=1):
    """uint64 [W, n]: the last word changes at every run, the others are constant."""
    ids = np.repeat(np.arange(len(lengths), dtype=np.uint64) * np.uint64(3) + np.uint64(5), lengths)
    return np.stack([np.full(len(ids), 7 + w, dtype=np.uint64) for w in range(W - 1)] + [ids], 0)


def run_kernel(words: np.ndarray, perm=None):
    got = _C.unique_rows(dev(words.view(np.int64)), None if perm is None else dev(np.asarray(perm, dtype=np.int64)))
    assert got.is_cuda and got.dtype == torch.int64 and got.dim() == 1
    return got.cpu().numpy()


def check_runs(lengths, W=1):
    words = words_of_runs(lengths, W)
    got = run_kernel(words)
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64) if len(lengths) else np.zeros(0, np.int64)
    assert got.tolist() == starts.tolist() == heads_by_loop(words)
    return got


# ------------------------------------------------------------------ the kernel
def sizes():
    t = T()
    return [0, 1, 2, 63, 64, 65, t - 1, t, t + 1, 2 * t + 100]


@pytest.mark.parametrize("which", range(10))
def test_every_size_random_runs_all_distinct_and_all_equal(which):
    n = sizes()[which]
    rng = np.random.default_rng(n)
    words = np.sort(rng.integers(0, max(n // 3, 2), n).astype(np.uint64))[None, :]
    assert run_kernel(words).tolist() == heads_by_loop(words)
    distinct = (np.arange(n, dtype=np.uint64) * np.uint64(2))[None, :]
    assert run_kernel(distinct).tolist() == list(range(n))
    same = np.full((1, n), 9, dtype=np.uint64)
    assert run_kernel(same).tolist() == ([0] if n else [])


def test_runs_that_end_at_lane_wave_and_tile_boundaries():
    t = T()
    # run boundaries at positions 63, 64 and 65, at a lane's end (8, 504), a wave's end (512, 1024), the
    # tile's end (t), one short of it and one past it
    cuts = [8, 63, 64, 65, WAVE_ROWS - LANE_ROWS, WAVE_ROWS, 2 * WAVE_ROWS, t - 1, t, t + 1, t + WAVE_ROWS, 2 * t]
    n = 2 * t + 100
    lengths = np.diff([0] + cuts + [n]).tolist()
    got = check_runs(lengths)
    assert got.tolist() == [0] + cuts
    # a run that ends exactly with the tile and the wave: the next head is the first position of a tile
    check_runs([t, t])
    check_runs([WAVE_ROWS] * 5)


def test_runs_of_length_1_2_64_and_more_than_a_tile():
    t = T()
    check_runs([1, 2, 64, t + 1, 1, 1, 2, 64, 2, 1])
    check_runs([t + 1, t + 1])
    check_runs([2] * (t // 2 + 37))
    check_runs([64] * 40 + [1] * 70)


@pytest.mark.parametrize("W", [1, 8])
def test_only_the_last_word_differs(W):
    t = T()
    rng = np.random.default_rng(W)
    lengths = rng.integers(1, 9, t // 2).tolist()
    words = words_of_runs(lengths, W)
    assert words.shape[0] == W
    got = run_kernel(words)
    assert got.tolist() == heads_by_loop(words) and len(got) == len(lengths)
    # every word but one constant, the differing word in the middle
    if W == 8:
        mid = words[[0, 1, 2, 7, 3, 4, 5, 6]]
        assert run_kernel(mid).tolist() == heads_by_loop(mid)


@pytest.mark.parametrize("n", [65, 2 * 2048 + 100])
def test_with_the_order_of_the_radix_argsort(n):
    rng = np.random.default_rng(n)
    a = rng.integers(-20, 20, n).astype(np.int32)
    b = rng.choice(np.array([0.0, -0.0, np.nan, 1.5], dtype=np.float32), n)
    words = _C.sort_encode([dev(a), dev(b)], [False, False])
    perm = _C.sort_argsort(words)
    kept = _C.unique_rows(words, perm)
    hw, hp = words.cpu().numpy().view(np.uint64), perm.cpu().numpy()
    want = heads_by_loop(hw, hp)
    assert kept.cpu().numpy().tolist() == want
    # the stable order makes every kept row the first of its key tuple in input order
    first = {}
    for i in range(n):
        first.setdefault((int(hw[0, i]), int(hw[1, i])), i)
    assert want == [first[k] for k in sorted(first)]
    # the kept rows are ready for the row gather
    (ga,) = _C.take_rows(kept, [dev(a)])
    assert ga.cpu().numpy().tolist() == a[want].tolist()


def test_two_runs_give_equal_bytes():
    n = 2 * T() + 100
    rng = np.random.default_rng(5)
    words = dev(np.sort(rng.integers(0, 500, n)).astype(np.int64)[None, :])
    perm = torch.arange(n, dtype=torch.int64, device=DEV)
    a, b, c = _C.unique_rows(words, None), _C.unique_rows(words, None), _C.unique_rows(words, perm)
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() == c.cpu().numpy().tobytes()


def test_the_bindings_refuse():
    w = torch.zeros((2, 16), dtype=torch.int64, device=DEV)
    p = torch.arange(16, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="unique_rows: the words must be a device tensor"):
        _C.unique_rows(w.cpu(), None)
    with pytest.raises(TypeError, match="unique_rows: the words must be int64"):
        _C.unique_rows(w.to(torch.int32), None)
    with pytest.raises(ValueError, match=r"unique_rows: words \[W, n\] expected"):
        _C.unique_rows(w[0], None)
    with pytest.raises(ValueError, match="unique_rows: 1..8 words per row, got 9"):
        _C.unique_rows(torch.zeros((9, 4), dtype=torch.int64, device=DEV), None)
    with pytest.raises(ValueError, match="unique_rows: 1..8 words per row, got 0"):
        _C.unique_rows(torch.zeros((0, 4), dtype=torch.int64, device=DEV), None)
    with pytest.raises(ValueError, match="unique_rows: the words must be contiguous"):
        _C.unique_rows(torch.zeros((16, 2), dtype=torch.int64, device=DEV).t(), None)
    with pytest.raises(ValueError, match=r"unique_rows: the order must hold one entry per row \(\[16\]\)"):
        _C.unique_rows(w, p[:15])
    with pytest.raises(ValueError, match="unique_rows: the order must be a device tensor on the words' device"):
        _C.unique_rows(w, p.cpu())
    with pytest.raises(TypeError, match="unique_rows: the order must be int64"):
        _C.unique_rows(w, p.to(torch.int32))
    assert _C.unique_rows(w, p).cpu().tolist() == [0]


# ------------------------------------------------------------------ frames
def frame_columns(n, seed):
    rng = np.random.default_rng(seed)
    return {
        "id": rng.integers(0, n // 4, n).astype(np.int32),        # about four rows per key
        "f": rng.choice(np.array([0.0, -0.0, np.nan, 1.5, -1.5], dtype=np.float32), n),
        "v": rng.standard_normal((n, 3)).astype(np.float32),
        "x": rng.standard_normal(n),
        "i": np.arange(n, dtype=np.int64),
    }


def on_device(df):
    return all(c.is_cuda for b in df.local_blocks().values() if b.nrows for c in b.columns.values())


def same_bytes(device, host):
    assert device.columns == host.columns and device.num_partitions == host.num_partitions
    assert {p: b.nrows for p, b in device.local_blocks().items()} == {p: b.nrows for p, b in host.local_blocks().items()}
    for name in host.columns:
        assert device.to_numpy(name).tobytes() == host.to_numpy(name).tobytes(), name


_HOST = {}


def host_result(n):
    """The host path's result rows of the 3T + 100 row frame: the same for every partitioning."""
    if n not in _HOST:
        out = tfs.from_columns(frame_columns(n, 21), num_partitions=1).dropDuplicates(["id", "f"])
        _HOST[n] = {c: out.to_numpy(c).tobytes() for c in out.columns}
    return _HOST[n]


@pytest.mark.parametrize("nparts", [1, 3, 7])
def test_device_resident_frames_match_the_host_path(nparts):
    n = 3 * T() + 100                                              # (more than one tile in a partition of three)
    host_df = tfs.from_columns(frame_columns(n, 21), num_partitions=nparts)
    before = tfs.metrics.snapshot().get("distinct_device_partitions", 0)
    device = host_df.cache_on_device(DEV).dropDuplicates(["id", "f"])
    assert on_device(device)
    assert tfs.metrics.snapshot().get("distinct_device_partitions", 0) - before >= nparts
    same_bytes(device, host_df.dropDuplicates(["id", "f"]))
    for name, want in host_result(n).items():
        assert device.to_numpy(name).tobytes() == want, name


def test_an_empty_and_a_one_row_partition():
    n = 2 * T() + 300
    cols = frame_columns(n, 22)
    nparts, empty, one_row = 7, 3, 5
    edges = [(p * n) // nparts for p in range(nparts + 1)]
    keep = np.ones(n, dtype=bool)
    keep[edges[empty]:edges[empty + 1]] = False
    keep[edges[one_row] + 1:edges[one_row + 1]] = False
    host_df = tfs.from_columns(dict(cols, keep=keep.astype(np.int32)), num_partitions=nparts)
    host_df = host_df.filter(host_df.keep > 0).select(*cols)
    dev_df = host_df.cache_on_device(DEV)
    sizes_ = {p: b.nrows for p, b in dev_df.local_blocks().items()}
    assert sizes_[empty] == 0 and sizes_[one_row] == 1
    device = dev_df.dropDuplicates(["id"])
    assert on_device(device)
    same_bytes(device, host_df.dropDuplicates(["id"]))
    same_bytes(dev_df.select("id", "f").distinct(), host_df.select("id", "f").distinct())


def test_a_string_column_rides_along_with_device_keys():
    n = 500
    cols = frame_columns(n, 23)
    cols["s"] = np.array([f"row-{i}" for i in range(n)], dtype=object)
    host_df = tfs.from_columns(cols, num_partitions=3)
    device = host_df.cache_on_device(DEV).dropDuplicates(["id"])
    host = host_df.dropDuplicates(["id"])
    same_bytes(device.drop("s"), host.drop("s"))
    assert [r.s for r in device.select("s").collect()] == [r.s for r in host.select("s").collect()]


def test_readme_example_on_device_frames():
    mon, tue = frame_columns(400, 24), frame_columns(300, 25)
    mon["t"], tue["t"] = np.zeros(400, dtype=np.int32), np.ones(300, dtype=np.int32)
    monday = tfs.from_columns(mon, num_partitions=3).cache_on_device(DEV)
    tuesday = tfs.from_columns(tue, num_partitions=2).cache_on_device(DEV)
    both = monday.union(tuesday)
    assert both.num_partitions == 5 and both.count() == 700
    ids = both.dropDuplicates(["id"])
    every = set(mon["id"].tolist()) | set(tue["id"].tolist())
    assert ids.to_numpy("id").tolist() == sorted(every) and on_device(ids)
    won = dict(zip(ids.to_numpy("id").tolist(), ids.to_numpy("t").tolist()))
    assert all(won[k] == 0 for k in set(mon["id"].tolist()))       # monday's row wins
    pairs = {(a, b) for a, b in zip(mon["id"].tolist() + tue["id"].tolist(), mon["t"].tolist() + tue["t"].tolist())}
    assert both.select("id", "t").distinct().count() == len(pairs)
    common = monday.select("id").intersect(tuesday.select("id"))
    only = monday.select("id").subtract(tuesday.select("id"))
    assert common.to_numpy("id").tolist() == sorted(set(mon["id"].tolist()) & set(tue["id"].tolist()))
    assert only.to_numpy("id").tolist() == sorted(set(mon["id"].tolist()) - set(tue["id"].tolist()))
    assert on_device(common) and on_device(only)


def test_union_of_two_device_frames_copies_nothing():
    a = tfs.from_columns(frame_columns(300, 26), num_partitions=2).cache_on_device(DEV)
    b = tfs.from_columns(frame_columns(200, 27), num_partitions=3).cache_on_device(DEV)
    u = a.union(b)
    blocks = u.local_blocks()
    assert sorted(blocks) == [0, 1, 2, 3, 4] and on_device(u)
    src = {**a.local_blocks(), **{2 + p: blk for p, blk in b.local_blocks().items()}}
    for q, blk in blocks.items():
        for name, col in blk.columns.items():
            assert col.data_ptr() == src[q].columns[name].data_ptr(), (q, name)


# ------------------------------------------------------------------ two ranks, one GPU
def _results(a, b):
    out = {"union": a.union(b).dropDuplicates(["id"]), "distinct": a.select("id", "f").distinct(),
           "intersect": a.select("id").intersect(b.select("id"))}
    return {k: {"cols": {c: v.to_numpy(c).tobytes().hex() for c in v.columns}, "on_device": on_device(v)}
            for k, v in out.items()}


def _frames(device):
    a = tfs.from_columns(frame_columns(T() + 200, 28), num_partitions=5).cache_on_device(device)
    b = tfs.from_columns(frame_columns(700, 29), num_partitions=2).cache_on_device(device)
    return a, b


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
    res = _results(*_frames(None))
    res["device"] = engine.compute_device().type
    with open(os.path.join(outdir, f"r{rank}.json"), "w") as f:
        json.dump(res, f)
    dist.shutdown()


def test_setops_two_ranks_share_one_gpu(tmp_path):
    ctx = mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=False)
    deadline = time.monotonic() + 120
    while not ctx.join(timeout=1):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("the ranks did not finish in 120 s")
    outs = [json.load(open(tmp_path / f"r{r}.json")) for r in range(2)]
    single = _results(*_frames(DEV))
    for o in outs:
        assert o.pop("device") == "cuda"
        assert o == single                                          # every output column, byte for byte; on the device
    assert all(v["on_device"] for v in single.values())
