"""DataFrame.join on the device: the probe / expand / row-gather kernels of
kernels/join.hip against the specification of tests/test_join.py (a dict from
the key's word tuple to the right rows), and device-resident frames against
the host path of the same frames, bit for bit."""
import bisect
import json
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import tensorframes_amd as tfs
from tensorframes_amd._native import _C

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_join import same_bits, spec_join, spec_words  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# row size in bytes -> (dtype, cell shape): the kinds of tests/test_gpu_sort.py
ROW_KINDS = {
    1: (torch.uint8, ()),
    4: (torch.int32, ()),
    8: (torch.int64, ()),
    12: (torch.float32, (3,)),
    16: (torch.float64, (2,)),
    20: (torch.float32, (5,)),
    2048: (torch.float32, (512,)),
}


def _T():
    return _C.join_tile_rows()


def _dev_words(words: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int64)).to(DEV)


def test_tile_rows_exported():
    t = _T()
    assert isinstance(t, int) and t >= 64 and t % 64 == 0


# ------------------------------------------------------------------ probe
def _probe_sizes():
    t = _C.sort_tile_rows()
    s = [0, 1, 63, 64, 65, t - 1, t, t + 1, 3 * t + 7]
    return sorted({(s[i], s[(i + k) % len(s)]) for i in range(len(s)) for k in (0, 4)})


def _key_words(W, rows, lo, hi, rng):
    """[W, rows] words of 2 * (hi - lo) different tuples: the last word holds a
    value of [lo, hi), the words before it tie often (a coin, or the value's parity)."""
    base, coin = rng.integers(lo, hi, rows), rng.integers(0, 2, rows)
    cols = [coin if w % 2 == 0 else base & 1 for w in range(W - 1)] + [base]
    return np.stack([spec_words(c.astype(np.int64)) for c in cols], 0) if rows else np.zeros((W, 0), np.uint64)


@pytest.mark.parametrize("W", [1, 2, 8])
def test_join_probe(W):
    rng = np.random.default_rng(100 + W)
    for n, m in _probe_sizes():
        lw = _key_words(W, n, -2, 12, rng)                     # hits, misses, below all and above all
        rw = _key_words(W, m, 0, 10, rng)
        sw = rw[:, np.lexsort(rw[::-1])] if m else rw
        sorted_tuples = [tuple(int(v) for v in sw[:, j]) for j in range(m)]
        mode = (n + m) % 3
        lo, cnt, mask = _C.join_probe(_dev_words(lw), _dev_words(sw), mode)
        assert lo.dtype == torch.int64 and cnt.dtype == torch.int64 and lo.shape == (n,) and cnt.shape == (n,)
        want_lo, want_cnt = [], []
        for i in range(n):
            t = tuple(int(v) for v in lw[:, i])
            a = bisect.bisect_left(sorted_tuples, t)
            want_lo.append(a)
            want_cnt.append(bisect.bisect_right(sorted_tuples, t) - a)
        assert lo.cpu().tolist() == want_lo, (n, m)
        assert cnt.cpu().tolist() == want_cnt, (n, m)
        if mode == 0:
            assert mask is None
        else:
            assert mask.dtype == torch.bool and mask.is_cuda
            assert mask.cpu().tolist() == [(c != 0) == (mode == 1) for c in want_cnt]
        if n > 64 and m > 64:
            assert 0 < sum(1 for c in want_cnt if c) < n       # the case holds hits and misses


def test_gather_words_gives_the_sorted_build_side():
    rng = np.random.default_rng(7)
    m = _C.sort_tile_rows() + 65
    rw = _key_words(2, m, 0, 50, rng)
    words = _dev_words(rw)
    perm = _C.sort_argsort(words)
    order = np.lexsort(rw[::-1])
    assert perm.cpu().tolist() == order.tolist()
    got = _C.join_gather_words(words, perm)
    assert got.cpu().numpy().view(np.uint64).tolist() == rw[:, order].tolist()


# ------------------------------------------------------------------ expand
def _check_expand(lo, cnt, perm):
    lo, cnt, perm = (np.asarray(a, dtype=np.int64) for a in (lo, cnt, perm))
    n = len(cnt)
    offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(cnt, out=offs[1:])
    want_li = np.repeat(np.arange(n, dtype=np.int64), cnt)
    want_ri = perm[lo[want_li] + (np.arange(int(offs[-1])) - offs[want_li])] if offs[-1] else np.zeros(0, np.int64)
    li, ri, got_offs = _C.join_expand(*(torch.from_numpy(a).to(DEV) for a in (lo, cnt, perm)))
    assert li.is_cuda and ri.is_cuda and li.dtype == torch.int64 and ri.dtype == torch.int64
    assert got_offs.cpu().tolist() == offs.tolist()
    assert li.shape == (int(offs[-1]),) and ri.shape == (int(offs[-1]),)
    assert torch.equal(li.cpu(), torch.from_numpy(want_li))
    assert torch.equal(ri.cpu(), torch.from_numpy(want_ri))
    return int(offs[-1])


def test_expand_one_left_row_spans_several_tiles():
    m = 2 * _T() + 5
    perm = np.random.default_rng(1).permutation(m)
    assert _check_expand([0, 0, 0], [m, m, m], perm) == 3 * m


def test_expand_long_runs_of_rows_without_a_match():
    n = 3 * _T() + 7
    cnt = np.zeros(n, dtype=np.int64)
    lo = np.zeros(n, dtype=np.int64)
    cnt[0], cnt[-1] = 2, 3
    lo[0], lo[-1] = 3, 0
    assert _check_expand(lo, cnt, [4, 2, 0, 1, 3]) == 5
    # the same with a hot row between the runs: the tiles inside it see one left row
    cnt[n // 2], lo[n // 2] = _T() + 1, 0
    _check_expand(lo, cnt, np.random.default_rng(2).permutation(_T() + 9))


def test_expand_no_match_at_all():
    for n in (0, 1, _T() + 3):
        assert _check_expand(np.zeros(n, np.int64), np.zeros(n, np.int64), np.arange(4)) == 0
    assert _check_expand(np.zeros(5, np.int64), np.zeros(5, np.int64), np.zeros(0, np.int64)) == 0


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_expand_unique_keys(delta):
    n = _T() + delta
    rng = np.random.default_rng(3 + delta)
    assert _check_expand(rng.permutation(n), np.ones(n, np.int64), rng.permutation(n)) == n


def test_expand_mixed_counts():
    rng = np.random.default_rng(12)
    T = _T()
    n, m = 2 * T + 9, 4 * T
    cnt = rng.choice(np.array([0, 0, 0, 1, 2, 5]), n)
    cnt[rng.integers(0, n)] = 3 * T                          # one hot key
    cnt[T - 3:T + 40] = 0                                    # a run of misses across a tile boundary
    lo = np.array([rng.integers(0, m - c + 1) for c in cnt])
    total = _check_expand(lo, cnt, rng.permutation(m))
    assert 4 * T < total < 100_000


# ------------------------------------------------------------------ take_rows
def _column(n, dtype, cell, seed):
    rng = np.random.default_rng(seed)
    if dtype.is_floating_point:
        return torch.from_numpy(rng.standard_normal((n,) + cell)).to(dtype)
    info = torch.iinfo(dtype)
    return torch.from_numpy(rng.integers(info.min, int(info.max) + 1, (n,) + cell, dtype=np.int64)).to(dtype)


def _take_bits(got, src, idx):
    want = src[idx]
    assert got.is_cuda and got.is_contiguous() and got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape)
    if want.numel():
        assert torch.equal(got.cpu().contiguous().view(torch.uint8), want.contiguous().view(torch.uint8))


@pytest.mark.parametrize("row_bytes", sorted(ROW_KINDS))
def test_take_rows_row_sizes(row_bytes):
    dtype, cell = ROW_KINDS[row_bytes]
    n_src = 1000
    src = _column(n_src, dtype, cell, row_bytes)
    dsrc = src.to(DEV)
    rng = np.random.default_rng(row_bytes)
    for n_out in (0, 1, 377, 2500):                           # fewer and more rows than the source, repeats
        idx = torch.from_numpy(rng.integers(0, n_src, n_out))
        if n_out >= 377:
            idx[:3] = torch.tensor([n_src - 1, 0, n_src - 1])
        (got,) = _C.take_rows(idx.to(DEV), [dsrc])
        _take_bits(got, src, idx)


def test_take_rows_sixteen_columns_per_call_and_seventeen_in_groups():
    from tensorframes_amd.frame.block import Block
    from tensorframes_amd.frame.join import _take_block
    kinds = [ROW_KINDS[k] for k in (1, 4, 8, 12, 16, 20, 2048)]
    n_src, n_out = 300, 700
    cols = [_column(n_src, *kinds[j % len(kinds)], seed=j) for j in range(17)]
    dcols = [c.to(DEV) for c in cols]
    idx = torch.from_numpy(np.random.default_rng(0).integers(0, n_src, n_out))
    didx = idx.to(DEV)
    for got, src in zip(_C.take_rows(didx, dcols[:16]), cols):
        _take_bits(got, src, idx)
    with pytest.raises(ValueError, match="16"):
        _C.take_rows(didx, dcols)
    names = [f"c{j}" for j in range(17)]
    out = _take_block(Block(n_src, dict(zip(names, dcols))), names, didx)
    for name, src in zip(names, cols):
        _take_bits(out[name], src, idx)


def test_binding_argument_errors():
    w = torch.zeros((2, 5), dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="device"):
        _C.join_probe(w.cpu(), w)
    with pytest.raises(ValueError, match="device"):
        _C.join_probe(w, w.cpu())
    with pytest.raises(TypeError, match="int64"):
        _C.join_probe(w.to(torch.int32), w)
    with pytest.raises(ValueError, match=r"\[W, n\]"):
        _C.join_probe(w[0], w)
    with pytest.raises(ValueError, match="1..8"):
        _C.join_probe(torch.zeros((9, 5), dtype=torch.int64, device=DEV), torch.zeros((9, 5), dtype=torch.int64,
                                                                                      device=DEV))
    with pytest.raises(ValueError, match="1..8"):
        _C.join_probe(w[:0], w[:0])
    with pytest.raises(ValueError, match="2 words per left row, 1 per build row"):
        _C.join_probe(w, w[:1])
    with pytest.raises(ValueError, match="mask"):
        _C.join_probe(w, w, 3)
    v = torch.zeros(5, dtype=torch.int64, device=DEV)
    with pytest.raises(TypeError, match="int64"):
        _C.join_expand(v.to(torch.int32), v, v)
    with pytest.raises(ValueError, match="one device"):
        _C.join_expand(v, v.cpu(), v)
    with pytest.raises(ValueError, match=r"lo \[n\], cnt \[n\]"):
        _C.join_expand(v, v[:4], v)
    with pytest.raises(ValueError, match="1..8"):
        _C.join_gather_words(torch.zeros((9, 5), dtype=torch.int64, device=DEV), v)
    with pytest.raises(ValueError, match="permutation"):
        _C.join_gather_words(w, v[:4])
    c = torch.zeros((5, 3), dtype=torch.float32, device=DEV)
    with pytest.raises(TypeError, match="int64"):
        _C.take_rows(v.to(torch.int32), [c])
    with pytest.raises(ValueError, match="device tensor"):
        _C.take_rows(v.cpu(), [c])
    with pytest.raises(ValueError, match="not on the indices' device"):
        _C.take_rows(v, [c.cpu()])
    with pytest.raises(ValueError, match="rows, column 0 has 5"):
        _C.take_rows(v, [c, c[:4]])
    with pytest.raises(ValueError, match="1..16"):
        _C.take_rows(v, [])
    with pytest.raises(ValueError, match="without rows"):
        _C.take_rows(v, [c[:0]])


# ------------------------------------------------------------------ frames
def _frame_columns(n, m, seed=0):
    rng = np.random.default_rng(seed)
    specials = np.array([np.nan, -0.0, 0.0, np.inf, -np.inf], dtype=np.float32)
    x = rng.integers(0, 40, n).astype(np.float32)
    x[::13] = specials[np.arange(len(x[::13])) % 5]
    y = rng.integers(0, 40, m).astype(np.float32)
    y[::7] = specials[(np.arange(len(y[::7])) + 2) % 5]
    lc = {"k": rng.integers(0, m, n).astype(np.int64), "x": x, "g": rng.integers(0, 3, n).astype(np.int32),
          "i": np.arange(n, dtype=np.int64), "lv": rng.standard_normal((n, 3)).astype(np.float32),
          "ls": np.array([f"l-{i}" * (1 + i % 3) for i in range(n)])}
    for j in range(14):                                     # more dense left columns than one kernel call takes
        lc[f"c{j}"] = rng.standard_normal(n)
    rc = {"k": rng.integers(0, m, m).astype(np.int64), "x": y, "g": rng.integers(0, 3, m).astype(np.int32),
          "j": np.arange(m, dtype=np.int64), "rv": rng.standard_normal((m, 2)),
          "rs": np.array([f"r-{i}" * (i % 4) for i in range(m)])}
    return lc, rc


def _equal_frames(a, b):
    assert a.columns == b.columns and a.count() == b.count()
    for name in a.columns:
        same_bits(a.to_numpy(name), b.to_numpy(name), name)
    la, lb = a.local_blocks(), b.local_blocks()
    assert {p: x.nrows for p, x in la.items()} == {p: x.nrows for p, x in lb.items()}


def test_device_resident_frames_match_the_host_path():
    T = _T()
    n, m = 2 * T + 77, T + 13
    lc, rc = _frame_columns(n, m)
    cut = n // 4 + 5                                        # the first of 4 partitions loses every row
    keep = lc["i"] >= cut
    lcf = {c: v[keep] for c, v in lc.items()}
    host_l = tfs.from_columns(lc, num_partitions=4)
    host_l = host_l.filter(host_l.i >= cut).cache()
    host_r = tfs.from_columns(rc, num_partitions=3)
    dev_l, dev_r = host_l.cache_on_device(DEV), host_r.cache_on_device(DEV)
    assert dev_l.local_blocks()[0].nrows == 0
    assert all(c.is_cuda for b in dev_r.local_blocks().values() for c in b.columns.values())
    for on in ("k", ["g", "x"]):
        keys = [on] if isinstance(on, str) else on
        drop = [c for c in ("k", "x", "g") if c not in keys]
        hl, hr, dl, dr = (f.drop(*drop) for f in (host_l, host_r, dev_l, dev_r))
        for how in ("inner", "left_semi", "left_anti"):
            got = dl.join(dr, on, how)
            for b in got.local_blocks().values():
                assert all(c.is_cuda for c in b.columns.values()), (on, how)      # outputs stay on the device
            _equal_frames(got, hl.join(hr, on, how))
            kind = {"inner": "inner", "left_semi": "semi", "left_anti": "anti"}[how]
            li, ri = spec_join([lcf[k] for k in keys], [rc[k] for k in keys], kind)
            assert got.to_numpy("i").tolist() == lcf["i"][li].tolist()
            if how == "inner":
                assert got.to_numpy("j").tolist() == ri.tolist()
                assert len(li) > n // 2
    # the left side's -0.0 key bits stay in the output
    out = dev_l.select("x", "i").join(dev_r.select("x", "j"), "x")
    gx, gi = out.to_numpy("x"), out.to_numpy("i")
    same_bits(gx, lc["x"][gi], "x")
    assert np.signbit(gx[gx == 0]).any() and not np.signbit(gx[gx == 0]).all()
    # rows are counted once
    before = tfs.metrics.snapshot()
    total = dev_l.join(dev_r.select("k", "j"), "k").count()
    after = tfs.metrics.snapshot()
    assert after.get("join_rows_left", 0) - before.get("join_rows_left", 0) == int(keep.sum())
    assert after.get("join_rows_build", 0) - before.get("join_rows_build", 0) == m
    assert after.get("join_rows_out", 0) - before.get("join_rows_out", 0) == total
    # an empty build side
    none = dev_r.filter(dev_r.j < 0)
    assert dev_l.join(none.select("k", "j"), "k").count() == 0
    assert dev_l.join(none, "k", "anti").count() == int(keep.sum())


def test_host_build_side_and_device_left_side():
    lc, rc = _frame_columns(500, 300, seed=3)
    left = tfs.from_columns(lc, num_partitions=2).cache_on_device(DEV)
    right = tfs.from_columns(rc, num_partitions=2).select("k", "j", "rs")
    out = left.join(right, "k")
    li, ri = spec_join([lc["k"]], [rc["k"]])
    assert out.to_numpy("i").tolist() == li.tolist() and out.to_numpy("j").tolist() == ri.tolist()
    assert out.to_numpy("rs").tolist() == rc["rs"][ri].tolist()


# ------------------------------------------------------------------ two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _spmd_result(tfs_mod, hows=("inner", "anti")):
    lc, rc = _frame_columns(3001, 901, seed=4)
    left = tfs_mod.from_columns(lc, num_partitions=5).select("g", "x", "i", "lv", "ls").cache_on_device()
    right = tfs_mod.from_columns(rc, num_partitions=3).select("g", "x", "j", "rv", "rs").cache_on_device()
    res = {}
    for how in hows:
        out = left.join(right, ["g", "x"], how)
        blocks = out.local_blocks()
        res[how] = {"on_host": sorted({n for b in blocks.values() for n, c in b.columns.items() if not c.is_cuda}),
                    "local": sorted(blocks),
                    "i": out.to_numpy("i").tolist(),
                    "j": out.to_numpy("j").tolist() if how == "inner" else [],
                    "rs": out.to_numpy("rs").tolist() if how == "inner" else []}
    return res


def _worker(rank, world, port, outdir, backend, hows):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), OMP_NUM_THREADS="1", TFA_SHM_COLLECTIVES="1")
    torch.set_num_threads(1)
    sys.path.insert(0, REPO)
    import tensorframes_amd as tfs_mod
    from tensorframes_amd.parallel import dist

    assert dist.init(backend=backend, force=world == 1)     # (a forced world of one runs the collectives too)
    res = _spmd_result(tfs_mod, hows)
    with open(os.path.join(outdir, f"r{rank}.json"), "w") as f:
        json.dump(res, f)
    dist.shutdown()


def _check_ranks(tmp_path, backend, world=2, hows=("inner", "anti")):
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), backend, hows), nprocs=world, join=True)
    outs = [json.load(open(tmp_path / f"r{r}.json")) for r in range(world)]
    one = _spmd_result(tfs, hows)
    lc, rc = _frame_columns(3001, 901, seed=4)
    li, ri = spec_join([lc["g"], lc["x"]], [rc["g"], rc["x"]])
    assert one["inner"]["i"] == li.tolist() and one["inner"]["j"] == ri.tolist() and len(li) > 1000
    for r, o in enumerate(outs):
        for how in hows:
            # dense build columns travel through the host when the device group is not RCCL
            assert set(o[how]["on_host"]) <= (set() if backend == "nccl" else {"j", "rv"}), (how, r)
            assert o[how]["local"] == [p for p in range(5) if p % world == r]
            for c in ("i", "j", "rs"):
                assert o[how][c] == one[how][c], (how, c, r)


def test_join_two_ranks_share_one_gpu(tmp_path):
    _check_ranks(tmp_path, "gloo")


def test_join_rccl_world_of_one(tmp_path):
    """The build side's device gather over RCCL, on one GPU: every column stays on the device."""
    _check_ranks(tmp_path, "nccl", world=1, hows=("inner",))


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_join_two_ranks_rccl(tmp_path):
    _check_ranks(tmp_path, "nccl")
