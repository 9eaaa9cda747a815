"""Device sort (csrc/kernels/sort.hip: `_C.sort_encode`, `_C.sort_argsort`,
`_C.permute_rows`, `_C.sort_bounds`) and `DataFrame.orderBy` /
`sortWithinPartitions` on device-resident frames.

Every comparison is exact: words, permutations and payload bits. The expected
order comes from the numpy lines below (the ordering table of
docs/MIGRATION.md, then `np.lexsort`), never from the code under test. No
test hands `permute_rows` an index outside its rows."""
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

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# row size in bytes -> (dtype, cell shape): the kinds of tests/test_gpu_compact.py
ROW_KINDS = {
    1: (torch.uint8, ()),
    4: (torch.int32, ()),
    8: (torch.int64, ()),
    12: (torch.float32, (3,)),
    16: (torch.float64, (2,)),
    20: (torch.float32, (5,)),
    2048: (torch.float32, (512,)),
}


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
    """words: uint64 arrays, most significant first -> the stable permutation."""
    return np.lexsort(list(words)[::-1])


def spec_passes(words) -> int:
    """8-bit digits that vary over the rows, summed over the words."""
    total = 0
    for w in words:
        if len(w) == 0:
            continue
        mask = int(np.bitwise_or.reduce(w ^ w[0]))
        total += sum(1 for d in range(8) if (mask >> (8 * d)) & 0xFF)
    return total


def spec_bounds(sorted_words: np.ndarray, splitters: np.ndarray):
    """Rows of the sorted tuples [n, W] lexicographically below each splitter [S, W]."""
    rows = [tuple(int(v) for v in r) for r in sorted_words]
    return [sum(1 for r in rows if r < tuple(int(v) for v in t)) for t in splitters]


def _tile():
    return _C.sort_tile_rows()


def _row_counts():
    t = _tile()
    return [0, 1, 63, 64, 65, t - 1, t, t + 1, 3 * t + 7]


def _same_bits(got: torch.Tensor, want: torch.Tensor):
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape)
    assert got.is_contiguous()
    a = got.cpu().contiguous().view(torch.uint8) if got.numel() else got.cpu()
    b = want.contiguous().view(torch.uint8) if want.numel() else want
    assert torch.equal(a, b)


def _words_of(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


def _as_words(words) -> torch.Tensor:
    return torch.from_numpy(np.stack(words, 0).view(np.int64)).to(DEV)


def test_tile_rows_exported():
    t = _tile()
    assert isinstance(t, int) and t >= 64 and t % 64 == 0


# ------------------------------------------------------------------ sort_encode
def _float_specials(dtype):
    fi = np.finfo(dtype)
    ubits = np.uint32 if dtype == np.float32 else np.uint64
    odd_nans = np.array([0xFFC00001, 0x7F800001] if dtype == np.float32
                        else [0xFFF8000000000001, 0x7FF0000000000001], dtype=ubits).view(dtype)
    vals = [np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, fi.tiny, -fi.tiny, fi.smallest_subnormal,
            -fi.smallest_subnormal, fi.max, fi.min, 1.0, -1.0]
    return np.concatenate([np.array(vals, dtype=dtype), odd_nans])


def _key_values(dtype, n, seed):
    """n values of `dtype`: the edge values first (when they fit), then random bit patterns."""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    if dt.kind == "f":
        edge = _float_specials(dtype)
        body = rng.integers(0, 2 ** 64 - 1, n, dtype=np.uint64, endpoint=True)
        body = (body >> np.uint64(32)).astype(np.uint32) if dt.itemsize == 4 else body
        body = body.view(dtype)                                             # every exponent, NaNs included
    elif dt.kind == "b":
        edge = np.array([False, True])
        body = rng.integers(0, 2, n).astype(bool)
    else:
        ii = np.iinfo(dtype)
        edge = np.array([ii.min, ii.max, 0, 1, ii.min + 1, ii.max - 1], dtype=dtype)
        if ii.min < 0:
            edge = np.concatenate([edge, np.array([-1], dtype=dtype)])
        body = rng.integers(ii.min, ii.max, n, dtype=np.int64, endpoint=True).astype(dtype)
    return np.concatenate([edge, body])[:n].copy()


ENCODE_DTYPES = [np.bool_, np.uint8, np.int8, np.int16, np.int32, np.int64, np.float32, np.float64]


@pytest.mark.parametrize("flip", [0, 1])
def test_sort_encode_matches_the_table(flip):
    for n in _row_counts():
        host = [_key_values(dt, n, seed=n + i) for i, dt in enumerate(ENCODE_DTYPES)]
        desc = [(i + flip) % 2 == 1 for i in range(len(host))]
        words = _C.sort_encode([torch.from_numpy(h).to(DEV) for h in host], desc)   # 8 keys, one launch
        assert words.is_cuda and words.dtype == torch.int64 and tuple(words.shape) == (8, n)
        got = _words_of(words)
        for i, (h, d) in enumerate(zip(host, desc)):
            assert np.array_equal(got[i], spec_words(h, d)), (n, ENCODE_DTYPES[i], d)
        for h, d in zip(host, desc):                                                # and each key on its own
            one = _C.sort_encode([torch.from_numpy(h).to(DEV)], [d])
            assert np.array_equal(_words_of(one)[0], spec_words(h, d))


def test_sort_encode_argument_errors():
    k = torch.zeros(8, dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="1..8"):
        _C.sort_encode([], [])
    with pytest.raises(ValueError, match="1..8"):
        _C.sort_encode([k] * 9, [False] * 9)
    with pytest.raises(ValueError, match="directions"):
        _C.sort_encode([k, k], [False])
    with pytest.raises(ValueError, match="device"):
        _C.sort_encode([k.cpu()], [False])
    with pytest.raises(ValueError, match="1-D"):
        _C.sort_encode([k.view(4, 2)], [False])
    with pytest.raises(ValueError, match="rows"):
        _C.sort_encode([k, k[:4]], [False, False])
    with pytest.raises(TypeError, match="not supported as a sort key"):
        _C.sort_encode([k.to(torch.float16)], [False])
    with pytest.raises(TypeError, match="not supported as a sort key"):
        _C.sort_encode([k.to(torch.bfloat16)], [False])


# ------------------------------------------------------------------ sort_argsort
def _argsort_key_sets(n, seed):
    """name -> list of uint64 word arrays [n] (most significant first)"""
    rng = np.random.default_rng(seed)
    i32 = rng.integers(-2 ** 31, 2 ** 31 - 1, n).astype(np.int32)
    f32 = _key_values(np.float32, n, seed)
    f64 = _key_values(np.float64, n, seed + 1)
    small = rng.integers(0, 1000, n).astype(np.int32)
    three = rng.integers(0, 3, n).astype(np.int64)
    asc = np.sort(rng.integers(0, 2 ** 40, n)).astype(np.int64)
    top = (rng.integers(0, 128, n).astype(np.int64) << 56)
    top32 = (rng.integers(0, 127, n).astype(np.int32) << 24)
    low = (rng.integers(0, 256, n).astype(np.int64) + (1 << 40))
    return {
        "random_i32": [spec_words(i32)],
        "random_f32_desc": [spec_words(f32, True)],
        "random_f64": [spec_words(f64)],
        "all_equal": [spec_words(np.full(n, 7, dtype=np.int64))],
        "sorted": [spec_words(asc)],
        "reversed": [spec_words(asc[::-1].copy())],
        "three_values": [spec_words(three)],
        "top_byte_only": [spec_words(top)],
        "top_byte_i32": [spec_words(top32)],
        "low_byte_only": [spec_words(low)],
        "small_range": [spec_words(small)],
        "two_words": [spec_words(three, True), spec_words(f32)],
        "three_words": [spec_words(three), spec_words(np.full(n, 1.5)), spec_words(small, True)],
        "three_words_mixed": [spec_words(rng.integers(0, 2, n).astype(np.uint8)), spec_words(f64, True),
                              spec_words(i32)],
    }


@pytest.mark.parametrize("name", sorted(_argsort_key_sets(4, 0)))
def test_sort_argsort(name):
    for n in _row_counts():
        words = _argsort_key_sets(n, seed=n)[name]
        perm = _C.sort_argsort(_as_words(words))
        assert perm.is_cuda and perm.dtype == torch.int64 and tuple(perm.shape) == (n,)
        assert torch.equal(perm.cpu(), torch.from_numpy(spec_order(words))), (name, n)
        assert _C.sort_last_passes() == spec_passes(words), (name, n)


def test_digit_skipping_pass_counts():
    n = 3 * _tile() + 7
    sets = _argsort_key_sets(n, seed=5)
    expect = {"small_range": 2, "all_equal": 0, "top_byte_only": 1, "top_byte_i32": 1, "low_byte_only": 1,
              "three_values": 1, "three_words": 3}
    for name, passes in expect.items():
        assert spec_passes(sets[name]) == passes, name                  # what the masks imply ...
        _C.sort_argsort(_as_words(sets[name]))
        assert _C.sort_last_passes() == passes, name                    # ... is what runs
    with pytest.raises(ValueError, match="words"):
        _C.sort_argsort(_as_words(sets["small_range"]).cpu())
    with pytest.raises(ValueError, match="words"):
        _C.sort_argsort(_as_words(sets["small_range"])[0])
    with pytest.raises(ValueError, match="1..8"):
        _C.sort_argsort(torch.zeros((9, 4), dtype=torch.int64, device=DEV))


# ------------------------------------------------------------------ permute_rows
def _column(n, dtype, cell, seed):
    g = torch.Generator().manual_seed(seed)
    shape = (n,) + tuple(cell)
    if dtype.is_floating_point:
        return torch.randn(shape, generator=g, dtype=dtype)
    hi = 255 if dtype == torch.uint8 else 2 ** 31 - 1
    return torch.randint(0, hi, shape, generator=g, dtype=torch.int64).to(dtype)


def _perms(n, seed=0):
    g = torch.Generator().manual_seed(99 + seed)
    return {"identity": torch.arange(n), "reverse": torch.arange(n - 1, -1, -1),
            "random": torch.randperm(n, generator=g)}


@pytest.mark.parametrize("row_bytes", sorted(ROW_KINDS))
def test_permute_row_sizes(row_bytes):
    dtype, cell = ROW_KINDS[row_bytes]
    for n in _row_counts():
        host = _column(n, dtype, cell, seed=n)
        assert (host[0].numel() * host.element_size() if n else row_bytes) == row_bytes
        dev = host.to(DEV)
        for name, p in _perms(n, seed=row_bytes).items():
            (out,) = _C.permute_rows(p.to(DEV), [dev])
            assert out.is_cuda
            _same_bits(out, host[p])


def test_sixteen_mixed_columns_and_seventeen_raise():
    n = 3 * _tile() + 7
    kinds = [ROW_KINDS[k] for k in (1, 4, 8, 12, 16, 20, 2048)]
    kinds += [(torch.uint8, (3,)), (torch.uint8, (4,)), (torch.uint8, (16,)), (torch.int32, (4,)),
              (torch.float64, ()), (torch.int64, (3,)), (torch.float32, (1, 2)), (torch.float32, (7, 9)),
              (torch.float32, (300,))]
    assert len(kinds) == 16
    hosts = [_column(n, dt, cell, seed=i) for i, (dt, cell) in enumerate(kinds)]
    devs = [h.to(DEV) for h in hosts]
    p = _perms(n)["random"]
    outs = _C.permute_rows(p.to(DEV), devs)
    assert len(outs) == 16
    for o, h in zip(outs, hosts):
        _same_bits(o, h[p])
    with pytest.raises(ValueError, match="16"):
        _C.permute_rows(p.to(DEV), devs + [devs[0]])
    with pytest.raises(ValueError):
        _C.permute_rows(p.to(DEV), [])


def test_permute_wide_and_odd_rows():
    n = 67
    p = _perms(n)["random"]
    for dtype, cell in ((torch.float64, (8200,)), (torch.uint8, (70001,)), (torch.uint8, (1001,)),
                        (torch.float32, (0,))):          # > 64 KiB rows, byte-wise wide rows, rows without bytes
        host = _column(n, dtype, cell, seed=3)
        (out,) = _C.permute_rows(p.to(DEV), [host.to(DEV)])
        _same_bits(out, host[p])


def test_permute_misaligned_bases_and_views():
    n = _tile() + 65
    p = _perms(n)["random"]
    # 16-byte rows whose base is only 4-byte aligned
    flat = _column(4 * n + 1, torch.float32, (), seed=12)
    dev = flat.to(DEV)[1:].view(n, 4)
    assert dev.data_ptr() % 16 == 4
    (out,) = _C.permute_rows(p.to(DEV), [dev])
    _same_bits(out, flat[1:].view(n, 4)[p])
    # 12-byte rows from a base 12 bytes past a 16-byte boundary; 4-byte rows from an odd base
    host = _column(n + 1, torch.float32, (3,), seed=5)
    (out,) = _C.permute_rows(p.to(DEV), [host.to(DEV)[1:]])
    _same_bits(out, host[1:][p])
    raw = _column(4 * n + 1, torch.uint8, (), seed=6)
    dev = raw.to(DEV)[1:].view(n, 4)
    assert dev.data_ptr() % 4 == 1
    (out,) = _C.permute_rows(p.to(DEV), [dev])
    _same_bits(out, raw[1:].view(n, 4)[p])
    # a non-contiguous column and a strided permutation
    wide = _column(n, torch.float32, (6,), seed=7)
    (out,) = _C.permute_rows(p.to(DEV), [wide.to(DEV)[:, ::2]])
    _same_bits(out, wide[:, ::2][p])
    both = torch.stack([p, p], 1).to(DEV)
    (out,) = _C.permute_rows(both[:, 0], [wide.to(DEV)])
    _same_bits(out, wide[p])


def test_permute_argument_errors_come_before_any_launch():
    n = 10
    dev = torch.zeros(n, dtype=torch.float32, device=DEV)
    ok = torch.arange(n, device=DEV)
    with pytest.raises(ValueError, match="device"):
        _C.permute_rows(ok.cpu(), [dev])
    with pytest.raises(TypeError, match="int64"):
        _C.permute_rows(ok.to(torch.int32), [dev])
    with pytest.raises(ValueError, match="one entry per row"):
        _C.permute_rows(ok[:5], [dev])
    with pytest.raises(ValueError, match="device"):
        _C.permute_rows(ok, [dev.cpu()])
    with pytest.raises(ValueError, match="rows"):
        _C.permute_rows(ok, [dev, dev[:4]])
    with pytest.raises(ValueError, match="row dimension"):
        _C.permute_rows(ok, [torch.zeros((), device=DEV)])


# ------------------------------------------------------------------ sort_bounds
@pytest.mark.parametrize("W", [1, 2, 3])
def test_sort_bounds(W):
    rng = np.random.default_rng(W)
    for n in (0, 1, 65, 1500):
        words = [rng.integers(0, 6, n).astype(np.uint64) << np.uint64(61 if w == 0 else 0) for w in range(W)]
        dev_words = _as_words(words) if n else torch.zeros((W, 0), dtype=torch.int64, device=DEV)
        perm = _C.sort_argsort(dev_words)
        sorted_words = np.stack(words, 1)[spec_order(words)] if n else np.zeros((0, W), dtype=np.uint64)
        below = np.zeros((1, W), dtype=np.uint64)                           # below every row
        above = np.full((1, W), 2 ** 64 - 1, dtype=np.uint64)               # above every row
        picks = [below, above]
        if n:
            picks.append(sorted_words[[0, n // 2, n - 1]])                  # equal to runs of duplicates
            between = sorted_words[[n // 3]].copy()
            between[0, W - 1] += np.uint64(1)
            picks.append(between)
        splitters = np.concatenate(picks, 0)
        got = _C.sort_bounds(dev_words, perm, torch.from_numpy(splitters.view(np.int64)))
        assert got.is_cuda and got.dtype == torch.int64
        assert got.cpu().tolist() == spec_bounds(sorted_words, splitters), (W, n)
        assert got.cpu().tolist()[:2] == [0, n]
    with pytest.raises(ValueError, match="splitters"):
        _C.sort_bounds(dev_words, perm, torch.zeros((2, W + 1), dtype=torch.int64))
    with pytest.raises(ValueError, match="permutation"):
        _C.sort_bounds(dev_words, perm[:3], torch.zeros((2, W), dtype=torch.int64))


# ------------------------------------------------------------------ frames
def _frame_columns(n, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n).astype(np.float32)
    x[::17] = np.nan
    x[5::29] = -0.0
    cols = {"k": rng.integers(0, 1000, n).astype(np.int32), "x": x, "g": rng.integers(-5, 5, n).astype(np.int64),
            "v": rng.standard_normal((n, 3)).astype(np.float32), "i": np.arange(n, dtype=np.int64),
            "h": rng.standard_normal((n, 2)),
            "s": np.array([f"name-{i}" * (1 + i % 4) for i in range(n)])}
    for j in range(14):                                   # more dense device columns than one kernel call takes
        cols[f"c{j}"] = (x + j).astype(np.float64)
    return cols


def _mixed_device_frame(host):
    """The frame on the device, except column `h`, which stays on the host."""
    from tensorframes_amd.frame.block import Block
    from tensorframes_amd.frame.dataframe import DataFrame, _Materialized
    dev = host.cache_on_device(DEV)
    blocks = {p: Block(b.nrows, {n: (c.cpu() if n == "h" else c) for n, c in b.columns.items()})
              for p, b in dev.local_blocks().items()}
    return DataFrame(dev.schema, _Materialized(blocks), dev.num_partitions)


def _equal_frames(a, b, names):
    assert a.count() == b.count()
    for name in names:
        x, y = a.to_numpy(name), b.to_numpy(name)
        assert x.dtype == y.dtype and x.shape == y.shape
        if x.dtype.kind in "OUS":
            assert x.tolist() == y.tolist(), name
        else:
            assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes(), name


@pytest.mark.parametrize("nparts", [1, 4])
def test_device_resident_frames_match_the_host_path(nparts):
    n = 2 * _tile() + 77
    cols = _frame_columns(n)
    host = tfs.from_columns(cols, num_partitions=nparts)
    dev = _mixed_device_frame(host)
    assert all(b.columns["s"].is_cuda and not b.columns["h"].is_cuda for b in dev.local_blocks().values())
    keysets = [lambda f: (f.g.desc(), f.x), lambda f: ("k",), lambda f: ((f.x * 2.0).desc(), "g")]
    words = [[spec_words(cols["g"], True), spec_words(cols["x"])], [spec_words(cols["k"])],
             [spec_words(cols["x"] * np.float32(2.0), True), spec_words(cols["g"])]]
    for keys, w in zip(keysets, words):
        got = dev.orderBy(*keys(dev))
        for b in got.local_blocks().values():
            for name, c in b.columns.items():
                assert c.is_cuda == (name != "h"), name            # what was on the device stays there
        _equal_frames(got, host.orderBy(*keys(host)), host.columns)
        assert got.to_numpy("i").tolist() == spec_order(w).tolist()
        inside = dev.sortWithinPartitions(*keys(dev))
        assert all(c.is_cuda == (name != "h") for b in inside.local_blocks().values() for name, c in b.columns.items())
        _equal_frames(inside, host.sortWithinPartitions(*keys(host)), host.columns)
    # an int32 key in [0, 1000): two radix passes per partition, every row counted once
    before = tfs.metrics.snapshot()
    dev.sortWithinPartitions("k").count()
    after = tfs.metrics.snapshot()
    assert after.get("sort_radix_passes", 0) - before.get("sort_radix_passes", 0) == 2 * nparts
    assert after.get("sort_rows", 0) - before.get("sort_rows", 0) == n
    top = dev.orderBy(dev.x.desc()).limit(10)
    assert top.to_numpy("i").tolist() == spec_order([spec_words(cols["x"], True)])[:10].tolist()
    empty = dev.filter(dev.k < 0).orderBy("k")
    assert empty.count() == 0


def test_host_resident_frame_on_a_gpu_engine():
    n = _tile() + 9
    cols = _frame_columns(n, seed=2)
    host = tfs.from_columns(cols, num_partitions=3)
    out = host.orderBy((host.x + host.x).desc(), "g")
    want = spec_order([spec_words(cols["x"] + cols["x"], True), spec_words(cols["g"])])
    for name in ("i", "x", "v", "s"):
        got = out.to_numpy(name)
        assert got.tolist() == cols[name][want].tolist() or \
            np.ascontiguousarray(got).tobytes() == np.ascontiguousarray(cols[name][want]).tobytes(), name


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
    import tensorframes_amd as tfs
    from tensorframes_amd import engine
    from tensorframes_amd.parallel import dist

    assert dist.init(backend="gloo")
    cols = _frame_columns(3001, seed=4)
    df = tfs.from_columns(cols, num_partitions=5).cache_on_device()
    on_device = all(c.is_cuda for b in df.local_blocks().values() for c in b.columns.values())
    out = df.orderBy(df.g.desc(), "x")
    rows = out.collect()
    res = {"device": engine.compute_device().type, "on_device": on_device, "nparts": out.num_partitions,
           "i": [r.i for r in rows], "s": [r.s for r in rows],
           "local": {str(p): b.columns["i"].tolist() for p, b in out.local_blocks().items()}}
    with open(os.path.join(outdir, f"r{rank}.json"), "w") as f:
        json.dump(res, f)
    dist.shutdown()


def test_order_by_two_ranks_share_one_gpu(tmp_path):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    outs = [json.load(open(tmp_path / f"r{r}.json")) for r in range(2)]
    cols = _frame_columns(3001, seed=4)
    want = spec_order([spec_words(cols["g"], True), spec_words(cols["x"])])
    parts = {}
    for r, o in enumerate(outs):
        assert o["device"] == "cuda" and o["on_device"] and o["nparts"] == 5
        assert o["i"] == want.tolist()
        assert o["s"] == cols["s"][want].tolist()
        assert sorted(int(p) for p in o["local"]) == [p for p in range(5) if p % 2 == r]
        parts.update({int(p): v for p, v in o["local"].items()})
    assert [i for p in range(5) for i in parts[p]] == want.tolist()
