"""The device kernels under `DataFrame.describe` / `summary` / `approxQuantile`
(csrc/kernels/stats.hip: column_moments, select_hist) and the frame paths that
use them, on the GPU.

Expected values come from numpy and Python written here: the ordering table
(`spec_words`, copied from tests/test_gpu_sort.py), `np.bincount`, and exact
rational arithmetic for mean and M2 (numpy's two-pass f64 above 4097 rows,
whose own distance from exact on these inputs is <= 2e-16). The bound on mean,
M2 and stddev is the 1e-11 relative derived in tests/test_describe.py. No test
hands a kernel an index out of range or a length that does not fit its data."""
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
from tensorframes_amd._native import _C

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-11
DTYPES = [np.uint8, np.int8, np.int16, np.int32, np.int64, np.float32, np.float64]
PROBS = [0.0, 0.1, 0.25, 0.5, 0.75, 0.9, 1.0]


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


def canonical(v):
    v = np.asarray(v)
    if v.dtype.kind != "f":
        return v
    return np.where(np.isnan(v), np.array(np.nan, dtype=v.dtype), v + v.dtype.type(0.0)).astype(v.dtype)


def spec_quantiles(x: np.ndarray, probs) -> np.ndarray:
    s = x[np.argsort(spec_words(x), kind="stable")]
    return canonical(s[[max(math.ceil(p * len(x)) - 1, 0) for p in probs]])


def as_doubles(v) -> np.ndarray:
    return np.array([float(t) for t in np.asarray(v).reshape(-1)], dtype=np.float64)


def spec_hist(words: np.ndarray, prefixes, prefix_bits: int) -> np.ndarray:
    out = np.zeros((len(prefixes), 256), dtype=np.int64)
    for q, pre in enumerate(prefixes):
        sel = np.ones(len(words), dtype=bool) if prefix_bits == 0 else \
            (words >> np.uint64(64 - prefix_bits)) == (np.uint64(pre) >> np.uint64(64 - prefix_bits))
        digit = (words[sel] >> np.uint64(56 - prefix_bits)) & np.uint64(255)
        out[q] = np.bincount(digit.astype(np.int64), minlength=256)
    return out


_EXACT = {}


def exact_mean_m2(x: np.ndarray):
    """(mean, M2) of the f64-converted data: exact rationals up to 4097 rows, numpy two-pass f64 above."""
    key = (x.dtype.str, x.tobytes())
    if key not in _EXACT:
        xd = x.astype(np.float64)
        if len(x) <= 4097:
            fx = [Fraction(float(v)) for v in xd]
            mean = sum(fx) / len(fx)
            _EXACT[key] = (float(mean), float(sum((v - mean) ** 2 for v in fx)))
        else:
            mean = xd.mean()
            mean += (xd - mean).mean()
            _EXACT[key] = (float(mean), float(((xd - mean) ** 2).sum()))
    return _EXACT[key]


def close(got: float, want: float):
    if want == 0.0:
        assert got == 0.0, (got, want)
    else:
        err = abs(got - want) / abs(want)
        assert err <= BOUND, (got, want, err)
    return 0.0 if want == 0.0 else abs(got - want) / abs(want)


def _tile():
    return int(_C.stats_tile_rows())


def _row_counts():
    t = _tile()
    return [0, 1, 63, 64, 65, t - 1, t, t + 1, 3 * t + 7]


def centred(dtype, n, seed=0):
    """Data far from zero relative to its spread (1e4 + N(0, 1) for floats)."""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return (1e4 + rng.standard_normal(n)).astype(dt)
    if dt.itemsize == 1:
        return np.clip(np.rint(100 + 5 * rng.standard_normal(n)), 0, 127).astype(dt)
    return np.rint(10000 + 100 * rng.standard_normal(n)).astype(dt)


def wide(dtype, n, seed=1):
    """The whole range of the type, with the float specials."""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    if dt.kind == "f":
        x = rng.standard_normal(n).astype(dt)
        fi = np.finfo(dt)
        for j, s in enumerate([np.nan, np.inf, -np.inf, 0.0, -0.0, fi.tiny / 4, -fi.tiny / 4, fi.max][:n // 2]):
            x[(j * 7) % n] = s
        return x
    ii = np.iinfo(dt)
    x = rng.integers(ii.min, ii.max, n, dtype=dt, endpoint=True)
    if n >= 4:
        x[0], x[n // 2] = ii.max, ii.min
    return x


def dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def check_record(mo, ex, x: np.ndarray, exact_only=False):
    """One column's record against the specification."""
    mo, ex = mo.cpu().numpy(), ex.cpu().numpy().view(np.uint64)
    n = len(x)
    assert mo[0] == float(n)
    if n == 0:
        assert math.isnan(mo[1]) and math.isnan(mo[2])
        assert ex[0] == np.uint64(0xFFFFFFFFFFFFFFFF) and ex[1] == 0
        return
    w = spec_words(x)
    assert ex[0] == w.min() and ex[1] == w.max()
    if not exact_only:
        mean, m2 = exact_mean_m2(x)
        print(f"{x.dtype.name} n={n}: mean {close(mo[1], mean):.2e} M2 {close(mo[2], m2):.2e}")


def test_tile_rows_exported():
    assert _tile() == int(_C.sort_tile_rows()) and _tile() % 256 == 0


# ------------------------------------------------------------------ column_moments
@pytest.mark.parametrize("dtype", DTYPES)
def test_column_moments_every_row_count(dtype):
    big = _row_counts()[-1]
    c, w = centred(dtype, big), wide(dtype, big)
    for n in _row_counts():
        mo, ex = _C.column_moments([dev(c[:n]), dev(w[:n])])
        assert mo.is_cuda and ex.is_cuda and mo.dtype == torch.float64 and ex.dtype == torch.int64
        assert tuple(mo.shape) == (2, 3) and tuple(ex.shape) == (2, 2)
        check_record(mo[0], ex[0], c[:n])
        check_record(mo[1], ex[1], w[:n], exact_only=True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_column_moments_misaligned_views(dtype):
    t = _tile()
    c = centred(dtype, 2 * t + 11, seed=3)
    whole = dev(c)
    for start, stop in ((1, None), (3, t + 2), (1, 2), (5, 5)):
        view = whole[start:stop]
        assert view.is_contiguous() and (start * c.itemsize) % 16 != 0
        mo, ex = _C.column_moments([view])
        check_record(mo[0], ex[0], c[start:stop])
    # what the bytes around a view hold does not reach its record
    host = c.copy()
    host[0] = host[-1] = np.array(0, dtype=c.dtype)
    other = dev(host)
    a, b = _C.column_moments([whole[1:-1]]), _C.column_moments([other[1:-1]])
    assert a[0].cpu().numpy().tobytes() == b[0].cpu().numpy().tobytes()
    assert a[1].cpu().numpy().tobytes() == b[1].cpu().numpy().tobytes()


def test_uint8_column_of_odd_length():
    x = centred(np.uint8, 4033, seed=5)
    whole = dev(x)
    for a, b in ((0, 4033), (1, 4032), (13, 1000), (2, 3)):
        assert (b - a) % 2 == 1
        mo, ex = _C.column_moments([whole[a:b]])
        check_record(mo[0], ex[0], x[a:b])


def _mixed_columns(n, count):
    return [(centred if j % 2 else wide)(DTYPES[j % len(DTYPES)], n, seed=20 + j) for j in range(count)]


def test_sixteen_mixed_columns_and_seventeen_raise():
    n = _tile() + 65
    cols = _mixed_columns(n, 17)
    tens = [dev(c) for c in cols]
    tens[4] = dev(np.concatenate([cols[4][:1], cols[4]]))[1:]        # one of them misaligned
    mo, ex = _C.column_moments(tens[:16])
    assert tuple(mo.shape) == (16, 3) and tuple(ex.shape) == (16, 2)
    for j in range(16):
        m1, e1 = _C.column_moments([tens[j]])
        assert m1.cpu().numpy().tobytes() == mo[j:j + 1].cpu().numpy().tobytes(), j
        assert e1.cpu().numpy().tobytes() == ex[j:j + 1].cpu().numpy().tobytes(), j
        check_record(mo[j], ex[j], cols[j], exact_only=bool(j % 2 == 0))
    with pytest.raises(ValueError, match="1..16"):
        _C.column_moments(tens)
    with pytest.raises(ValueError, match="1..16"):
        _C.column_moments([])


def test_column_moments_is_the_same_on_every_run():
    n = 3 * _tile() + 7
    tens = [dev(centred(np.float32, n, seed=7)), dev(wide(np.float64, n, seed=8)), dev(wide(np.int64, n, seed=9))]
    first = _C.column_moments(tens)
    for _ in range(3):
        again = _C.column_moments(tens)
        assert again[0].cpu().numpy().tobytes() == first[0].cpu().numpy().tobytes()
        assert again[1].cpu().numpy().tobytes() == first[1].cpu().numpy().tobytes()


def test_column_moments_argument_errors_come_before_any_launch():
    x = dev(np.arange(64, dtype=np.float32))
    with pytest.raises(ValueError, match="device tensor"):
        _C.column_moments([x.cpu()])
    with pytest.raises(ValueError, match="device tensor"):
        _C.column_moments([x, x.cpu()])
    with pytest.raises(ValueError, match="1-D"):
        _C.column_moments([x.reshape(8, 8)])
    with pytest.raises(ValueError, match="rows"):
        _C.column_moments([x, x[:63]])
    with pytest.raises(TypeError, match="not supported"):
        _C.column_moments([x > 3])
    with pytest.raises(TypeError, match="not supported"):
        _C.column_moments([x.half()])
    with pytest.raises(TypeError, match="not supported"):
        _C.column_moments([x.to(torch.complex64)])
    with pytest.raises(ValueError, match="contiguous"):
        _C.column_moments([x[::2]])
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="device"):
            _C.column_moments([x, x.to("cuda:1")])


# ------------------------------------------------------------------ select_hist
def _hist_data(dtype, n, seed):
    """Clustered values: whole digits stay empty and long prefixes are shared."""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    if dt.kind == "f":
        x = (rng.integers(0, 40, n) * 0.25 - 3.0).astype(dt)
        x[::19] = np.nan
        x[3::23] = -0.0
        return x
    if dt.itemsize == 1:
        return rng.integers(10, 60, n).astype(dt)
    base = {2: 12000, 4: -70000, 8: 1 << 45}[dt.itemsize]
    return (base + rng.integers(0, 600, n) * 4).astype(dt)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("prefix_bits", [0, 8, 32, 56])
def test_select_hist_matches_bincount(dtype, prefix_bits):
    t = _tile()
    for n in (0, 1, 65, t + 1, 3 * t + 7):
        x = _hist_data(dtype, n, seed=n + prefix_bits)
        w = spec_words(x)
        col = dev(np.concatenate([x[:1], x]))[1:] if n else dev(x)       # a misaligned base as well
        some = [int(v) for v in w[:: max(n // 13, 1)][:13]] or [0]
        none = 0x0123456789ABCDEF                                        # (matches no row's prefix)
        sets = [[some[0]]] if prefix_bits == 0 else \
            [[some[0]], [none], (some + [none] * 16)[:14] + [some[0], some[0]]]
        for prefixes in sets:
            pre = torch.from_numpy(np.array(prefixes, dtype=np.uint64).view(np.int64))
            got = _C.select_hist(col, pre, prefix_bits)
            assert got.is_cuda and got.dtype == torch.int64 and tuple(got.shape) == (len(prefixes), 256)
            got = got.cpu().numpy()
            want = spec_hist(w, prefixes, prefix_bits)
            assert (got == want).all(), (n, prefixes)
            if prefix_bits == 0:
                assert got.sum() == n
            else:
                assert not got[[p == none for p in prefixes]].any()      # no row: an all-zero histogram
                if len(prefixes) == 16:
                    assert (got[14] == got[0]).all() and (got[15] == got[0]).all()   # equal prefixes, equal rows
            if n > 256:
                assert (want.sum(0) == 0).sum() > 100                    # several digits are empty
        if n and prefix_bits:
            again = _C.select_hist(col, pre.to(DEV), prefix_bits)        # device prefixes are read back first
            assert (again.cpu().numpy() == got).all()


def test_select_hist_argument_errors_come_before_any_launch():
    x = dev(np.arange(64, dtype=np.float32))
    one = torch.zeros(1, dtype=torch.int64)
    for bits in (-8, 4, 57, 64):
        with pytest.raises(ValueError, match="prefix_bits"):
            _C.select_hist(x, one, bits)
    with pytest.raises(ValueError, match="1..16"):
        _C.select_hist(x, torch.zeros(17, dtype=torch.int64), 8)
    with pytest.raises(ValueError, match="1..16"):
        _C.select_hist(x, torch.zeros(0, dtype=torch.int64), 8)
    with pytest.raises(ValueError, match="one histogram"):
        _C.select_hist(x, torch.zeros(2, dtype=torch.int64), 0)
    with pytest.raises(ValueError, match="int64 prefixes"):
        _C.select_hist(x, torch.zeros(1, dtype=torch.int32), 8)
    with pytest.raises(ValueError, match="device tensor"):
        _C.select_hist(x.cpu(), one, 8)
    with pytest.raises(ValueError, match="1-D"):
        _C.select_hist(x.reshape(8, 8), one, 8)
    with pytest.raises(TypeError, match="not supported"):
        _C.select_hist(x > 3, one, 8)
    with pytest.raises(ValueError, match="contiguous"):
        _C.select_hist(x[::2], one, 8)


# ------------------------------------------------------------------ frames
def _frame_columns(n, seed=0):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal(n)
    z[::17] = np.nan
    z[5::29] = -0.0
    z[7::31] = np.inf
    return {"x": (1e4 + rng.standard_normal(n)).astype(np.float32), "z": z,
            "k": rng.integers(0, 1000, n).astype(np.int32),
            "g": rng.integers(np.iinfo(np.int64).min, np.iinfo(np.int64).max, n, dtype=np.int64, endpoint=True),
            "u": rng.integers(0, 256, n).astype(np.uint8), "h": 1e4 + rng.standard_normal(n),
            "v": rng.standard_normal((n, 3)).astype(np.float32), "s": np.array([f"name-{i}" for i in range(n)])}


NUMERIC = ["x", "z", "k", "g", "u", "h"]


def _mixed_device_frame(host):
    """The frame on the device, except column `h`, which stays on the host."""
    from tensorframes_amd.frame.block import Block
    from tensorframes_amd.frame.dataframe import DataFrame, _Materialized
    on_dev = host.cache_on_device(DEV)
    blocks = {p: Block(b.nrows, {n: (c.cpu() if n == "h" else c) for n, c in b.columns.items()})
              for p, b in on_dev.local_blocks().items()}
    return DataFrame(on_dev.schema, _Materialized(blocks), on_dev.num_partitions)


def _table(out):
    labels = out.to_numpy("summary").tolist()
    return {c: dict(zip(labels, out.to_numpy(c).tolist())) for c in out.columns if c != "summary"}


def _delta(fn):
    before = tfs.metrics.snapshot()
    res = fn()
    after = tfs.metrics.snapshot()
    return res, {k: after.get(k, 0) - before.get(k, 0) for k in ("stats_rows", "quantile_passes")}


def _check_describe(t, cols):
    for name in NUMERIC:
        x = cols[name]
        s = x[np.argsort(spec_words(x), kind="stable")]
        want = [float(len(x)), float(canonical(s[0])), float(canonical(s[-1]))]
        got = [t[name]["count"], t[name]["min"], t[name]["max"]]
        assert np.array(got).tobytes() == np.array(want).tobytes(), name
    for name in ("x", "h", "k", "u"):
        mean, m2 = exact_mean_m2(cols[name])
        close(t[name]["mean"], mean)
        close(t[name]["stddev"], math.sqrt(m2 / (len(cols[name]) - 1)))
    assert math.isnan(t["z"]["mean"]) and math.isnan(t["z"]["stddev"])     # a NaN in the column propagates


@pytest.mark.parametrize("nparts", [1, 4])
def test_device_resident_frames_match_the_host_path(nparts):
    n = 2 * _tile() + 77
    cols = _frame_columns(n)
    host = tfs.from_columns(cols, num_partitions=nparts)
    mixed = _mixed_device_frame(host)
    placement = {p: {name: c.is_cuda for name, c in b.columns.items()} for p, b in mixed.local_blocks().items()}
    assert all(pl["x"] and pl["s"] and not pl["h"] for pl in placement.values())
    out, d = _delta(mixed.describe)
    assert out.columns == ["summary"] + NUMERIC and d == {"stats_rows": n * len(NUMERIC), "quantile_passes": 0}
    _check_describe(_table(out), cols)
    q, d = _delta(lambda: mixed.approxQuantile(NUMERIC, PROBS, 0.0))
    want = np.stack([as_doubles(spec_quantiles(cols[c], PROBS)) for c in NUMERIC])
    assert np.array(q).tobytes() == want.tobytes()
    assert np.array(host.approxQuantile(NUMERIC, PROBS, 0.0)).tobytes() == want.tobytes()
    # passes per column and pass (not per partition): x <= 4, z 8, k 2, g 8, u 1, h <= 8
    assert d["stats_rows"] == n * len(NUMERIC) and 21 <= d["quantile_passes"] <= 31
    _, d = _delta(lambda: mixed.approxQuantile("k", [0.5], 0.0))
    assert d == {"stats_rows": n, "quantile_passes": 2}                   # an int32 column in [0, 1000)
    s = _table(mixed.summary("count", "2.5%", "50%", "max"))
    for c in NUMERIC:
        w = as_doubles(spec_quantiles(cols[c], [0.025, 0.5]))
        assert np.array([s[c]["2.5%"], s[c]["50%"]]).tobytes() == w.tobytes(), c
    # what was on the device stays there, what was on the host stays on the host
    assert placement == {p: {name: c.is_cuda for name, c in b.columns.items()}
                         for p, b in mixed.local_blocks().items()}
    empty = mixed.filter(mixed.k < 0)
    assert empty.approxQuantile("x", [0.5], 0.0) == [] and _table(empty.describe("x"))["x"]["count"] == 0.0


def test_host_resident_frame_on_a_gpu_engine():
    n = _tile() + 9
    cols = _frame_columns(n, seed=2)
    host = tfs.from_columns(cols, num_partitions=3)
    _check_describe(_table(host.describe()), cols)
    want = np.stack([as_doubles(spec_quantiles(cols[c], PROBS)) for c in NUMERIC])
    assert np.array(host.approxQuantile(NUMERIC, PROBS, 0.0)).tobytes() == want.tobytes()


def _results(df):
    d, s = df.describe(), df.summary()
    return {"describe": {c: d.to_numpy(c).tobytes().hex() for c in d.columns if c != "summary"},
            "summary": {c: s.to_numpy(c).tobytes().hex() for c in s.columns if c != "summary"},
            "q": np.array(df.approxQuantile(NUMERIC, PROBS, 0.0)).tobytes().hex()}


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
    df = tfs.from_columns(_frame_columns(3001, seed=4), num_partitions=5).cache_on_device()
    res = _results(df)
    res["device"] = engine.compute_device().type
    res["on_device"] = all(b.columns[c].is_cuda for b in df.local_blocks().values() for c in NUMERIC)
    with open(os.path.join(outdir, f"r{rank}.json"), "w") as f:
        json.dump(res, f)
    dist.shutdown()


def test_describe_two_ranks_share_one_gpu(tmp_path):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    outs = [json.load(open(tmp_path / f"r{r}.json")) for r in range(2)]
    cols = _frame_columns(3001, seed=4)
    single = _results(tfs.from_columns(cols, num_partitions=5).cache_on_device(DEV))
    for o in outs:
        assert o["device"] == "cuda" and o["on_device"]
        for key in ("describe", "summary", "q"):
            assert o[key] == single[key], key
    want = np.stack([as_doubles(spec_quantiles(cols[c], PROBS)) for c in NUMERIC])
    assert single["q"] == want.tobytes().hex()
