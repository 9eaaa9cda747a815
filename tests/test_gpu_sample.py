"""The device kernels under `sample` / `randomSplit` / `sampleBy` / `F.rand` /
`F.randn` (csrc/kernels/random.hip) and the frame paths that use them, on the
GPU.

Kernel level: every expected value comes from the Philox4x32-10 written here
from its definition, on Python ints; u is an integer over 2^53, so masks and
counts are compared exactly (a bound that is a float is compared as a
`Fraction`). The normal draw is held to 2^-48 * max(1, r), r = sqrt(-2 ln u1):
r carries a relative error of a few ulp of log halved by sqrt (at most 2^-51),
cos an absolute error of at most 2^-50 from the rounded argument plus 2^-51
from the function; the sum is at most r * 2^-49 and the bound doubles it.
Frame level: the device path is compared with the host path
(tests/test_sample.py holds that one to the definition).
No test hands a kernel a length that disagrees with its tensors or an index
out of range."""
import bisect
import functools
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import tensorframes_amd as tfs
from tensorframes_amd import functions as F
from tensorframes_amd._native import _C

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]

DEV = "cuda:0"
M32 = 0xFFFFFFFF
SEEDS = [0, 2 ** 64 - 1, 0x299F31D0A4093822]
ROW0S = [0, 1, 2 ** 32 - 3, 2 ** 40 + 5]   # the third: the counter carries into word 1 inside a tile
CASES = [(s, r) for s in SEEDS for r in ROW0S]


def T():
    return int(_C.random_tile_rows())


def sizes():
    t = T()
    return [1, 2, 63, 64, 65, t - 1, t, t + 1, 2 * t + 7]


# ------------------------------------------------------------------ the specification
def philox(counter, key):
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for r in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        if r < 9:
            k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def test_the_specification_reproduces_the_known_answers():
    assert philox((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert philox((M32,) * 4, (M32,) * 2) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    assert philox((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == \
        (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)


@functools.lru_cache(maxsize=None)
def words(seed, row0, purpose, n):
    """The four words of the rows row0 .. row0 + n, computed once per stream."""
    key = (seed & M32, seed >> 32)
    return [philox(((row0 + i) & M32, (row0 + i) >> 32, purpose, 0), key) for i in range(n)]


def stream(seed, row0, purpose):
    return words(seed, row0, purpose, 2 * T() + 7)


def x53(a, b):
    return ((a << 32) | b) >> 11


def u_ints(seed, row0, purpose=0):
    """u * 2^53 of every row of the stream, as ints."""
    return [x53(w[0], w[1]) for w in stream(seed, row0, purpose)]


def thr(f):
    """The int t with (u >= f) == (x >= t) and (u < f) == (x < t) for u = x * 2^-53."""
    return math.ceil(Fraction(f) * 2 ** 53)


def as_u(x):
    return x * 2.0 ** -53  # (an integer below 2^53 times a power of two: exact)


def normal_and_r(w):
    u1 = (x53(w[0], w[1]) + 1) * 2.0 ** -53
    u2 = x53(w[2], w[3]) * 2.0 ** -53
    r = math.sqrt(-2.0 * math.log(u1))
    return r * math.cos(2.0 * math.pi * u2), r


def poisson_cdf(lam):
    term = math.exp(-lam)
    cdf = [term]
    j = 0
    while cdf[-1] < 1.0 - 2.0 ** -53 and len(cdf) < 64:
        j += 1
        term *= lam / j
        cdf.append(cdf[-1] + term)
    return cdf


def host(t):
    assert t.is_cuda and t.dim() == 1
    return t.cpu().numpy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------ kernels
def test_no_rows_launch_nothing():
    for got, dt in ((_C.random_uniform(1, 0, 0), torch.float64), (_C.random_normal(1, 0, 0), torch.float64),
                    (_C.random_mask(1, 0, 0, 0.0, 1.0), torch.uint8),
                    (_C.random_poisson(1, 0, 0, dev(np.array([1.0]))), torch.int64),
                    (_C.random_mask_by(1, 0, dev(np.zeros((1, 0), dtype=np.int64)), dev(np.array([3], dtype=np.int64)),
                                       dev(np.array([0.5]))), torch.uint8),
                    (_C.random_expand(dev(np.zeros(0, dtype=np.int64))), torch.int64)):
        assert got.is_cuda and got.dtype == dt and tuple(got.shape) == (0,)


@pytest.mark.parametrize("seed,row0", CASES)
def test_uniform_is_exact(seed, row0):
    want = np.array([as_u(x) for x in u_ints(seed, row0)])
    for n in sizes():
        got = _C.random_uniform(seed, row0, n)
        assert got.dtype == torch.float64
        assert host(got).tobytes() == want[:n].tobytes(), n


@pytest.mark.parametrize("seed,row0", CASES)
def test_normal_is_within_the_derived_bound(seed, row0):
    zr = [normal_and_r(w) for w in stream(seed, row0, 1)]
    want = np.array([z for z, _ in zr])
    bound = np.array([2.0 ** -48 * max(1.0, r) for _, r in zr])
    for n in sizes():
        got = host(_C.random_normal(seed, row0, n))
        assert got.shape == (n,)
        err = np.abs(got - want[:n])
        assert np.all(err <= bound[:n]), (n, float((err / bound[:n]).max()))


@pytest.mark.parametrize("seed,row0", CASES)
def test_mask_is_exact(seed, row0):
    xs = u_ints(seed, row0)
    lo, hi = 0.3, 0.85
    want = np.array([thr(lo) <= x < thr(hi) for x in xs], dtype=np.uint8)
    for n in sizes():
        got = _C.random_mask(seed, row0, n, lo, hi)
        assert got.dtype == torch.uint8
        assert np.array_equal(host(got), want[:n]), n


def test_mask_bounds():
    seed, row0, n = 5, 11, T() + 9
    xs = u_ints(seed, row0)[:n]
    assert not host(_C.random_mask(seed, row0, n, 0.0, 0.0)).any()
    assert host(_C.random_mask(seed, row0, n, 0.0, 1.0)).all()
    assert not host(_C.random_mask(seed, row0, n, 0.25, 0.25)).any()
    for r in (0, 70, n - 1):  # a bound that is row r's u: the lower bound keeps the row, the upper does not
        b = as_u(xs[r])
        low = host(_C.random_mask(seed, row0, n, b, 1.0))
        up = host(_C.random_mask(seed, row0, n, 0.0, b))
        assert low[r] == 1 and up[r] == 0
        assert np.array_equal(low, np.array([x >= xs[r] for x in xs], dtype=np.uint8))
        assert np.array_equal(up, np.array([x < xs[r] for x in xs], dtype=np.uint8))


def strata_tables():
    """(table words as unsigned ints, ascending; fractions) for 1, 2 and 4096
    strata, with and without the smallest and the largest word."""
    out = []
    for S in (1, 2, 4096):
        inner = [1000 + 7 * i for i in range(S - 1)] + [2 ** 63 + 12345]
        fr = [((i * 37 + 4) % 11) / 10.0 for i in range(S)]  # 0.4, 0.8, ... with 0 and 1 among them
        out.append((inner, fr))
        if S == 1:
            out.append(([0], [0.6]))
            out.append(([2 ** 64 - 1], [0.6]))
        else:
            out.append(([0] + inner[1:-1] + [2 ** 64 - 1], fr))
    return out


@pytest.mark.parametrize("ti", range(7))
def test_mask_by_is_exact(ti):
    tw, tf = strata_tables()[ti]
    seed, row0 = SEEDS[ti % 3], ROW0S[(ti + 2) % 4]
    xs = u_ints(seed, row0)
    S = len(tw)
    # table hits (first, last, middle), a word below, between and above all entries, the extremes
    cand = [tw[0], tw[-1], tw[S // 2], tw[S // 3], tw[0] - 3, tw[0] + 1, tw[-1] + 9, tw[S // 2] + 2, 0, 2 ** 64 - 1,
            2 ** 63 - 1, 2 ** 63]
    cand = [min(max(c, 0), 2 ** 64 - 1) for c in cand]
    nmax = 2 * T() + 7
    rw = [cand[(i * 5 + i // 7) % len(cand)] for i in range(nmax)]
    look = {w: thr(f) for w, f in zip(tw, tf)}
    want = np.array([x < look.get(w, 0) for x, w in zip(xs, rw)], dtype=np.uint8)
    assert want.any() and not want.all()
    rw_np = np.array(rw, dtype=np.uint64).view(np.int64)
    table = (dev(np.array(tw, dtype=np.uint64).view(np.int64)), dev(np.array(tf, dtype=np.float64)))
    for n in sizes():
        got = _C.random_mask_by(seed, row0, dev(rw_np[:n].reshape(1, n)), *table)
        assert got.dtype == torch.uint8
        assert np.array_equal(host(got), want[:n]), n


@pytest.mark.parametrize("seed,row0", CASES)
def test_poisson_counts_are_exact(seed, row0):
    xs = u_ints(seed, row0, 2)
    tables = [[0.5], [1.0], poisson_cdf(16.0), [(k + 1) / 64.0 for k in range(64)], poisson_cdf(0.3)]
    assert len(tables[2]) == 64 and len(tables[3]) == 64
    for cdf in tables:
        ts = [thr(c) for c in cdf]  # (c <= u) == (thr(c) <= x); the tables are non-decreasing
        assert ts == sorted(ts)
        want = np.array([bisect.bisect_right(ts, x) for x in xs], dtype=np.int64)
        table = dev(np.array(cdf, dtype=np.float64))
        for n in sizes():
            got = _C.random_poisson(seed, row0, n, table)
            assert got.dtype == torch.int64
            assert np.array_equal(host(got), want[:n]), (len(cdf), n)


def test_expand_repeats_rows_in_order():
    rng = np.random.default_rng(3)
    for n in (1, 5, T() + 3):
        counts = rng.integers(0, 5, n).astype(np.int64)
        counts[0] = 0
        counts[n // 2] = 64
        got = host(_C.random_expand(dev(counts)))
        assert np.array_equal(got, np.repeat(np.arange(n, dtype=np.int64), counts))
    assert tuple(_C.random_expand(dev(np.zeros(7, dtype=np.int64))).shape) == (0,)


# ------------------------------------------------------------------ frames
def frames(strings=False):
    """(host frame, device-cached frame) of three partitions with 0, 5 and
    T + 3 rows."""
    t = T() + 3
    n = 3 * t
    keep = np.zeros(n, dtype=np.int32)
    keep[t:t + 5] = 1
    keep[2 * t:] = 1
    rng = np.random.default_rng(8)
    cols = {"k": rng.integers(0, 6, n).astype(np.int32), "x": rng.standard_normal(n).astype(np.float32),
            "i": np.arange(n, dtype=np.int64)}
    if strings:
        cols["s"] = [f"row-{i}" for i in range(n)]
    df = tfs.from_columns(dict(cols, keep=keep), num_partitions=3)
    df = df.filter(df.keep > 0).select(*cols)
    hostf = df.to_host()
    assert [hostf.local_blocks()[p].nrows for p in range(3)] == [0, 5, T() + 3]
    return hostf, hostf.cache_on_device(DEV)


def same_bytes(a, b, names):
    for c in names:
        x, y = a.to_numpy(c), b.to_numpy(c)
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), c


def on_device(out):
    for b in out.local_blocks().values():
        for c in b.columns.values():
            if isinstance(c, torch.Tensor):
                assert c.is_cuda


def device_partitions(fn):
    before = tfs.metrics.snapshot()
    out = fn()
    after = tfs.metrics.snapshot()
    return out, {k: after.get(k, 0) - before.get(k, 0) for k in ("sample_device_partitions", "sample_host_partitions",
                                                                 "sample_rows_in", "sample_rows_out")}


def check(hostf, devf, op, names, passes=1):
    """op on the device-cached frame gives op on the host frame, bit for bit,
    and stays on the device; `passes`: the sampling frames op stacks."""
    want = op(hostf)
    got = op(devf)
    _, m = device_partitions(got.local_blocks)
    assert m["sample_device_partitions"] == 2 * passes and m["sample_host_partitions"] == 0
    assert m["sample_rows_in"] == (T() + 8) * passes
    on_device(got)
    assert [b.nrows for _, b in sorted(got.local_blocks().items())] == \
        [b.nrows for _, b in sorted(want.local_blocks().items())]
    same_bytes(want, got, names)
    return want, got


def test_frame_sample_gives_the_host_bytes():
    hostf, devf = frames()
    names = ["k", "x", "i"]
    want, _ = check(hostf, devf, lambda d: d.sample(0.4, 9), names)
    assert 0 < want.count() < T() + 8
    want, _ = check(hostf, devf, lambda d: d.sample(True, 1.5, 9), names)
    assert want.count() > T() + 8
    check(hostf, devf, lambda d: d.sample(True, 0.0, 9), names)
    for i in range(3):
        check(hostf, devf, lambda d: d.randomSplit([3, 1, 1], 4)[i], names)
    check(hostf, devf, lambda d: d.sampleBy("k", {0: 1.0, 2: 0.5, 5: 0.0, 77: 1.0}, 2), names)
    check(hostf, devf, lambda d: d.sampleBy("k", {}, 2), names)


def test_frame_rand_columns_give_the_host_bytes():
    hostf, devf = frames()
    want, got = check(hostf, devf, lambda d: d.withColumn("r", F.rand(6)).select("i", "r", F.randn(7).alias("z")),
                      ["i", "r"], passes=2)
    a, b = want.to_numpy("z"), got.to_numpy("z")
    # both sides within the kernel test's bound of the exact value: twice the bound between them
    xs = [normal_and_r(w) for w in words(7, 0, 1, T() + 8)]
    bound = np.array([2.0 * 2.0 ** -48 * max(1.0, r) for _, r in xs])
    assert np.all(np.abs(a - b) <= bound)
    assert np.all(np.abs(a - np.array([z for z, _ in xs])) <= bound)


def test_frame_with_a_string_column_keeps_the_right_strings():
    hostf, devf = frames(strings=True)
    for op in (lambda d: d.sample(0.3, 12), lambda d: d.sample(True, 1.2, 12),
               lambda d: d.sampleBy("k", {1: 0.7, 3: 1.0}, 12)):
        want, got = op(hostf), op(devf)
        rows = got.collect()
        assert rows == want.collect() and len(rows) > 0
        assert all(r.s == f"row-{r.i}" for r in rows)
