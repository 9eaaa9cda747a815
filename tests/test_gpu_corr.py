"""The device kernels under `F.corr` / `F.covar_samp` / `F.covar_pop` and
`df.stat.corr` / `df.stat.cov` (csrc/kernels/stats.hip: column_pair_moments;
csrc/kernels/group_stats.hip: group_pair_moments, merge_pair_records,
pair_results) and the frame paths that use them, on the GPU.

Expected values are written here: exact rational arithmetic over the
f64-converted data gives the co-moment C = sum (x - mean_x)(y - mean_y) and
both M2, each rounded once (the values are scaled to integers by a power of
two first, so the sums are Python ints and the one division is a
`fractions.Fraction`), Python ints give n and the count of non-finite rows.

Tolerances are those derived in tests/test_corr.py, for the same data
(x = 1e4 + z, y = 1e4 + 0.6 z + 0.8 w, kappa = 1e4, r near 0.6; a smaller
kappa for the integer dtypes): C within 1e-11 * sqrt(M2x * M2y), both M2
within 1e-11 relative, corr within 2e-11 absolute, the covariances within the
C bound over n / n - 1, n and the non-finite count exact.

The device merge contracts a + d * f into one fused operation (the build's
-ffp-contract=fast) and numpy does not, so the host `_pair_chan` and
`merge_pair_records` agree bit for bit where the merged records come from
identical inputs (both deltas are zero and the merge is one rounding, fused
or not) or one side is empty, and within the bounds elsewhere; `pair_results`
has nothing to contract and is compared bit for bit.

No test hands a kernel an index out of range or lengths that do not agree;
those are refused by the bindings, and that is what is tested."""
import json
import math
import os
import socket
import sys
import time
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import tensorframes_amd as tfs
from tensorframes_amd import functions as F
from tensorframes_amd._native import _C
from tensorframes_amd.frame import group_agg as GA

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-11
CORR_BOUND = 2e-11
DTYPES = [np.uint8, np.int8, np.int16, np.int32, np.int64, np.float32, np.float64]
PAIR_STATS = ["corr", "covar_samp", "covar_pop"]


def _chunk():
    return int(_C.group_chunk_rows())


# ------------------------------------------------------------------ the specification
def cast(v, dt):
    dt = np.dtype(dt)
    if dt.kind == "f":
        return (1e4 + v).astype(dt)
    if dt.itemsize == 1:
        return np.clip(np.rint(100 + 5 * v), 0 if dt.kind == "u" else -128, 127).astype(dt)
    return np.rint(10000 + 100 * v).astype(dt)


def pair_data(dx, dy, n, seed=0):
    """x = 1e4 + z, y = 1e4 + 0.6 z + 0.8 w, cast to the column dtypes (integers: a scaled, rounded form)."""
    rng = np.random.default_rng(seed)
    z, w = rng.standard_normal(n), rng.standard_normal(n)
    return cast(z, dx), cast(0.6 * z + 0.8 * w, dy)


def _scaled(x: np.ndarray):
    """(Python ints, D) with value = int / D exactly, D a power of two."""
    ratios = [float(v).as_integer_ratio() for v in x.astype(np.float64)]
    d = max((r[1] for r in ratios), default=1)
    return [r[0] * (d // r[1]) for r in ratios], d


_EXACT = {}


def exact(x: np.ndarray, y: np.ndarray):
    """(C, M2x, M2y) of the f64-converted data in exact arithmetic, each rounded once."""
    key = (x.dtype.str, x.tobytes(), y.dtype.str, y.tobytes())
    if key not in _EXACT:
        (ix, dx), (iy, dy) = _scaled(x), _scaled(y)
        n = len(ix)
        sx, sy = sum(ix), sum(iy)
        # n * sum (x - mx)(y - my) = n * sum xy - sx * sy, in integers
        c = Fraction(n * sum(a * b for a, b in zip(ix, iy)) - sx * sy, n * dx * dy)
        m2x = Fraction(n * sum(a * a for a in ix) - sx * sx, n * dx * dx)
        m2y = Fraction(n * sum(b * b for b in iy) - sy * sy, n * dy * dy)
        _EXACT[key] = (float(c), float(m2x), float(m2y))
    return _EXACT[key]


def check_record(r: np.ndarray, x: np.ndarray, y: np.ndarray, where=""):
    """One pair record [7] against the rows it stands for (finite data)."""
    f = r[:6].view(np.float64)
    assert f[0] == float(len(x)) and int(r[6]) == 0, (where, f[0], r[6])
    if len(x) == 0:
        assert not r.any(), (where, r)
        return
    c, m2x, m2y = exact(x, y)
    scale = math.sqrt(m2x * m2y)
    assert abs(f[5] - c) <= BOUND * scale, (where, f[5], c, abs(f[5] - c) / max(scale, 1e-300))
    for got, want in ((f[3], m2x), (f[4], m2y)):
        assert abs(got - want) <= BOUND * want, (where, got, want)
    for got, col in ((f[1], x), (f[2], y)):
        mean = float(col.astype(np.float64).mean())
        assert abs(got - mean) <= BOUND * abs(mean), (where, got, mean)


def spec(fn: str, x: np.ndarray, y: np.ndarray):
    """(expected value, absolute bound) of pair statistic `fn` over the group's rows."""
    n = len(x)
    bad = int((~(np.isfinite(x.astype(np.float64)) & np.isfinite(y.astype(np.float64)))).sum())
    if n == 0 or bad:
        return math.nan, 0.0
    c, m2x, m2y = exact(x, y)
    scale = math.sqrt(m2x * m2y)
    if fn == "covar_pop":
        return c / n, BOUND * scale / n
    if fn == "covar_samp":
        return (c / (n - 1), BOUND * scale / (n - 1)) if n >= 2 else (math.nan, 0.0)
    if m2x == 0 or m2y == 0:
        return math.nan, 0.0
    return c / scale, CORR_BOUND


def check_value(got, fn, x, y, where=""):
    got = np.asarray(got)[()]
    assert got.dtype == np.float64, (where, fn, got.dtype)
    want, bound = spec(fn, x, y)
    if math.isnan(want):
        assert math.isnan(got), (where, fn, got)
    else:
        assert abs(float(got) - want) <= bound, (where, fn, got, want, abs(float(got) - want), bound)


def dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def dense(xs, ys) -> np.ndarray:
    rec = _C.column_pair_moments([c if isinstance(c, torch.Tensor) else dev(c) for c in xs],
                                 [c if isinstance(c, torch.Tensor) else dev(c) for c in ys])
    assert rec.is_cuda and rec.dtype == torch.int64 and tuple(rec.shape) == (len(xs), 7)
    return rec.cpu().numpy()


# ------------------------------------------------------------------ column_pair_moments
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 17, 70001])
def test_dense_row_counts(n):
    x, y = pair_data(np.float32, np.float64, n, seed=n % 3)
    h = x.astype(np.float64) * 0.5
    rec = dense([x, y, h], [y, x, h])
    check_record(rec[0], x, y, n)
    check_record(rec[1], y, x, n)
    check_record(rec[2], h, h, n)
    assert rec.tobytes() == dense([x, y, h], [y, x, h]).tobytes()       # the same bits on every run
    # (x, y) and (y, x) are one co-moment
    assert abs(rec[0, 5:6].view(np.float64)[0] - rec[1, 5:6].view(np.float64)[0]) <= 2 * BOUND * math.sqrt(
        exact(x, y)[1] * exact(x, y)[2])


@pytest.mark.parametrize("dx", DTYPES, ids=lambda d: np.dtype(d).name)
def test_dense_every_pair_of_dtypes(dx):
    n = 4097
    rng = np.random.default_rng(11)
    z, w = rng.standard_normal(n), rng.standard_normal(n)
    x = cast(z, dx)
    ys = [cast(0.6 * z + 0.8 * w, dy) for dy in DTYPES]
    rec = dense([x] * 7, ys)
    for j, y in enumerate(ys):
        check_record(rec[j], x, y, (dx, DTYPES[j]))


@pytest.mark.parametrize("dx,dy", [(np.float32, np.float64), (np.float64, np.float32), (np.uint8, np.int16),
                                   (np.int64, np.int8), (np.float32, np.float32)])
def test_dense_misaligned_views(dx, dy):
    n = 2 * 4096 + 29
    bx, by = pair_data(dx, dy, n + 3, seed=12)
    tx, ty = dev(bx), dev(by)
    for ox, oy in ((1, 0), (0, 3), (1, 3), (2, 2)):
        vx, vy = tx[ox:ox + n], ty[oy:oy + n]
        assert vx.is_contiguous() and vy.is_contiguous()
        assert (vx.data_ptr() % 16 != 0) == (ox * bx.itemsize % 16 != 0)
        assert (vy.data_ptr() % 16 != 0) == (oy * by.itemsize % 16 != 0)
        if (ox, oy) == (1, 3):
            assert vx.data_ptr() % 16 != 0 and vy.data_ptr() % 16 != 0
        rec = dense([vx], [vy])
        check_record(rec[0], bx[ox:ox + n], by[oy:oy + n], (dx, dy, ox, oy))
        # the result depends on the rows alone, not on where the column starts
        assert rec.tobytes() == dense([vx.clone()], [vy.clone()]).tobytes()


def test_dense_sixteen_pairs_share_columns():
    n = 4096 + 33
    rng = np.random.default_rng(13)
    z = rng.standard_normal((4, n))
    cols = [cast(z[0], np.float32), cast(0.6 * z[0] + 0.8 * z[1], np.float64), cast(z[2], np.int32),
            cast(0.3 * z[2] - 0.9 * z[3], np.uint8)]
    tcols = [dev(c) for c in cols]
    pairs = [(a, b) for a in range(4) for b in range(4)]
    rec = dense([tcols[a] for a, _ in pairs], [tcols[b] for _, b in pairs])
    for j, (a, b) in enumerate(pairs):
        check_record(rec[j], cols[a], cols[b], (a, b))
    # a pair's record does not depend on its company
    assert dense([tcols[1]], [tcols[3]])[0].tobytes() == rec[pairs.index((1, 3))].tobytes()
    with pytest.raises(ValueError, match="1..16 pairs"):
        _C.column_pair_moments([tcols[0]] * 17, [tcols[1]] * 17)


def test_dense_no_rows_and_non_finite_rows():
    e = torch.empty(0, dtype=torch.float32, device=DEV)
    rec = _C.column_pair_moments([e, e.to(torch.int64)], [e.to(torch.float64), e])
    assert rec.is_cuda and tuple(rec.shape) == (2, 7) and not rec.cpu().numpy().any()   # the empty record: zeros
    n = 4096 + 100
    x, y = pair_data(np.float64, np.float32, n, seed=14)
    x[0], x[17] = np.nan, np.inf                                        # rows of whole runs and of the tail
    y[17], y[4000], y[n - 1] = -np.inf, np.inf, np.nan
    rec = dense([x, y], [y, y])
    assert int(rec[0, 6]) == 4 and int(rec[1, 6]) == 3
    assert rec[:, 0].view(np.float64).tolist() == [float(n), float(n)]
    outs = _C.pair_results(dev(rec[None]), [0, 0, 0, 1], PAIR_STATS + ["corr"])
    assert all(math.isnan(float(o[0])) for o in outs)


def test_bindings_refuse_what_does_not_fit():
    x, y = dev(np.arange(100, dtype=np.float64)), dev(np.arange(100, dtype=np.float32))
    perm, offsets = _C.segment_csr(dev(np.zeros(100, dtype=np.int64)), 1)
    for call in (lambda xs, ys: _C.column_pair_moments(xs, ys),
                 lambda xs, ys: _C.group_pair_moments(xs, ys, perm, offsets),
                 lambda xs, ys: _C.group_both_moments([x], xs, ys, perm, offsets)):
        with pytest.raises(ValueError, match="first columns"):
            call([x, x], [y])
        with pytest.raises(ValueError, match="rows"):
            call([x], [y[:99].contiguous()])
        with pytest.raises(ValueError, match="rows"):
            call([x, x[:50].contiguous()], [y, y])
        with pytest.raises(ValueError, match="device"):
            call([x], [y.cpu()])
        with pytest.raises(ValueError, match="contiguous"):
            call([x[::2]], [y[::2]])
        with pytest.raises(TypeError, match="not supported"):
            call([x.to(torch.float16)], [y])
        with pytest.raises(ValueError, match="1..16 pairs"):
            call([], [])
    with pytest.raises(ValueError, match="perm has 99 entries"):
        _C.group_pair_moments([x], [y], perm[:99].contiguous(), offsets)
    with pytest.raises(ValueError, match="offsets"):
        _C.group_pair_moments([x], [y], perm, offsets[:0])
    with pytest.raises(TypeError, match="int64"):
        _C.group_pair_moments([x], [y], perm.to(torch.int32), offsets)
    rec = _C.group_pair_moments([x], [y], perm, offsets)
    with pytest.raises(ValueError, match="records"):
        _C.merge_pair_records(rec[:, :, :6].contiguous(), offsets)
    with pytest.raises(ValueError, match="not a pair statistic"):
        _C.pair_results(rec, [0], ["avg"])
    with pytest.raises(ValueError, match="names pair 1"):
        _C.pair_results(rec, [1], ["corr"])
    with pytest.raises(ValueError, match="one statistic per output"):
        _C.pair_results(rec, [0, 0], ["corr"])


# ------------------------------------------------------------------ group_pair_moments
def ids_of(sizes, seed=0):
    ids = np.repeat(np.arange(len(sizes), dtype=np.int64), sizes)
    np.random.default_rng(seed).shuffle(ids)
    return ids


def grouped(xs, ys, ids, ng) -> np.ndarray:
    perm, offsets = _C.segment_csr(dev(ids), ng)
    rec = _C.group_pair_moments([dev(c) for c in xs], [dev(c) for c in ys], perm, offsets)
    assert rec.is_cuda and rec.dtype == torch.int64 and tuple(rec.shape) == (ng, len(xs), 7)
    return rec.cpu().numpy()


def check_grouped(rec, xs, ys, ids, ng):
    oracle = GA._host_pair_records([torch.from_numpy(c) for c in xs], [torch.from_numpy(c) for c in ys], ids, ng) \
        if np.bincount(ids, minlength=ng).min() > 0 else None
    for g in range(ng):
        rows = np.nonzero(ids == g)[0]
        for q, (x, y) in enumerate(zip(xs, ys)):
            check_record(rec[g, q], x[rows], y[rows], (g, q))
            if oracle is not None:                                      # n and the count: the host oracle's, exactly
                assert rec[g, q, 0] == oracle[g, q, 0] and rec[g, q, 6] == oracle[g, q, 6]


@pytest.mark.parametrize("dx,dy", [(np.float32, np.float64), (np.float64, np.int32), (np.uint8, np.float32),
                                   (np.int16, np.int64), (np.int8, np.int8)])
def test_grouped_every_segment_size_in_one_call(dx, dy):
    c = _chunk()
    sizes = [1, 2, 63, 64, 65, c - 1, c, c + 1, 3 * c + 7]
    ids = ids_of(sizes)
    x, y = pair_data(dx, dy, len(ids), seed=21)
    rec = grouped([x, y], [y, y], ids, len(sizes))
    check_grouped(rec, [x, y], [y, y], ids, len(sizes))
    assert rec.tobytes() == grouped([x, y], [y, y], ids, len(sizes)).tobytes()
    # with the one-column records of the same CSR: the work items built once, the same bits
    perm, offsets = _C.segment_csr(dev(ids), len(sizes))
    one, two = _C.group_both_moments([dev(x)], [dev(x), dev(y)], [dev(y), dev(y)], perm, offsets)
    assert two.cpu().numpy().tobytes() == rec.tobytes()
    assert one.cpu().numpy().tobytes() == _C.group_moments([dev(x)], perm, offsets).cpu().numpy().tobytes()


def test_grouped_half_of_the_rows_in_one_key():
    c = _chunk()
    n = 40 * c + 11
    rng = np.random.default_rng(22)
    ids = np.where(rng.random(n) < 0.5, 0, rng.integers(1, 30, n)).astype(np.int64)
    assert (ids == 0).sum() > 8 * c                                     # more chunks than one thread folds
    x, y = pair_data(np.float32, np.float64, n, seed=23)
    rec = grouped([x], [y], ids, 30)
    check_grouped(rec, [x], [y], ids, 30)
    assert rec.tobytes() == grouped([x], [y], ids, 30).tobytes()


def test_grouped_record_follows_the_segments_row_order():
    c = _chunk()
    sizes = [3, 2 * c + 31, 65, 1]
    ids = ids_of(sizes, seed=24)
    n = len(ids)
    x, y = pair_data(np.float64, np.float32, n, seed=25)
    perm, offsets = _C.segment_csr(dev(ids), len(sizes))
    p, o = perm.cpu().numpy(), offsets.cpu().numpy()
    p2 = np.concatenate([p[o[g]:o[g + 1]][::-1] for g in range(len(sizes))])   # every segment's rows reversed
    got = _C.group_pair_moments([dev(x)], [dev(y)], dev(p2), offsets).cpu().numpy()
    # the same rows in that order, laid out densely and read through the identity
    want = _C.group_pair_moments([dev(x[p2])], [dev(y[p2])], dev(np.arange(n, dtype=np.int64)), offsets).cpu().numpy()
    assert got.tobytes() == want.tobytes()
    for g in range(len(sizes)):
        check_record(got[g, 0], x[ids == g], y[ids == g], g)
    # a group's record does not depend on the other groups
    keep = np.nonzero(ids != 2)[0]
    ids3 = np.where(ids[keep] == 3, 2, ids[keep])
    alone = grouped([x[keep]], [y[keep]], ids3, 3)
    first = _C.group_pair_moments([dev(x)], [dev(y)], perm, offsets).cpu().numpy()
    assert alone[1].tobytes() == first[1].tobytes() and alone[2].tobytes() == first[3].tobytes()


def test_grouped_no_rows_and_empty_segments():
    e = torch.empty(0, dtype=torch.float64, device=DEV)
    perm = torch.empty(0, dtype=torch.int64, device=DEV)
    rec = _C.group_pair_moments([e], [e.to(torch.int32)], perm, torch.zeros(3, dtype=torch.int64, device=DEV))
    assert rec.is_cuda and tuple(rec.shape) == (2, 1, 7) and not rec.cpu().numpy().any()
    ids = np.array([0, 0, 3, 3, 3], dtype=np.int64)                     # segments 1 and 2 hold no rows
    x, y = pair_data(np.float64, np.float64, 5, seed=26)
    rec = grouped([x], [y], ids, 4)
    for g in range(4):
        check_record(rec[g, 0], x[ids == g], y[ids == g], g)


# ------------------------------------------------------------------ merge_pair_records / pair_results
def _record(n, mx, my, m2x, m2y, c, bad=0):
    r = np.zeros(7, dtype=np.int64)
    r[:6] = np.array([n, mx, my, m2x, m2y, c], dtype=np.float64).view(np.int64)
    r[6] = bad
    return r


def test_merge_pair_records_against_the_host_merge():
    x, y = pair_data(np.float64, np.float32, 3000, seed=31)
    ids = np.random.default_rng(32).integers(0, 6, 3000).astype(np.int64)
    parts = [grouped([x[a:b], y[a:b]], [y[a:b], y[a:b]], ids[a:b], 6)
             for a, b in ((0, 1000), (1000, 1700), (1700, 3000))]
    empty = np.zeros((6, 2, 7), dtype=np.int64)
    # group g: its three partition records in order, empty records in the mix (first, between, last)
    stacked = np.stack([empty, parts[0], empty, parts[1], parts[2], empty], 1).reshape(36, 2, 7)
    offsets = np.arange(0, 37, 6).astype(np.int64)
    got = _C.merge_pair_records(dev(stacked), dev(offsets))
    assert got.is_cuda and tuple(got.shape) == (6, 2, 7)
    got = got.cpu().numpy()
    host = GA._merge_pair_records(stacked, offsets)
    for g in range(6):
        check_record(got[g, 0], x[ids == g], y[ids == g], g)
        check_record(got[g, 1], y[ids == g], y[ids == g], g)
        check_record(host[g, 0], x[ids == g], y[ids == g], g)
    assert got[..., 0].tobytes() == host[..., 0].tobytes() and got[..., 6].tobytes() == host[..., 6].tobytes()
    # identical inputs: every delta is zero, the merge is one rounding, and the two agree bit for bit
    same = np.stack([empty, parts[0], parts[0], empty, parts[0], parts[0]], 1).reshape(36, 2, 7)
    got = _C.merge_pair_records(dev(same), dev(offsets)).cpu().numpy()
    assert got.tobytes() == GA._merge_pair_records(same, offsets).tobytes()
    f = got[..., :6].view(np.float64)
    assert (f[..., 0] == 4 * parts[0][..., 0].view(np.float64)).all()
    # one record among empty ones comes through bit for bit; a group without records is the empty record
    lone = np.concatenate([empty[:1], parts[1][:1], empty[:1]])
    got = _C.merge_pair_records(dev(lone), dev(np.array([0, 3, 3, 3], dtype=np.int64))).cpu().numpy()
    assert got[0].tobytes() == parts[1][0].tobytes() and not got[1:].any()
    assert got.tobytes() == GA._merge_pair_records(lone, np.array([0, 3], dtype=np.int64)).tobytes() + bytes(2 * 2 * 56)
    # the non-finite counts add
    a, b = parts[0][:1].copy(), parts[1][:1].copy()
    a[0, 0, 6], b[0, 0, 6], b[0, 1, 6] = 2, 5, 1
    got = _C.merge_pair_records(dev(np.concatenate([a, b])), dev(np.array([0, 2], dtype=np.int64))).cpu().numpy()
    assert got[0, :, 6].tolist() == [7, 1]


def test_pair_results_against_the_host_results():
    x, y = pair_data(np.float64, np.float32, 2000, seed=33)
    ids = np.random.default_rng(34).integers(0, 5, 2000).astype(np.int64)
    real = grouped([x, y], [y, y], ids, 5)
    nan = math.nan
    made = np.stack([
        _record(0, 0, 0, 0, 0, 0),                                      # no rows
        _record(1, 3.0, 4.0, 0.0, 0.0, 0.0),                            # one row
        _record(2, 2.0, 5.0, 2.0, 8.0, -4.0),                           # rows (1, 7), (3, 3): corr -1
        _record(3, 1.0, 2.0, 0.0, 6.0, 0.0),                            # x constant
        _record(3, 1.0, 2.0, 6.0, 0.0, 0.0),                            # y constant
        _record(4, 1.0, 2.0, 4.0, 9.0, 6.000000000000001),              # not clamped
        _record(4, 1.0, 2.0, 4.0, 9.0, 3.0, bad=1),                     # a non-finite row
        _record(5, nan, 2.0, nan, 9.0, nan, bad=2),
    ])
    made = np.stack([made, made[::-1]], 1)                              # two pairs per group
    for recs in (real, made):
        pairs, stats = [0, 0, 0, 1, 1, 1], PAIR_STATS * 2
        outs = _C.pair_results(dev(recs), pairs, stats)
        host = GA._pair_results(recs, pairs, stats)
        for o, h in zip(outs, host):
            assert o.is_cuda and o.dtype == torch.float64 and tuple(o.shape) == (recs.shape[0],)
            assert o.cpu().numpy().tobytes() == h.tobytes(), (o, h)
    corr, samp, pop = (o.cpu().numpy() for o in _C.pair_results(dev(made), [0, 0, 0], PAIR_STATS))
    np.testing.assert_array_equal(corr, [nan, nan, -1.0, nan, nan, 6.000000000000001 / 6.0, nan, nan])
    assert corr[5] > 1.0
    np.testing.assert_array_equal(samp, [nan, nan, -4.0, 0.0, 0.0, 6.000000000000001 / 3.0, nan, nan])
    np.testing.assert_array_equal(pop, [nan, 0.0, -2.0, 0.0, 0.0, 6.000000000000001 / 4.0, nan, nan])
    for g in range(5):
        for o, st in zip(_C.pair_results(dev(real), [0, 0, 0], PAIR_STATS), PAIR_STATS):
            check_value(o.cpu().numpy()[g], st, x[ids == g], y[ids == g], (g, st))
    none = _C.pair_results(dev(real[:0]), [0], ["corr"])
    assert tuple(none[0].shape) == (0,)


# ------------------------------------------------------------------ frames
def _frame_columns(seed=0):
    c = _chunk()
    sizes = [1, 2, 65, c + 1, 3 * c + 7, 300]
    k = np.array([-3, 0, 4, 9, 11, 2 ** 31 - 1], dtype=np.int32)[ids_of(sizes, seed=seed)]
    n = len(k)
    x, y = pair_data(np.float32, np.float64, n, seed=seed + 1)
    rng = np.random.default_rng(seed + 2)
    z = rng.standard_normal(n)
    z[np.nonzero(k == 9)[0][::40]] = np.nan                             # one group with NaNs
    return {"k": k, "x": x, "y": y, "z": z, "i": cast(rng.standard_normal(n), np.int32),
            "u": cast(0.5 * (x - 1e4) + rng.standard_normal(n), np.uint8)}


def _exprs():
    return [F.corr("x", "y"), F.covar_samp("x", "y"), F.covar_pop("y", "x"), F.avg("x"), F.corr("x", "z"),
            F.corr("u", "x"), F.count("*"), F.covar_samp("i", "u"), F.stddev("y")]


PAIRS = {"corr(x, y)": ("corr", "x", "y"), "covar_samp(x, y)": ("covar_samp", "x", "y"),
         "covar_pop(y, x)": ("covar_pop", "y", "x"), "corr(x, z)": ("corr", "x", "z"), "corr(u, x)": ("corr", "u", "x"),
         "covar_samp(i, u)": ("covar_samp", "i", "u")}
METRICS = ("pair_agg_device_partitions", "pair_agg_host_partitions", "pair_agg_rows", "group_agg_device_partitions",
           "group_agg_host_partitions")


def _delta(fn):
    before = tfs.metrics.snapshot()
    res = fn()
    after = tfs.metrics.snapshot()
    return res, {k: after.get(k, 0) - before.get(k, 0) for k in METRICS}


def _keyed(out):
    res = {}
    for b in out.local_blocks().values():
        cols = {n: b.columns[n].cpu().numpy() for n in out.columns}
        for r in range(b.nrows):
            res[cols["k"][r].item()] = {n: cols[n][r] for n in out.columns if n != "k"}
    return res


def _check_keyed(rows, cols):
    k = cols["k"]
    assert set(rows) == set(np.unique(k).tolist())
    for g, vals in rows.items():
        at = k == g
        for name, (fn, a, b) in PAIRS.items():
            check_value(vals[name], fn, cols[a][at], cols[b][at], (g, name))
        assert int(vals["count(1)"]) == int(at.sum())
        assert math.isnan(vals["corr(x, z)"]) == (g == 9 or at.sum() == 1)


@pytest.mark.parametrize("nparts", [1, 4, 7])
def test_device_resident_frames(nparts):
    cols = _frame_columns()
    n = len(cols["k"])
    host = tfs.from_columns(cols, num_partitions=nparts)
    on_dev = host.cache_on_device(DEV)
    (out, blocks), d = _delta(lambda: (lambda o: (o, o.local_blocks()))(on_dev.groupBy("k").agg(*_exprs())))
    assert d == {"pair_agg_device_partitions": nparts, "pair_agg_host_partitions": 0, "pair_agg_rows": 5 * n,
                 "group_agg_device_partitions": nparts, "group_agg_host_partitions": 0}
    assert all(c.is_cuda for b in blocks.values() for c in b.columns.values())       # the result stays on the device
    assert out.columns == ["k"] + [e.output_name for e in _exprs()]
    _check_keyed(_keyed(out), cols)
    # the one-column results are those of a call without pair expressions
    alone = _keyed(on_dev.groupBy("k").agg(F.avg("x"), F.count("*"), F.stddev("y")))
    for g, vals in _keyed(out).items():
        for c in ("avg(x)", "count(1)", "stddev_samp(y)"):
            assert vals[c].tobytes() == alone[g][c].tobytes()
    # pair expressions alone: no one-column pass at all
    (only, _), d = _delta(lambda: (lambda o: (o, o.local_blocks()))(on_dev.groupBy("k").agg(F.corr("x", "y"))))
    assert d["group_agg_device_partitions"] == 0 and d["pair_agg_device_partitions"] == nparts
    for g, vals in _keyed(only).items():
        assert vals["corr(x, y)"].tobytes() == _keyed(out)[g]["corr(x, y)"].tobytes()
    # no keys: the dense kernel per partition, one row on the host, the same on every rank
    whole, d = _delta(lambda: on_dev.agg(*_exprs()))
    assert d == {"pair_agg_device_partitions": nparts, "pair_agg_host_partitions": 0, "pair_agg_rows": 5 * n,
                 "group_agg_device_partitions": nparts, "group_agg_host_partitions": 0}
    for name, (fn, a, b) in PAIRS.items():
        check_value(whole.to_numpy(name)[0], fn, cols[a], cols[b], name)
    assert math.isnan(whole.to_numpy("corr(x, z)")[0])
    got, d = _delta(lambda: (on_dev.corr("x", "y"), on_dev.stat.cov("x", "y")))
    assert d["pair_agg_device_partitions"] == 2 * nparts and d["pair_agg_rows"] == 2 * n
    assert np.array(got).tobytes() == np.array([whole.to_numpy("corr(x, y)")[0],
                                                whole.to_numpy("covar_samp(x, y)")[0]]).tobytes()
    # the host path of the same frame agrees within the bounds (both are held to exact above)
    ref, d = _delta(lambda: host.agg(*_exprs()))
    assert d["pair_agg_host_partitions"] == nparts and d["pair_agg_device_partitions"] == 0
    assert abs(float(ref.to_numpy("corr(x, y)")[0]) - got[0]) <= 2 * CORR_BOUND


def test_a_frame_with_one_host_partition_takes_the_host_path():
    from tensorframes_amd.frame.block import Block
    from tensorframes_amd.frame.dataframe import DataFrame, _Materialized
    cols = _frame_columns(seed=3)
    on_dev = tfs.from_columns(cols, num_partitions=4).cache_on_device(DEV)
    blocks = {p: (Block(b.nrows, {n: c.cpu() for n, c in b.columns.items()}) if p == 2 else b)
              for p, b in on_dev.local_blocks().items()}
    mixed = DataFrame(on_dev.schema, _Materialized(blocks), 4)
    out, d = _delta(lambda: _keyed(mixed.groupBy("k").agg(*_exprs())))
    assert d["pair_agg_host_partitions"] == 4 and d["pair_agg_device_partitions"] == 0
    assert d["group_agg_host_partitions"] == 4 and d["group_agg_device_partitions"] == 0
    _check_keyed(out, cols)
    host = _keyed(tfs.from_columns(cols, num_partitions=4).groupBy("k").agg(*_exprs()))
    for g in out:
        for name in out[g]:
            assert out[g][name].tobytes() == host[g][name].tobytes()
    # without keys each partition is read where it lives
    whole, d = _delta(lambda: mixed.agg(F.corr("x", "y")))
    assert d["pair_agg_host_partitions"] == 1 and d["pair_agg_device_partitions"] == 3
    check_value(whole.to_numpy("corr(x, y)")[0], "corr", cols["x"], cols["y"])


# ------------------------------------------------------------------ two ranks, one GPU
def _results(df):
    out = df.groupBy("k").agg(*_exprs())
    rows = {str(g): {n: v.tobytes().hex() for n, v in vals.items()} for g, vals in _keyed(out).items()}
    whole = df.agg(*_exprs())
    return {"rows": rows, "whole": {c: whole.to_numpy(c).tobytes().hex() for c in whole.columns},
            "scalars": [np.float64(df.corr("x", "y")).tobytes().hex(), np.float64(df.cov("i", "u")).tobytes().hex()],
            "on_device": all(c.is_cuda for b in out.local_blocks().values() for c in b.columns.values())}


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
    df = tfs.from_columns(_frame_columns(seed=4), num_partitions=5).cache_on_device()
    res = _results(df)
    res["device"] = engine.compute_device().type
    with open(os.path.join(outdir, f"r{rank}.json"), "w") as f:
        json.dump(res, f)
    dist.shutdown()


def test_pair_agg_two_ranks_share_one_gpu(tmp_path):
    ctx = mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=False)
    deadline = time.monotonic() + 120
    while not ctx.join(timeout=1):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("the ranks did not finish in 120 s")
    outs = [json.load(open(tmp_path / f"r{r}.json")) for r in range(2)]
    single = _results(tfs.from_columns(_frame_columns(seed=4), num_partitions=5).cache_on_device(DEV))
    assert single["on_device"]
    rows = {}
    for o in outs:
        assert o["device"] == "cuda" and o["on_device"]
        assert not set(o["rows"]) & set(rows)                           # a key lives on one rank
        rows.update(o["rows"])
        assert o["whole"] == single["whole"] and o["scalars"] == single["scalars"]
    assert rows == single["rows"] and len(rows) == 6
