"""The device kernels under `Window` / `.over()` (csrc/kernels/window_scan.hip:
window_scan, window_finish) and the frame paths that use them, on the GPU.

Kernel level: expected values are brute force written here. Heads come from a
plain loop over the ordering words (`spec_words`, copied from
tests/test_gpu_group_agg.py), integer sums are Python ints masked to 64 bits,
float sums are `fractions.Fraction` sums rounded once. Head indexes, peer
counts, integer sums and extreme words are exact.

Float sums of the positive 1e4 + N(0, 1) data are held to terms * 2^-53 * 10
relative. The terms follow the kernel, which differs from the issue's sketch
in that a value passes the lane / wave / block combine twice (once in the
tile-aggregate launch, once in the write launch) and the second launch scans
the tile aggregates 64 at a step with a wave scan instead of one by one:
  rows per lane, twice (the lane's aggregate, then its rescan)       2 * 8
  wave shuffle steps, twice                                          2 * 6
  earlier waves of the block, twice                                  2 * 3
  the wave scan over 64 tile aggregates                              6
  the steps of 64 tiles in sequence                                  ceil(tiles / 64)
  the tile's prefix and the lane's carry                             2
  the partitions folded, the carry applied in the finish             nparts + 1
  avg's division                                                     1
The frame-level tests compare the device path with the host path, whose terms
are the rows of a value + the partitions (tests/test_window.py): the bound is
the sum of the two.
No test hands a kernel an index out of range or lengths that do not agree."""
import json
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
from tensorframes_amd import Window, functions as F
from tensorframes_amd._native import _C

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.uint8, np.int8, np.int16, np.int32, np.int64, np.float32, np.float64]
MASK = (1 << 64) - 1
UP, UF, CR = Window.unboundedPreceding, Window.unboundedFollowing, Window.currentRow
ROWS_PER_LANE = 8


def T():
    return int(_C.window_tile_rows())


def kernel_terms(n, nparts=1):
    tiles = -(-n // T())
    return 2 * ROWS_PER_LANE + 2 * 6 + 2 * 3 + 6 + -(-tiles // 64) + 2 + nparts + 1 + 1


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


def dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def words_of(group_lengths, peer_lengths=None):
    """uint64 [2, n]: word 0 changes at every group, word 1 at every peer run
    (peer_lengths: run lengths over all rows; default one run per row)."""
    n = int(sum(group_lengths))
    g = np.repeat(np.arange(len(group_lengths), dtype=np.uint64) * np.uint64(3) + np.uint64(5), group_lengths)
    if peer_lengths is None:
        p = np.arange(n, dtype=np.uint64)
    else:
        assert sum(peer_lengths) == n
        p = np.repeat(np.arange(len(peer_lengths), dtype=np.uint64), peer_lengths)
    return np.stack([g, p], 0)


def heads(words, P, reverse):
    """(group head, peer head) flags by a plain loop over the (mirrored) rows."""
    W, n = words.shape
    seq = words[:, ::-1] if reverse else words
    gh, ph = [False] * n, [False] * n
    for m in range(n):
        if m == 0:
            gh[m] = ph[m] = True
            continue
        ph[m] = any(int(seq[w, m]) != int(seq[w, m - 1]) for w in range(W))
        gh[m] = any(int(seq[w, m]) != int(seq[w, m - 1]) for w in range(P))
    return gh, ph


def brute_scan(words, P, reverse, kinds, cols):
    """Expected [C][n] as Python values, in original row positions: ints
    (indexes, counts, integer sums as signed 64-bit, words) or floats."""
    W, n = words.shape
    gh, ph = heads(words, P, reverse)
    out, used = [], 0
    for kind in kinds:
        x = xw = None
        if kind in ("sum_i64", "sum_f64", "min_word", "max_word"):
            x = cols[used][::-1] if reverse else cols[used]
            xw = [int(w) for w in spec_words(x)]
            used += 1
        res, acc, cur_g, cur_p, cnt, ext = [None] * n, None, 0, 0, 0, None
        for m in range(n):
            if gh[m]:
                cur_g, cnt = m, 0
            if ph[m]:
                cur_p, cnt = m, cnt + 1
            if kind == "group_head":
                v = n - 1 - cur_g if reverse else cur_g
            elif kind == "peer_head":
                v = n - 1 - cur_p if reverse else cur_p
            elif kind == "peer_count":
                v = cnt
            elif kind == "sum_i64":
                acc = (int(x[m]) if gh[m] else acc + int(x[m])) & MASK
                v = acc - (1 << 64) if acc >> 63 else acc
            elif kind == "sum_f64":
                acc = Fraction(float(x[m])) if gh[m] else acc + Fraction(float(x[m]))
                v = float(acc)
            else:
                ext = xw[m] if gh[m] else (min(ext, xw[m]) if kind == "min_word" else max(ext, xw[m]))
                v = ext
            res[n - 1 - m if reverse else m] = v
        out.append(res)
    return out


def check_scan(words, P, reverse, kinds, cols, terms=None):
    n = words.shape[1]
    got = _C.window_scan(dev(words.view(np.int64)), P, reverse, kinds, [dev(c) for c in cols]).cpu().numpy()
    assert got.shape == (len(kinds), n) and got.dtype == np.int64
    want = brute_scan(words, P, reverse, kinds, cols)
    for c, kind in enumerate(kinds):
        if kind == "sum_f64":
            g = got[c].view(np.float64)
            bound = (terms or kernel_terms(n)) * 2.0 ** -53 * 10
            for i in range(n):
                assert abs(g[i] - want[c][i]) <= bound * abs(want[c][i]), (kind, i, g[i], want[c][i], bound)
        elif kind in ("min_word", "max_word"):
            assert got[c].view(np.uint64).tolist() == want[c], kind
        else:
            assert got[c].tolist() == want[c], kind
    return got


def values(dtype, n, seed=0, wide=False):
    """Floats: 1e4 + N(0, 1). Integers: the whole range of the type; int64
    only with `wide` (its wrapping sums), else below 2^38, so that the f64 sum
    of any column of integers here is exact whatever the order."""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return (1e4 + rng.standard_normal(n)).astype(dt)
    ii = np.iinfo(dt)
    if dt.itemsize == 8 and not wide:
        return rng.integers(0, 1 << 38, n, dtype=dt)
    return rng.integers(ii.min, ii.max, n, dtype=dt, endpoint=True)


INDEX = ["group_head", "peer_head", "peer_count"]
VALUE = ["sum_i64", "sum_f64", "min_word", "max_word"]


def value_cols(n, seed=0):
    return [values(np.int64, n, seed, wide=True), values(np.float32, n, seed + 1), values(np.float64, n, seed + 2),
            values(np.int32, n, seed + 3)]


# ------------------------------------------------------------------ window_scan
def test_tile_rows_exported():
    assert T() >= 64 and T() % 64 == 0 and T() // 256 == ROWS_PER_LANE


def _sizes():
    t = T()
    return [1, 2, 63, 64, 65, t - 1, t, t + 1, 2 * t + 7, 5 * t + 3]


@pytest.mark.parametrize("reverse", [False, True])
def test_every_size_with_mixed_groups(reverse):
    for n in _sizes():
        rng = np.random.default_rng(n)
        lens, left = [], n
        while left:
            k = int(min(left, rng.integers(1, 40)))
            lens.append(k)
            left -= k
        peers, left = [], n
        while left:
            k = int(min(left, rng.integers(1, 4)))
            peers.append(k)
            left -= k
        check_scan(words_of(lens, peers), 1, reverse, INDEX + VALUE, value_cols(n, n))


@pytest.mark.parametrize("reverse", [False, True])
def test_every_row_its_own_group(reverse):
    n = 2 * T() + 7
    check_scan(words_of([1] * n), 1, reverse, INDEX + VALUE, value_cols(n))


@pytest.mark.parametrize("reverse", [False, True])
def test_one_group_holds_every_row_so_the_carry_crosses_every_tile(reverse):
    n = 5 * T() + 3
    check_scan(words_of([n]), 1, reverse, INDEX + VALUE, value_cols(n))


@pytest.mark.parametrize("reverse", [False, True])
def test_groups_at_tile_edges(reverse):
    t = T()
    # a group starting on a tile's last row, one ending on a tile's first row,
    # one covering exactly one whole tile between two others
    for lens in ([t - 1, 5, t], [t + 1, t - 1, 9], [t - 3, 3, t, 11], [3, t - 3, t, t, 2]):
        n = sum(lens)
        check_scan(words_of(lens), 1, reverse, INDEX + VALUE, value_cols(n, n))


@pytest.mark.parametrize("reverse", [False, True])
def test_peer_runs_of_lengths_1_2_64_and_a_tile_plus_one(reverse):
    t = T()
    peers = [1, 2, 64, t + 1, 1, 2, 64, 5]
    n = sum(peers)
    check_scan(words_of([67, n - 67], peers), 1, reverse, INDEX + VALUE[:1], [values(np.int64, n)])
    check_scan(words_of([n], peers), 1, reverse, INDEX, [])


@pytest.mark.parametrize("reverse", [False, True])
def test_no_partition_words_is_one_group(reverse):
    n = T() + 65
    w = words_of([7] * (n // 7) + [n % 7] if n % 7 else [7] * (n // 7), [3] * (n // 3) + ([n % 3] if n % 3 else []))
    got = check_scan(w, 0, reverse, INDEX + VALUE, value_cols(n))
    assert set(got[0].tolist()) == {n - 1 if reverse else 0}
    none = np.zeros((0, n), dtype=np.uint64)                       # no words at all: one group, one peer run
    got = check_scan(none, 0, reverse, INDEX, [])
    assert set(got[1].tolist()) == {n - 1 if reverse else 0} and set(got[2].tolist()) == {1}


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_value_dtype(dtype):
    n = T() + 131
    x = values(dtype, n, 3)
    lens = [100, T() - 50, 81]
    kinds = ["sum_i64" if np.dtype(dtype).kind != "f" else "sum_f64", "sum_f64", "min_word", "max_word"]
    check_scan(words_of(lens), 1, False, INDEX[:1] + kinds, [x] * 4)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_column_one_element_into_its_buffer(dtype):
    n = T() + 9
    buf = dev(values(dtype, n + 1, 4))
    col = buf[1:]
    assert col.is_contiguous() and col.data_ptr() == buf.data_ptr() + buf.element_size()
    words = words_of([n // 2, n - n // 2])
    kinds = ["group_head", "sum_f64", "max_word"]
    got = _C.window_scan(dev(words.view(np.int64)), 1, False, kinds, [col, col]).cpu().numpy()
    want = brute_scan(words, 1, False, kinds, [col.cpu().numpy()] * 2)
    assert got[0].tolist() == want[0] and got[2].view(np.uint64).tolist() == want[2]
    if np.dtype(dtype).kind == "f":
        g, bound = got[1].view(np.float64), kernel_terms(n) * 2.0 ** -53 * 10
        assert all(abs(a - b) <= bound * abs(b) for a, b in zip(g.tolist(), want[1]))
    else:
        assert got[1].view(np.float64).tolist() == want[1]          # (sums of integers below 2^53: exact)


def test_sixteen_channels_in_one_call():
    n = T() + 77
    kinds = INDEX + ["sum_i64", "sum_f64", "min_word", "max_word"] * 3 + ["sum_i64"]
    cols = [values(DTYPES[j % 7] if kinds[3 + j] != "sum_f64" else np.float64, n, j, wide=True) for j in range(13)]
    assert len(kinds) == 16
    check_scan(words_of([40, T(), 37], None), 1, False, kinds, cols)


def test_no_rows_launches_nothing():
    w = torch.empty((2, 0), dtype=torch.int64, device=DEV)
    out = _C.window_scan(w, 1, False, INDEX + ["sum_i64"], [torch.empty(0, dtype=torch.int32, device=DEV)])
    assert tuple(out.shape) == (4, 0) and out.dtype == torch.int64
    outs = _C.window_finish(out[:3].contiguous(), out[:2].contiguous(), INDEX, [0] * 3, [0] * 3, False, False, 0, 0,
                            ["row_number", "count"], ["rows", "whole"], [0, 0], [torch.uint8] * 2)
    assert [tuple(o.shape) for o in outs] == [(0,), (0,)] and [o.dtype for o in outs] == [torch.int32, torch.int64]


def test_two_runs_give_equal_bytes():
    n = 5 * T() + 3
    words = dev(words_of([n // 3, n - n // 3]).view(np.int64))
    cols = [dev(c) for c in value_cols(n)]
    a = _C.window_scan(words, 1, False, INDEX + VALUE, cols).cpu().numpy().tobytes()
    b = _C.window_scan(words, 1, False, INDEX + VALUE, cols).cpu().numpy().tobytes()
    assert a == b


def test_bindings_refuse_what_does_not_fit():
    n = 100
    words = dev(words_of([n]).view(np.int64))
    x = dev(values(np.float32, n))
    with pytest.raises(ValueError, match="device"):
        _C.window_scan(words.cpu(), 1, False, INDEX, [])
    with pytest.raises(TypeError, match="int64"):
        _C.window_scan(words.to(torch.int32), 1, False, INDEX, [])
    with pytest.raises(ValueError, match="contiguous"):
        _C.window_scan(words[:, ::2], 1, False, INDEX, [])
    with pytest.raises(ValueError, match="P"):
        _C.window_scan(words, 3, False, INDEX, [])
    with pytest.raises(ValueError, match="kind"):
        _C.window_scan(words, 1, False, ["nope"], [])
    with pytest.raises(ValueError, match="device"):
        _C.window_scan(words, 1, False, ["sum_f64"], [x.cpu()])
    with pytest.raises(TypeError, match="not supported"):
        _C.window_scan(words, 1, False, ["sum_f64"], [x.to(torch.float16)])
    with pytest.raises(ValueError, match="contiguous"):
        _C.window_scan(words, 1, False, ["sum_f64"], [dev(values(np.float32, 2 * n))[::2]])
    with pytest.raises(ValueError, match="rows"):
        _C.window_scan(words, 1, False, ["sum_f64"], [x[:50].contiguous()])
    with pytest.raises(ValueError, match="value column"):
        _C.window_scan(words, 1, False, ["sum_f64", "min_word"], [x])
    with pytest.raises(ValueError, match="channels"):
        _C.window_scan(words, 1, False, INDEX * 6, [])
    fwd = _C.window_scan(words, 1, False, INDEX, [])
    rev = _C.window_scan(words, 1, True, INDEX[:2], [])
    ok = dict(kinds=INDEX, carry=[0] * 3, total=[0] * 3, has_carry=False, has_total=False, carry_rows=0,
              total_rows=0, fns=["dense_rank"], frames=["rows"], chans=[2], dtypes=[torch.uint8])
    assert _C.window_finish(fwd, rev, **ok)[0].dtype == torch.int32
    with pytest.raises(ValueError, match="device"):
        _C.window_finish(fwd.cpu(), rev, **ok)
    with pytest.raises(TypeError, match="int64"):
        _C.window_finish(fwd, rev.to(torch.int32), **ok)
    with pytest.raises(ValueError, match="reverse scan"):
        _C.window_finish(fwd, rev[:, :50].contiguous(), **ok)
    with pytest.raises(ValueError, match="contiguous"):
        _C.window_finish(fwd, _C.window_scan(words, 1, True, INDEX[:2] * 2, [])[::2], **ok)
    with pytest.raises(ValueError, match="channel"):
        _C.window_finish(fwd, rev, **dict(ok, chans=[3]))
    with pytest.raises(ValueError, match="cannot read"):
        _C.window_finish(fwd, rev, **dict(ok, fns=["sum"]))
    with pytest.raises(ValueError, match="not a window function"):
        _C.window_finish(fwd, rev, **dict(ok, fns=["median"]))
    with pytest.raises(ValueError, match="not a frame"):
        _C.window_finish(fwd, rev, **dict(ok, frames=["sliding"]))
    with pytest.raises(ValueError, match="group_head"):
        _C.window_finish(fwd, rev, **dict(ok, kinds=INDEX[::-1]))
    with pytest.raises(TypeError, match="not supported"):
        _C.window_finish(fwd, rev, **dict(ok, dtypes=[torch.float16]))


# ------------------------------------------------------------------ window_finish
@pytest.mark.parametrize("dtype", DTYPES)
def test_finish_gathers_per_frame_applies_the_carry_and_decodes(dtype):
    t = T()
    lens = [70, t, 45]
    n = sum(lens)
    peers = [1, 2, 64, 3] + [5] * ((n - 70) // 5) + ([(n - 70) % 5] if (n - 70) % 5 else [])
    assert sum(peers) == n
    words = words_of(lens, peers)
    x = values(dtype, n, 5)
    fl = np.dtype(dtype).kind == "f"
    kinds = INDEX + ["sum_f64" if fl else "sum_i64", "sum_f64", "min_word", "max_word"]
    cols = [x] * 4
    dw = dev(words.view(np.int64))
    fwd = _C.window_scan(dw, 1, False, kinds, [dev(c) for c in cols])
    rev = _C.window_scan(dw, 1, True, kinds[:2], [])
    f, r = fwd.cpu().numpy(), rev.cpu().numpy()
    carry = [0, 0, 4, 1000 if not fl else int(np.float64(1000.0).view(np.int64)), int(np.float64(1000.0).view(np.int64)),
             int(spec_words(np.array([x.min()], dtype=x.dtype))[0]) + 0, int(spec_words(np.array([x[:70].max()]))[0])]
    total = [0, 0, 99, 7 if not fl else int(np.float64(7.0).view(np.int64)), int(np.float64(7.0).view(np.int64)),
             int(spec_words(np.array([x.min()], dtype=x.dtype))[0]), int(spec_words(np.array([x.max()], dtype=x.dtype))[0])]
    sg = lambda u: u - (1 << 64) if u >= (1 << 63) else u  # noqa: E731
    fns = ["row_number", "rank", "dense_rank"] + [fn for fn in ("count", "sum", "avg", "min", "max") for _ in range(3)]
    frames = ["rows"] * 3 + ["rows", "range", "whole"] * 5
    chan = {"row_number": 0, "rank": 0, "dense_rank": 2, "count": 0, "sum": 3, "avg": 4, "min": 5, "max": 6}
    chans = [chan[fn] for fn in fns]
    tdt = torch.from_numpy(x[:1]).dtype
    outs = []
    for a in range(0, len(fns), 16):
        outs += _C.window_finish(fwd, rev, kinds, [sg(c) for c in carry], [sg(c) for c in total], True, True, 10, 5000,
                                 fns[a:a + 16], frames[a:a + 16], chans[a:a + 16], [tdt] * len(fns[a:a + 16]))
    gh, ph, gl, pl = f[0], f[1], r[0], r[1]
    idx = np.arange(n)
    first, last = gh == 0, gl == n - 1
    for fn, fr, c, o in zip(fns, frames, chans, outs):
        got = o.cpu().numpy()
        tt = idx if fr == "rows" else (pl if fr == "range" else gl)
        whole = last & (fr == "whole")
        rows = np.where(whole, 5000, tt - gh + 1 + np.where(first, 10, 0))
        if fn == "row_number":
            want = idx - gh + 1 + np.where(first, 10, 0)
        elif fn == "rank":
            want = ph - gh + 1 + np.where(first, 10, 0)
        elif fn == "count":
            want = rows
        else:
            v = f[c][tt]
            if fn == "dense_rank":
                want = np.where(first, v + 4, v)
            elif fn == "sum" and not fl:
                want = np.where(whole, 7, np.where(first, v + 1000, v))
            elif fn in ("sum", "avg"):
                s = np.where(whole, 7.0, np.where(first, 1000.0 + v.view(np.float64), v.view(np.float64)))
                want = s if fn == "sum" else s / rows
            else:
                u = v.view(np.uint64)
                cw, tw = np.uint64(carry[c]), np.uint64(total[c])
                u = np.where(first, np.minimum(u, cw) if fn == "min" else np.maximum(u, cw), u)
                u = np.where(whole, tw, u)
                srt = np.sort(x)
                table = {int(w): val for w, val in zip(spec_words(srt).tolist(), srt)}
                want = np.array([table[int(w)] for w in u], dtype=x.dtype)
                want = want + x.dtype.type(0) if fl else want
        assert got.tobytes() == np.asarray(want).astype(got.dtype).tobytes(), (fn, fr)
    assert [o.dtype for o in outs[:4]] == [torch.int32] * 3 + [torch.int64]


# ------------------------------------------------------------------ frames
def frame_columns(n, seed, heavy=False):
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, 9, n).astype(np.int32)
    if heavy:
        ids = np.where(rng.random(n) < 0.6, 4, ids).astype(np.int32)
    return {
        "id": ids,
        "t": rng.integers(0, n // 3, n).astype(np.int32),
        "score": (1e4 + rng.standard_normal(n)).astype(np.float32),
        "x": 1e4 + rng.standard_normal(n),
        "q": rng.integers(-(1 << 62), 1 << 62, n).astype(np.int64),
        "i": np.arange(n, dtype=np.int64),
    }


EXACT = ["id", "t", "i", "rn", "r", "d", "c", "si", "sw", "lo", "hi"]
FLOAT = ["fs", "fr", "fw", "av"]


def all_items():
    w = Window.partitionBy("id").orderBy("t")
    rows, rng_, whole = w.rowsBetween(UP, CR), w.rangeBetween(UP, CR), w.rowsBetween(UP, UF)
    return [F.row_number().over(w).alias("rn"), F.rank().over(w).alias("r"), F.dense_rank().over(w).alias("d"),
            F.count("*").over(rng_).alias("c"), F.sum("q").over(rows).alias("si"), F.sum("q").over(whole).alias("sw"),
            F.min("x").over(rng_).alias("lo"), F.max("score").over(whole).alias("hi"),
            F.sum("x").over(rows).alias("fs"), F.sum("score").over(rng_).alias("fr"),
            F.sum("x").over(whole).alias("fw"), F.avg("score").over(rows).alias("av")]


def uneven(cols, nparts, empty, one_row):
    n = len(cols["i"])
    edges = [(p * n) // nparts for p in range(nparts + 1)]
    keep = np.ones(n, dtype=bool)
    keep[edges[empty]:edges[empty + 1]] = False
    keep[edges[one_row] + 1:edges[one_row + 1]] = False
    df = tfs.from_columns(dict(cols, keep=keep.astype(np.int32)), num_partitions=nparts)
    return df.filter(df.keep > 0).select(*cols)


def compare_device_with_host(host_df, names, n, nparts):
    host = host_df.select(*names, *all_items())
    device = host_df.cache_on_device(DEV).select(*names, *all_items())
    blocks = device.local_blocks()
    assert all(c.is_cuda for b in blocks.values() if b.nrows for c in b.columns.values())
    for name in EXACT:
        assert device.to_numpy(name).tobytes() == host.to_numpy(name).tobytes(), name
    bound = (kernel_terms(n, nparts) + n + nparts + 1) * 2.0 ** -53 * 10
    for name in FLOAT:
        a, b = device.to_numpy(name), host.to_numpy(name)
        assert a.dtype == np.float64 and (np.abs(a - b) <= bound * np.abs(b)).all(), name
    return device


@pytest.mark.parametrize("nparts", [1, 3, 7])
def test_device_resident_frames_match_the_host_path(nparts):
    n = 3 * T() + 100                                              # (more than one tile in a partition of three)
    cols = frame_columns(n, nparts)
    compare_device_with_host(tfs.from_columns(cols, num_partitions=nparts), list(cols), n, nparts)


def test_a_group_spanning_partitions_and_an_empty_partition():
    n = 2 * T() + 300
    cols = frame_columns(n, 11, heavy=True)
    out = compare_device_with_host(uneven(cols, 7, empty=3, one_row=5), list(cols), n, 7)
    ids = [set(b.columns["id"].tolist()) for _, b in sorted(out.local_blocks().items())]
    assert sum(4 in s for s in ids) >= 3


def test_readme_example_on_a_device_frame():
    cols = frame_columns(500, 12)
    scored = tfs.from_columns(cols, num_partitions=3).cache_on_device(DEV)
    w = Window.partitionBy("id").orderBy(tfs.desc("score"))
    top3 = scored.withColumn("rn", F.row_number().over(w)).filter(tfs.col("rn") <= 3)
    assert top3.count() == 3 * len(set(cols["id"].tolist()))
    both = scored.select("id", "score", F.rank().over(w).alias("r"), F.sum("score").over(w).alias("running"))
    assert both.columns == ["id", "score", "r", "running"] and both.count() == 500
    tot = scored.withColumn("total", F.sum("x").over(Window.partitionBy("id")))
    assert abs(tot.withColumn("share", tot.x / tfs.col("total")).to_numpy("share").sum() - 9.0) < 1e-9
    cum = scored.withColumn("cum", F.sum("x").over(Window.orderBy("t").rowsBetween(UP, CR)))
    assert abs(cum.to_numpy("cum")[-1] - cols["x"].sum()) <= 1e-9 * cols["x"].sum()


# ------------------------------------------------------------------ two ranks, one GPU
def _results(df, names):
    out = df.select(*names, *all_items())
    return {"cols": {c: out.to_numpy(c).tobytes().hex() for c in out.columns},
            "on_device": all(c.is_cuda for b in out.local_blocks().values() if b.nrows for c in b.columns.values())}


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
    cols = frame_columns(T() + 200, 13, heavy=True)
    res = _results(tfs.from_columns(cols, num_partitions=5).cache_on_device(), list(cols))
    res["device"] = engine.compute_device().type
    with open(os.path.join(outdir, f"r{rank}.json"), "w") as f:
        json.dump(res, f)
    dist.shutdown()


def test_window_two_ranks_share_one_gpu(tmp_path):
    ctx = mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=False)
    deadline = time.monotonic() + 120
    while not ctx.join(timeout=1):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("the ranks did not finish in 120 s")
    outs = [json.load(open(tmp_path / f"r{r}.json")) for r in range(2)]
    cols = frame_columns(T() + 200, 13, heavy=True)
    single = _results(tfs.from_columns(cols, num_partitions=5).cache_on_device(DEV), list(cols))
    assert single["on_device"]
    for o in outs:
        assert o["device"] == "cuda" and o["on_device"]
        assert o["cols"] == single["cols"]                          # every output column, byte for byte
