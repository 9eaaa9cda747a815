"""The specification of the order aggregates (median / percentile,
percentile_approx, mode, countDistinct), shared by tests/test_order_agg.py and
tests/test_gpu_order_agg.py: plain Python over the rows.

A group's rows are sorted by their ordering words (`spec_words`, copied from
tests/test_gpu_window.py); ranks are picked by the two rules, the
interpolation is Spark's formula in Python floats (CPython contracts nothing:
two rounded products and one rounded sum), distinct counts are `len(set(...))`
and the mode a `collections.Counter` over words with the smallest word on
ties. Typed results are canonical (the quiet NaN, +0.0), and a NaN
interpolation is the quiet NaN."""
import math
from collections import Counter

import numpy as np


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


def canonical(v, dtype):
    """The value as a typed result holds it: the quiet NaN, +0.0."""
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        if np.isnan(v):
            return np.array([0x7FC00000 if dtype == np.float32 else 0x7FF8000000000000],
                            dtype=np.uint32 if dtype == np.float32 else np.uint64).view(dtype)[0]
        if v == 0:
            return dtype.type(0.0)
    return dtype.type(v)


def quiet(v: float) -> np.float64:
    return np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0] if math.isnan(v) else np.float64(v)


def approx_rank(p: float, n: int) -> int:
    return max(math.ceil(p * n) - 1, 0)


def interpolate(p: float, vals) -> float:
    """Spark's Percentile over the sorted values (floats)."""
    n = len(vals)
    pos = p * (n - 1)
    lo, hi = math.floor(pos), math.ceil(pos)
    v_lo, v_hi = float(vals[lo]), float(vals[hi])
    if lo == hi:
        return quiet(v_lo)
    return quiet((hi - pos) * v_lo + (pos - lo) * v_hi)


def spec(cols, keys, exprs):
    """exprs: [(name, fn, value columns, percentages, is_list)], fn one of
    percentile, percentile_approx, mode, count_distinct.
    -> (key words of the groups in ascending order [(w, ...)], {name: numpy array})"""
    n = len(next(iter(cols.values())))
    kw = [spec_words(cols[k]) for k in keys]
    gkey = [tuple(int(w[i]) for w in kw) for i in range(n)]
    groups = {}
    for i in range(n):
        groups.setdefault(gkey[i], []).append(i)
    order = sorted(groups)
    out = {}
    for name, fn, vcols, ps, is_list in exprs:
        vw = [spec_words(cols[v]) for v in vcols]
        val = cols[vcols[-1]]
        dt = val.dtype
        res = []
        for g in order:
            rows = sorted(groups[g], key=lambda i: tuple(int(w[i]) for w in vw))
            if fn == "count_distinct":
                res.append(len({tuple(int(w[i]) for w in vw) for i in rows}))
                continue
            sv = [canonical(val[i], dt) for i in rows]              # (values come back from their words)
            if fn == "mode":
                cnt = Counter(int(vw[0][i]) for i in rows)
                top = max(cnt.values())
                best = min(w for w, c in cnt.items() if c == top)
                res.append(canonical(next(val[i] for i in rows if int(vw[0][i]) == best), dt))
            elif fn == "percentile_approx":
                got = [sv[approx_rank(p, len(sv))] for p in ps]
                res.append(got if is_list else got[0])
            else:
                got = [interpolate(p, sv) for p in ps]
                res.append(got if is_list else got[0])
        out_dt = np.int64 if fn == "count_distinct" else (np.float64 if fn == "percentile" else dt)
        out[name] = np.array(res, dtype=out_dt)
    return order, out
