"""DataFrame.describe / summary / approxQuantile.

Two passes over the described columns, both collective (every rank calls):

* moments: every local partition yields one record per column -- n, mean, M2
  (the sum of squared deviations from the mean) and the smallest and largest
  order-preserving word (the table of the sort path). Device-resident columns
  go through `_C.column_moments` (kernels/stats.hip: Welford per lane, Chan's
  merge above it), up to 16 per call, one D2H of the records per partition;
  host columns through numpy (two-pass f64). The records travel in one
  [nparts, C, 5] table of bit patterns (one host all-reduce; every rank fills
  the rows of its own partitions) and every rank merges them in partition
  order with Chan's formula: for a given partitioning the result has the same
  bits on every rank and for every world size.
* quantiles: an exact order statistic by most-significant-digit-first radix
  selection over the words. Per column, all requested ranks together: start
  below the leading 8-bit digits on which the column's smallest and largest
  word agree, then per pass one 256-bin histogram per distinct prefix
  (`_C.select_hist` on the device, numpy on the host), one host all-reduce of
  [P, 256] int64, and every target walks the cumulative counts to its digit.
  At most 8 read-only passes, no row moves, and integer histograms add
  exactly: the answer does not depend on ranks or partitions.
"""
from __future__ import annotations

import math
import numbers
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ..parallel import dist
from ._scalar_columns import _SIGN, _decode_sort_word, _flatten, _np_dtype, _scalar_column, _stat_columns
from .block import Block

_MOMENTS_GROUP = 16  # columns per _C.column_moments call (kernels.h kMaxPackCols)
_MAX_PROBABILITIES = 16  # per approxQuantile call: the prefixes one _C.select_hist call takes
_DESCRIBE = ("count", "mean", "stddev", "min", "max")
_SUMMARY = ("count", "mean", "stddev", "min", "25%", "50%", "75%", "max")
_ALL_ONES = (1 << 64) - 1


def _is_float(dt: np.dtype) -> bool:
    return dt.kind == "f"


# ------------------------------------------------------------------ moments
def _bits(x: float) -> int:
    return int(np.float64(x).view(np.int64))


def _from_bits(b: int) -> float:
    return float(np.int64(b).view(np.float64))


def _as_i64(word: int) -> int:
    return word - (1 << 64) if word >= _SIGN else word


def _host_record(c: torch.Tensor) -> List[int]:
    """One partition's record of a host column, as bit patterns."""
    from .dataframe import _host_sort_words
    n = int(c.shape[0])
    if n == 0:
        return [_bits(0.0), _bits(math.nan), _bits(math.nan), -1, 0]
    with np.errstate(all="ignore"):
        x = c.detach().contiguous().numpy().astype(np.float64)
        mean = float(x.sum() / n)
        dev = x - mean
        # (two passes; the second also takes out what rounding left in the mean)
        mean += float(dev.sum() / n)
        dev = x - mean
        m2 = float((dev * dev).sum())
    w = _host_sort_words(c, False)
    return [_bits(float(n)), _bits(mean), _bits(m2), _as_i64(int(w.min())), _as_i64(int(w.max()))]


def _block_records(b: Block, names: Sequence[str], what: str) -> np.ndarray:
    """int64 [C, 5]: the records of one partition's columns, as bit patterns."""
    from .._native import _C
    out = np.zeros((len(names), 5), dtype=np.int64)
    cols = [_scalar_column(b, n, what) for n in names]
    by_dev: Dict[torch.device, List[int]] = {}
    for i, c in enumerate(cols):
        if c.is_cuda:
            by_dev.setdefault(c.device, []).append(i)
        else:
            out[i] = _host_record(c)
    for dev, idx in by_dev.items():
        recs = []
        for g in range(0, len(idx), _MOMENTS_GROUP):
            mo, ex = _C.column_moments([cols[i].contiguous() for i in idx[g:g + _MOMENTS_GROUP]])
            recs.append(torch.cat([mo.view(torch.int64), ex], 1))
        out[idx] = (recs[0] if len(recs) == 1 else torch.cat(recs, 0)).cpu().numpy()  # (the partition's one D2H)
    return out


def _merge(a: Tuple[int, float, float], b: Tuple[int, float, float]) -> Tuple[int, float, float]:
    """Chan's merge of (n, mean, M2), `a` the earlier rows."""
    if b[0] == 0:
        return a
    if a[0] == 0:
        return b
    n = a[0] + b[0]
    delta = b[1] - a[1]
    f = b[0] / n
    return n, a[1] + delta * f, a[2] + b[2] + delta * delta * (a[0] * f)


class _Moments:
    """Global n, mean, M2 and extreme words of the described columns."""

    def __init__(self, names: Sequence[str], dtypes: Sequence[np.dtype], table: np.ndarray):
        self.names = list(names)
        self.dtypes = list(dtypes)
        self.n: List[int] = []
        self.mean: List[float] = []
        self.m2: List[float] = []
        self.lo: List[int] = []
        self.hi: List[int] = []
        for c, dt in enumerate(dtypes):
            acc = (0, math.nan, math.nan)
            lo, hi = _ALL_ONES, 0
            for p in range(table.shape[0]):  # (partition order: the same on every rank)
                r = table[p, c]
                n = int(_from_bits(r[0]))
                if n == 0:
                    continue
                acc = _merge(acc, (n, _from_bits(r[1]), _from_bits(r[2])))
                lo = min(lo, int(r[3]) & _ALL_ONES)
                hi = max(hi, int(r[4]) & _ALL_ONES)
            n, mean, m2 = acc
            if n and _is_float(dt):
                # a NaN or an infinity propagates as in a plain sum / n, whatever
                # the order the rows were met in: the extremes tell what is there
                top, bottom = float(_decode_sort_word(hi, dt)), float(_decode_sort_word(lo, dt))
                if math.isnan(top) or (top == math.inf and bottom == -math.inf):
                    mean, m2 = math.nan, math.nan
                elif top == math.inf or bottom == -math.inf:
                    mean, m2 = (math.inf if top == math.inf else -math.inf), math.nan
            self.n.append(n)
            self.mean.append(mean)
            self.m2.append(m2)
            self.lo.append(lo)
            self.hi.append(hi)

    def stddev(self, c: int) -> float:
        return math.sqrt(self.m2[c] / (self.n[c] - 1)) if self.n[c] >= 2 else math.nan

    def extreme(self, c: int, which: str):
        """The decoded smallest / largest value (in the column's dtype), None without rows."""
        if self.n[c] == 0:
            return None
        return _decode_sort_word(self.lo[c] if which == "min" else self.hi[c], self.dtypes[c])


def _moments(df, blocks: Dict[int, Block], names: Sequence[str], what: str) -> _Moments:
    from ..utils.logging import metrics
    table = torch.zeros((df.num_partitions, len(names), 5), dtype=torch.int64)
    rows = 0
    for pid in sorted(blocks):
        if names:
            table[pid] = torch.from_numpy(_block_records(blocks[pid], names, what))
        rows += blocks[pid].nrows * len(names)
    metrics.add("stats_rows", rows)
    dist.all_reduce_host_(table, "Sum")  # (every rank fills the rows of its own partitions; the others are zero)
    return _Moments(names, [_np_dtype(df, n) for n in names], table.numpy())


# ------------------------------------------------------------------ quantiles
def _host_hist(words: np.ndarray, prefixes: Sequence[int], prefix_bits: int) -> np.ndarray:
    """select_hist on the host: int64 [P, 256]."""
    out = np.zeros((len(prefixes), 256), dtype=np.int64)
    digit = ((words >> np.uint64(56 - prefix_bits)) & np.uint64(255)).astype(np.int64)
    for q, pre in enumerate(prefixes):
        if prefix_bits == 0:
            out[q] = np.bincount(digit, minlength=256)
        else:
            sel = (words >> np.uint64(64 - prefix_bits)) == np.uint64(pre >> (64 - prefix_bits))
            out[q] = np.bincount(digit[sel], minlength=256)
    return out


def _select_words(blocks: Dict[int, Block], name: str, lo: int, hi: int, ranks: Sequence[int], what: str) -> List[int]:
    """The words at the 0-based positions `ranks` of the column's sorted order
    (collective). lo / hi: the column's smallest and largest word."""
    from .._native import _C
    from ..utils.logging import metrics
    from .dataframe import _host_sort_words
    if lo == hi:
        return [lo] * len(ranks)
    skip = 0  # leading digits every word shares
    while (lo ^ hi) >> (56 - 8 * skip) == 0:
        skip += 1
    start = (lo >> (64 - 8 * skip)) << (64 - 8 * skip) if skip else 0
    prefix = [start] * len(ranks)
    left = [int(r) for r in ranks]
    cols = {pid: _scalar_column(b, name, what) for pid, b in blocks.items() if b.nrows}
    host_words = {pid: _host_sort_words(c, False) for pid, c in cols.items() if not c.is_cuda}
    for bits in range(8 * skip, 64, 8):
        uniq = sorted(set(prefix))
        pre = torch.from_numpy(np.array(uniq, dtype=np.uint64).view(np.int64))
        hist = torch.zeros((len(uniq), 256), dtype=torch.int64)
        on_dev: Dict[torch.device, List[torch.Tensor]] = {}
        for pid in sorted(cols):
            c = cols[pid]
            if c.is_cuda:
                on_dev.setdefault(c.device, []).append(_C.select_hist(c.contiguous(), pre, bits))
            else:
                hist += torch.from_numpy(_host_hist(host_words[pid], uniq, bits))
        for hs in on_dev.values():
            hist += (hs[0] if len(hs) == 1 else torch.stack(hs, 0).sum(0)).cpu()  # (one D2H per device and pass)
        dist.all_reduce_host_(hist, "Sum")
        metrics.add("quantile_passes", 1)
        cum = np.cumsum(hist.numpy(), 1)
        for t in range(len(ranks)):
            row = cum[uniq.index(prefix[t])]
            d = int(np.searchsorted(row, left[t], side="right"))  # the first digit with cum > remaining rank
            if d > 255:
                raise RuntimeError(f"{what}: the histograms of '{name}' hold fewer rows than the moments pass counted")
            left[t] -= int(row[d - 1]) if d else 0
            prefix[t] |= d << (56 - bits)
    return prefix


def _check_probabilities(probabilities, what: str) -> List[float]:
    if isinstance(probabilities, (str, bytes)) or not isinstance(probabilities, (list, tuple, np.ndarray)):
        raise TypeError(f"{what}: probabilities must be a list of numbers in [0, 1], got {probabilities!r}")
    ps = []
    for p in probabilities:
        if isinstance(p, bool) or not isinstance(p, numbers.Real):
            raise TypeError(f"{what}: probabilities must be numbers in [0, 1], got {p!r}")
        if not 0.0 <= float(p) <= 1.0:  # (also refuses NaN)
            raise ValueError(f"{what}: probabilities must lie in [0, 1], got {p!r}")
        ps.append(float(p))
    if len(ps) > _MAX_PROBABILITIES:
        raise ValueError(f"{what}: at most {_MAX_PROBABILITIES} probabilities per call, got {len(ps)}")
    return ps


def _quantile_values(blocks: Dict[int, Block], mom: _Moments, c: int, ps: Sequence[float], what: str) -> list:
    """The values (in the column's dtype) at the probabilities ps of column c; [] without rows."""
    n = mom.n[c]
    if n == 0 or not ps:
        return []
    ranks = [max(math.ceil(p * n) - 1, 0) for p in ps]
    words = _select_words(blocks, mom.names[c], mom.lo[c], mom.hi[c], ranks, what)
    return [_decode_sort_word(w, mom.dtypes[c]) for w in words]


def approx_quantile(df, col, probabilities, relativeError=0.0):  # noqa: N803
    """`DataFrame.approxQuantile`: see there."""
    what = "approxQuantile"
    single = isinstance(col, str)
    if not single and not isinstance(col, (list, tuple)):
        raise TypeError(f"{what}: a column name or a list of names is expected, got {type(col).__name__}")
    names = [col] if single else list(col)
    if not names:
        raise ValueError(f"{what}: at least one column is expected")
    names = _stat_columns(df, names, what)
    ps = _check_probabilities(probabilities, what)
    if isinstance(relativeError, bool) or not isinstance(relativeError, numbers.Real):
        raise TypeError(f"{what}: relativeError must be a number >= 0, got {relativeError!r}")
    if not float(relativeError) >= 0.0:
        raise ValueError(f"{what}: relativeError must be >= 0, got {relativeError!r}")

    def run():
        blocks = df._blocks()
        mom = _moments(df, blocks, names, what)
        return [[float(v) for v in _quantile_values(blocks, mom, c, ps, what)] for c in range(len(names))]
    out = dist.agreed(what, run)
    return out[0] if single else out


def _statistics(stats: Sequence[Any], what: str) -> List[Tuple[str, Optional[float]]]:
    """[(label, probability or None)] of summary's statistics."""
    out = []
    for s in stats:
        if not isinstance(s, str):
            raise TypeError(f"{what}: statistics are names such as 'mean' or '25%', got {type(s).__name__}")
        t = s.strip()
        if t.lower() in _DESCRIBE:
            out.append((t.lower(), None))
            continue
        try:
            pct = float(t[:-1]) if t.endswith("%") else math.nan
        except ValueError:
            pct = math.nan
        if not 0.0 <= pct <= 100.0:
            raise ValueError(f"{what}: '{s}' is not a statistic; expected one of {', '.join(_DESCRIBE)} or a "
                             f"percentile such as '25%' (any number in [0, 100])")
        out.append((t, pct / 100.0))
    return out


def _stat_frame(df, names: Sequence[str], stats: Sequence[Tuple[str, Optional[float]]], what: str):
    """The result frame of describe / summary: one partition, a string column
    `summary` and one double column per described column."""
    from .dataframe import from_columns
    if "summary" in names:
        raise ValueError(f"{what}: a described column cannot be called 'summary' (the result's label column); "
                         f"rename it first")
    ps: List[float] = []
    for _, p in stats:
        if p is not None and p not in ps:
            ps.append(p)
    ps = _check_probabilities(ps, what)

    def run():
        blocks = df._blocks()
        mom = _moments(df, blocks, names, what)
        quant = [dict(zip(ps, _quantile_values(blocks, mom, c, ps, what))) for c in range(len(names))]
        return mom, quant
    mom, quant = dist.agreed(what, run)
    cols: Dict[str, Any] = {"summary": np.array([label for label, _ in stats])}
    for c, name in enumerate(names):
        vals = []
        for label, p in stats:
            if p is not None:
                v = quant[c].get(p)
                vals.append(math.nan if v is None else float(v))
            elif label == "count":
                vals.append(float(mom.n[c]))
            elif label == "mean":
                vals.append(mom.mean[c])
            elif label == "stddev":
                vals.append(mom.stddev(c))
            else:
                v = mom.extreme(c, label)
                vals.append(math.nan if v is None else float(v))
        cols[name] = np.array(vals, dtype=np.float64)
    return from_columns(cols, num_partitions=1)


def describe(df, *cols):
    """`DataFrame.describe`: see there."""
    names = _stat_columns(df, cols, "describe")
    return _stat_frame(df, names, [(s, None) for s in _DESCRIBE], "describe")


def summary(df, *statistics):
    """`DataFrame.summary`: see there."""
    stats = _statistics(_flatten(statistics) or _SUMMARY, "summary")
    return _stat_frame(df, _stat_columns(df, (), "summary"), stats, "summary")


class DataFrameStatFunctions:
    """`df.stat`: Spark's accessor for the statistics functions."""

    def __init__(self, df):
        self.df = df

    def approxQuantile(self, col, probabilities, relativeError=0.0):  # noqa: N802, N803
        return approx_quantile(self.df, col, probabilities, relativeError)

    approx_quantile = approxQuantile

    def corr(self, col1, col2, method="pearson"):
        return _pair_statistic(self.df, "corr", col1, col2, method)

    def cov(self, col1, col2):
        return _pair_statistic(self.df, "covar_samp", col1, col2, "pearson")

    def crosstab(self, col1, col2):
        """`DataFrame.crosstab`: the contingency table of two columns."""
        from .pivot import crosstab
        return crosstab(self.df, col1, col2)

    def sampleBy(self, col, fractions, seed=None):  # noqa: N802
        """`DataFrame.sampleBy`: a stratified sample by the values of `col`."""
        return self.df.sampleBy(col, fractions, seed)

    sample_by = sampleBy


def _pair_statistic(df, fn: str, col1, col2, method) -> float:
    """`df.stat.corr` / `df.stat.cov`: `DataFrame.agg` of one pair expression,
    as a Python float (an action, and collective)."""
    from .. import functions as F
    from .group_agg import frame_agg
    what = "corr" if fn == "corr" else "cov"
    if method != "pearson":
        raise ValueError(f"{what}: only the 'pearson' method is supported, got {method!r}")
    for c in (col1, col2):
        if not isinstance(c, str):
            raise TypeError(f"{what}: column names are expected, got {type(c).__name__}")
    out = frame_agg(df, [getattr(F, fn)(col1, col2).alias(what)], what)
    return float(out.to_numpy(what)[0])
