"""`Correlation`: the correlation / covariance matrix of a vector column
(`pyspark.ml.stat.Correlation`; `cov` is this project's addition, the
counterpart of `RowMatrix.computeCovariance`).

Every partition is reduced on its own to one float64 record (n, mean[d],
C[d, d]) with C = sum_r (x_r - mean)(x_r - mean)^T: device-resident partitions
through `_C.vector_moments` (kernels/vector_moments.hip: column means, a centred
SYRK on the f64 MFMA, a fold in slice order), host partitions through numpy
(shift by the partition mean, then xc.T @ xc). The records travel as one
zero-filled [nparts, 1 + d + d * d] table (one host all-reduce; every rank
fills the rows of its own partitions) and every rank merges them in ascending
partition order with Chan's formula

    C = C_a + C_b + delta delta^T * n_a n_b / n

skipping empty partitions: never sum(x x^T) - n mean mean^T, and for a given
partitioning the same bits on every rank and for every world size.

`Summarizer` (`pyspark.ml.stat.Summarizer`): the per-component metrics of a
vector column, optionally weighted, as expressions for `DataFrame.select` /
`DataFrame.agg`. The same scheme with a record that is linear in d: a header
(rows of positive weight, W = sum w, Q = sum w^2, bad weights) and eight fields
per component (the weighted mean, M2 = sum w (x - mean)^2, sum w |x|, sum w
x^2, the counts of entries != 0 and of non-finite entries, the smallest and
largest sort word), as int64 bit patterns: device-resident partitions through
`_C.vector_summary` (kernels/vector_summary.hip: one read of the column),
host partitions through numpy (two passes), one zero-filled int64 [nparts, 4 +
8 d] table, Chan's weighted merge in ascending partition order.
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np
import torch

from ..frame.block import Block
from ..frame.column_info import ColumnInformation
from ..frame.types import BinaryType, StringType, StructType
from ..parallel import dist
from ..utils import dtypes as D

MAX_COMPONENTS = 512  # a partition's record is 1 + d + d * d doubles: about 2 MB at the limit


def _vector_column(df, column, what: str, limit: int = MAX_COMPONENTS) -> int:
    """The number of components d (1 <= d <= limit) of the vector column, or the typed error."""
    from .. import core
    if not isinstance(column, str):
        raise TypeError(f"{what}: a column name is expected, got {type(column).__name__}")
    if column not in df.schema:
        raise ValueError(f"{what}: Column {column} not found in {df.columns}")
    f = df.schema[column]
    stf = ColumnInformation(f).stf
    if isinstance(f.dataType, (StringType, BinaryType)) or stf is None:
        raise core.InvalidTypeException(
            f"{what}: '{column}' ({f.dataType}) is not a dense vector column of float32 or float64")
    if stf.tf_dtype not in (D.DT_FLOAT, D.DT_DOUBLE):
        raise core.InvalidTypeException(
            f"{what}: '{column}' holds {D.dtype_name(stf.tf_dtype)} cells; cast them to float32 or float64 first")
    if stf.shape.num_dims == 1:
        raise core.InvalidDimensionException(
            f"{what}: '{column}' is a scalar column; a vector column (one cell [d] per row) is expected (F.corr and "
            f"df.stat.corr take two scalar columns)")
    if stf.shape.num_dims != 2:
        raise core.InvalidDimensionException(
            f"{what}: '{column}' holds a cell of rank {stf.shape.num_dims - 1} per row, not a vector [d]")
    d = stf.shape[1]
    if d is None or int(d) < 0:
        raise core.InvalidDimensionException(
            f"{what}: the cells of '{column}' have no fixed length in the schema; run analyze() first")
    if not 1 <= int(d) <= limit:
        raise ValueError(f"{what}: '{column}' has cells of {int(d)} components; 1 to {limit} are supported")
    return int(d)


def _host_record(x: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(mean [d], C [d, d]) of the rows x [n, d] (n >= 1), float64."""
    with np.errstate(all="ignore"):
        x = x.astype(np.float64)
        n = x.shape[0]
        mean = x.sum(0) / n
        xc = x - mean
        mean = mean + xc.sum(0) / n  # (the second pass takes out what rounding left in the mean)
        xc = x - mean
        c = np.triu(xc.T @ xc)
    return mean, c + np.triu(c, 1).T  # (the lower triangle is a copy of the upper)


def _merge(a, b):
    """Chan's merge of (n, mean, C), `a` the earlier rows."""
    if a is None:
        return b
    n = a[0] + b[0]
    with np.errstate(all="ignore"):
        delta = b[1] - a[1]
        f = b[0] / n
        return n, a[1] + delta * f, a[2] + b[2] + np.outer(delta, delta) * (a[0] * f)


def _moments(df, blocks: Dict[int, Block], column: str, d: int, what: str):
    """The merged (n, mean, C) of the column over all ranks, None without rows (collective)."""
    from .. import core, engine
    from .._native import _C
    from ..utils.logging import metrics
    table = torch.zeros((df.num_partitions, 1 + d + d * d), dtype=torch.float64)
    rows = 0
    rng = torch.cuda.is_initialized()
    if rng:
        torch.cuda.nvtx.range_push("tfa.vector_moments")
    try:
        for pid in sorted(blocks):
            b = blocks[pid]
            if not b.nrows:
                continue
            c = b.columns[column]
            if not isinstance(c, torch.Tensor) or c.dim() != 2 or c.shape[1] != d:
                raise core.InvalidDimensionException(
                    f"{what}: the column '{column}' does not hold one dense vector [{d}] per row in partition {pid}")
            table[pid, 0] = b.nrows
            if c.is_cuda and engine.gpu_available():
                mean, cm = _C.vector_moments(c.contiguous())
                table[pid, 1:] = torch.cat([mean, cm.reshape(-1)]).cpu()  # (the partition's one D2H)
                metrics.add("vector_moments_device_partitions")
            else:
                mean, cm = _host_record(c.detach().cpu().numpy())
                table[pid, 1:1 + d] = torch.from_numpy(mean)
                table[pid, 1 + d:] = torch.from_numpy(cm.reshape(-1))
                metrics.add("vector_moments_host_partitions")
            rows += b.nrows
    finally:
        if rng:
            torch.cuda.nvtx.range_pop()
    metrics.add("vector_moments_rows", rows)
    dist.all_reduce_host_(table, "Sum")  # (every rank fills the rows of its own partitions; the others are zero)
    tab = table.numpy()
    acc = None
    for p in range(tab.shape[0]):  # (partition order: the same on every rank)
        if tab[p, 0] > 0:
            acc = _merge(acc, (float(tab[p, 0]), tab[p, 1:1 + d].copy(), tab[p, 1 + d:].reshape(d, d).copy()))
    return acc


def _covariance(acc, d: int) -> np.ndarray:
    if acc is None or acc[0] < 2:
        return np.full((d, d), np.nan)
    with np.errstate(all="ignore"):
        cov = acc[2] / (acc[0] - 1.0)
    bad = ~np.isfinite(np.diagonal(cov))  # a NaN or an infinity among the component's values
    cov[bad, :] = np.nan
    cov[:, bad] = np.nan
    return cov


def _correlation(acc, d: int) -> np.ndarray:
    cov = _covariance(acc, d)
    var = np.diagonal(cov).copy()
    with np.errstate(all="ignore"):
        r = cov / np.sqrt(np.outer(var, var))  # (unclamped, as F.corr)
    bad = ~(np.isfinite(var) & (var > 0))  # constant components: NaN where Spark gives null
    r[bad, :] = np.nan
    r[:, bad] = np.nan
    r[np.diag_indices(d)] = np.where(bad, np.nan, 1.0)
    return r


def _matrix_frame(df, column: str, name: str, finish, what: str):
    from ..frame.dataframe import DataFrame, _Derived, tensor_field
    d = _vector_column(df, column, what)

    def compute(blocks):
        acc = dist.agreed(what, lambda: _moments(df, blocks, column, d, what))
        if dist.rank() != 0:  # (partition 0 lives on rank 0)
            return {}
        return {0: Block(1, {name: torch.from_numpy(finish(acc, d)).reshape(1, d, d)})}
    schema = StructType([tensor_field(name, torch.float64, [d, d])])
    return DataFrame(schema, _Derived(df, compute, streamable=False), 1)


class Correlation:
    """`pyspark.ml.stat.Correlation` for a dense vector column of float32 or
    float64 cells `[d]`, 1 <= d <= 512. The results are lazy frames of one
    partition and one row; evaluating them is collective."""

    @staticmethod
    def corr(df, column, method="pearson"):
        """The Pearson correlation matrix as one `double[d, d]` cell in a column
        `pearson(<column>)`: r_ij = C_ij / sqrt(C_ii C_jj), the diagonal exactly
        1.0, exactly symmetric. A constant component, or one that holds a NaN
        or an infinity, has a NaN row and column."""
        if method != "pearson":
            raise NotImplementedError(f"Correlation.corr: the method {method!r} is not implemented; only 'pearson' is")
        return _matrix_frame(df, column, f"pearson({column})", _correlation, "Correlation.corr")

    @staticmethod
    def cov(df, column):
        """The sample covariance matrix (divisor n - 1) as one `double[d, d]`
        cell in a column `cov(<column>)`; all NaN below two rows. Not part of
        Spark's class: the counterpart of `RowMatrix.computeCovariance`."""
        return _matrix_frame(df, column, f"cov({column})", _covariance, "Correlation.cov")


# ------------------------------------------------------------------ Summarizer
METRICS = ("mean", "sum", "variance", "std", "count", "numNonZeros", "max", "min", "normL2", "normL1")
MAX_SUMMARY_COMPONENTS = 65536  # (a record is 4 + 8 d words: linear in d)
_HEADER, _FIELDS = 4, 8  # kernels.h: kVectorSummaryHeader, kVectorSummaryFields


class SummaryExpression:
    """Metrics of one vector column, optionally weighted: what
    `Summarizer.metrics(...).summary(...)` and the shortcuts return, for
    `DataFrame.select` / `DataFrame.agg`. Every metric becomes its own column
    `<metric>(<featuresCol>)`."""

    __slots__ = ("metrics", "features", "weight", "_alias")

    def __init__(self, metrics, features: str, weight=None, alias=None):
        self.metrics = tuple(metrics)
        self.features = features
        self.weight = weight
        self._alias = alias

    def alias(self, name: str) -> "SummaryExpression":
        if not isinstance(name, str) or not name:
            raise TypeError(f"alias: a non-empty column name is expected, got {name!r}")
        if len(self.metrics) != 1:
            raise ValueError(f"alias: {self!r} makes {len(self.metrics)} columns; only an expression of a single "
                             f"metric can be renamed")
        return SummaryExpression(self.metrics, self.features, self.weight, name)

    name = alias

    @property
    def output_names(self):
        if self._alias is not None:
            return [self._alias]
        return [f"{m}({self.features})" for m in self.metrics]

    def __repr__(self):
        return f"SummaryExpression<{', '.join(self.output_names)}>"


def _column_name(what: str, col) -> str:
    from ..functions import _make  # (a name or a plain column reference, with the functions' errors)
    return _make(what, col).column


class SummaryBuilder:
    """`Summarizer.metrics(...)` before its `.summary(featuresCol, weightCol=None)`."""

    __slots__ = ("metrics",)

    def __init__(self, metrics):
        self.metrics = tuple(metrics)

    def summary(self, featuresCol, weightCol=None) -> SummaryExpression:  # noqa: N803
        what = "Summarizer.summary"
        return SummaryExpression(self.metrics, _column_name(what, featuresCol),
                                 None if weightCol is None else _column_name(what, weightCol))


class Summarizer:
    """`pyspark.ml.stat.Summarizer` for a dense vector column of float32 or
    float64 cells `[d]`, 1 <= d <= 65536, optionally weighted by a numeric scalar
    column: mean, sum, variance, std, count, numNonZeros, max, min, normL2 and
    normL1 per component from one read of the column. The expressions go to
    `DataFrame.select` or `DataFrame.agg`; the result is a lazy frame of one
    partition and one row, and evaluating it is collective."""

    @staticmethod
    def metrics(*names) -> SummaryBuilder:
        """The named metrics, in this order, one output column each."""
        if not names:
            raise ValueError(f"Summarizer.metrics: at least one metric is expected ({', '.join(METRICS)})")
        for i, n in enumerate(names):
            if n not in METRICS:
                raise ValueError(f"Summarizer.metrics: {n!r} is not a metric ({', '.join(METRICS)})")
            if n in names[:i]:
                raise ValueError(f"Summarizer.metrics: the metric {n!r} is repeated")
        return SummaryBuilder(names)


def _shortcut(metric: str):
    def fn(col, weightCol=None):  # noqa: N803
        return Summarizer.metrics(metric).summary(col, weightCol)
    fn.__name__ = metric
    fn.__doc__ = f"`Summarizer.metrics(\"{metric}\").summary(col, weightCol)`: one column `{metric}(<col>)`."
    return staticmethod(fn)


for _m in METRICS:
    setattr(Summarizer, _m, _shortcut(_m))


def _host_summary(x: np.ndarray, w, d: int) -> np.ndarray:
    """The record [4 + 8 d] (int64 bit patterns, the layout of `_C.vector_summary`)
    of the rows x [n, d] with weights w [n] or None: two passes, the weighted
    mean and then sum w (x - mean)^2."""
    from ..frame.dataframe import _host_sort_words
    rec = np.zeros(_HEADER + _FIELDS * d, dtype=np.int64)
    f = rec[_HEADER:].reshape(_FIELDS, d)
    f[6] = -1  # (the empty record: all ones in the smallest word)
    with np.errstate(all="ignore"):
        x = x.astype(np.float64)
        w = np.ones(x.shape[0]) if w is None else w.astype(np.float64)
        usable = (w >= 0) & ~np.isinf(w)
        keep = usable & (w > 0)
        rec[3] = int((~usable).sum())
        x, w = x[keep], w[keep][:, None]
        rec[0] = x.shape[0]
        if not x.shape[0]:
            return rec
        W = w.sum()
        rec[1:3] = np.array([W, (w * w).sum()]).view(np.int64)
        mean = (w * x).sum(0) / W
        mean = mean + (w * (x - mean)).sum(0) / W  # (the second pass takes out what rounding left in the mean)
        xc = x - mean
        f[0] = mean.view(np.int64)
        f[1] = (w * xc * xc).sum(0).view(np.int64)
        f[2] = (w * np.abs(x)).sum(0).view(np.int64)
        f[3] = (w * x * x).sum(0).view(np.int64)
        f[4] = (x != 0).sum(0)
        f[5] = (~np.isfinite(x)).sum(0)
        words = _host_sort_words(torch.from_numpy(x), False)
        f[6] = words.min(0).view(np.int64)
        f[7] = words.max(0).view(np.int64)
    return rec


def _unpack(rec: np.ndarray, d: int):
    """(W, [mean, M2, L1, S2] f64 [4, d], [nnz, non-finite] [2, d], smallest word, largest word) of a record."""
    f = rec[_HEADER:].reshape(_FIELDS, d)
    return float(rec[1:2].view(np.float64)[0]), f[:4].view(np.float64).copy(), f[4:6].copy(), \
        f[6].view(np.uint64).copy(), f[7].view(np.uint64).copy()


def _merge_summary(a, b):
    """Chan's weighted merge of two unpacked records of positive weight, `a` the earlier rows."""
    if a is None:
        return b
    W = a[0] + b[0]
    with np.errstate(all="ignore"):
        delta = b[1][0] - a[1][0]
        fr = b[0] / W
        sums = a[1] + b[1]  # (L1 and S2 add; the mean and M2 rows are replaced below)
        sums[0] = a[1][0] + delta * fr
        sums[1] = a[1][1] + b[1][1] + delta * delta * (a[0] * fr)
    return W, sums, a[2] + b[2], np.minimum(a[3], b[3]), np.maximum(a[4], b[4])


def _summary(df, blocks: Dict[int, Block], features: str, weight, d: int, wanted, what: str):
    """The merged record of the column over all ranks: (count, W, Q, unpacked
    record or None without a row of positive weight). Collective; raises the
    ValueError of a bad weight, or of an empty frame asked for more than the
    count, on every rank alike."""
    from .. import core, engine
    from .._native import _C
    from ..frame._scalar_columns import _scalar_column
    from ..utils.logging import metrics
    table = torch.zeros((df.num_partitions, _HEADER + _FIELDS * d), dtype=torch.int64)
    rows = 0
    rng = torch.cuda.is_initialized()
    if rng:
        torch.cuda.nvtx.range_push("tfa.vector_summary")
    try:
        for pid in sorted(blocks):
            b = blocks[pid]
            if not b.nrows:
                continue
            c = b.columns[features]
            if not isinstance(c, torch.Tensor) or c.dim() != 2 or c.shape[1] != d:
                raise core.InvalidDimensionException(
                    f"{what}: the column '{features}' does not hold one dense vector [{d}] per row in partition {pid}")
            w = None if weight is None else _scalar_column(b, weight, what)
            if c.is_cuda and engine.gpu_available():
                rec = _C.vector_summary(c.contiguous(), None if w is None else w.to(c.device).contiguous())
                table[pid] = rec.cpu()  # (the partition's one D2H)
                metrics.add("vector_summary_device_partitions")
            else:
                table[pid] = torch.from_numpy(_host_summary(c.detach().cpu().numpy(),
                                                            None if w is None else w.detach().cpu().numpy(), d))
                metrics.add("vector_summary_host_partitions")
            rows += b.nrows
    finally:
        if rng:
            torch.cuda.nvtx.range_pop()
    metrics.add("vector_summary_rows", rows)
    dist.all_reduce_host_(table, "Sum")  # (every rank fills the rows of its own partitions; the others are zero)
    tab = table.numpy()
    bad = int(tab[:, 3].sum())
    if bad:
        raise ValueError(f"{what}: the weight column '{weight}' holds {bad} negative, NaN or infinite weights")
    count, q, acc = 0, 0.0, None
    for p in range(tab.shape[0]):  # (partition order: the same on every rank)
        if tab[p, 0] > 0:
            count += int(tab[p, 0])
            q += float(tab[p, 2:3].view(np.float64)[0])
            acc = _merge_summary(acc, _unpack(tab[p], d))
    if acc is None and any(m != "count" for m in wanted):
        raise ValueError(f"{what}: '{features}' has no row of positive weight; only count is defined there")
    return count, q, acc


def _metric(metric: str, count: int, q: float, acc, d: int) -> torch.Tensor:
    from ..frame._scalar_columns import _decode_sort_word
    if metric == "count":
        return torch.tensor([count], dtype=torch.int64)
    W, (mean, m2, l1, s2), (nnz, nonfinite), lo, hi = acc
    nan = np.where(nonfinite > 0, np.nan, 0.0)  # a NaN or an infinity among the component's counted values
    with np.errstate(all="ignore"):
        if metric == "mean":
            v = mean + nan
        elif metric == "sum":
            v = mean * W + nan
        elif metric in ("variance", "std"):
            den = W - q / W
            v = np.maximum(m2 / den, 0.0) if den > 0 else np.zeros(d)
            v = (np.sqrt(v) if metric == "std" else v) + nan
        elif metric == "numNonZeros":
            v = nnz.astype(np.float64)
        elif metric == "normL1":
            v = l1
        elif metric == "normL2":
            v = np.sqrt(s2)
        else:
            v = _decode_sort_word(lo if metric == "min" else hi, np.float64)
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).reshape(1, d)


def summary_frame(df, items, what: str):
    """`df.select(...)` / `df.agg(...)` of `SummaryExpression`s only: one row,
    one column per metric in the order given; expressions that share (features,
    weight) share one pass over the column."""
    from ..frame._scalar_columns import _ineligible
    from ..frame.dataframe import DataFrame, _Derived, tensor_field
    outs, groups = [], {}  # (output name, metric, group); group (features, weight) -> [d, metrics wanted]
    for it in items:
        if not isinstance(it, SummaryExpression):
            shown = repr(it) if isinstance(it, str) else type(it).__name__
            raise TypeError(f"{what}: Summarizer expressions cannot be mixed with anything else in one call, got "
                            f"{shown}; make the summary a call of its own")
        key = (it.features, it.weight)
        if key not in groups:
            d = _vector_column(df, it.features, what, MAX_SUMMARY_COMPONENTS)
            if it.weight is not None:
                if it.weight not in df.schema:
                    raise ValueError(f"{what}: Column {it.weight} not found in {df.columns}")
                err = _ineligible(df, it.weight, what)
                if err is not None:
                    raise err
            groups[key] = [d, []]
        for name, m in zip(it.output_names, it.metrics):
            if any(name == o[0] for o in outs):
                raise ValueError(f"{what}: duplicate output column name '{name}'; give one of them an .alias()")
            outs.append((name, m, key))
            groups[key][1].append(m)

    def compute(blocks):
        def merged():
            return {key: _summary(df, blocks, key[0], key[1], d, wanted, what) for key, (d, wanted) in groups.items()}
        recs = dist.agreed(what, merged)
        if dist.rank() != 0:  # (partition 0 lives on rank 0)
            return {}
        return {0: Block(1, {name: _metric(m, *recs[key], groups[key][0]) for name, m, key in outs})}
    schema = StructType([tensor_field(name, torch.int64, []) if m == "count" else
                         tensor_field(name, torch.float64, [groups[key][0]]) for name, m, key in outs])
    return DataFrame(schema, _Derived(df, compute, streamable=False), 1)
