"""Named aggregate functions for `GroupedData.agg` / `DataFrame.agg`.

    from tensorframes_amd import functions as F
    scored.groupBy("id").agg(F.avg("score"), F.stddev("score"), F.max("score"))

Each function takes a column name or a plain column reference (`tfs.col("x")`,
`df["x"]`) and returns an `AggregateExpression`; `.alias(name)` renames its
output column. `corr`, `covar_samp` and `covar_pop` take two columns and return
a `PairAggregateExpression`, accepted wherever the others are. `median`,
`percentile`, `percentile_approx`, `mode`, `countDistinct` and
`approx_count_distinct` need a group's rows in order and return an
`OrderAggregateExpression`, accepted in `agg` as well (frame/order_agg.py);
they are reachable through these functions only, not through the dict form of
`agg`. These reduce a column over the rows of a group. They are not `Column.sum()` and friends,
which reduce the cell of one row.
"""
from __future__ import annotations

import numbers
from typing import Optional, Sequence, Tuple

from .frame.column import Column

__all__ = ["AggregateExpression", "PairAggregateExpression", "OrderAggregateExpression", "median", "percentile",
           "percentile_approx", "mode", "countDistinct", "count_distinct", "approx_count_distinct", "count", "sum", "avg", "mean", "min", "max", "stddev",
           "stddev_samp", "stddev_pop", "variance", "var_samp", "var_pop", "corr", "covar_samp", "covar_pop",
           "row_number", "rank", "dense_rank", "rand", "randn"]

# the canonical statistic behind every accepted name (the dict form of agg uses the same table)
FUNCTIONS = {
    "count": "count", "sum": "sum", "avg": "avg", "mean": "avg", "min": "min", "max": "max",
    "stddev": "stddev_samp", "stddev_samp": "stddev_samp", "stddev_pop": "stddev_pop",
    "variance": "var_samp", "var_samp": "var_samp", "var_pop": "var_pop",
}


class AggregateExpression:
    """One aggregate of one column: `fn` is the canonical statistic, `column`
    the value column's name (None for `count("*")` / `count(1)`)."""

    __slots__ = ("fn", "column", "_alias")

    def __init__(self, fn: str, column: Optional[str], alias: Optional[str] = None):
        self.fn = fn
        self.column = column
        self._alias = alias

    def alias(self, name: str) -> "AggregateExpression":
        if not isinstance(name, str) or not name:
            raise TypeError(f"alias: a non-empty column name is expected, got {name!r}")
        return AggregateExpression(self.fn, self.column, name)

    name = alias

    @property
    def output_name(self) -> str:
        if self._alias is not None:
            return self._alias
        return f"{self.fn}({self.column if self.column is not None else 1})"

    def over(self, spec):
        """This aggregate over the rows of a window (`Window.partitionBy(...)`
        ...): one value per row, for `DataFrame.withColumn` / `select`. count,
        sum, avg / mean, min and max; the output types are those of
        `groupBy().agg`."""
        from .frame.window import _AGGREGATES, WindowExpression
        if self.fn not in _AGGREGATES:
            raise NotImplementedError(f"{self.fn}({self.column}).over: {self.fn} is not supported over a window; "
                                      f"count, sum, avg, min and max are")
        return WindowExpression(self.fn, self.column, spec, self._alias)

    def __repr__(self):
        return f"AggregateExpression<{self.output_name}>"


class PairAggregateExpression:
    """One aggregate of two columns read together: `fn` is corr, covar_samp or
    covar_pop, `x` and `y` the value columns' names. The output is float64."""

    __slots__ = ("fn", "x", "y", "_alias")

    def __init__(self, fn: str, x: str, y: str, alias: Optional[str] = None):
        self.fn = fn
        self.x = x
        self.y = y
        self._alias = alias

    def alias(self, name: str) -> "PairAggregateExpression":
        if not isinstance(name, str) or not name:
            raise TypeError(f"alias: a non-empty column name is expected, got {name!r}")
        return PairAggregateExpression(self.fn, self.x, self.y, name)

    name = alias

    @property
    def output_name(self) -> str:
        if self._alias is not None:
            return self._alias
        return f"{self.fn}({self.x}, {self.y})"

    def over(self, spec):
        raise NotImplementedError(f"{self.fn}({self.x}, {self.y}).over: pair aggregates are not supported over a "
                                  f"window; count, sum, avg, min and max are")

    def __repr__(self):
        return f"PairAggregateExpression<{self.output_name}>"


_MAX_PERCENTAGES = 16  # kernels.h kMaxPercentages


class OrderAggregateExpression:
    """One aggregate that needs the rows of a group in order: `fn` is
    percentile, percentile_approx, mode or count_distinct, `columns` the value
    columns' names (several for count_distinct alone), `percentages` the
    percentages of the first two (`is_list`: they were given as a list, and
    the output cell has shape [Q])."""

    __slots__ = ("fn", "columns", "percentages", "is_list", "_label", "_alias")

    def __init__(self, fn: str, columns: Sequence[str], percentages: Tuple[float, ...] = (), is_list: bool = False,
                 label: Optional[str] = None, alias: Optional[str] = None):
        self.fn = fn
        self.columns = tuple(columns)
        self.percentages = tuple(percentages)
        self.is_list = is_list
        self._label = label
        self._alias = alias

    def alias(self, name: str) -> "OrderAggregateExpression":
        if not isinstance(name, str) or not name:
            raise TypeError(f"alias: a non-empty column name is expected, got {name!r}")
        return OrderAggregateExpression(self.fn, self.columns, self.percentages, self.is_list, self._label, name)

    name = alias

    @property
    def output_name(self) -> str:
        if self._alias is not None:
            return self._alias
        return self._label if self._label is not None else f"{self.fn}({', '.join(self.columns)})"

    def over(self, spec):
        raise NotImplementedError(f"{self.output_name}.over: order aggregates are not supported over a window; "
                                  f"count, sum, avg, min and max are")

    def __repr__(self):
        return f"OrderAggregateExpression<{self.output_name}>"


class RankingFunction:
    """`row_number()`, `rank()` or `dense_rank()` before its `.over(spec)`."""

    __slots__ = ("fn",)

    def __init__(self, fn: str):
        self.fn = fn

    def over(self, spec):
        from .frame.window import WindowExpression
        return WindowExpression(self.fn, None, spec)

    def __repr__(self):
        return f"RankingFunction<{self.fn}()>"


def _make(fn: str, col) -> AggregateExpression:
    if isinstance(col, Column):
        if not col.is_reference:
            raise TypeError(f"{fn}: '{col.output_name}' is a computed Column; aggregates take a column name or a "
                            f"plain column reference. Add it to the frame first: df.withColumn(name, expr), then "
                            f"{fn}(name)")
        if col.sort_order is not None:
            raise TypeError(f"{fn}: '{col.output_name}.{col.sort_order}()' is a sort order, not a column")
        return AggregateExpression(FUNCTIONS.get(fn, fn), col._expr[1])
    if not isinstance(col, str):
        raise TypeError(f"{fn}: a column name or a column reference is expected, got {type(col).__name__}")
    return AggregateExpression(FUNCTIONS.get(fn, fn), col)


def _make_pair(fn: str, col1, col2) -> PairAggregateExpression:
    # (the rules, and the errors, of the one-column functions for each argument)
    return PairAggregateExpression(fn, _make(fn, col1).column, _make(fn, col2).column)


def count(col) -> AggregateExpression:
    """Rows per group. `count("*")` and `count(1)` count rows; frames hold no
    nulls, so `count(x)` is the same number."""
    if (isinstance(col, str) and col == "*") or (isinstance(col, int) and not isinstance(col, bool) and col == 1):
        return AggregateExpression("count", None)
    return _make("count", col)


def sum(col) -> AggregateExpression:  # noqa: A001
    """int64 (wrapping) for integer columns, float64 for float32 / float64."""
    return _make("sum", col)


def avg(col) -> AggregateExpression:
    return _make("avg", col)


def mean(col) -> AggregateExpression:
    """The same as `avg`."""
    return _make("mean", col)


def min(col) -> AggregateExpression:  # noqa: A001
    """The smallest value in `orderBy`'s order, in the column's own type."""
    return _make("min", col)


def max(col) -> AggregateExpression:  # noqa: A001
    """The largest value in `orderBy`'s order (NaN after +inf), in the column's own type."""
    return _make("max", col)


def stddev(col) -> AggregateExpression:
    """The sample standard deviation (NaN for a group of one row)."""
    return _make("stddev", col)


def stddev_samp(col) -> AggregateExpression:
    return _make("stddev_samp", col)


def stddev_pop(col) -> AggregateExpression:
    return _make("stddev_pop", col)


def variance(col) -> AggregateExpression:
    """The sample variance (NaN for a group of one row)."""
    return _make("variance", col)


def var_samp(col) -> AggregateExpression:
    return _make("var_samp", col)


def var_pop(col) -> AggregateExpression:
    return _make("var_pop", col)


def corr(col1, col2) -> PairAggregateExpression:
    """Pearson's correlation coefficient of two columns, C / sqrt(M2_x * M2_y)
    with C the sum of (x - mean_x)(y - mean_y): NaN for a group without rows or
    with a constant column (one row included), and for a group with a NaN or
    an infinity in either column. Not clamped, as in Spark: a value such as
    1.0000000000000002 can occur."""
    return _make_pair("corr", col1, col2)


def covar_samp(col1, col2) -> PairAggregateExpression:
    """The sample covariance C / (n - 1) (NaN for a group of one row)."""
    return _make_pair("covar_samp", col1, col2)


def covar_pop(col1, col2) -> PairAggregateExpression:
    """The population covariance C / n."""
    return _make_pair("covar_pop", col1, col2)


def _percentages(fn: str, percentage):
    """(the percentages as floats, whether they came as a list)"""
    is_list = isinstance(percentage, (list, tuple))
    ps = list(percentage) if is_list else [percentage]
    if is_list and not 1 <= len(ps) <= _MAX_PERCENTAGES:
        raise ValueError(f"{fn}: a list of 1..{_MAX_PERCENTAGES} percentages is expected, got {len(ps)}")
    out = []
    for p in ps:
        if isinstance(p, bool) or not isinstance(p, numbers.Real):
            raise TypeError(f"{fn}: a percentage is a number in [0, 1] (or a list of them), got {p!r}")
        if not 0.0 <= float(p) <= 1.0:  # (also refuses NaN)
            raise ValueError(f"{fn}: a percentage must lie in [0, 1], got {p!r}")
        out.append(float(p))
    return tuple(out), is_list


def _percentage_text(ps, is_list: bool) -> str:
    return f"array({', '.join(repr(p) for p in ps)})" if is_list else repr(ps[0])


def median(col) -> OrderAggregateExpression:
    """`percentile(col, 0.5)` (float64)."""
    c = _make("median", col).column
    return OrderAggregateExpression("percentile", (c,), (0.5,), False, f"median({c})")


def percentile(col, percentage) -> OrderAggregateExpression:
    """The exact percentile, linearly interpolated as Spark's `Percentile`
    (float64): with N rows, pos = p (N - 1), lo = floor(pos), hi = ceil(pos),
    the value at sorted position lo when lo == hi and otherwise
    (hi - pos) v_lo + (pos - lo) v_hi. `percentage`: a number in [0, 1], or a
    list of 1..16 of them (a cell of shape [Q]). NaNs count as rows and sort
    last."""
    c = _make("percentile", col).column
    ps, is_list = _percentages("percentile", percentage)
    return OrderAggregateExpression("percentile", (c,), ps, is_list, f"percentile({c}, {_percentage_text(ps, is_list)})")


def percentile_approx(col, percentage, accuracy=10000) -> OrderAggregateExpression:
    """The element of the column at 0-based rank max(ceil(p N) - 1, 0) of the
    group's ascending order, in the column's own type: `approxQuantile`'s rule.
    It is exact; `accuracy` must be a positive int and is otherwise ignored."""
    c = _make("percentile_approx", col).column
    ps, is_list = _percentages("percentile_approx", percentage)
    if isinstance(accuracy, bool) or not isinstance(accuracy, numbers.Integral):
        raise TypeError(f"percentile_approx: accuracy must be a positive int, got {accuracy!r}")
    if accuracy <= 0:
        raise ValueError(f"percentile_approx: accuracy must be a positive int, got {accuracy!r}")
    return OrderAggregateExpression("percentile_approx", (c,), ps, is_list,
                                    f"percentile_approx({c}, {_percentage_text(ps, is_list)}, {int(accuracy)})")


def mode(col) -> OrderAggregateExpression:
    """The value with the most rows in the group, in the column's own type;
    among ties the smallest in `orderBy`'s order."""
    c = _make("mode", col).column
    return OrderAggregateExpression("mode", (c,), label=f"mode({c})")


def countDistinct(col, *cols) -> OrderAggregateExpression:  # noqa: N802
    """The number of distinct value tuples in the group (int64); values compare
    as in `orderBy`: NaN equals NaN (and counts), -0.0 equals 0.0."""
    names = [_make("countDistinct", c).column for c in (col,) + cols]
    return OrderAggregateExpression("count_distinct", names, label=f"count(DISTINCT {', '.join(names)})")


count_distinct = countDistinct


def approx_count_distinct(col, rsd=0.05) -> OrderAggregateExpression:
    """The exact distinct count (int64); `rsd` must be > 0 and is otherwise
    ignored, as `relativeError` is in `approxQuantile`."""
    c = _make("approx_count_distinct", col).column
    if isinstance(rsd, bool) or not isinstance(rsd, numbers.Real):
        raise TypeError(f"approx_count_distinct: rsd must be a number > 0, got {rsd!r}")
    if not rsd > 0:
        raise ValueError(f"approx_count_distinct: rsd must be > 0, got {rsd!r}")
    return OrderAggregateExpression("count_distinct", (c,), label=f"approx_count_distinct({c})")


def row_number() -> RankingFunction:
    """1, 2, 3, ... within the group, in the spec's order (int32); ties keep
    the input's order."""
    return RankingFunction("row_number")


def rank() -> RankingFunction:
    """The row number of the first of the row's peers (rows whose order keys
    tie): 1, 1, 3, ... (int32)."""
    return RankingFunction("rank")


def dense_rank() -> RankingFunction:
    """Distinct order-key tuples of the group up to the row's: 1, 1, 2, ... (int32)."""
    return RankingFunction("dense_rank")


def rand(seed=None):
    """One uniform float64 in [0, 1) per row, for `DataFrame.withColumn` /
    `select`: a pure function of (seed, global row index), the same bits on
    the host and on the device and for every number of ranks. `seed=None`
    draws a seed when the column is added. No Column: add it first, then
    compute with it."""
    from .frame.sampling import RandomExpression
    return RandomExpression("rand", seed)


def randn(seed=None):
    """One standard normal float64 per row (Box-Muller over the row's Philox
    words; see `rand`)."""
    from .frame.sampling import RandomExpression
    return RandomExpression("randn", seed)
