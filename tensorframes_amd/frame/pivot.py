"""GroupedData.pivot(...).agg(...) and DataFrame.stat.crosstab: one row per
key, one column per (pivot value, expression).

* stages 1 and 2 are those of `groupBy(keys, pivot).agg(...)`
  (group_agg._merged_records) with one difference: across ranks a record is
  routed by the hash of the grouping keys alone, so every pivot value of a key
  lands on the key's rank (no keys: on rank 0). What comes out is the long
  table, one merged record per (key tuple, pivot value) in ascending
  (keys..., pivot) order, finalised column by column by group_agg._outputs.
* the spread: the distinct key tuples and the CSR of each key's records
  (`group_ids` on the key columns), the sort word of every record's pivot
  value and the words of the V listed values go to `_C.pivot_spread`
  (kernels/pivot.hip), which writes every output as a [V, G] tensor: the
  column of value j is the contiguous slice [j]. Host partitions do the same
  in numpy.

A cell whose (key, value) has no rows holds 0 where the output is int64 (count,
integer sums) and NaN where it is floating. Every output bit is that of
`groupBy(keys, pivot).agg(...)` for the cell's (key, value), for every world
size and from run to run.
"""
from __future__ import annotations

import numbers
from typing import Any, Dict, List, Optional, Sequence

import numpy as np
import torch

from ..functions import FUNCTIONS, AggregateExpression
from ..parallel import dist
from ..utils import dtypes as D
from ._scalar_columns import _aggregate_dtype, _stat_columns, _tf_dtype
from .block import Block
from .group_agg import _MAX_COLS, _check_keys, _columns_of, _merged_records, _needed, _outputs, _specs
from .types import StructType

MAX_VALUES = 1024    # kernels.h kMaxPivotValues
MAX_COLUMNS = 4096   # values times expressions
_NAN_BITS = {torch.float64: 0x7FF8000000000000, torch.float32: 0x7FC00000}


# ------------------------------------------------------------------ values
def _words(values: np.ndarray) -> np.ndarray:
    """uint64 sort words of a numpy array of pivot values (sort_words.h)."""
    from .dataframe import _host_sort_words
    return _host_sort_words(torch.from_numpy(np.ascontiguousarray(values)), False)


def _canonical(values: np.ndarray) -> np.ndarray:
    """-0.0 is 0.0, every NaN the one NaN: the value its sort word stands for."""
    if values.dtype.kind == "f":
        values = values.copy()
        values[values == 0] = 0.0
        values[np.isnan(values)] = np.nan
    return values


def _explicit_values(values, dt: np.dtype, pivot_col: str) -> np.ndarray:
    if isinstance(values, np.ndarray):
        values = list(values.reshape(-1))
    if not isinstance(values, (list, tuple)):
        raise TypeError(f"pivot: values must be a list of numbers, got {type(values).__name__}")
    if len(values) == 0:
        raise ValueError("pivot: values must not be empty; leave it out to take the distinct values of "
                         f"'{pivot_col}'")
    out = np.empty(len(values), dtype=dt)
    for i, v in enumerate(values):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (numbers.Real, np.number)):
            raise ValueError(f"pivot: value {v!r} is not a number ({type(v).__name__}); '{pivot_col}' is {dt}")
        same, c = False, None
        whole = isinstance(v, (numbers.Integral, np.integer))
        with np.errstate(all="ignore"):
            try:
                if dt.kind == "i":
                    same = (whole or float(v) == int(v)) and np.iinfo(dt).min <= int(v) <= np.iinfo(dt).max
                    c = dt.type(int(v)) if same else None
                else:
                    c = dt.type(v)
                    if whole:
                        same = bool(np.isfinite(c)) and int(c) == int(v)
                    else:
                        same = bool(np.isnan(c)) if v != v else float(c) == float(v)
            except (OverflowError, ValueError):
                same = False
        if not same:
            raise ValueError(f"pivot: value {v!r} does not convert to the {dt} of '{pivot_col}' without change")
        out[i] = c
    out = _canonical(out)
    w = _words(out)
    if len(np.unique(w)) != len(w):
        seen: Dict[int, Any] = {}
        for v, x in zip(values, w.tolist()):
            if x in seen:
                raise ValueError(f"pivot: the values {seen[x]!r} and {v!r} are the same value of '{pivot_col}'")
            seen[x] = v
    return out


def _discovered_values(df, pivot_col: str, dt: np.dtype) -> np.ndarray:
    """The distinct values of the pivot column, ascending with NaN last (eager
    and collective)."""
    got = np.asarray(df.select(pivot_col).distinct().to_numpy(pivot_col)).reshape(-1).astype(dt, copy=False)
    got = _canonical(got)
    w = _words(got)
    _, first = np.unique(w, return_index=True)  # (ascending words; one value per word)
    return got[first]


def _value_text(v) -> str:
    if isinstance(v, np.integer):
        return str(int(v))
    if np.isnan(v):
        return "NaN"
    if np.isinf(v):
        return "Infinity" if v > 0 else "-Infinity"
    return str(v)


def _check_count(nvalues: int, nexprs: Optional[int] = None) -> None:
    if nvalues > MAX_VALUES:
        raise ValueError(f"pivot: {nvalues} pivot values; at most {MAX_VALUES} are supported (list the values to "
                         f"keep, or filter the frame first)")
    if nexprs is not None and nvalues * nexprs > MAX_COLUMNS:
        raise ValueError(f"pivot: {nvalues} values times {nexprs} expressions are {nvalues * nexprs} output columns; "
                         f"at most {MAX_COLUMNS} are supported")


# ------------------------------------------------------------------ the spread
def _host_spread(offsets: np.ndarray, pivot_words: np.ndarray, value_words: np.ndarray, vals: Sequence[np.ndarray],
                 fills: Sequence[int]) -> List[np.ndarray]:
    """The host form of `_C.pivot_spread`: [V, G] per column."""
    G, V = len(offsets) - 1, len(value_words)
    group = np.repeat(np.arange(G, dtype=np.int64), np.diff(offsets))
    order = np.argsort(value_words, kind="stable")
    sorted_words = value_words[order]
    pos = np.minimum(np.searchsorted(sorted_words, pivot_words), V - 1)
    hit = sorted_words[pos] == pivot_words
    rows, cols = order[pos[hit]], group[hit]
    outs = []
    for v, f in zip(vals, fills):
        bits = np.dtype(f"i{v.dtype.itemsize}")
        o = np.full((V, G), np.array(f, dtype=np.int64).astype(bits), dtype=bits)
        o[rows, cols] = v.view(bits)[hit]
        outs.append(o.view(v.dtype))
    return outs


def _spread(on_device: bool, keys_u: List[torch.Tensor], pivot_u: torch.Tensor, value_words: np.ndarray,
            outs: List[torch.Tensor], fills: List[int]):
    """(distinct key columns [G], G, per output a [V, G] tensor) from the long
    table in ascending (keys..., pivot) order."""
    from .. import engine
    from .._native import _C
    from ..ops import groupby as G_
    from .dataframe import _host_sort_words
    m = int(pivot_u.shape[0])
    dev = pivot_u.device
    if keys_u:
        ids, gkeys, G = G_.group_ids([k.contiguous() for k in keys_u])
    else:
        ids, gkeys, G = engine.device_full(m, 0, torch.int64, dev), [], 1
    wide: List[torch.Tensor] = []
    if on_device:
        _, offsets = _C.segment_csr(ids, G)
        pw = _C.sort_encode([pivot_u.contiguous()], [False])[0].contiguous()
        vw = torch.from_numpy(value_words.view(np.int64).copy()).to(dev)
        for a in range(0, len(outs), _MAX_COLS):
            wide += _C.pivot_spread(offsets, pw, vw, [o.contiguous() for o in outs[a:a + _MAX_COLS]],
                                    fills[a:a + _MAX_COLS])
    else:
        offsets = np.concatenate([[0], np.cumsum(np.bincount(ids.numpy(), minlength=G))]).astype(np.int64)
        pw = _host_sort_words(pivot_u, False)
        wide = [torch.from_numpy(o) for o in
                _host_spread(offsets, pw, value_words, [o.contiguous().numpy() for o in outs], fills)]
    return gkeys, G, wide


# ------------------------------------------------------------------ the frames
class PivotedData:
    """`GroupedData.pivot(pivot_col, values)`: the frame, the grouping keys,
    the pivot column and its values (in output order), waiting for `agg`."""

    def __init__(self, df, keys: Sequence[str], pivot_col: str, values: np.ndarray):
        self.df = df
        self.keys = list(keys)
        self.pivot_col = pivot_col
        self.values = values

    def agg(self, *exprs):
        """One row per key; per pivot value, in order, one column per
        expression in call order, named by the value alone (one expression) or
        `<value>_<expression's output name>` (several). Expressions, output
        types and values are those of `GroupedData.agg` on the keys plus the
        pivot column; order aggregates (median, percentile, mode,
        countDistinct) are not supported. A cell whose (key, value) has no rows
        holds 0 where the output is int64 (count, integer sums) and NaN where
        it is floating (Spark: null); `min` / `max` of an integer column have
        no such stand-in and raise ValueError (cast to double first). A key has
        a row as soon as it has any row in the input. One output partition per
        rank, keys in ascending order; device-resident when the input was
        (kernels/pivot.hip); lazy."""
        return pivot_agg(self, list(exprs), "pivot.agg")

    def count(self):
        """Rows per (key, pivot value), int64; 0 where there are none."""
        return pivot_agg(self, [AggregateExpression("count", None)], "pivot.count")

    def _stat(self, fn: str, cols):
        names = _stat_columns(self.df, cols, fn)
        if not [c for cs in cols for c in (cs if isinstance(cs, (list, tuple)) else [cs])]:
            names = [n for n in names if n not in self.keys and n != self.pivot_col]
        if not names:
            raise ValueError(f"{fn}: the frame has no numeric scalar column besides the keys and the pivot column")
        return pivot_agg(self, [AggregateExpression(FUNCTIONS[fn], n) for n in names], f"pivot.{fn}")

    def sum(self, *cols):
        """`agg(F.sum(c), ...)` of the named columns, or of every numeric scalar column that is no key or pivot."""
        return self._stat("sum", cols)

    def avg(self, *cols):
        """`agg(F.avg(c), ...)` of the named columns, or of every numeric scalar column that is no key or pivot."""
        return self._stat("avg", cols)

    mean = avg

    def min(self, *cols):
        """`agg(F.min(c), ...)` of the named float columns (integer columns: cast to double first)."""
        return self._stat("min", cols)

    def max(self, *cols):
        """`agg(F.max(c), ...)` of the named float columns (integer columns: cast to double first)."""
        return self._stat("max", cols)

    def __repr__(self):
        return f"PivotedData<groupBy({', '.join(self.keys)}) pivot({self.pivot_col}: {len(self.values)} values)>"


def pivot(grouped, pivot_col, values=None) -> PivotedData:
    """`GroupedData.pivot`: see there."""
    from .column import Column
    df, keys = grouped.df, list(grouped.keys)
    if isinstance(pivot_col, Column):
        if not pivot_col.is_reference:
            raise TypeError(f"pivot: '{pivot_col.output_name}' is a computed column; the pivot column is a column "
                            f"name or a plain column reference (add it with withColumn first)")
        if pivot_col.sort_order is not None:
            raise TypeError(f"pivot: '{pivot_col.output_name}.{pivot_col.sort_order}()' is a sort order, not a column")
        pivot_col = pivot_col._expr[1]
    if not isinstance(pivot_col, str):
        raise TypeError(f"pivot: a column name or a column reference is expected, got {type(pivot_col).__name__}")
    if pivot_col not in df.schema:
        raise ValueError(f"pivot: Column {pivot_col} not found in {df.columns}")
    if pivot_col in keys:
        raise ValueError(f"pivot: '{pivot_col}' is one of the grouping keys; the pivot column must be another column")
    _check_keys(df, keys + [pivot_col], "pivot")
    dt = np.dtype(D.numpy_dtype(_tf_dtype(df, pivot_col)))
    if values is None:
        vals = _discovered_values(df, pivot_col, dt)
    else:
        vals = _explicit_values(values, dt, pivot_col)
    _check_count(len(vals))
    return PivotedData(df, keys, pivot_col, vals)


def pivot_agg(pivoted: PivotedData, exprs: Sequence[Any], what: str):
    from ..utils.logging import metrics
    from .dataframe import DataFrame, _Derived, tensor_field
    from .order_agg import has_order_aggregates
    from .window import refuse_window_expression
    df, keys, pcol, values = pivoted.df, pivoted.keys, pivoted.pivot_col, pivoted.values
    refuse_window_expression(what, exprs)
    if has_order_aggregates(exprs):
        raise NotImplementedError(f"{what}: order aggregates (median, percentile, percentile_approx, mode, "
                                  f"countDistinct) are not supported under pivot; use groupBy({', '.join(keys + [pcol])})"
                                  f".agg(...) and reshape its result")
    specs = _specs(df, [], exprs, what)
    for s in specs:
        if s.fn in ("min", "max") and not _aggregate_dtype(df, s.fn, s.column).is_floating_point:
            raise ValueError(f"{what}: {s.fn}({s.column}) of an integer column has no value for a cell without rows "
                             f"(frames hold no nulls); cast the column first: "
                             f"withColumn(name, col('{s.column}').cast(\"double\"))")
    V = len(values)
    _check_count(V, len(specs))
    all_keys = keys + [pcol]
    texts = [_value_text(v) for v in values]
    names = [t if len(specs) == 1 else f"{t}_{s.name}" for t in texts for s in specs]
    seen = set(keys)
    for n in names:
        if n in seen:
            raise ValueError(f"{what}: the output column '{n}' appears twice (or is a key); use .alias() to rename "
                             f"an expression")
        seen.add(n)
    vcols, pairs = _columns_of(specs, what)
    single = any(s.pair is None for s in specs)
    vdt = ([D.torch_dtype(_tf_dtype(df, v)) for v in vcols] or [torch.uint8]) if single else []
    is_float = [t.is_floating_point for t in vdt]
    kdt = [D.torch_dtype(_tf_dtype(df, k)) for k in all_keys]
    out_dt = [torch.float64 if s.pair is not None else _aggregate_dtype(df, s.fn, s.column) for s in specs]
    fills = [_NAN_BITS[t] if t.is_floating_point else 0 for t in out_dt]
    scol = [vcols.index(s.column) if s.column is not None else 0 for s in specs]
    spair = [pairs.index(s.pair) if s.pair is not None else 0 for s in specs]
    needed = _needed(all_keys, vcols, pairs)
    keep_on_device = any(b.columns[n].is_cuda for b in (df._cached or {}).values() if b.nrows for n in needed
                         if isinstance(b.columns[n], torch.Tensor))
    world = max(1, dist.world_size())
    value_words = _words(values) if V else np.zeros(0, dtype=np.uint64)
    out_fields = [tensor_field(n, out_dt[i % len(specs)], []) for i, n in enumerate(names)]

    def empty():
        cols: Dict[str, Any] = {k: torch.empty(0, dtype=t) for k, t in zip(keys, kdt)}
        cols.update({n: torch.empty(0, dtype=out_dt[i % len(specs)]) for i, n in enumerate(names)})
        return {p: Block(0, dict(cols)) for p in dist.local_partitions(world)}

    def compute(blocks):
        if V == 0:  # (no rank had a row when the values were looked up)
            return empty()
        nparts = sum(1 for b in blocks.values() if b.nrows)
        got = _merged_records(blocks, all_keys, len(keys), vcols, pairs, single, kdt, is_float, needed, what)
        if got is None:
            return empty()
        on_device, ukeys, merged, pmerged = got
        metrics.add(f"pivot_{'device' if on_device else 'host'}_partitions", nparts)
        outs = _outputs(specs, scol, spair, vdt, merged, pmerged, on_device)
        gkeys, G, wide = _spread(on_device, list(ukeys[:-1]), ukeys[-1], value_words, outs, fills)
        metrics.add("pivot_cells", G * V * len(specs))
        keep = on_device and keep_on_device
        cols: Dict[str, Any] = {k: (u if keep else u.cpu()) for k, u in zip(keys, gkeys)}
        for j in range(V):
            for a in range(len(specs)):
                o = wide[a][j]
                cols[names[j * len(specs) + a]] = o if keep else o.cpu()
        return {dist.rank(): Block(G, cols)}

    def compute_agreed(blocks):
        return dist.agreed(what, lambda: compute(blocks))

    fields = [df.schema[k] for k in keys] + out_fields
    return DataFrame(StructType(fields), _Derived(df, compute_agreed, streamable=False), world)


def crosstab(df, col1, col2):
    """`DataFrame.stat.crosstab`: see there."""
    for c in (col1, col2):
        if not isinstance(c, str):
            raise TypeError(f"crosstab: column names are expected, got {type(c).__name__}")
        if c not in df.schema:
            raise ValueError(f"crosstab: Column {c} not found in {df.columns}")
    if col1 == col2:
        raise ValueError(f"crosstab: two different columns are expected, got '{col1}' twice")
    name = f"{col1}_{col2}"
    wide = df.groupBy(col1).pivot(col2).count()
    if name in wide.columns:
        raise ValueError(f"crosstab: the key column's name '{name}' is also the name of a value of '{col2}'")
    return wide.withColumnRenamed(col1, name)
