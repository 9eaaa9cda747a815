"""Window / WindowSpec and `.over()`: ranking functions and running
aggregates over the rows of a group, shaped as in `pyspark.sql.Window`.

    w = Window.partitionBy("id").orderBy(tfs.desc("score"))
    scored.withColumn("rn", F.row_number().over(w))

The frame is sorted globally by (partition keys ascending, order keys) with
orderBy's sample sort; the result holds the input's rows in that order (the
sort is stable), in the same number of partitions. Then

* every partition is scanned on its own: the words of its sorted key columns
  (`_C.sort_encode`, or numpy on the host), one segmented inclusive scan per
  channel forwards (`_C.window_scan`: the head index of the row's group and of
  its peer run, the count of peer heads, sums and extreme words of the value
  columns) and the two index channels in reverse (the last row of the group
  and of the peer run). Host partitions go through the numpy form below.
* every partition contributes one int64 record (its row count, the words of
  its first and last row, whether it is a single group, the rows and the
  partial of every channel of its first and of its last group) to an
  [nparts, ...] table that crosses ranks with one host all-reduce.
* every rank folds the records in ascending partition order, skipping empty
  partitions: the carry-in of a partition is the fold `carry (+) local` (the
  carry on the left) of the earlier pieces of its first group; the total of a
  group that runs past a partition's end is the fold over all its pieces.
* `_C.window_finish` (or numpy) applies the carry to the rows of the first
  group, gathers per frame (the row, its last peer, the group's last row or
  the folded total) and decodes to the typed output columns.

The sample sort cuts its slices at lower bounds of splitter tuples, so rows
with an equal full key tuple land in one partition: peers never span
partitions, groups may. The fold checks this and raises rather than produce
wrong range-frame values.

For a given input partitioning every output bit is the same for every world
size and from run to run; the ranking functions, counts, integer sums, min
and max do not depend on the partitioning either.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ..parallel import dist
from ..utils import dtypes as D
from ._scalar_columns import (_aggregate_dtype, _block_on_device, _decode_sort_word, _ineligible, _scalar_column,
                              _tf_dtype)
from .block import Block
from .column import Column, _describe

_MAX_CHANNELS = 16  # kernels.h kMaxPackCols: channels per scan, outputs per _C.window_finish call
_RANKING = ("row_number", "rank", "dense_rank")
_AGGREGATES = ("count", "sum", "avg", "min", "max")
_ROWS, _RANGE, _WHOLE = "rows", "range", "whole"
_OP_ADD_I64, _OP_ADD_F64, _OP_MIN, _OP_MAX = range(4)
_KIND_OP = {"group_head": _OP_MAX, "peer_head": _OP_MAX, "peer_count": _OP_ADD_I64, "sum_i64": _OP_ADD_I64,
            "sum_f64": _OP_ADD_F64, "min_word": _OP_MIN, "max_word": _OP_MAX}
_MASK = (1 << 64) - 1


# ------------------------------------------------------------------ the spec
class WindowSpec:
    """Partition keys, order keys and a frame; immutable, every method returns
    a new spec."""

    __slots__ = ("_partition", "_order", "_frame")

    def __init__(self, partition=(), order=(), frame=None):
        self._partition = tuple(partition)
        self._order = tuple(order)
        self._frame = frame  # None or (kind, start, end)

    @staticmethod
    def _flatten(cols) -> List[Any]:
        return [c for cs in cols for c in (cs if isinstance(cs, (list, tuple)) else [cs])]

    def partitionBy(self, *cols) -> "WindowSpec":  # noqa: N802
        keys = []
        for c in self._flatten(cols):
            if isinstance(c, Column):
                if not c.is_reference:
                    raise TypeError(f"Window.partitionBy: '{c.output_name}' is a computed Column; partition keys are "
                                    f"column names or plain column references (add it with withColumn first)")
                if c.sort_order is not None:
                    raise TypeError(f"Window.partitionBy: '{c.output_name}.{c.sort_order}()' is a sort order; "
                                    f"partition keys have none")
                c = c._expr[1]
            if not isinstance(c, str):
                raise TypeError(f"Window.partitionBy: a column name or a column reference is expected, got "
                                f"{type(c).__name__}")
            keys.append(c)
        return WindowSpec(keys, self._order, self._frame)

    def orderBy(self, *cols) -> "WindowSpec":  # noqa: N802
        keys = []
        for c in self._flatten(cols):
            if isinstance(c, str):
                c = Column._ref(c)
            if not isinstance(c, Column):
                raise TypeError(f"Window.orderBy: a column name or a Column is expected, got {type(c).__name__}")
            keys.append(c)
        return WindowSpec(self._partition, keys, self._frame)

    def _between(self, kind: str, start, end) -> "WindowSpec":
        for v in (start, end):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"Window.{kind}Between: integer bounds (or Window.unboundedPreceding, "
                                f"Window.unboundedFollowing, Window.currentRow) are expected, got {v!r}")
        return WindowSpec(self._partition, self._order, (kind, int(start), int(end)))

    def rowsBetween(self, start, end) -> "WindowSpec":  # noqa: N802
        return self._between("rows", start, end)

    def rangeBetween(self, start, end) -> "WindowSpec":  # noqa: N802
        return self._between("range", start, end)

    partition_by, order_by, rows_between, range_between = partitionBy, orderBy, rowsBetween, rangeBetween

    def _sort_identity(self) -> tuple:
        """What decides the sort: specs that agree on it share one."""
        return (self._partition,
                tuple((_describe(c._expr), c.sort_order == "desc") for c in self._order))

    def __repr__(self):
        order = ", ".join(_describe(c._expr) + (" DESC" if c.sort_order == "desc" else "") for c in self._order)
        return f"WindowSpec<partitionBy({', '.join(self._partition)}) orderBy({order}) frame={self._frame}>"


class Window:
    """`Window.partitionBy(...)`, `Window.orderBy(...)`, the frame bounds."""

    unboundedPreceding = -(1 << 63)  # noqa: N815
    unboundedFollowing = (1 << 63) - 1  # noqa: N815
    currentRow = 0  # noqa: N815

    @staticmethod
    def partitionBy(*cols) -> WindowSpec:  # noqa: N802
        return WindowSpec().partitionBy(*cols)

    @staticmethod
    def orderBy(*cols) -> WindowSpec:  # noqa: N802
        return WindowSpec().orderBy(*cols)

    @staticmethod
    def rowsBetween(start, end) -> WindowSpec:  # noqa: N802
        return WindowSpec().rowsBetween(start, end)

    @staticmethod
    def rangeBetween(start, end) -> WindowSpec:  # noqa: N802
        return WindowSpec().rangeBetween(start, end)

    partition_by, order_by, rows_between, range_between = partitionBy, orderBy, rowsBetween, rangeBetween


def _bound_name(v: int) -> str:
    if v <= Window.unboundedPreceding:
        return "unboundedPreceding"
    if v >= Window.unboundedFollowing:
        return "unboundedFollowing"
    return "currentRow" if v == 0 else str(v)


class WindowExpression:
    """`fn` (a ranking function or an aggregate of `column`) over `spec`. It
    is no Column: only `DataFrame.withColumn` and `DataFrame.select` take it."""

    __slots__ = ("fn", "column", "spec", "_alias", "frame")

    def __init__(self, fn: str, column: Optional[str], spec: WindowSpec, alias: Optional[str] = None):
        if not isinstance(spec, WindowSpec):
            raise TypeError(f"{fn}().over: a WindowSpec is expected (Window.partitionBy(...), Window.orderBy(...)), "
                            f"got {type(spec).__name__}")
        self.fn, self.column, self.spec, self._alias = fn, column, spec, alias
        self.frame = None
        _resolve_frame(self)  # (the refusals that need no frame of rows are raised where the expression is written)

    def alias(self, name: str) -> "WindowExpression":
        if not isinstance(name, str) or not name:
            raise TypeError(f"alias: a non-empty column name is expected, got {name!r}")
        return WindowExpression(self.fn, self.column, self.spec, name)

    name = alias

    @property
    def has_alias(self) -> bool:
        return self._alias is not None

    @property
    def output_name(self) -> str:
        if self._alias is not None:
            return self._alias
        arg = "" if self.fn in _RANKING else (self.column if self.column is not None else "1")
        return f"{self.fn}({arg}) OVER (...)"

    def __repr__(self):
        return f"WindowExpression<{self.output_name}>"

    def _refuse(self, *_a, **_k):
        raise TypeError(f"'{self.output_name}' is a window expression: it belongs in DataFrame.withColumn(name, ...) "
                        f"or DataFrame.select(...); add it as a column first, then compute with that column")

    __add__ = __radd__ = __sub__ = __rsub__ = __mul__ = __rmul__ = __truediv__ = __rtruediv__ = _refuse
    __neg__ = __invert__ = __and__ = __rand__ = __or__ = __ror__ = _refuse
    __lt__ = __le__ = __gt__ = __ge__ = _refuse
    __eq__ = __ne__ = _refuse  # type: ignore[assignment]
    __hash__ = None  # type: ignore[assignment]
    __bool__ = _refuse


def refuse_window_expression(what: str, items: Sequence[Any]) -> None:
    """The TypeError of an operator that is given a window expression (or a
    random expression, frame/sampling.py: the same rule)."""
    from .sampling import refuse_random_expression
    refuse_random_expression(what, items)
    for it in items:
        for x in (it if isinstance(it, (list, tuple)) else [it]):
            if isinstance(x, WindowExpression):
                raise TypeError(f"{what}: '{x.output_name}' is a window expression; it belongs in "
                                f"DataFrame.withColumn(name, ...) or DataFrame.select(...). Add it as a column "
                                f"first, then use that column in {what}")


def _resolve_frame(e: "WindowExpression") -> str:
    spec = e.spec
    ordered = bool(spec._order)
    if e.fn in _RANKING:
        if not ordered:
            raise ValueError(f"{e.fn}().over: a ranking function needs an orderBy in its window spec")
        if spec._frame is not None:
            raise ValueError(f"{e.fn}().over: a ranking function takes no frame; drop "
                             f"{spec._frame[0]}Between from the spec")
        e.frame = _ROWS
        return e.frame
    if spec._frame is None:
        e.frame = _RANGE if ordered else _WHOLE
        return e.frame
    kind, start, end = spec._frame
    if start <= Window.unboundedPreceding and end >= Window.unboundedFollowing:
        e.frame = _WHOLE
    elif start <= Window.unboundedPreceding and end == Window.currentRow:
        # (without order keys every row of the group is a peer of every other)
        e.frame = _ROWS if kind == "rows" else (_RANGE if ordered else _WHOLE)
    else:
        raise NotImplementedError(
            f"{e.fn}().over: the frame {kind}Between({_bound_name(start)}, {_bound_name(end)}) is not supported; "
            f"the frames are (unboundedPreceding, currentRow) by rows or by range and (unboundedPreceding, "
            f"unboundedFollowing)")
    return e.frame


# ------------------------------------------------------------------ the scan on the host
def _seg_accumulate(ufunc, x: np.ndarray, heads: np.ndarray) -> np.ndarray:
    """ufunc.accumulate over every group on its own, in row order."""
    out = x.copy()
    n = len(x)
    starts = np.nonzero(heads)[0]
    ends = np.append(starts[1:], n)
    for a, b in zip(starts[ends - starts > 1].tolist(), ends[ends - starts > 1].tolist()):
        out[a:b] = ufunc.accumulate(x[a:b])
    return out


def _host_channel_input(kind: str, col: torch.Tensor) -> np.ndarray:
    from .dataframe import _host_sort_words
    a = col.detach().cpu().contiguous().numpy()
    if kind == "sum_i64":
        return a.astype(np.int64)
    if kind == "sum_f64":
        return a.astype(np.float64)
    return _host_sort_words(col, False)


def _host_scan(words: np.ndarray, P: int, kinds: Sequence[str], cols: Sequence[torch.Tensor]):
    """(fwd int64 [C, n], rev int64 [2, n]): `_C.window_scan` forwards over all
    channels and in reverse over the two index channels, in numpy. Float sums
    add in row order."""
    W, n = words.shape
    idx = np.arange(n, dtype=np.int64)
    ghead = np.zeros(n, dtype=bool)
    phead = np.zeros(n, dtype=bool)
    if n:
        for w in range(W):
            d = words[w, 1:] != words[w, :-1]
            phead[1:] |= d
            if w < P:
                ghead[1:] |= d
        ghead[0] = phead[0] = True
    gh = np.maximum.accumulate(np.where(ghead, idx, 0)) if n else idx
    ph = np.maximum.accumulate(np.where(phead, idx, 0)) if n else idx
    glast = np.append(ghead[1:], True) if n else ghead
    plast = np.append(phead[1:], True) if n else phead
    gl = np.minimum.accumulate(np.where(glast, idx, n - 1)[::-1])[::-1] if n else idx
    pl = np.minimum.accumulate(np.where(plast, idx, n - 1)[::-1])[::-1] if n else idx
    fwd = np.zeros((len(kinds), n), dtype=np.int64)
    used = 0
    for c, kind in enumerate(kinds):
        if kind == "group_head":
            fwd[c] = gh
        elif kind == "peer_head":
            fwd[c] = ph
        elif kind == "peer_count":
            cs = np.cumsum(phead.astype(np.int64))
            fwd[c] = cs - cs[gh] + 1 if n else cs
        else:
            x = _host_channel_input(kind, cols[used])
            used += 1
            if not n:
                continue
            if kind == "sum_i64":
                cs = np.cumsum(x)  # (int64: wraps)
                fwd[c] = cs - (cs[gh] - x[gh])
            elif kind == "sum_f64":
                with np.errstate(all="ignore"):
                    fwd[c] = _seg_accumulate(np.add, x, ghead).view(np.int64)
            else:
                fwd[c] = _seg_accumulate(np.minimum if kind == "min_word" else np.maximum, x, ghead).view(np.int64)
    return fwd, np.stack([gl, pl], 0)


def _comb(op: int, a: int, b: int) -> int:
    """carry (+) local on 64-bit patterns (Python ints in [0, 2^64)), `a` the
    earlier rows: the arithmetic of kernels/window_scan.hip comb."""
    if op == _OP_ADD_I64:
        return (a + b) & _MASK
    if op == _OP_ADD_F64:
        with np.errstate(all="ignore"):
            s = np.array([a], dtype=np.uint64).view(np.float64) + np.array([b], dtype=np.uint64).view(np.float64)
        return int(s.view(np.uint64)[0])
    return min(a, b) if op == _OP_MIN else max(a, b)


def _comb_array(op: int, a: int, v: np.ndarray) -> np.ndarray:
    """carry (+) every element of the int64 patterns v."""
    if op == _OP_ADD_I64:
        return v + np.array([a], dtype=np.uint64).view(np.int64)[0]
    if op == _OP_ADD_F64:
        with np.errstate(all="ignore"):
            return (np.array([a], dtype=np.uint64).view(np.float64)[0] + v.view(np.float64)).view(np.int64)
    u = v.view(np.uint64)
    return (np.minimum(u, np.uint64(a)) if op == _OP_MIN else np.maximum(u, np.uint64(a))).view(np.int64)


def _signed(u: int) -> int:
    return u - (1 << 64) if u >= (1 << 63) else u


def _host_finish(fwd: np.ndarray, rev: np.ndarray, kinds: Sequence[str], carry: Sequence[int], total: Sequence[int],
                 has_carry: bool, has_total: bool, carry_rows: int, total_rows: int, fns: Sequence[str],
                 frames: Sequence[str], chans: Sequence[int], dtypes: Sequence[torch.dtype]) -> List[torch.Tensor]:
    """`_C.window_finish` in numpy."""
    n = fwd.shape[1]
    idx = np.arange(n, dtype=np.int64)
    gh, ph, gl, pl = fwd[0], fwd[1], rev[0], rev[1]
    first = (gh == 0) if has_carry else np.zeros(n, dtype=bool)
    is_open = (gl == n - 1) if has_total else np.zeros(n, dtype=bool)
    before = np.where(first, np.int64(carry_rows), np.int64(0))
    outs: List[torch.Tensor] = []
    for fn, fr, c, dt in zip(fns, frames, chans, dtypes):
        if fn == "row_number":
            outs.append(torch.from_numpy((idx - gh + 1 + before).astype(np.int32)))
            continue
        if fn == "rank":
            outs.append(torch.from_numpy((ph - gh + 1 + before).astype(np.int32)))
            continue
        t = idx if fr == _ROWS else (pl if fr == _RANGE else gl)
        whole = is_open if fr == _WHOLE else np.zeros(n, dtype=bool)
        rows = np.where(whole, np.int64(total_rows), t - gh + 1 + before)
        if fn == "count":
            outs.append(torch.from_numpy(rows.astype(np.int64)))
            continue
        op = _KIND_OP[kinds[c]]
        v = fwd[c][t] if n else fwd[c]
        v = np.where(first, _comb_array(op, carry[c], v), v)
        v = np.where(whole, np.array([total[c]], dtype=np.uint64).view(np.int64)[0], v).astype(np.int64)
        if fn == "dense_rank":
            o = v.astype(np.int32)
        elif fn == "sum":
            o = v if kinds[c] == "sum_i64" else v.view(np.float64)
        elif fn == "avg":
            with np.errstate(all="ignore"):
                o = v.view(np.float64) / rows.astype(np.float64)
        else:
            np_dt = torch.empty(0, dtype=dt).numpy().dtype
            o = np.asarray(_decode_sort_word(v.view(np.uint64), np_dt)).reshape(-1).astype(np_dt)
        outs.append(torch.from_numpy(np.ascontiguousarray(o)))
    return outs


# ------------------------------------------------------------------ the fold
def _fold(table: np.ndarray, W: int, P: int, kinds: Sequence[str]):
    """table int64 [nparts, 4 + 2 W + 2 C]: per partition nrows, single group,
    rows of the first group, rows of the last group, the words of the first
    and of the last row, the partials of the first and of the last group.
    -> per partition (has_carry, has_total, carry_rows, total_rows,
    carry [C], total [C]) as Python ints, the patterns unsigned; the fold runs
    in ascending partition order over the partitions that hold rows."""
    nparts = table.shape[0]
    C = len(kinds)
    ops = [_KIND_OP[k] for k in kinds]
    u = table.view(np.uint64)
    res = [dict(has_carry=False, has_total=False, carry_rows=0, total_rows=0, carry=[0] * C, total=[0] * C)
           for _ in range(nparts)]
    open_key = None   # the first P words of the group that is still open
    last_row = None   # all W words of the last row seen
    acc_rows, acc = 0, [0] * C
    span: List[int] = []  # the partitions whose last group is the open one

    def close():
        # (in the last partition of the span the group ends: there its value is carry (+) local)
        for q in span[:-1]:
            res[q].update(has_total=True, total_rows=acc_rows, total=list(acc))

    for p in range(nparts):
        nrows = int(table[p, 0])
        if nrows == 0:
            continue
        single = bool(table[p, 1])
        first_rows, last_rows = int(table[p, 2]), int(table[p, 3])
        fw = [int(x) for x in u[p, 4:4 + W]]
        lw = [int(x) for x in u[p, 4 + W:4 + 2 * W]]
        fpart = [int(x) for x in u[p, 4 + 2 * W:4 + 2 * W + C]]
        lpart = [int(x) for x in u[p, 4 + 2 * W + C:4 + 2 * W + 2 * C]]
        if W > P and last_row is not None and fw == last_row:
            raise RuntimeError(f"window: internal error: the rows at the end of an earlier partition and at the "
                               f"start of partition {p} have equal keys, so a peer run spans partitions; the "
                               f"sort is expected to keep equal key tuples in one partition")
        continues = open_key is not None and fw[:P] == open_key
        if continues:
            res[p].update(has_carry=True, carry_rows=acc_rows, carry=list(acc))
            acc_rows += first_rows
            acc = [_comb(op, a, b) for op, a, b in zip(ops, acc, fpart)]
            span.append(p)
        if not (continues and single):  # the open group ends before this partition's last group
            if span:
                close()
            span, acc_rows, acc = [p], last_rows, list(lpart)
        open_key, last_row = lw[:P], lw
    if span:
        close()
    return res


# ------------------------------------------------------------------ planning
class _Plan:
    """The channels and outputs of the expressions that share one sort."""

    def __init__(self):
        self.kinds: List[str] = ["group_head", "peer_head"]
        self.cols: List[Optional[str]] = [None, None]
        self.fns: List[str] = []
        self.frames: List[str] = []
        self.chans: List[int] = []
        self.vcols: List[Optional[str]] = []
        self.names: List[str] = []

    def channel(self, kind: str, col: Optional[str]) -> int:
        for c, (k, v) in enumerate(zip(self.kinds, self.cols)):
            if k == kind and v == col:
                return c
        self.kinds.append(kind)
        self.cols.append(col)
        return len(self.kinds) - 1


def _out_dtype(df, e: WindowExpression) -> torch.dtype:
    # (the ranking functions exist over a window only; the aggregates follow groupBy().agg)
    return torch.int32 if e.fn in _RANKING else _aggregate_dtype(df, e.fn, e.column)


def _device_cached(df) -> bool:
    """A frame cached on the device: its window columns are computed there and
    the result stays there, also when an exchange between ranks staged the
    sorted rows through the host."""
    return any(isinstance(c, torch.Tensor) and c.is_cuda for b in (df._cached or {}).values() if b.nrows
               for c in b.columns.values())


def _window_frame(df, spec: WindowSpec, outs: Sequence[Tuple[str, WindowExpression]], what: str,
                  keep_on_device: bool = False):
    """The lazy frame of `df`'s columns plus one column per (name, expression)
    of `outs`, all over the keys of `spec` (their frames may differ), in the
    defined row order."""
    from .. import core, engine
    from ..utils.logging import metrics
    from .dataframe import DataFrame, _Derived, _host_sort_words, _sort_frame, tensor_field
    pkeys = list(spec._partition)
    for k in pkeys:
        if k not in df.schema:
            raise ValueError(f"{what}: the partition key {k} is not found in {df.columns}")
    # computed order keys become temporary columns, as in orderBy
    okeys: List[str] = []
    desc: List[bool] = []
    extra: List[Column] = []
    taken = set(df.columns) | {n for n, _ in outs}
    for c in spec._order:
        desc.append(c.sort_order == "desc")
        if c.is_reference:
            if c._expr[1] not in df.schema:
                raise ValueError(f"{what}: the order key {c._expr[1]} is not found in {df.columns}")
            okeys.append(c._expr[1])
        else:
            k = 0
            while f"tfa_sort_key_{k}" in taken:
                k += 1
            taken.add(f"tfa_sort_key_{k}")
            okeys.append(f"tfa_sort_key_{k}")
            extra.append(Column(c._expr, f"tfa_sort_key_{k}"))
    plan = _Plan()
    for name, e in outs:
        if e.column is not None:
            if e.column not in df.schema:
                raise ValueError(f"{what}: Column {e.column} not found in {df.columns}")
            if e.fn != "count":
                err = _ineligible(df, e.column, what)
                if err is not None:
                    raise err
        col = e.column if e.fn != "count" else None
        if e.fn == "dense_rank":
            ch = plan.channel("peer_count", None)
        elif e.fn == "sum":
            fl = D.torch_dtype(_tf_dtype(df, col)).is_floating_point
            ch = plan.channel("sum_f64" if fl else "sum_i64", col)
        elif e.fn == "avg":
            ch = plan.channel("sum_f64", col)
        elif e.fn in ("min", "max"):
            ch = plan.channel(f"{e.fn}_word", col)
        else:
            ch = 0
        plan.fns.append(e.fn)
        plan.frames.append(e.frame)
        plan.chans.append(ch)
        plan.vcols.append(col)
        plan.names.append(name)
    if len(plan.kinds) > _MAX_CHANNELS:
        raise ValueError(f"{what}: the window expressions over one spec need {len(plan.kinds)} scan channels, at "
                         f"most {_MAX_CHANNELS} fit one call; split the call")
    base = df._select_columns(list(df.columns) + extra) if extra else df
    keys = pkeys + okeys
    P, W = len(pkeys), len(keys)
    if keys:
        srt = _sort_frame(base, [Column._ref(k).asc() for k in pkeys] +
                          [Column._ref(k).desc() if d else Column._ref(k).asc() for k, d in zip(okeys, desc)],
                          True, True, what)
    else:
        srt = base
    kdesc = [False] * P + desc
    out_dt = [_out_dtype(df, e) for _, e in outs]
    vdt = [D.torch_dtype(_tf_dtype(df, v)) if v is not None else torch.uint8 for v in plan.vcols]
    value_cols = [c for c in plan.cols if c is not None]
    needed = keys + [v for v in value_cols if v not in keys]
    nparts = df.num_partitions
    C = len(plan.kinds)
    width = 4 + 2 * W + 2 * C

    def scan_block(b: Block):
        """(on_device, fwd, rev, record) of one partition with rows."""
        n = b.nrows
        kcols = [_scalar_column(b, k, what) for k in keys]
        vals = [_scalar_column(b, v, what) for v in value_cols]
        on_device = engine.gpu_available() and _block_on_device(b, needed)
        rec = np.zeros(width, dtype=np.int64)
        if on_device:
            from .._native import _C
            dev = kcols[0].device
            words = _C.sort_encode([k.contiguous() for k in kcols], kdesc) if W else \
                torch.empty((0, n), dtype=torch.int64, device=dev)
            fwd = _C.window_scan(words, P, False, plan.kinds, [v.contiguous() for v in vals])
            rev = _C.window_scan(words, P, True, plan.kinds[:2], [])
            ends = torch.stack([rev[0, 0], rev[0, 0].new_tensor(n - 1)])
            small = torch.cat([rev[0, :1], fwd[0, n - 1:], words[:, 0], words[:, n - 1],
                               fwd.index_select(1, ends).t().reshape(-1)]).cpu().numpy()
            metrics.add("window_device_partitions")
        else:
            words_h = np.stack([_host_sort_words(k, d) for k, d in zip(kcols, kdesc)], 0) if W else \
                np.zeros((0, n), dtype=np.uint64)
            fwd, rev = _host_scan(words_h, P, plan.kinds, vals)
            e0 = int(rev[0, 0])
            small = np.concatenate([rev[0, :1], fwd[0, n - 1:], words_h[:, 0].view(np.int64),
                                    words_h[:, n - 1].view(np.int64), fwd[:, e0], fwd[:, n - 1]])
            metrics.add("window_host_partitions")
        e0, last_head = int(small[0]), int(small[1])
        rec[0], rec[1], rec[2], rec[3] = n, int(e0 == n - 1), e0 + 1, n - last_head
        rec[4:] = small[2:]
        return on_device, fwd, rev, rec

    def compute(blocks: Dict[int, Block]) -> Dict[int, Block]:
        rng = torch.cuda.is_initialized()
        if rng:
            torch.cuda.nvtx.range_push("tfa.window")
        try:
            if keep_on_device and engine.gpu_available():
                # (an exchange between ranks may have staged the sorted rows through the host)
                blocks = {pid: b.to(engine.compute_device()) for pid, b in blocks.items()}
            table = torch.zeros((nparts, width), dtype=torch.int64)
            scans = {}
            rows = 0
            for pid in sorted(blocks):
                b = blocks[pid]
                if b.nrows:
                    scans[pid] = scan_block(b)
                    table[pid] = torch.from_numpy(scans[pid][3])
                    rows += b.nrows
            dist.all_reduce_host_(table, "Sum")  # (every rank fills the rows of its own partitions)
            tab = table.numpy()
            if int(tab[:, 0].sum()) >= (1 << 31) and any(f in _RANKING for f in plan.fns):
                raise ValueError(f"{what}: the ranking functions are int32, as in Spark; a frame of "
                                 f"{int(tab[:, 0].sum())} rows does not fit")
            folded = _fold(tab, W, P, plan.kinds)
            res: Dict[int, Block] = {}
            for pid in sorted(blocks):
                b = blocks[pid]
                cols = dict(b.columns)
                if not b.nrows:
                    ref = next((c for c in b.columns.values() if isinstance(c, torch.Tensor)), None)
                    dev = ref.device if ref is not None else torch.device("cpu")
                    cols.update({nm: torch.empty(0, dtype=t, device=dev) for nm, t in zip(plan.names, out_dt)})
                    res[pid] = Block(0, cols)
                    continue
                on_device, fwd, rev, _ = scans[pid]
                f = folded[pid]
                made: List[torch.Tensor] = []
                for a in range(0, len(plan.fns), _MAX_CHANNELS):
                    sl = slice(a, a + _MAX_CHANNELS)
                    args = (plan.kinds, f["carry"], f["total"], f["has_carry"], f["has_total"], f["carry_rows"],
                            f["total_rows"], plan.fns[sl], plan.frames[sl], plan.chans[sl], vdt[sl])
                    if on_device:
                        from .._native import _C
                        made.extend(_C.window_finish(fwd, rev, plan.kinds, [_signed(x) for x in f["carry"]],
                                                     [_signed(x) for x in f["total"]], *args[3:]))
                    else:
                        made.extend(_host_finish(fwd, rev, *args))
                cols.update(zip(plan.names, made))
                res[pid] = Block(b.nrows, cols)
        finally:
            if rng:
                torch.cuda.nvtx.range_pop()
        metrics.add("window_rows", rows)
        metrics.add("window_scan_passes", 2 * len(scans))
        return res

    def compute_agreed(blocks):
        return dist.agreed(what, lambda: compute(blocks))

    from .types import StructType
    fields = list(srt.schema.fields) + [tensor_field(nm, t, []) for nm, t in zip(plan.names, out_dt)]
    out = DataFrame(StructType(fields), _Derived(srt, compute_agreed, streamable=False), nparts)
    if extra:
        keep = [c for c in out.columns if not any(c == x.output_name for x in extra)]
        out = out._project([(c, c) for c in keep])
    return out


def apply_windows(df, items: Sequence[Tuple[str, Any]], what: str):
    """`items`: (output name, column name | WindowExpression) in output order.
    The expressions that share a sort are evaluated together, the groups one
    after the other; the result is projected to `items`."""
    groups: List[Tuple[WindowSpec, List[Tuple[str, WindowExpression]]]] = []
    tmp: Dict[int, str] = {}
    taken = set(df.columns) | {n for n, _ in items}
    k = 0
    for i, (_, it) in enumerate(items):
        if not isinstance(it, WindowExpression):
            continue
        while f"tfa_window_{k}" in taken:
            k += 1
        tmp[i] = f"tfa_window_{k}"
        taken.add(tmp[i])
        ident = it.spec._sort_identity()
        for spec, members in groups:
            if spec._sort_identity() == ident:
                members.append((tmp[i], it))
                break
        else:
            groups.append((it.spec, [(tmp[i], it)]))
    cur = df
    keep_on_device = _device_cached(df)
    for spec, members in groups:
        cur = _window_frame(cur, spec, members, what, keep_on_device)
    return cur._project([(tmp[i] if i in tmp else it, name) for i, (name, it) in enumerate(items)])
