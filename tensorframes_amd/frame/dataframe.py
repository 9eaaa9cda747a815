"""A partitioned, lazily evaluated columnar DataFrame (the Spark substrate).

TensorFrames runs on Spark DataFrames (reference: README.md:3-9); Spark is not
available here, so this module provides the subset of DataFrame behaviour the
TensorFrames operators rely on (reference: SURVEY.md §2.4):

* a schema of `StructField`s whose metadata carries tensor shape/type info;
* an ordered list of partitions; operators are lazy and run when an action
  (`collect`, `count`, `first`, ...) forces them;
* `groupBy(...)` for keyed aggregation, `repartition`, `cache`/`persist`;
* SPMD distribution: under torch.distributed every rank holds the partitions
  ``p % world_size == rank``; actions gather results to every rank.

Dense numeric columns are stored as one tensor per partition (see block.py),
which can live in page-locked host memory (DMA source/target) or, after
`cache_on_device()`, in HBM.
"""
from __future__ import annotations

import math
import numbers
from typing import Any, Callable, Dict, Iterable, List, Optional, Sequence, Union

import numpy as np
import torch

from ..parallel import dist
from ..utils import dtypes as D
from .block import (Block, ObjectColumn, RaggedColumn, StringColumn, build_column, build_rows, column_values, concat_blocks,
                    is_dense)
from .column import Column, compile_expressions
from .column_info import ColumnInformation, DataFrameInfo, explain_schema
from .sampling import RandomExpression, refuse_random_expression
from .window import WindowExpression, refuse_window_expression
from .types import (ArrayType, BinaryType, BooleanType, DataType, DoubleType, FloatType, IntegerType,
                    LongType, NumericType, Row, StringType, StructField, StructType, scalar_type_of)


# ------------------------------------------------------------------ sources
class _Source:
    def compute(self) -> Dict[int, Block]:
        raise NotImplementedError


class _Materialized(_Source):
    def __init__(self, blocks: Dict[int, Block]):
        self._blocks = blocks

    def compute(self):
        return self._blocks


class _Failed(_Source):
    """A frame whose (eager) computation failed on this rank: the error is
    raised when an action evaluates it, inside the action's agreed local phase
    (parallel/dist.agreed), so every rank raises together."""

    def __init__(self, err: BaseException):
        self._err = err

    def compute(self):
        raise self._err


class _Generated(_Source):
    def __init__(self, num_partitions: int, fn: Callable[[int], Block]):
        self._n = num_partitions
        self._fn = fn

    def compute(self):
        return {p: self._fn(p) for p in dist.local_partitions(self._n)}


class _Derived(_Source):
    """Partitions computed from the parent's. `fn` maps any subset of the
    parent's local blocks {pid: block} to the same pids; when `streamable`,
    actions may evaluate partition by partition (bounded memory)."""

    def __init__(self, parent: "DataFrame", fn: Callable[[Dict[int, Block]], Dict[int, Block]],
                 streamable: bool = True):
        self._parent = parent
        self._fn = fn
        self.streamable = streamable

    def compute(self):
        return self._fn(self._parent._blocks())

    def iterate(self):
        """Streams the parent's partitions through fn in small groups: up to
        `Config.stream_group_bytes` of input per call, so a pipelined engine
        call spans several partitions (one H2D ramp-up per group, not per
        partition) while memory stays bounded."""
        from ..config import config
        from .. import engine
        group: Dict[int, Block] = {}
        nbytes = 0
        pending = None  # (group, results, completion handles) enqueued, not yet waited
        progs = set()
        try:
            for pid, b in self._parent._iter_blocks():
                group[pid] = b
                nbytes += _block_bytes(b)
                if nbytes >= config.stream_group_bytes or len(group) >= _MAX_GROUP_PARTITIONS:
                    # enqueue this group, THEN wait for (and hand out) the
                    # previous one: the chunk pipeline never drains between groups
                    nxt = self._start_group(group, progs)
                    if pending is not None:
                        yield from self._finish_group(pending)
                    pending = nxt
                    group, nbytes = {}, 0
            if group:
                nxt = self._start_group(group, progs)
                if pending is not None:
                    yield from self._finish_group(pending)
                pending = nxt
            if pending is not None:
                done, pending = pending, None
                yield from self._finish_group(done)
        finally:
            if pending is not None:
                engine.wait_pipelines(pending[2])
            for prog in progs:
                prog.release_pipeline()

    def _start_group(self, group: Dict[int, Block], progs: set):
        from .. import engine
        with engine.deferred_pipelines() as handles:
            res = self._fn(group)
        progs.update(h[0] for h in handles)
        return group, res, list(handles)

    def _finish_group(self, pending):
        from .. import engine
        group, res, handles = pending
        engine.wait_pipelines(handles)
        for pid in sorted(group):
            yield pid, res[pid]


class _Union(_Source):
    """The partitions of two parents side by side (DataFrame.union): the left
    parent's partition q stays q, the right parent's partition p becomes
    n1 + p, its columns under the left parent's names (`relabel`: a new Block
    over the same column objects; nothing is copied). Ownership is
    p % world: when world == 1 or n1 % world == 0 the right parent's blocks
    stay where they are and the source streams; otherwise one exchange moves
    each of them whole to the owner of n1 + p (collective: not streamable)."""

    def __init__(self, left: "DataFrame", right: "DataFrame", relabel: Callable[[Block], Block],
                 keep_on_device: bool = False):
        self._left = left
        self._right = right
        self._relabel = relabel
        self._keep_on_device = keep_on_device  # the right parent is device-resident: what the exchange staged goes back

    @property
    def streamable(self) -> bool:
        w = dist.world_size()
        return w == 1 or self._left.num_partitions % w == 0

    def compute(self):
        n1, n2 = self._left.num_partitions, self._right.num_partitions
        if self.streamable:
            res = dict(self._left._blocks())
            res.update({n1 + p: self._relabel(b) for p, b in self._right._blocks().items()})
            return res

        def exchange():
            from .. import engine
            from ..parallel import frame_comm
            res = dict(self._left._blocks())
            right = {p: self._relabel(b) for p, b in self._right._blocks().items()}
            counts = frame_comm.partition_rows({p: b.nrows for p, b in right.items()}, n2)
            pieces = {p: ([(n1 + p, 0, counts[p])] if counts[p] else []) for p in range(n2)}
            schema = self._left.schema
            got = frame_comm.exchange_pieces(right, schema.names, schema, n1 + n2, pieces)
            got = {q: b for q, b in got.items() if q >= n1}
            if self._keep_on_device and engine.gpu_available():
                got = {q: b.to(engine.compute_device()) for q, b in got.items()}
            res.update(got)
            return res
        return dist.agreed("union", exchange)

    def iterate(self):
        n1 = self._left.num_partitions
        yield from self._left._iter_blocks()
        for p, b in self._right._iter_blocks():
            yield n1 + p, self._relabel(b)


_MAX_GROUP_PARTITIONS = 16  # bound for columns whose size is only estimated


def _block_bytes(b: Block) -> int:
    """Bytes of the block's tensor columns; other columns (strings, ragged
    cells) count 64 bytes per row."""
    n = 0
    for c in b.columns.values():
        n += c.numel() * c.element_size() if isinstance(c, torch.Tensor) else 64 * b.nrows
    return n


# ------------------------------------------------------------------ DataFrame
class DataFrame:
    def __init__(self, schema: StructType, source: _Source, num_partitions: int):
        self._schema = schema
        self._source = source
        self._nparts = num_partitions
        self._persist = False
        self._cached: Optional[Dict[int, Block]] = None

    # -- metadata
    @property
    def schema(self) -> StructType:
        return self._schema

    @property
    def columns(self) -> List[str]:
        return self._schema.names

    @property
    def dtypes(self):
        return [(f.name, f.dataType.simpleString()) for f in self._schema.fields]

    @property
    def num_partitions(self) -> int:
        return self._nparts

    def getNumPartitions(self) -> int:  # noqa: N802
        return self._nparts

    @property
    def rdd(self):
        return self  # `df.rdd.getNumPartitions()` compatibility

    def __repr__(self):
        return "DataFrame[" + ", ".join(f"{n}: {t}" for n, t in self.dtypes) + "]"

    def printSchema(self):  # noqa: N802
        print(explain_schema(self._schema), end="")

    # -- columns
    def __getattr__(self, name: str) -> Column:
        # only reached when the ordinary lookup fails: answers for schema names
        # alone, and not before `_schema` exists (copy / pickle probe a blank
        # instance for dunder methods; asking `self._schema` here would recurse)
        schema = self.__dict__.get("_schema")
        if schema is None or name.startswith("__") or name not in schema:
            raise AttributeError(f"'{type(self).__name__}' object has no attribute '{name}'")
        return Column._ref(name, schema[name])

    def __getitem__(self, item):
        """`df["x"]` -> Column; `df[["a", "b"]]` -> select; `df[predicate]` -> filter."""
        if isinstance(item, str):
            if item not in self._schema:
                raise ValueError(f"Column {item} not found in {self.columns}")
            return Column._ref(item, self._schema[item])
        if isinstance(item, Column):
            return self.filter(item)
        if isinstance(item, (list, tuple)):
            return self.select(*item)
        if isinstance(item, numbers.Integral) and not isinstance(item, bool):
            if not -len(self._schema.fields) <= item < len(self._schema.fields):
                raise IndexError(f"column index {item} out of range for {len(self._schema.fields)} columns")
            f = self._schema.fields[item]
            return Column._ref(f.name, f)
        raise TypeError(f"DataFrame[...] takes a column name, a list of columns or a boolean Column, "
                        f"got {type(item).__name__}")

    def explain_tensors(self) -> str:
        """`DataFrame[double[?,2], ...]` (reference: src/main/scala/org/tensorframes/DataFrameInfo.scala:10-17)."""
        return DataFrameInfo.get(self._schema).explain()

    explainTensors = explain_tensors  # noqa: N815

    # -- evaluation
    def _blocks(self) -> Dict[int, Block]:
        if self._cached is not None:
            return self._cached
        b = self._source.compute()
        if self._persist:
            self._cached = b
        return b

    def _iter_blocks(self):
        """Local (pid, block) pairs in pid order, streamed through generated and
        streamable derived sources so only a bounded group of partitions
        (`Config.stream_group_bytes`) is alive at a time."""
        if self._cached is not None or self._persist:
            blocks = self._blocks()
            for pid in sorted(blocks):
                yield pid, blocks[pid]
            return
        src = self._source
        if isinstance(src, _Generated):
            for p in dist.local_partitions(src._n):
                yield p, src._fn(p)
        elif isinstance(src, _Derived) and src.streamable:
            yield from src.iterate()
        elif isinstance(src, _Union) and src.streamable:
            yield from src.iterate()
        else:
            blocks = self._blocks()
            for pid in sorted(blocks):
                yield pid, blocks[pid]

    def foreach_block(self, fn: Callable[[int, Block], Any]) -> List[Any]:
        """Applies fn(pid, block) to every local partition, streaming (an action)."""
        return [fn(pid, b) for pid, b in self._iter_blocks()]

    def to_arrow(self):
        """All rows as a `pyarrow.Table` (frame/arrow_io.py)."""
        from .arrow_io import to_arrow
        return to_arrow(self)

    def write_parquet(self, path: str, row_group_rows: int = 1 << 20) -> str:
        """One Parquet file per partition under `path` (frame/arrow_io.py)."""
        from .arrow_io import write_parquet
        return write_parquet(self, path, row_group_rows)

    def write_checkpoint(self, path: str) -> str:
        """Write every partition + the schema under `path` (see frame/checkpoint.py)."""
        from .checkpoint import write_checkpoint
        return write_checkpoint(self, path)

    def cache(self) -> "DataFrame":
        self._persist = True
        return self

    def persist(self, *_args) -> "DataFrame":
        return self.cache()

    def unpersist(self) -> "DataFrame":
        self._persist = False
        self._cached = None
        return self

    def cache_on_device(self, device=None) -> "DataFrame":
        """Device-resident copy: dense columns moved to HBM once, reused by every
        following operator (iterative workloads do not re-cross PCIe)."""
        from ..engine import compute_device
        dev = torch.device(device) if device is not None else compute_device()
        blocks = {p: b.to(dev) for p, b in self._blocks().items()}
        df = DataFrame(self._schema, _Materialized(blocks), self._nparts)
        df._persist = True
        df._cached = blocks
        return df

    def to_host(self) -> "DataFrame":
        blocks = {p: b.to(torch.device("cpu")) for p, b in self._blocks().items()}
        return DataFrame(self._schema, _Materialized(blocks), self._nparts)

    def local_blocks(self) -> Dict[int, Block]:
        return self._blocks()

    # -- actions
    @staticmethod
    def _column_payload(col, a: int = 0, b: Optional[int] = None):
        """A column slice in a cheap-to-pickle form: dense columns as one numpy
        array (a buffer, not one object per cell), others as value lists."""
        if is_dense(col):
            t = col[a:b]
            return t.detach().cpu().numpy()
        return column_values(col)[a:b]

    def _rows_of(self, nrows: int, payload: Dict[str, Any]) -> List[Row]:
        """Row objects straight from the column buffers (native convertBack,
        runtime/packer.cpp build_rows; reference: DataOps.scala:20-61)."""
        return build_rows(self._schema.names, [(nrows, [payload[n] for n in self._schema.names])])

    def collect(self, to: Optional[int] = None) -> List[Row]:
        """All rows, in partition order, as Row objects built natively from the
        column buffers (runtime/packer.cpp build_rows).

        Across ranks the rows go to every rank (SPMD programs branch on the
        result, so every rank must see it) or, with `to=<rank>` (or
        `Config.collect_to`), only to that rank, the Spark driver's view
        (reference: ExperimentalOperations.scala:92); the others get [].
        Dense columns move as tensors (one padded gather per column), only
        ragged / string columns are pickled (parallel/frame_comm.py)."""
        from ..config import config
        from ..parallel import frame_comm
        names = self._schema.names
        if to is None and config.collect_to != "all":
            to = int(config.collect_to) if str(config.collect_to).isdigit() else 0
        # evaluated once, partition by partition; agreed across ranks (a rank
        # that fails makes every rank raise, none waits in the gather)
        local = dist.agreed("collect", lambda: list(self._iter_blocks()))
        if not dist.is_distributed():
            return build_rows(names, [(b.nrows, [self._column_payload(b.columns[n]) for n in names])
                                      for _, b in local if b.nrows])
        parts = frame_comm.gather_blocks(local, names, self._schema, self._nparts, root=to)
        if parts is None:
            return []
        return build_rows(names, [(nrows, cols) for _, nrows, cols in parts])

    def count(self) -> int:
        """Rows over all ranks: one int64 all-reduce."""
        n = torch.tensor([dist.agreed("count", lambda: sum(b.nrows for _, b in self._iter_blocks()))],
                         dtype=torch.int64)
        return int(dist.all_reduce_host_(n, "Sum").item())

    def first(self) -> Optional[Row]:
        rows = self.take(1)
        return rows[0] if rows else None

    head = first

    def take(self, n: int) -> List[Row]:
        """The first n rows in partition order. Partitions are evaluated in
        order and evaluation stops once n rows are in hand (later partitions
        are never computed); across ranks, each partition's owner broadcasts
        only the rows still needed, dense columns as tensors."""
        if n <= 0:
            return []
        from ..parallel import frame_comm
        got = frame_comm.take_rows(self._iter_blocks(), self._schema.names, self._schema, self._nparts, n)
        return build_rows(self._schema.names, got)[:n]

    def show(self, n: int = 20):
        rows = self.take(n)
        print(" | ".join(self.columns))
        for r in rows:
            print(" | ".join(str(v) for v in r))

    def toPandas(self):  # noqa: N802
        import pandas as pd
        rows = self.collect()
        return pd.DataFrame([list(r) for r in rows], columns=self.columns)

    def to_numpy(self, column: str) -> np.ndarray:
        """All rows of a column as one array, on every rank (dense columns are
        gathered as tensors)."""
        from ..parallel import frame_comm
        blocks = dist.agreed("to_numpy", self._blocks)
        local = [(pid, blocks[pid]) for pid in sorted(blocks)]
        if not dist.is_distributed():
            parts = [(pid, b.nrows, [self._column_payload(b.columns[column])]) for pid, b in local if b.nrows]
        else:
            parts = frame_comm.gather_blocks(local, [column], self._schema, self._nparts)
        arrs = [c[0] if isinstance(c[0], np.ndarray) else np.asarray(c[0], dtype=object) for _, _, c in parts]
        return np.concatenate(arrs, 0) if arrs else np.zeros((0,))

    # -- transformations
    def select(self, *cols) -> "DataFrame":
        """Columns by name or `Column` expressions, mixed. A plain reference
        (aliased or not) is zero-copy: the same tensor under the new name, the
        field copied with all of its metadata. Computed expressions of one
        select run as ONE map_blocks over a generated graph."""
        names = [c for cs in cols for c in (cs if isinstance(cs, (list, tuple)) else [cs])]
        if any(isinstance(n, RandomExpression) for n in names):
            return self._select_randoms(names)
        if any(isinstance(n, WindowExpression) for n in names):
            return self._select_windows(names)
        if any(isinstance(n, Column) for n in names):
            return self._select_columns(names)
        for n in names:
            if n not in self._schema:
                raise ValueError(f"Column {n} not found in {self.columns}")
        schema = StructType([self._schema[n] for n in names])
        return DataFrame(schema, _Derived(self, lambda bs: {p: b.select(names) for p, b in bs.items()}),
                         self._nparts)

    def _project(self, pairs: Sequence[tuple]) -> "DataFrame":
        """Zero-copy projection: [(column here, name there)]."""
        pairs = list(pairs)
        schema = StructType([self._schema[src] if src == dst else self._schema[src].copy(name=dst)
                             for src, dst in pairs])

        def fn(bs):
            return {p: Block(b.nrows, {dst: b.columns[src] for src, dst in pairs}) for p, b in bs.items()}
        return DataFrame(schema, _Derived(self, fn), self._nparts)

    def _select_columns(self, items: Sequence[Any]) -> "DataFrame":
        from .. import core
        outs: List[tuple] = []  # (output name, source column or None, expression)
        for it in items:
            if isinstance(it, str):
                it = Column._ref(it)
            elif not isinstance(it, Column):
                raise TypeError(f"select: a column name or a Column is expected, got {type(it).__name__}")
            it._no_sort_order("select")
            if it.is_reference:
                src = it._expr[1]
                if src not in self._schema:
                    raise ValueError(f"Column {src} not found in {self.columns}")
                outs.append((it.output_name, src, None))
            else:
                outs.append((it.output_name, None, it._expr))
        seen = set()
        for name, _, _ in outs:
            if name in seen:
                raise ValueError(f"select: duplicate output column name '{name}'; give one of them an .alias()")
            seen.add(name)
        base = self
        computed = [(i, e) for i, (_, src, e) in enumerate(outs) if src is None]
        tmp: Dict[int, str] = {}
        if computed:
            k = 0
            for i, _ in computed:  # graph node names that meet no column name
                while f"tfa_expr_{k}" in self._schema:
                    k += 1
                tmp[i] = f"tfa_expr_{k}"
                k += 1
            fetches, feed, infos = compile_expressions(self, [(tmp[i], e) for i, e in computed])
            for (i, _), (dt, _) in zip(computed, infos):
                if dt == D.DT_BOOL:
                    raise core.InvalidTypeException(
                        f"select: '{outs[i][0]}' is a boolean expression, which no column type can hold; "
                        f"cast it, e.g. .cast(\"int\"), or use it in filter()")
            base = core.map_blocks(fetches, self, feed_dict=feed)
        return base._project([(tmp[i] if src is None else src, name) for i, (name, src, _) in enumerate(outs)])

    def _select_windows(self, items: Sequence[Any]) -> "DataFrame":
        """select with window expressions (frame/window.py) next to names and
        plain column references."""
        from .window import apply_windows
        outs: List[tuple] = []  # (output name, source column or the window expression)
        for it in items:
            if isinstance(it, WindowExpression):
                if not it.has_alias:
                    raise ValueError(f"select: the window expression '{it.output_name}' needs a name; give it an "
                                     f".alias()")
                outs.append((it.output_name, it))
                continue
            if isinstance(it, str):
                it = Column._ref(it)
            elif not isinstance(it, Column):
                raise TypeError(f"select: a column name, a Column or a window expression is expected, got "
                                f"{type(it).__name__}")
            it._no_sort_order("select")
            if not it.is_reference:
                raise TypeError(f"select: the computed Column '{it.output_name}' stands next to a window expression; "
                                f"split the call: add the window columns first (select or withColumn), then "
                                f"compute with them")
            if it._expr[1] not in self._schema:
                raise ValueError(f"Column {it._expr[1]} not found in {self.columns}")
            outs.append((it.output_name, it._expr[1]))
        seen = set()
        for name, _ in outs:
            if name in seen:
                raise ValueError(f"select: duplicate output column name '{name}'; give one of them an .alias()")
            seen.add(name)
        return apply_windows(self, outs, "select")

    def _select_randoms(self, items: Sequence[Any]) -> "DataFrame":
        """select with random expressions (`F.rand`, `F.randn`:
        frame/sampling.py) next to names and plain column references."""
        from .sampling import apply_randoms
        outs: List[tuple] = []  # (output name, source column or the random expression)
        for it in items:
            if isinstance(it, RandomExpression):
                outs.append((it.output_name, it))
                continue
            if isinstance(it, WindowExpression):
                raise TypeError(f"select: the window expression '{it.output_name}' stands next to a random "
                                f"expression; split the call: add one of them with withColumn first")
            if isinstance(it, str):
                it = Column._ref(it)
            elif not isinstance(it, Column):
                raise TypeError(f"select: a column name, a Column or a random expression is expected, got "
                                f"{type(it).__name__}")
            it._no_sort_order("select")
            if not it.is_reference:
                raise TypeError(f"select: the computed Column '{it.output_name}' stands next to a random expression; "
                                f"split the call: add the random columns first (select or withColumn), then "
                                f"compute with them")
            if it._expr[1] not in self._schema:
                raise ValueError(f"Column {it._expr[1]} not found in {self.columns}")
            outs.append((it.output_name, it._expr[1]))
        seen = set()
        for name, _ in outs:
            if name in seen:
                raise ValueError(f"select: duplicate output column name '{name}'; give one of them an .alias()")
            seen.add(name)
        return apply_randoms(self, outs, "select")

    def withColumn(self, name: str, expr: Column) -> "DataFrame":  # noqa: N802
        """Appends column `name`; an existing column of that name is replaced
        in place (keeps its position), as in Spark. `expr` is a Column, a
        window expression (`F.row_number().over(w)`, `F.sum("x").over(w)`),
        which gives the rows in the window's sort order, or a random
        expression (`F.rand(seed)`, `F.randn(seed)`: one float64 draw per row,
        rows and partitions as they are)."""
        if isinstance(expr, RandomExpression):
            from .sampling import apply_randoms
            if not isinstance(name, str) or not name:
                raise TypeError(f"withColumn: a non-empty column name is expected, got {name!r}")
            outs = [(c, expr if c == name else c) for c in self.columns]
            if name not in self._schema:
                outs.append((name, expr))
            return apply_randoms(self, outs, "withColumn")
        if isinstance(expr, WindowExpression):
            from .window import apply_windows
            if not isinstance(name, str) or not name:
                raise TypeError(f"withColumn: a non-empty column name is expected, got {name!r}")
            outs = [(c, expr if c == name else c) for c in self.columns]
            if name not in self._schema:
                outs.append((name, expr))
            return apply_windows(self, outs, "withColumn")
        if not isinstance(expr, Column):
            raise TypeError(f"withColumn: a Column expression is expected, got {type(expr).__name__}")
        expr._no_sort_order("withColumn")
        new = expr.alias(name)
        if name in self._schema:
            return self._select_columns([new if c == name else c for c in self.columns])
        return self._select_columns(list(self.columns) + [new])

    with_column = withColumn

    def toDF(self, *names) -> "DataFrame":  # noqa: N802
        """The same columns under new names."""
        names = [c for cs in names for c in (cs if isinstance(cs, (list, tuple)) else [cs])]
        if len(names) != len(self.columns):
            raise ValueError(f"toDF: {len(names)} names given for {len(self.columns)} columns "
                             f"({', '.join(self.columns)})")
        if len(set(names)) != len(names):
            raise ValueError(f"toDF: duplicate column names in {names}")
        return self._project(list(zip(self.columns, names)))

    to_df = toDF

    def filter(self, cond: Column) -> "DataFrame":  # noqa: A003
        """Rows for which the boolean Column `cond` is true, in order; schema,
        metadata and the number of partitions are unchanged (partition-local:
        no collectives). Device-resident partitions are compacted on the
        device by the row-compaction kernels (kernels/compact.hip); of a host
        partition only the predicate's inputs travel to the GPU and only the
        mask comes back."""
        refuse_window_expression("filter", [cond])
        if not isinstance(cond, Column):
            raise TypeError(f"filter: a boolean Column is expected (e.g. df.x > 3), got {type(cond).__name__}")
        cond._no_sort_order("filter")
        return _filter_frame(self, cond)

    where = filter

    def limit(self, n: int) -> "DataFrame":
        """The first n rows in partition order; the number of partitions is
        unchanged (later partitions become empty). Across ranks the rows per
        partition are agreed with one host all-reduce."""
        if not isinstance(n, numbers.Integral) or isinstance(n, bool) or n < 0:
            raise ValueError(f"limit: a non-negative row count is expected, got {n!r}")
        n = int(n)
        nparts = self._nparts

        def fn(bs):
            from ..parallel import frame_comm
            counts = frame_comm.partition_rows({p: b.nrows for p, b in bs.items()}, nparts)
            res, before = {}, 0
            for p in range(nparts):
                if p in bs:
                    keep = max(0, min(counts[p], n - before))
                    res[p] = bs[p] if keep == counts[p] else bs[p].slice(0, keep)
                before += counts[p]
            return res
        return DataFrame(self._schema, _Derived(self, fn, streamable=False), nparts)

    def sortWithinPartitions(self, *cols, ascending=True) -> "DataFrame":  # noqa: N802
        """Every partition sorted on its own by the keys `cols` (names or
        Columns, `.asc()` / `.desc()` or `ascending=` a bool or one bool per
        key); schema, metadata and the number of partitions are unchanged
        (partition-local: no collectives). The sort is stable; NaN sorts after
        +inf, -0.0 equals 0.0. Device-resident partitions are sorted on the
        device (kernels/sort.hip)."""
        return _sort_frame(self, cols, ascending, False, "sortWithinPartitions")

    sort_within_partitions = sortWithinPartitions

    def orderBy(self, *cols, ascending=True) -> "DataFrame":  # noqa: N802
        """The rows in the global order of the keys `cols` (see
        `sortWithinPartitions` for the keys): the number of partitions is
        unchanged and reading them in order gives the sorted rows. Rows with
        equal keys keep their input order (partition order, then row order),
        so the result does not depend on the number of ranks. A sample sort:
        local sort, agreed splitters, one exchange of contiguous slices, local
        sort of what arrived."""
        return _sort_frame(self, cols, ascending, True, "orderBy")

    sort = orderBy
    order_by = orderBy

    def join(self, other: "DataFrame", on, how: str = "inner") -> "DataFrame":
        """Equi-join with `other` on the key column(s) `on` (a name or a list
        of up to 8 names that both frames hold, with the same type on both
        sides). `how`: "inner" (the keys, this frame's other columns, then
        `other`'s), "left_semi" / "semi" (this frame's rows that have a
        match) or "left_anti" / "anti" (those that have none). Keys compare
        as in `orderBy`: NaN equals NaN, -0.0 equals 0.0.

        A broadcast join: `other` is gathered whole on every rank, so it
        should be the small side. The result has this frame's partitions;
        partition p holds the matches of this frame's partition p in row
        order, a row's matches in `other`'s global row order -- the same for
        every world size and every partitioning of `other`. Device-resident
        partitions are joined on the device (kernels/join.hip)."""
        from .join import _join_frame
        return _join_frame(self, other, on, how)

    def union(self, other: "DataFrame") -> "DataFrame":
        """The rows of this frame, then the rows of `other`, columns resolved
        by POSITION (as in Spark): names and metadata are this frame's, an
        analyzed lead dimension becomes unknown and the cell shapes must
        agree. Column types must be equal: there is no implicit widening
        (`.cast()` one side first). The result has `num_partitions +
        other.num_partitions` partitions, this frame's first, so
        `a.union(b).dropDuplicates(["id"])` prefers `a`'s rows. Lazy; blocks
        are never copied and device-resident blocks stay on the device.
        Across ranks, `other`'s partitions move to their new owners in one
        exchange unless this frame's partition count divides by the world
        size."""
        from .setops import _union_frame
        return _union_frame(self, other, False, "union")

    unionAll = union  # noqa: N815
    union_all = union

    def unionByName(self, other: "DataFrame") -> "DataFrame":  # noqa: N802
        """`union` with `other`'s columns resolved by NAME: they are reordered
        to this frame's order; a missing or an extra name is a ValueError."""
        from .setops import _union_frame
        return _union_frame(self, other, True, "unionByName")

    union_by_name = unionByName

    def dropDuplicates(self, subset=None) -> "DataFrame":  # noqa: N802
        """One row per distinct tuple of the key columns `subset` (a list of
        names; None: every column). Keys follow `orderBy`'s rules (up to 8
        numeric scalar columns; NaN equals NaN, -0.0 equals 0.0); the other
        columns may be of any kind and follow the kept rows.

        Defined differences from Spark: the kept row is the FIRST occurrence
        in input order (partition order, then row order; Spark keeps an
        arbitrary one), and the result is in the order of `orderBy(*keys)`,
        ascending, in the same number of partitions. Neither the kept rows
        nor their order and placement depend on the number of ranks.
        Sort-based: every partition is sorted and reduced to its distinct
        rows BEFORE the exchange of `orderBy` (at most the locally distinct
        rows travel), what arrives is sorted and reduced again.
        Device-resident partitions use the sort kernels and kernels/unique.hip."""
        from .setops import _distinct_frame
        return _distinct_frame(self, subset, "dropDuplicates")

    drop_duplicates = dropDuplicates

    def distinct(self) -> "DataFrame":
        """`dropDuplicates()` over every column."""
        from .setops import _distinct_frame
        return _distinct_frame(self, None, "distinct")

    def intersect(self, other: "DataFrame") -> "DataFrame":
        """The distinct rows of this frame that `other` holds too (columns by
        position, types as in `union`): `distinct()`, then a left-semi
        broadcast join on all columns, so the result keeps `distinct`'s order
        and `join`'s limits (`other` is gathered on every rank; at most 8
        columns, all numeric scalars)."""
        from .setops import _semi_frame
        return _semi_frame(self, other, "left_semi", "intersect")

    def subtract(self, other: "DataFrame") -> "DataFrame":
        """The distinct rows of this frame that `other` does not hold (see
        `intersect`; a left-anti join)."""
        from .setops import _semi_frame
        return _semi_frame(self, other, "left_anti", "subtract")

    def sample(self, withReplacement=None, fraction=None, seed=None) -> "DataFrame":  # noqa: N803
        """A random subset of the rows, in Spark's call forms: `sample(0.1)`,
        `sample(0.1, 3)`, `sample(False, 0.1, 3)`, `sample(fraction=0.1,
        seed=3)`. Without replacement a row is kept when its uniform draw u is
        below `fraction` (in [0, 1]); with replacement row i appears
        Poisson(`fraction`) times, consecutively (`fraction` <= 16). Rows keep
        their order and their partitions. A draw is a pure function of (seed,
        global row index): the same rows for every number of ranks, every
        partitioning of the same row sequence, on the host and on the device
        (kernels/random.hip), and for every action on the frame, also with
        `seed=None` (drawn once, when `sample` is called). docs/MIGRATION.md
        has the generator in full."""
        from .sampling import sample_frame
        return sample_frame(self, withReplacement, fraction, seed)

    def randomSplit(self, weights, seed=None) -> List["DataFrame"]:  # noqa: N802
        """One frame per weight (positive, finite): the weights are normalised
        to bounds 0 = b_0 <= ... <= b_k = 1 and split i keeps the rows with
        b_i <= u < b_{i+1}, all under one seed, so every row lands in exactly
        one split (see `sample` for u)."""
        from .sampling import random_split
        return random_split(self, weights, seed)

    random_split = randomSplit

    def sampleBy(self, col, fractions, seed=None) -> "DataFrame":  # noqa: N802
        """A stratified sample: a row whose `col` value is key k is kept when
        u < fractions[k] (a dict from key to a fraction in [0, 1]); keys not
        in the dict are dropped, as in Spark. `col` is a numeric scalar
        column under `orderBy`'s key rules; keys compare as there (NaN
        matches NaN, -0.0 matches 0.0). At most 4096 strata."""
        from .sampling import sample_by
        return sample_by(self, col, fractions, seed)

    sample_by = sampleBy

    def describe(self, *cols) -> "DataFrame":
        """count, mean, stddev, min and max of the named columns, or of every
        numeric scalar column (uint8, int8, int16, int32, int64, float,
        double; the others are skipped) when none is named: a one-partition
        frame with a string column `summary` (the row labels) and one DOUBLE
        column per described column (Spark returns strings). An action, and
        collective: every rank calls it. `stddev` is the sample standard
        deviation (NaN below two rows); `min` / `max` follow `orderBy`'s
        order (NaN after +inf). Device-resident columns are read once by the
        moments kernel (kernels/stats.hip); for a given partitioning the
        result has the same bits for every number of ranks."""
        from .stats import describe
        return describe(self, *cols)

    def summary(self, *statistics) -> "DataFrame":
        """`describe` of every numeric scalar column with chosen statistics:
        any of "count", "mean", "stddev", "min", "max" and percentiles such as
        "25%" (any number in [0, 100], at most 16); by default count, mean,
        stddev, min, 25%, 50%, 75%, max. Percentiles are exact
        (`approxQuantile`)."""
        from .stats import summary
        return summary(self, *statistics)

    def approxQuantile(self, col, probabilities, relativeError=0.0):  # noqa: N802, N803
        """The quantiles of a numeric scalar column at `probabilities` (at
        most 16 numbers in [0, 1]) as a list of floats, or for a list of
        columns one such list per column. Quantile p is the row at 0-based
        position max(ceil(p * N) - 1, 0) of `orderBy(col)` (numpy's
        `inverted_cdf`); NaNs count as rows and sort last. Every
        `relativeError` >= 0 returns the exact value: a radix selection over
        the order-preserving words of the sort path, at most 8 read-only
        passes over the column (kernels/stats.hip on the device), no row
        moves. An empty frame gives []. An action, and collective."""
        from .stats import approx_quantile
        return approx_quantile(self, col, probabilities, relativeError)

    approx_quantile = approxQuantile

    def agg(self, *exprs) -> "DataFrame":
        """Named aggregates over the whole frame, `groupBy().agg(...)` without
        keys: `agg(F.count("*"), F.avg("x"), F.max("x"))` with `tfs.functions`
        as F, or `agg({"x": "sum"})`. One row, in one partition, identical on
        every rank; names, types and values as in `GroupedData.agg`. A frame
        without rows gives count 0, sum 0 and NaN for avg, stddev and variance;
        a `min` or `max` of it raises ValueError. An action, and collective."""
        from .group_agg import group_agg
        return group_agg(GroupedData(self, []), list(exprs))

    def corr(self, col1, col2, method="pearson") -> float:
        """Pearson's correlation coefficient of two numeric scalar columns as a
        Python float (`df.stat.corr`): `agg(F.corr(col1, col2))`, NaN where
        Spark gives null (no rows, a constant column, a NaN or an infinity in
        either column). Any `method` but "pearson" raises ValueError. An
        action, and collective."""
        return self.stat.corr(col1, col2, method)

    def cov(self, col1, col2) -> float:
        """The sample covariance of two numeric scalar columns as a Python
        float (`df.stat.cov`): `agg(F.covar_samp(col1, col2))`, NaN below two
        rows. An action, and collective."""
        return self.stat.cov(col1, col2)

    def crosstab(self, col1, col2) -> "DataFrame":
        """The contingency table of two numeric scalar columns
        (`df.stat.crosstab`): `groupBy(col1).pivot(col2).count()` with the key
        column renamed `<col1>_<col2>`. One row per value of `col1`, ascending,
        one int64 column per distinct value of `col2` (ascending, NaN last),
        0 for a pair that never occurs. Unlike Spark the first column keeps
        `col1`'s numeric type. The distinct values of `col2` are looked up
        when this is called (collective); the counts are lazy."""
        return self.stat.crosstab(col1, col2)

    @property
    def stat(self):
        """Spark's `df.stat` accessor (`df.stat.approxQuantile(...)`,
        `df.stat.corr(...)`, `df.stat.cov(...)`, `df.stat.crosstab(...)`)."""
        from .stats import DataFrameStatFunctions
        return DataFrameStatFunctions(self)

    def drop(self, *names) -> "DataFrame":
        return self.select([n for n in self.columns if n not in names])

    def withColumnRenamed(self, existing: str, new: str) -> "DataFrame":  # noqa: N802
        fields = [f.copy(name=new) if f.name == existing else f for f in self._schema.fields]

        def fn(bs):
            return {p: Block(b.nrows, {(new if k == existing else k): v for k, v in b.columns.items()})
                    for p, b in bs.items()}
        return DataFrame(StructType(fields), _Derived(self, fn), self._nparts)

    def with_schema(self, schema: StructType) -> "DataFrame":
        """Same data, new schema (used by `analyze` to attach metadata)."""
        df = DataFrame(schema, _Derived(self, lambda bs: bs), self._nparts)
        return df

    def repartition(self, n: int) -> "DataFrame":
        """n even partitions in row order. Each rank receives only the rows of
        the partitions it owns: dense columns in one all-to-all per column
        (RCCL for device-resident frames), other columns pickled."""
        from ..parallel import frame_comm
        names = self.columns
        nin = self._nparts

        def fn(bs):
            return frame_comm.repartition_blocks(bs, names, self._schema, nin, n)
        return DataFrame(self._schema, _Derived(self, fn, streamable=False), n)

    def coalesce(self, n: int) -> "DataFrame":
        return self.repartition(min(n, self._nparts))

    def groupBy(self, *cols) -> "GroupedData":  # noqa: N802
        names = [c for cs in cols for c in (cs if isinstance(cs, (list, tuple)) else [cs])]
        refuse_random_expression("groupBy", names)
        for n in names:
            if n not in self._schema:
                raise ValueError(f"groupBy: column {n} not found in {self.columns}")
        return GroupedData(self, names)

    groupby = groupBy

    # -- TensorFrames method forms (reference: src/main/scala/org/tensorframes/dsl/Implicits.scala:25-116)
    def map_blocks(self, fetches, trim: bool = False, **kw) -> "DataFrame":
        from .. import core
        return core.map_blocks(fetches, self, trim=trim, **kw)

    mapBlocks = map_blocks  # noqa: N815

    def map_blocks_trimmed(self, fetches, **kw) -> "DataFrame":
        from .. import core
        return core.map_blocks(fetches, self, trim=True, **kw)

    mapBlocksTrimmed = map_blocks_trimmed  # noqa: N815

    def map_rows(self, fetches, feed_dict=None, **kw) -> "DataFrame":
        from .. import core
        return core.map_rows(fetches, self, feed_dict=feed_dict, **kw)

    mapRows = map_rows  # noqa: N815

    def reduce_blocks(self, fetches, **kw):
        from .. import core
        return core.reduce_blocks(fetches, self, **kw)

    reduceBlocks = reduce_blocks  # noqa: N815

    def reduce_rows(self, fetches, **kw):
        from .. import core
        return core.reduce_rows(fetches, self, **kw)

    reduceRows = reduce_rows  # noqa: N815

    def analyze(self) -> "DataFrame":
        from .. import core
        return core.analyze(self)

    def block(self, col_name: str, tf_name: Optional[str] = None):
        from .. import core
        return core.block(self, col_name, tf_name)

    def row(self, col_name: str, tf_name: Optional[str] = None):
        from .. import core
        return core.row(self, col_name, tf_name)


# ------------------------------------------------------------------ filter
_COMPACT_GROUP = 16  # columns per _C.compact_rows call (kernels.h kMaxPackCols)


def _filter_frame(df: DataFrame, cond: Column) -> DataFrame:
    """The lazy frame of `df.filter(cond)`. The predicate is validated here (one
    bool per row, typed errors) and compiled to one program; every partition
    then runs it directly -- not through map_blocks: the mask never becomes a
    column -- and drops the rows the mask rejects."""
    from .. import core, engine
    from ..utils.logging import metrics
    (fetch,), feed, ((dt, rank),) = compile_expressions(df, [("tfa_filter_mask", cond._expr)])
    what = cond.output_name
    if dt != D.DT_BOOL:
        raise core.InvalidTypeException(
            f"filter: the condition '{what}' is of type {D.dtype_name(dt)}, not boolean; compare it, "
            f"e.g. ({what}) != 0")
    if rank != 0:
        raise core.InvalidDimensionException(
            f"filter: the condition '{what}' yields a boolean cell of rank {rank} per row, not one value; "
            f"reduce it with .all() or .any()")
    spec = core._resolve([fetch])
    summary = core.analyze_graph(spec)
    out = summary[spec.fetch_names[0]]
    if out.tf_dtype != D.DT_BOOL:
        raise core.InvalidTypeException(f"filter: the condition '{what}' is of type {D.dtype_name(out.tf_dtype)}, "
                                        f"not boolean")
    if out.shape is not None and out.shape.num_dims != 1:
        raise core.InvalidDimensionException(f"filter: the condition '{what}' has block shape {out.shape}, "
                                             f"expected one value per row")
    feed_names = [s.name for s in summary.values() if s.is_input]
    feed_cols = [feed[n] for n in feed_names]
    prog = engine.program_for_spec(spec, spec.fetch_refs, feed_names)
    hints = {n: (summary[n].tf_dtype, list(core._col_info(df.schema[c]).shape.dims))
             for n, c in zip(feed_names, feed_cols)}
    separable = bool(feed_names) and bool(prog.row_separable(hints))

    def mask_of(b: Block) -> torch.Tensor:
        ins = core._dense_inputs(b, feed_cols, "filter")
        if ins and all(t.is_cuda for t in ins) and len({t.device for t in ins}) == 1:
            m = engine.run_program(prog, ins, ins[0].device)[0]  # stays on the device
        elif not engine.gpu_available() or not ins:
            m = engine.run_program(prog, ins, None)[0]
            m = m.cpu() if m.is_cuda else m
        elif separable and engine.worth_pipelining(ins):
            # a large host partition: chunked H2D / compute / D2H; the mask is
            # needed now, so the pipelined run is waited for here
            with engine.deferred_pipelines() as handles:
                m = engine.run_segments_pipelined(prog, [ins], [[((b.nrows,), torch.bool)]])[0][0]
            engine.wait_pipelines(handles)
            prog.release_pipeline()
        else:
            m = engine.run_block_host(prog, ins, False)[0]
        if m.dim() != 1 or m.shape[0] != b.nrows:
            raise core.InvalidDimensionException(
                f"filter: the condition '{what}' produced shape {tuple(m.shape)} for a block of {b.nrows} rows")
        return m if m.dtype == torch.bool else m != 0

    def compute(blocks: Dict[int, Block]) -> Dict[int, Block]:
        res: Dict[int, Block] = {}
        rows_in = kept = 0
        rng = torch.cuda.is_initialized()
        if rng:
            torch.cuda.nvtx.range_push("tfa.filter")
        try:
            for pid in sorted(blocks):
                b = blocks[pid]
                if b.nrows == 0:
                    res[pid] = b
                    continue
                res[pid] = _filter_block(b, mask_of(b))
                rows_in += b.nrows
                kept += res[pid].nrows
        finally:
            if rng:
                torch.cuda.nvtx.range_pop()
        metrics.add("filter_rows_in", rows_in)
        metrics.add("filter_rows_kept", kept)
        return res

    return DataFrame(df.schema, _Derived(df, compute), df.num_partitions)


def _filter_block(b: Block, mask: torch.Tensor) -> Block:
    """Rows of `b` whose mask entry is true, order kept. A device mask compacts
    the device columns with the native kernels (dense columns 16 per call,
    strings through the kept-row index); whatever lives on the host is
    indexed there."""
    from .._native import _C
    cols: Dict[str, Any] = {}
    dev_dense = [n for n, c in b.columns.items() if mask.is_cuda and isinstance(c, torch.Tensor)
                 and c.device == mask.device and c.dim() >= 1]
    if not dev_dense:
        hm = mask.cpu() if mask.is_cuda else mask
        idx = None
        for n, c in b.columns.items():
            if isinstance(c, torch.Tensor):
                cols[n] = c[hm.to(c.device)] if c.is_cuda else c[hm]
            else:
                if idx is None:
                    idx = torch.nonzero(hm).reshape(-1).numpy()
                cols[n] = c.take(idx)
        return Block(int(hm.sum().item()), cols)
    others = [n for n in b.columns if n not in dev_dense]
    index = None
    total = 0
    for g in range(0, len(dev_dense), _COMPACT_GROUP):
        names = dev_dense[g:g + _COMPACT_GROUP]
        outs, total, ix = _C.compact_rows(mask, [b.columns[n] for n in names], bool(others) and index is None)
        index = ix if ix is not None else index
        cols.update(zip(names, outs))
    host_idx = hm = None
    for n in others:
        c = b.columns[n]
        if isinstance(c, StringColumn) and c.is_cuda and c.device == mask.device:
            offs, data = _C.gather_strings(c.offsets, c.data, index)
            cols[n] = StringColumn(offs.to(mask.device), data, c.binary)
        elif isinstance(c, torch.Tensor):
            hm = mask.cpu() if hm is None else hm
            cols[n] = c[hm.to(c.device)]
        else:
            if host_idx is None:
                host_idx = index.cpu().numpy()
            cols[n] = c.take(host_idx)
    return Block(int(total), {n: cols[n] for n in b.columns})


# ------------------------------------------------------------------ sort
_PERMUTE_GROUP = 16  # columns per _C.permute_rows call (kernels.h kMaxPackCols)
_MAX_SORT_KEYS = 8   # kernels.h kMaxSortKeys
_SORT_SAMPLES_PER_PARTITION = 4  # orderBy: samples a partition gives, times the partition count
_SORT_KEY_DTYPES = (D.DT_BOOL, D.DT_UINT8, D.DT_INT8, D.DT_INT16, D.DT_INT32, D.DT_INT64, D.DT_FLOAT, D.DT_DOUBLE)


def _host_sort_words(key: torch.Tensor, descending: bool) -> np.ndarray:
    """The order-preserving unsigned 64-bit word of every row of one key
    column, on the host (the same table as kernels/sort.hip)."""
    a = key.detach().cpu().contiguous().numpy()
    if a.dtype == np.float32:
        b = a.view(np.uint32).copy()
        b[np.isnan(a)] = 0x7FC00000
        b[b == 0x80000000] = 0
        neg = (b >> 31).astype(bool)
        w = np.where(neg, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
        return (~w if descending else w).astype(np.uint64)
    if a.dtype == np.float64:
        b = a.view(np.uint64).copy()
        b[np.isnan(a)] = 0x7FF8000000000000
        b[b == 0x8000000000000000] = 0
        neg = (b >> 63).astype(bool)
        w = np.where(neg, ~b, b | np.uint64(0x8000000000000000)).astype(np.uint64)
    elif a.dtype in (np.bool_, np.uint8):
        w = a.astype(np.uint64)
    else:
        w = a.astype(np.int64).view(np.uint64) ^ np.uint64(0x8000000000000000)
    return ~w if descending else w


def _sort_order_of(b: Block, keys: Sequence[str], desc: Sequence[bool]):
    """(words [W, n], perm [n], radix passes) of one partition: the stable
    order of its rows by the key tuples. Device tensors when every key column
    is on one device (encode + radix argsort kernels), numpy arrays otherwise
    (the same words, np.lexsort: the CPU oracle)."""
    from .. import core
    from .._native import _C
    if b.nrows == 0:
        return np.zeros((len(keys), 0), dtype=np.uint64), np.zeros(0, dtype=np.int64), 0
    cols = [b.columns[k] for k in keys]
    for k, c in zip(keys, cols):
        if not isinstance(c, torch.Tensor) or c.dim() != 1:
            raise core.InvalidDimensionException(
                f"sort: the key column '{k}' does not hold one scalar per row in this partition; reduce the cell "
                f"first (.sum(), .max(), ...)")
    if all(c.is_cuda for c in cols) and len({c.device for c in cols}) == 1:
        words = _C.sort_encode(cols, [bool(d) for d in desc])
        perm = _C.sort_argsort(words)
        return words, perm, int(_C.sort_last_passes())
    words = np.stack([_host_sort_words(c, d) for c, d in zip(cols, desc)], 0)
    perm = np.lexsort(words[::-1])  # (stable; the last key given to lexsort is the primary one)
    return words, perm.astype(np.int64), 0


def _permute_block(b: Block, perm) -> Block:
    """Rows of `b` in the order perm (a device int64 tensor or a numpy array):
    device dense columns through the row-permute kernel, 16 per call, device
    strings through the string gather; whatever lives on the host is indexed
    there."""
    from .._native import _C
    cols: Dict[str, Any] = {}
    on_dev = isinstance(perm, torch.Tensor) and perm.is_cuda
    dev_dense = [n for n, c in b.columns.items() if on_dev and isinstance(c, torch.Tensor)
                 and c.device == perm.device and c.dim() >= 1]
    for g in range(0, len(dev_dense), _PERMUTE_GROUP):
        names = dev_dense[g:g + _PERMUTE_GROUP]
        cols.update(zip(names, _C.permute_rows(perm, [b.columns[n] for n in names])))
    host_t = host_np = None
    for n, c in b.columns.items():
        if n in cols:
            continue
        if host_t is None:
            host_t = perm.cpu() if isinstance(perm, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(perm))
            host_np = host_t.numpy()
        if isinstance(c, StringColumn) and c.is_cuda:
            idx = perm if on_dev and perm.device == c.device else host_t.to(c.device)
            offs, data = _C.gather_strings(c.offsets, c.data, idx)
            cols[n] = StringColumn(offs.to(c.device), data, c.binary)
        elif isinstance(c, torch.Tensor):
            cols[n] = c.index_select(0, host_t.to(c.device))
        else:
            cols[n] = c.take(host_np)
    return Block(b.nrows, {n: cols[n] for n in b.columns})


def _sort_block(b: Block, keys: Sequence[str], desc: Sequence[bool], stats: List[int]):
    """(sorted block, words, perm) of one partition; words / perm are None for
    a partition of fewer than two rows only when they are not needed."""
    words, perm, passes = _sort_order_of(b, keys, desc)
    stats[0] += b.nrows
    stats[1] += passes
    return (_permute_block(b, perm) if b.nrows > 1 else b), words, perm


def _lower_bounds(words, perm, splitters: np.ndarray) -> List[int]:
    """For each splitter tuple [S, W] (uint64): the rows of the sorted order
    whose word tuple is lexicographically below it."""
    from .._native import _C
    if len(splitters) == 0:
        return []
    if isinstance(words, torch.Tensor):
        sp = torch.from_numpy(np.ascontiguousarray(splitters).view(np.int64))
        return _C.sort_bounds(words, perm, sp).cpu().tolist()
    sw = words[:, perm]  # [W, n] in sorted order
    n = sw.shape[1]
    out = []
    for t in splitters:
        lo, hi = 0, n
        for w in range(sw.shape[0]):  # narrow [lo, hi) to the rows equal to the splitter's prefix
            seg = sw[w, lo:hi]
            a = lo + int(np.searchsorted(seg, t[w], side="left"))
            hi = lo + int(np.searchsorted(seg, t[w], side="right"))
            lo = a
            if lo == hi:
                break
        out.append(lo)
    return out


def _order_blocks(blocks: Dict[int, Block], names: Sequence[str], schema: StructType, nparts: int,
                  keys: Sequence[str], desc: Sequence[bool], stats: List[int]) -> Dict[int, Block]:
    """orderBy's sample sort over this rank's partitions (collective)."""
    from ..parallel import frame_comm
    W = len(keys)
    local: Dict[int, Block] = {}
    order: Dict[int, tuple] = {}
    samples = []
    m = _SORT_SAMPLES_PER_PARTITION * nparts
    for pid in sorted(blocks):
        local[pid], words, perm = _sort_block(blocks[pid], keys, desc, stats)
        order[pid] = (words, perm)
        n = blocks[pid].nrows
        if n:
            # evenly spaced rows of the sorted order (no RNG: the same on every run)
            take = min(n, m)
            pos = np.array([((2 * j + 1) * n) // (2 * take) for j in range(take)], dtype=np.int64)
            if isinstance(words, torch.Tensor):
                rows = perm[torch.from_numpy(pos).to(perm.device)]
                samples.append(words[:, rows].cpu().numpy().view(np.uint64).T)
            else:
                samples.append(words[:, perm[pos]].T)
    mine = np.concatenate(samples, 0) if samples else np.zeros((0, W), dtype=np.uint64)
    every = np.concatenate(dist.all_gather_object(mine), 0) if dist.is_distributed() else mine
    if len(every):
        every = every[np.lexsort(every.T[::-1])]
        splitters = np.stack([every[(q * len(every)) // nparts] for q in range(1, nparts)], 0) \
            if nparts > 1 else np.zeros((0, W), dtype=np.uint64)
    else:
        splitters = np.zeros((0, W), dtype=np.uint64)
    # contiguous slices of every sorted local partition, one per output partition
    table = torch.zeros((nparts, max(nparts, 1)), dtype=torch.int64)
    for pid, b in local.items():
        cuts = [0] + (_lower_bounds(*order[pid], splitters) if b.nrows else [0] * (nparts - 1)) + [b.nrows]
        for q in range(nparts):
            table[pid, q] = cuts[q + 1] - cuts[q]
    dist.all_reduce_host_(table, "Sum")  # (every rank fills the rows of its own partitions)
    pieces: Dict[int, List[tuple]] = {}
    for p, lens in enumerate(table.tolist()):
        start, pieces[p] = 0, []
        for q in range(nparts):
            if lens[q]:
                pieces[p].append((q, start, lens[q]))
            start += lens[q]
    got = frame_comm.exchange_pieces(local, names, schema, nparts, pieces, stay_local=True)
    # the pieces arrived in source-partition order: one more stable sort per block
    return {q: _sort_block(b, keys, desc, stats)[0] for q, b in got.items()}


def _check_sort_key(f: StructField, shown: str, what: str) -> None:
    """The typed refusals of a key column of orderBy and of the operators built
    on its order (dropDuplicates, distinct): a numeric scalar per row."""
    from .. import core
    if isinstance(f.dataType, (StringType, BinaryType)):
        raise core.InvalidTypeException(
            f"{what}: '{shown}' is a {type(f.dataType).__name__[:-4].lower()} column; string and binary "
            f"columns are not supported as sort keys yet")
    stf = ColumnInformation(f).stf
    if stf is None:
        raise core.InvalidTypeException(f"{what}: the type of '{shown}' ({f.dataType}) is not supported as a "
                                        f"sort key")
    if stf.tf_dtype in (D.DT_HALF, D.DT_BFLOAT16):
        raise core.InvalidTypeException(f"{what}: '{shown}' is {D.dtype_name(stf.tf_dtype)}; half and bfloat16 "
                                        f"columns are not supported as sort keys yet (cast to float)")
    if stf.tf_dtype not in _SORT_KEY_DTYPES:
        raise core.InvalidTypeException(f"{what}: '{shown}' is {D.dtype_name(stf.tf_dtype)}, which is not "
                                        f"supported as a sort key")
    if stf.shape.num_dims != 1:
        raise core.InvalidDimensionException(
            f"{what}: the key '{shown}' holds a cell of rank {max(stf.shape.num_dims - 1, 0)} per row, not a "
            f"scalar; reduce the cell first (.sum(), .max(), ...)")


def _sort_frame(df: DataFrame, cols: Sequence[Any], ascending, global_order: bool, what: str) -> DataFrame:
    """The lazy frame of orderBy / sortWithinPartitions: everything is
    validated here (typed errors); computed keys become temporary columns
    (through the select path) that are projected away afterwards."""
    from .. import core
    from ..utils.logging import metrics
    items = [c for cs in cols for c in (cs if isinstance(cs, (list, tuple)) else [cs])]
    refuse_window_expression(what, items)
    if not items:
        raise ValueError(f"{what}: at least one sort key is expected")
    if len(items) > _MAX_SORT_KEYS:
        raise ValueError(f"{what}: at most {_MAX_SORT_KEYS} sort keys, got {len(items)}")
    if isinstance(ascending, (bool, np.bool_)):
        asc = [bool(ascending)] * len(items)
    elif isinstance(ascending, (list, tuple)) and all(isinstance(a, (bool, np.bool_, int)) for a in ascending):
        if len(ascending) != len(items):
            raise ValueError(f"{what}: ascending holds {len(ascending)} entries for {len(items)} sort keys")
        asc = [bool(a) for a in ascending]
    else:
        raise TypeError(f"{what}: ascending must be a bool or a list of one bool per key, got {ascending!r}")
    keys: List[str] = []
    desc: List[bool] = []
    extra: List[Column] = []
    taken = set(df.columns)
    for it, a in zip(items, asc):
        if isinstance(it, str):
            it = Column._ref(it)
        elif not isinstance(it, Column):
            raise TypeError(f"{what}: a column name or a Column is expected, got {type(it).__name__}")
        desc.append((it.sort_order == "desc") if it.sort_order is not None else not a)
        if it.is_reference:
            if it._expr[1] not in df.schema:
                raise ValueError(f"{what}: column {it._expr[1]} not found in {df.columns}")
            keys.append(it._expr[1])
        else:
            k = 0
            while f"tfa_sort_key_{k}" in taken:
                k += 1
            taken.add(f"tfa_sort_key_{k}")
            keys.append(f"tfa_sort_key_{k}")
            extra.append(Column(it._expr, f"tfa_sort_key_{k}"))
    base = df._select_columns(list(df.columns) + extra) if extra else df
    for k, it in zip(keys, items):
        _check_sort_key(base.schema[k], it if isinstance(it, str) else it.output_name, what)
    names = base.columns
    schema = base.schema
    nparts = df.num_partitions

    def compute(blocks: Dict[int, Block]) -> Dict[int, Block]:
        stats = [0, 0]  # rows sorted, radix passes
        rng = torch.cuda.is_initialized()
        if rng:
            torch.cuda.nvtx.range_push("tfa.sort")
        try:
            if global_order:
                res = _order_blocks(blocks, names, schema, nparts, keys, desc, stats)
            else:
                res = {pid: _sort_block(b, keys, desc, stats)[0] for pid, b in blocks.items()}
        finally:
            if rng:
                torch.cuda.nvtx.range_pop()
        metrics.add("sort_rows", stats[0])
        metrics.add("sort_radix_passes", stats[1])
        return res

    out = DataFrame(schema, _Derived(base, compute, streamable=not global_order), nparts)
    return out._project([(c, c) for c in df.columns]) if extra else out


class GroupedData:
    def __init__(self, df: DataFrame, keys: List[str]):
        self.df = df
        self.keys = keys

    def aggregate(self, fetches, **kw) -> DataFrame:
        from .. import core
        return core.aggregate(fetches, self, **kw)

    def count(self) -> DataFrame:
        """Rows per key: the keys plus a column of ones go through `aggregate`
        with a Sum graph (device factorisation + segmented sum, keyed
        all-to-all across ranks); no rows are collected."""
        from .. import core, engine
        from ..graph import dsl as tf
        keys = list(self.keys)

        def fn(bs):
            out = {}
            for p, b in bs.items():
                kc = b.columns[keys[0]]
                dev = kc.device if isinstance(kc, torch.Tensor) else torch.device("cpu")
                cols = {k: b.columns[k] for k in keys}
                cols["count"] = engine.device_full(b.nrows, 1, torch.int64, dev)
                out[p] = Block(b.nrows, cols)
            return out
        fields = [self.df.schema[k] for k in keys] + [tensor_field("count", D.DT_INT64, [])]
        ones = DataFrame(StructType(fields), _Derived(self.df, fn), self.df._nparts)
        with tf.Graph().as_default():
            ci = tf.placeholder(tf.int64, [None], name="count_input")
            return core.aggregate(tf.reduce_sum(ci, [0], name="count"), ones.groupBy(*keys))

    def agg(self, *exprs) -> DataFrame:
        """Named aggregates per key: `agg(F.avg("x"), F.stddev("x"), F.max("y"))`
        with `tfs.functions` as F, or `agg({"x": "sum", "y": "max"})`. The
        result holds the key columns, then one column per expression in call
        order, named as Spark names them (`avg(x)`, `stddev_samp(x)`,
        `count(1)`; `.alias()` overrides). count and integer sums are int64
        (sums wrap), float sums, avg, stddev and variance float64, min / max
        the column's own type. Keys are numeric scalar columns, grouped as
        `groupBy(keys).count()` groups them; one output partition per rank,
        keys in ascending order. Values follow `describe`: sample statistics
        are NaN for a one-row group, a NaN in a group makes its sum, avg,
        stddev and variance NaN, min / max order NaN last and return -0.0 as
        0.0. `F.corr(a, b)`, `F.covar_samp(a, b)` and `F.covar_pop(a, b)` mix
        in freely (float64, `corr(a, b)`; at most 16 distinct ordered pairs
        per call): NaN where Spark gives null, and for a group with a NaN or an
        infinity in either column. Device-resident partitions are reduced by
        the grouped-moments kernels (kernels/group_stats.hip); for a given
        partitioning the result has the same bits for every number of ranks.
        `F.median`, `F.percentile`, `F.percentile_approx`, `F.mode`,
        `F.countDistinct` and `F.approx_count_distinct` mix in as well
        (frame/order_agg.py: one global sort per (keys, value columns),
        kernels/group_order.hip); a call that holds only these returns its
        rows in ascending key order, in this frame's number of partitions,
        with the same bits for every partitioning."""
        from .group_agg import group_agg
        return group_agg(self, list(exprs))

    def pivot(self, pivot_col, values=None):
        """One output column per value of `pivot_col` (a name or a plain column
        reference: an int32, int64, float or double scalar column that is no
        grouping key): returns a `PivotedData` whose `agg`, `count`, `sum`,
        `avg` / `mean`, `min` and `max` give one row per key and, per value,
        one column per expression. `values` lists the values, in output order
        (numbers that convert to the column's type without change; NaN is
        allowed, -0.0 means 0.0, no value twice). Without it the distinct
        values are looked up now (`select(pivot_col).distinct()`, collected:
        eager and collective, as in Spark) and come ascending, NaN last. At
        most 1024 values and 4096 output columns. `groupBy()` without keys
        gives one row. See `PivotedData.agg` (frame/pivot.py)."""
        from .pivot import pivot
        return pivot(self, pivot_col, values)

    def sum(self, *cols) -> DataFrame:
        """`agg(F.sum(c), ...)` of the named columns, or of every numeric scalar column that is not a key."""
        from .group_agg import group_stat
        return group_stat(self, "sum", cols)

    def avg(self, *cols) -> DataFrame:
        """`agg(F.avg(c), ...)` of the named columns, or of every numeric scalar column that is not a key."""
        from .group_agg import group_stat
        return group_stat(self, "avg", cols)

    mean = avg

    def min(self, *cols) -> DataFrame:
        """`agg(F.min(c), ...)` of the named columns, or of every numeric scalar column that is not a key."""
        from .group_agg import group_stat
        return group_stat(self, "min", cols)

    def max(self, *cols) -> DataFrame:
        """`agg(F.max(c), ...)` of the named columns, or of every numeric scalar column that is not a key."""
        from .group_agg import group_stat
        return group_stat(self, "max", cols)


def _sort_key(k):
    return tuple((0, v) if isinstance(v, numbers.Number) else (1, str(v)) for v in k)


# ------------------------------------------------------------------ construction
def _bounds(n: int, parts: int, p: int):
    """Row range of partition p when n rows are sliced evenly (Spark parallelize)."""
    return (p * n) // parts, ((p + 1) * n) // parts


def _infer_type(v) -> Optional[DataType]:
    if v is None:
        return None
    if isinstance(v, (bool, np.bool_)):
        return BooleanType()
    if isinstance(v, np.generic):
        return {np.dtype(np.float64): DoubleType(), np.dtype(np.float32): FloatType(),
                np.dtype(np.int32): IntegerType(), np.dtype(np.int64): LongType()}.get(v.dtype, DoubleType())
    if isinstance(v, float):
        return DoubleType()
    if isinstance(v, int):
        return LongType()
    if isinstance(v, str):
        return StringType()
    if isinstance(v, (bytes, bytearray)):
        return BinaryType()
    if isinstance(v, np.ndarray):
        t = _infer_type(v.reshape(-1)[0]) if v.size else DoubleType()
        for _ in range(v.ndim):
            t = ArrayType(t, False)
        return t
    if isinstance(v, (list, tuple)):
        inner = None
        for x in v:
            inner = _infer_type(x)
            if inner is not None:
                break
        return ArrayType(inner or DoubleType(), False)
    raise TypeError(f"cannot infer a column type for value {v!r} of type {type(v).__name__}")


def _tf_of(dt: DataType) -> Optional[int]:
    s = scalar_type_of(dt)
    return s.tf_dtype if isinstance(s, NumericType) else None


def _normalize_rows(data: Sequence[Any], names: Optional[List[str]]):
    rows = data if isinstance(data, list) else list(data)
    if not rows:
        return [], names or []
    r0 = rows[0]
    if isinstance(r0, Row) and r0.__fields__:
        names = names or list(r0.__fields__)
        return rows, names  # Rows are tuples already: no per-row copy
    if isinstance(r0, dict):
        names = names or list(r0.keys())
        return [tuple(r[n] for n in names) for r in rows], names
    if isinstance(r0, tuple):
        names = names or [f"_{i + 1}" for i in range(len(r0))]
        return rows, names
    if isinstance(r0, list):
        names = names or [f"_{i + 1}" for i in range(len(r0))]
        return [tuple(r) for r in rows], names
    names = names or ["value"]
    return [(r,) for r in rows], names


def _validate_all_rows(rows: List[tuple], st: StructType) -> None:
    """Width and null checks over ALL rows. In a multi-rank job every rank
    holds the same local `rows` but packs only its own partitions; checking
    the whole list first makes a bad row fail on every rank before any rank
    enters a collective (instead of one rank raising while the rest block)."""
    ncols = len(st.fields)
    bad = next((r for r in rows if len(r) != ncols), None)
    if bad is not None:
        raise ValueError(f"row {bad} has {len(bad)} values, schema has {ncols} columns")
    for i, f in enumerate(st.fields):
        if any(r[i] is None for r in rows):
            raise ValueError(f"column '{f.name}' contains null values; tensorframes_amd requires "
                             f"non-null columns (the reference silently accepted them)")


def create_dataframe(data, schema=None, num_partitions: Optional[int] = None) -> DataFrame:
    """Build a DataFrame from local data (rows, dicts, tuples, scalars, or a
    dict of column arrays). `schema`: a StructType, a list of column names, or None."""
    nparts = num_partitions or max(1, dist.world_size())
    if isinstance(data, dict):
        return from_columns(data, num_partitions=nparts, schema=schema if isinstance(schema, StructType) else None)
    import sys
    pd = sys.modules.get("pandas")  # a pandas frame can only exist if pandas is loaded
    if pd is not None:
        if isinstance(data, pd.DataFrame):
            return from_columns({c: data[c].to_numpy() if data[c].dtype != object else list(data[c])
                                 for c in data.columns}, num_partitions=nparts)
    names = schema if isinstance(schema, (list, tuple)) else None
    rows, names = _normalize_rows(data, list(names) if names else None)
    if isinstance(schema, StructType):
        st = schema
        names = st.names
    else:
        fields = []
        for i, n in enumerate(names):
            t = None
            for r in rows:
                t = _infer_type(r[i])
                if t is not None:
                    break
            if t is None:
                t = StringType()
            fields.append(StructField(n, t, True))
        st = StructType(fields)
    if not isinstance(rows, list):
        rows = list(rows)
    ncols = len(names)
    blocks = {}
    n = len(rows)
    if dist.world_size() > 1:
        _validate_all_rows(rows, st)  # every rank raises, not only the owner of the bad row
    from .._native import _C
    for p in dist.local_partitions(nparts):
        a, b = _bounds(n, nparts, p)
        cols = {}
        for i, f in enumerate(st.fields):
            tf = _tf_of(f.dataType)
            packed = None
            if tf is not None:
                # native pass over the row tuples (also checks widths and nulls)
                try:
                    packed = _C.pack_column(rows, i, ncols, a, b, tf)
                except ValueError as e:
                    if "wrong width" in str(e):
                        bad = next(r for r in rows[a:b] if len(r) != ncols)
                        raise ValueError(f"row {bad} has {len(bad)} values, schema has {ncols} columns")
                    raise ValueError(f"column '{f.name}' contains null values; tensorframes_amd requires "
                                     f"non-null columns (the reference silently accepted them)")
            if packed is not None:
                cols[f.name] = packed
                continue
            for r in rows[a:b]:
                if len(r) != ncols:
                    raise ValueError(f"row {r} has {len(r)} values, schema has {ncols} columns")
            vals = [r[i] for r in rows[a:b]]
            if any(v is None for v in vals):
                raise ValueError(f"column '{f.name}' contains null values; tensorframes_amd requires "
                                 f"non-null columns (the reference silently accepted them)")
            cols[f.name] = build_column(vals, tf)
        blocks[p] = Block(b - a, cols)
    return DataFrame(st, _Materialized(blocks), nparts)


createDataFrame = create_dataframe  # noqa: N816


def _field_for_array(name: str, arr) -> StructField:
    """Dense whole-column arrays know their cell shape: record it in the
    metadata (lead dim unknown), so no `analyze` pass is needed."""
    if isinstance(arr, StringColumn):
        return StructField(name, BinaryType() if arr.binary else StringType(), False)
    if isinstance(arr, torch.Tensor):
        tf = D.as_dtype(arr.dtype).enum
        shape = tuple(arr.shape)
    else:
        arr = np.asarray(arr)
        if arr.dtype.kind in ("U", "S", "O"):
            return StructField(name, StringType() if arr.dtype.kind != "S" else BinaryType(), False)
        tf = D.as_dtype(arr.dtype).enum
        shape = tuple(arr.shape)
    return tensor_field(name, tf, shape[1:])


def tensor_field(name: str, dtype, cell_shape: Sequence[Optional[int]] = ()) -> StructField:
    """A tensor column field: nested arrays of a numeric type with the block
    shape ``[?, *cell_shape]`` in the metadata."""
    from ..utils.shape import Shape
    tf = D.as_dtype(dtype).enum
    dims = [-1] + [-1 if d is None else int(d) for d in cell_shape]
    return ColumnInformation.struct_field(name, tf, Shape(dims))


def from_columns(columns: Dict[str, Any], num_partitions: Optional[int] = None,
                 schema: Optional[StructType] = None, pinned: bool = False) -> DataFrame:
    """DataFrame from whole-column arrays ``{name: array[rows, *cell]}`` (zero-copy
    for contiguous numpy/torch inputs; `pinned=True` page-locks dense columns)."""
    nparts = num_partitions or max(1, dist.world_size())
    cols = {}
    n = None
    for k, v in columns.items():
        if isinstance(v, (torch.Tensor, StringColumn)):
            t = v
        else:
            a = np.asarray(v)
            if a.dtype.kind in ("U", "S") and a.ndim == 1:
                t = a  # fixed-width strings: Arrow-layout StringColumn per partition, vectorised
            else:
                t = torch.from_numpy(np.asarray(a, order="C")) if a.dtype.kind not in ("U", "S", "O") else list(v)
        ln = t.shape[0] if isinstance(t, (torch.Tensor, np.ndarray)) else len(t)  # StringColumn: rows
        if n is None:
            n = ln
        elif ln != n:
            raise ValueError(f"column {k} has {ln} rows, expected {n}")
        cols[k] = t
    n = n or 0
    st = schema or StructType([_field_for_array(k, v) for k, v in cols.items()])
    blocks = {}
    for p in dist.local_partitions(nparts):
        a, b = _bounds(n, nparts, p)
        bc = {}
        for k, t in cols.items():
            if isinstance(t, torch.Tensor):
                s = t[a:b]
                if pinned:
                    from ..engine import pin
                    s = pin(s)
                bc[k] = s
            elif isinstance(t, np.ndarray):
                bc[k] = StringColumn.from_numpy(t[a:b])
            elif isinstance(t, StringColumn):
                bc[k] = t.slice(a, b)
            else:
                bc[k] = ObjectColumn(t[a:b])
        blocks[p] = Block(b - a, bc)
    return DataFrame(st, _Materialized(blocks), nparts)


def generate(schema: StructType, num_partitions: int, fn: Callable[[int], Block]) -> DataFrame:
    """Lazily generated partitions (synthetic data sets larger than host RAM are
    produced partition by partition, only on the owning rank)."""
    return DataFrame(schema, _Generated(num_partitions, fn), num_partitions)


def range_(n: int, num_partitions: Optional[int] = None, name: str = "id") -> DataFrame:
    """DataFrame of one int64 column `id` = 0..n-1, generated lazily per
    partition (Spark's `sqlContext.range`, used by the reference's perf suite)."""
    nparts = num_partitions or max(1, dist.world_size())

    def fn(p):
        a, b = _bounds(n, nparts, p)
        return Block(b - a, {name: torch.arange(a, b, dtype=torch.int64)})
    return generate(StructType([StructField(name, LongType(), False)]), nparts, fn)
