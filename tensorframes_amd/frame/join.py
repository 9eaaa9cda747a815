"""DataFrame.join: a broadcast equi-join.

The right frame is the build side: every rank materialises it whole, in
global row order (parallel/frame_comm.broadcast_frame, one collective per
`compute`), and every left partition is then probed on its own:

* keys of both sides become the order-preserving words of the sort path
  (equal words are Spark's key equality: NaN joins NaN, -0.0 joins 0.0);
* the build side is sorted once per target (the host, or a device) with the
  stable argsort, so equal keys keep right row order;
* a device-resident left partition runs the kernels of kernels/join.hip
  (probe, scan + expand, row gather); any other partition runs the numpy
  path below, which is also the CPU oracle of the device path.

Output partition p holds the matches of left partition p's rows in left row
order, a left row's matches in the right frame's global row order: the result
is the same for every world size and every partitioning of the right side.
"""
from __future__ import annotations

from typing import Any, Dict, List, Sequence

import numpy as np
import torch

from ..utils import dtypes as D
from .block import Block, StringColumn, col_slice
from .column import Column
from .column_info import ColumnInformation
from .types import BinaryType, StringType, StructType

_TAKE_GROUP = 16  # columns per _C.take_rows call (kernels.h kMaxPackCols)

_INNER = ("inner",)
_SEMI = ("left_semi", "leftsemi", "semi")
_ANTI = ("left_anti", "leftanti", "anti")
_UNSUPPORTED = ("left", "leftouter", "left_outer", "right", "rightouter", "right_outer", "outer", "full",
                "fullouter", "full_outer", "cross")


def _join_kind(how) -> str:
    if not isinstance(how, str):
        raise TypeError(f"join: how must be a string, got {type(how).__name__}")
    h = how.lower()
    if h in _INNER:
        return "inner"
    if h in _SEMI:
        return "semi"
    if h in _ANTI:
        return "anti"
    if h in _UNSUPPORTED:
        raise NotImplementedError(
            f"join: how='{how}' is not supported: an outer join fills the unmatched side with nulls and frames "
            f"cannot hold nulls (docs/MIGRATION.md: \"Nulls are rejected\"); a cross join has no keys. Supported: "
            f"{', '.join(_INNER + _SEMI + _ANTI)}")
    raise ValueError(f"join: unknown join type '{how}'; supported: {', '.join(_INNER + _SEMI + _ANTI)}")


def _key_tf(df, k: str, side: str) -> int:
    """The tf dtype of key column k of `df`, validated like a sort key."""
    from .. import core
    from .dataframe import _SORT_KEY_DTYPES
    f = df.schema[k]
    if isinstance(f.dataType, (StringType, BinaryType)):
        raise core.InvalidTypeException(
            f"join: the key '{k}' of the {side} frame is a {type(f.dataType).__name__[:-4].lower()} column; string "
            f"and binary columns are not supported as join keys yet")
    stf = ColumnInformation(f).stf
    if stf is None:
        raise core.InvalidTypeException(f"join: the type of the key '{k}' of the {side} frame ({f.dataType}) is not "
                                        f"supported as a join key")
    if stf.tf_dtype in (D.DT_HALF, D.DT_BFLOAT16):
        raise core.InvalidTypeException(f"join: the key '{k}' of the {side} frame is {D.dtype_name(stf.tf_dtype)}; "
                                        f"half and bfloat16 columns are not supported as join keys yet (cast to "
                                        f"float)")
    if stf.tf_dtype not in _SORT_KEY_DTYPES:
        raise core.InvalidTypeException(f"join: the key '{k}' of the {side} frame is {D.dtype_name(stf.tf_dtype)}, "
                                        f"which is not supported as a join key")
    if stf.shape.num_dims != 1:
        raise core.InvalidDimensionException(
            f"join: the key '{k}' of the {side} frame holds a cell of rank {max(stf.shape.num_dims - 1, 0)} per "
            f"row, not a scalar; reduce the cell first (.sum(), .max(), ...)")
    return stf.tf_dtype


def _key_columns(b: Block, keys: Sequence[str], side: str) -> List[torch.Tensor]:
    from .. import core
    cols = [b.columns[k] for k in keys]
    for k, c in zip(keys, cols):
        if not isinstance(c, torch.Tensor) or c.dim() != 1:
            raise core.InvalidDimensionException(
                f"join: the key column '{k}' of the {side} frame does not hold one scalar per row; reduce the cell "
                f"first (.sum(), .max(), ...)")
    return cols


class _BuildSide:
    """The right frame's rows (global order) with, per target, its key words
    in sorted order and the stable permutation that sorts them. Prepared
    lazily, once per target, and reused by every left partition."""

    def __init__(self, block: Block, keys: Sequence[str]):
        self.block = block
        self.keys = list(keys)
        self.cols = _key_columns(block, keys, "right")
        self._host = None
        self._dev: Dict[torch.device, tuple] = {}

    def host(self):
        """(sorted words uint64 [W, m], perm int64 [m]) as numpy arrays."""
        from .dataframe import _host_sort_words
        if self._host is None:
            m = self.block.nrows
            if m == 0:
                self._host = (np.zeros((len(self.keys), 0), dtype=np.uint64), np.zeros(0, dtype=np.int64))
            else:
                words = np.stack([_host_sort_words(c, False) for c in self.cols], 0)
                perm = np.lexsort(words[::-1]).astype(np.int64)  # (stable; the last key given is the primary one)
                self._host = (np.ascontiguousarray(words[:, perm]), perm)
        return self._host

    def device(self, dev: torch.device):
        """(sorted words int64 [W, m], perm int64 [m]) on `dev`."""
        from .. import engine
        from .._native import _C
        got = self._dev.get(dev)
        if got is None:
            m = self.block.nrows
            if m == 0:
                got = (engine.device_empty((len(self.keys), 0), torch.int64, dev),
                       engine.device_empty((0,), torch.int64, dev))
            else:
                words = _C.sort_encode([c.to(dev) for c in self.cols], [False] * len(self.cols))
                perm = _C.sort_argsort(words)
                got = (_C.join_gather_words(words, perm), perm)
            self._dev[dev] = got
        return got


def _host_probe(lw: np.ndarray, sw: np.ndarray):
    """lo, cnt (int64 [n]) of left words [W, n] in the sorted build words
    [W, m]: both sides' tuples are factorised together (one lexsort), the
    tuple ids of the build side are then ascending and searchsorted gives
    each left row's run of equal tuples."""
    n, m = lw.shape[1], sw.shape[1]
    if n == 0 or m == 0:
        return np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    if lw.shape[0] == 1:
        rid, lid = sw[0], lw[0]
    else:
        both = np.concatenate([sw, lw], 1)
        order = np.lexsort(both[::-1])
        srt = both[:, order]
        new = np.concatenate([[False], (srt[:, 1:] != srt[:, :-1]).any(0)])
        ids = np.empty(n + m, dtype=np.int64)
        ids[order] = np.cumsum(new)
        rid, lid = ids[:m], ids[m:]
    lo = np.searchsorted(rid, lid, side="left").astype(np.int64)
    hi = np.searchsorted(rid, lid, side="right").astype(np.int64)
    return lo, hi - lo


def _take_block(b: Block, names: Sequence[str], idx) -> Dict[str, Any]:
    """Rows idx (a device int64 tensor or a numpy array; any length, repeats
    allowed) of the named columns of `b`: device dense columns through the row
    gather kernel, 16 per call, device strings through the string gather;
    whatever lives on the host is indexed there."""
    from .._native import _C
    cols: Dict[str, Any] = {}
    on_dev = isinstance(idx, torch.Tensor) and idx.is_cuda
    dev_dense = [n for n in names if on_dev and isinstance(b.columns[n], torch.Tensor)
                 and b.columns[n].device == idx.device and b.columns[n].dim() >= 1]
    for g in range(0, len(dev_dense), _TAKE_GROUP):
        group = dev_dense[g:g + _TAKE_GROUP]
        cols.update(zip(group, _C.take_rows(idx, [b.columns[n] for n in group])))
    host_t = host_np = None
    for n in names:
        if n in cols:
            continue
        c = b.columns[n]
        if host_t is None:
            host_t = idx.cpu() if isinstance(idx, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(idx))
            host_np = host_t.numpy()
        if isinstance(c, StringColumn) and c.is_cuda:
            di = idx if on_dev and idx.device == c.device else host_t.to(c.device)
            offs, data = _C.gather_strings(c.offsets, c.data, di)
            cols[n] = StringColumn(offs.to(c.device), data, c.binary)
        elif isinstance(c, torch.Tensor):
            cols[n] = c.index_select(0, host_t.to(c.device))
        else:
            cols[n] = c.take(host_np)
    return cols


def _join_frame(left, right, on, how):
    """The lazy frame of `left.join(right, on, how)`: everything is validated
    here (typed errors); the build side is gathered when the frame is computed."""
    from .. import core
    from ..utils.logging import metrics
    from .dataframe import _MAX_SORT_KEYS, DataFrame, _Derived, _filter_block, _host_sort_words
    if not isinstance(right, DataFrame):
        raise TypeError(f"join: a DataFrame is expected as the right side, got {type(right).__name__}")
    kind = _join_kind(how)
    if on is None or isinstance(on, Column) or (isinstance(on, (list, tuple))
                                                and any(isinstance(k, Column) for k in on)):
        raise TypeError("join: only column names are supported as join keys (on='k' or on=['k1', 'k2']), not "
                        "Column conditions or on=None; give both frames' key columns one name first "
                        "(withColumnRenamed)")
    keys = [on] if isinstance(on, str) else list(on) if isinstance(on, (list, tuple)) else None
    if keys is None or not all(isinstance(k, str) for k in keys):
        raise TypeError(f"join: on must be a column name or a list of column names, got {on!r}; only name keys "
                        f"are supported (withColumnRenamed gives both sides one name)")
    if not keys:
        raise ValueError("join: at least one key column is expected")
    if len(keys) > _MAX_SORT_KEYS:
        raise ValueError(f"join: at most {_MAX_SORT_KEYS} key columns, got {len(keys)}")
    if len(set(keys)) != len(keys):
        raise ValueError(f"join: duplicate key names in {keys}")
    for k in keys:
        if k not in left.schema:
            raise ValueError(f"join: key column {k} not found in the left frame's {left.columns}")
        if k not in right.schema:
            raise ValueError(f"join: key column {k} not found in the right frame's {right.columns}")
    for k in keys:
        lt, rt = _key_tf(left, k, "left"), _key_tf(right, k, "right")
        if lt != rt:
            raise core.InvalidTypeException(
                f"join: the key '{k}' is {D.dtype_name(lt)} in the left frame and {D.dtype_name(rt)} in the right "
                f"frame; .cast one side to the other's type first")
    left_rest = [c for c in left.columns if c not in keys]
    right_rest = [c for c in right.columns if c not in keys]
    if kind == "inner":
        clash = [c for c in left_rest if c in right_rest]
        if clash:
            raise ValueError(f"join: the columns {clash} exist in both frames and are not join keys; the result "
                             f"would hold ambiguous columns. Rename or drop them on one side first")
        schema = StructType([left.schema[k] for k in keys] + [left.schema[c] for c in left_rest]
                            + [right.schema[c] for c in right_rest])
        need = keys + right_rest  # what travels of the build side
    else:
        schema = left.schema
        need = keys
    out_names = schema.names
    build_frame = right.select(need)
    build_schema, build_nparts = build_frame.schema, build_frame.num_partitions

    def join_block(b: Block, build: _BuildSide, stats: List[int]) -> Block:
        from .._native import _C
        m = build.block.nrows
        stats[0] += b.nrows
        if b.nrows == 0:
            if kind != "inner":
                return b
            cols = {n: b.columns[n] for n in keys + left_rest}
            cols.update({n: col_slice(build.block.columns[n], 0, 0) for n in right_rest})
            return Block(0, cols)
        lcols = _key_columns(b, keys, "left")
        on_dev = all(c.is_cuda for c in lcols) and len({c.device for c in lcols}) == 1
        if on_dev:
            dev = lcols[0].device
            sw, perm = build.device(dev)
            lw = _C.sort_encode(lcols, [False] * len(lcols))
            lo, cnt, mask = _C.join_probe(lw, sw, {"inner": 0, "semi": 1, "anti": 2}[kind])
            if kind != "inner":
                out = _filter_block(b, mask)
                stats[1] += out.nrows
                return out
            li, ri, _ = _C.join_expand(lo, cnt, perm)
        else:
            sw, perm = build.host()
            lw = np.stack([_host_sort_words(c, False) for c in lcols], 0)
            lo, cnt = _host_probe(lw, sw)
            if kind != "inner":
                keep = torch.from_numpy(cnt != 0 if kind == "semi" else cnt == 0)
                out = _filter_block(b, keep)
                stats[1] += out.nrows
                return out
            offs = np.zeros(b.nrows + 1, dtype=np.int64)
            np.cumsum(cnt, out=offs[1:])
            li = np.repeat(np.arange(b.nrows, dtype=np.int64), cnt)
            ri = perm[lo[li] + (np.arange(int(offs[-1]), dtype=np.int64) - offs[li])] if m else \
                np.zeros(0, dtype=np.int64)
        total = int(li.shape[0])
        stats[1] += total
        cols = _take_block(b, keys + left_rest, li)
        cols.update(_take_block(build.block, right_rest, ri))
        return Block(total, {n: cols[n] for n in out_names})

    def compute(blocks: Dict[int, Block]) -> Dict[int, Block]:
        from ..parallel import frame_comm
        rng = torch.cuda.is_initialized()
        if rng:
            torch.cuda.nvtx.range_push("tfa.join")
        try:
            # the build side: a collective, entered by every rank whatever it owns of the left side
            whole = frame_comm.broadcast_frame(build_frame._blocks(), need, build_schema, build_nparts)
            build = _BuildSide(whole, keys)
            stats = [0, 0]  # left rows probed, rows out
            res = {pid: join_block(blocks[pid], build, stats) for pid in sorted(blocks)}
        finally:
            if rng:
                torch.cuda.nvtx.range_pop()
        metrics.add("join_rows_left", stats[0])
        metrics.add("join_rows_build", whole.nrows)
        metrics.add("join_rows_out", stats[1])
        return res

    return DataFrame(schema, _Derived(left, compute, streamable=False), left.num_partitions)
