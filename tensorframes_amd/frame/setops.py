"""DataFrame.union / unionByName, dropDuplicates / distinct, intersect / subtract.

The set operations are sort-based: ordering, adjacent comparison and
compaction, on the foundations of `orderBy` (order-preserving key words, the
stable radix argsort, the row gather, the sample-sort exchange). Two documented
properties of the sort carry the semantics:

* it is stable and ties keep input order (partition order, then row order), so
  the first row of a run of equal key tuples is the first occurrence;
* the exchange cuts at lower bounds of splitter tuples, so rows with equal key
  tuples land in one partition.

`dropDuplicates` per local partition sorts, keeps the head of every run and
gathers only those rows: the exchange moves at most the locally distinct rows.
What arrives (pieces in source-partition order) is sorted and reduced once
more. Device-resident partitions use kernels/sort.hip and kernels/unique.hip;
any other partition runs the numpy path below, which is also the CPU oracle of
the device path.
"""
from __future__ import annotations

from typing import Dict, List, Sequence

import numpy as np
import torch

from ..parallel import dist
from ..utils import dtypes as D
from ..utils.shape import UNKNOWN
from .block import Block
from .column_info import SHAPE_KEY, ColumnInformation, SparkTFColInfo
from .types import StructType
from .window import _device_cached, refuse_window_expression


def _device_backed(df) -> bool:
    """A frame cached on the device, or derived from such frames without an
    action in between (a projection, a union): what is computed from it stays
    on the device, also when an exchange between ranks staged rows through
    the host."""
    from .dataframe import _Derived, _Union
    if df._cached is not None:
        return _device_cached(df)
    src = df._source
    if isinstance(src, _Derived):
        return _device_backed(src._parent)
    if isinstance(src, _Union):
        return _device_backed(src._left) and _device_backed(src._right)
    return False


# ------------------------------------------------------------------ distinct
def _heads(words, perm):
    """The source rows perm[i] of the positions i that start a run of equal
    word tuples in the sorted order, in order (`_C.unique_rows` in numpy)."""
    if isinstance(words, torch.Tensor):
        from .._native import _C
        return _C.unique_rows(words, perm)
    if words.shape[1] == 0:
        return np.zeros(0, dtype=np.int64)
    sw = words[:, perm]
    head = np.concatenate([[True], (sw[:, 1:] != sw[:, :-1]).any(0)])
    return perm[head]


def _words_of_rows(words, rows):
    """words[:, rows] ([W, m])."""
    if isinstance(words, torch.Tensor):
        from .._native import _C
        return torch.stack(_C.take_rows(rows, [words[w] for w in range(words.shape[0])]), 0)
    return words[:, rows]


def _distinct_block(b: Block, names: Sequence[str], keys: Sequence[str]):
    """(the first row of every distinct key tuple of `b` in the order of the
    tuples, their words [W, m]); device tensors for a device partition."""
    from .dataframe import _sort_order_of
    from .join import _take_block
    words, perm, _ = _sort_order_of(b, keys, [False] * len(keys))
    if b.nrows == 0:
        return b, words
    kept = _heads(words, perm)
    m = int(kept.shape[0])
    return Block(m, _take_block(b, names, kept)), _words_of_rows(words, kept)


def _distinct_blocks(blocks: Dict[int, Block], names: Sequence[str], schema: StructType, nparts: int,
                     keys: Sequence[str], keep_on_device: bool, stats: Dict[str, int]) -> Dict[int, Block]:
    """dropDuplicates over this rank's partitions (collective): orderBy's
    sample sort with the duplicates dropped on both sides of the exchange."""
    from .. import engine
    from ..parallel import frame_comm
    from .dataframe import _SORT_SAMPLES_PER_PARTITION, _lower_bounds
    W = len(keys)
    local: Dict[int, Block] = {}
    swords: Dict[int, object] = {}
    samples = []
    take_max = _SORT_SAMPLES_PER_PARTITION * nparts
    for pid in sorted(blocks):
        b = blocks[pid]
        stats["distinct_rows_in"] += b.nrows
        local[pid], swords[pid] = _distinct_block(b, names, keys)
        on_dev = isinstance(swords[pid], torch.Tensor)
        if b.nrows:
            stats["distinct_device_partitions" if on_dev else "distinct_host_partitions"] += 1
        m = local[pid].nrows
        stats["distinct_rows_exchanged"] += m
        if m:
            # evenly spaced survivors (no RNG: the same on every run)
            take = min(m, take_max)
            pos = np.array([((2 * j + 1) * m) // (2 * take) for j in range(take)], dtype=np.int64)
            if on_dev:
                sw = swords[pid]
                samples.append(sw[:, torch.from_numpy(pos).to(sw.device)].cpu().numpy().view(np.uint64).T)
            else:
                samples.append(swords[pid][:, pos].T)
    mine = np.concatenate(samples, 0) if samples else np.zeros((0, W), dtype=np.uint64)
    every = np.concatenate(dist.all_gather_object(mine), 0) if dist.is_distributed() else mine
    if len(every) and nparts > 1:
        every = every[np.lexsort(every.T[::-1])]
        splitters = np.stack([every[(q * len(every)) // nparts] for q in range(1, nparts)], 0)
    else:
        splitters = np.zeros((0, W), dtype=np.uint64)
    # contiguous slices of every partition's survivors, one per output partition
    table = torch.zeros((nparts, max(nparts, 1)), dtype=torch.int64)
    for pid, b in local.items():
        m = b.nrows
        if m and len(splitters):
            sw = swords[pid]
            ident = torch.arange(m, dtype=torch.int64, device=sw.device) if isinstance(sw, torch.Tensor) else \
                np.arange(m, dtype=np.int64)
            cuts = [0] + _lower_bounds(sw, ident, splitters) + [m]
        else:
            cuts = [0] + [0] * (nparts - 1) + [m]
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
    # the pieces arrived in source-partition order: the stable sort puts the
    # earliest partition's row first in every run
    res: Dict[int, Block] = {}
    ends = torch.zeros((nparts, 1 + 2 * W), dtype=torch.int64)
    for q in sorted(got):
        b = got[q]
        if keep_on_device and engine.gpu_available():
            # (an exchange between ranks may have staged the rows through the host)
            b = b.to(engine.compute_device())
        res[q], sw = _distinct_block(b, names, keys)
        m = res[q].nrows
        stats["distinct_rows_kept"] += m
        if m:
            if isinstance(sw, torch.Tensor):
                fl = sw[:, [0, m - 1]].cpu().numpy()
            else:
                fl = np.ascontiguousarray(sw[:, [0, m - 1]]).view(np.int64)
            ends[q, 0] = m
            ends[q, 1:1 + W] = torch.from_numpy(np.ascontiguousarray(fl[:, 0]))
            ends[q, 1 + W:] = torch.from_numpy(np.ascontiguousarray(fl[:, 1]))
    dist.all_reduce_host_(ends, "Sum")  # (every rank fills the rows of its own partitions)
    last = None
    for q, row in enumerate(ends.tolist()):
        if row[0] == 0:
            continue
        if last is not None and row[1:1 + W] == last:
            raise RuntimeError(f"distinct: internal error: the last row of an earlier partition and the first row "
                               f"of partition {q} have equal keys, so a duplicate survives; the exchange is "
                               f"expected to keep equal key tuples in one partition")
        last = row[1 + W:]
    return res


_METRICS = ("distinct_rows_in", "distinct_rows_exchanged", "distinct_rows_kept", "distinct_device_partitions",
            "distinct_host_partitions")


def _distinct_frame(df, subset, what: str):
    """The lazy frame of dropDuplicates / distinct: everything is validated
    here (typed errors)."""
    from ..utils.logging import metrics
    from .dataframe import _MAX_SORT_KEYS, DataFrame, _check_sort_key, _Derived
    refuse_window_expression(what, [subset] if subset is not None else [])
    if subset is None:
        keys = list(df.columns)
    else:
        if isinstance(subset, str) or not isinstance(subset, (list, tuple)):
            raise TypeError(f"{what}: subset must be a list of column names, got {subset!r}")
        if not all(isinstance(k, str) for k in subset):
            raise TypeError(f"{what}: subset must hold column names, got {subset!r}")
        if not subset:
            raise ValueError(f"{what}: an empty subset names no key column; leave it out to compare every column")
        keys = list(dict.fromkeys(subset))
    for k in keys:
        if k not in df.schema:
            raise ValueError(f"{what}: column {k} not found in {df.columns}")
    if not keys:
        raise ValueError(f"{what}: the frame has no columns")
    if len(keys) > _MAX_SORT_KEYS:
        raise ValueError(f"{what}: at most {_MAX_SORT_KEYS} key columns, got {len(keys)}"
                         + ("" if subset is not None else "; name the columns that identify a row in "
                                                          "dropDuplicates(subset)"))
    for k in keys:
        _check_sort_key(df.schema[k], k, what)
    names, schema, nparts = df.columns, df.schema, df.num_partitions
    keep_on_device = _device_backed(df)

    def compute(blocks: Dict[int, Block]) -> Dict[int, Block]:
        stats = {m: 0 for m in _METRICS}
        rng = torch.cuda.is_initialized()
        if rng:
            torch.cuda.nvtx.range_push("tfa.distinct")
        try:
            res = _distinct_blocks(blocks, names, schema, nparts, keys, keep_on_device, stats)
        finally:
            if rng:
                torch.cuda.nvtx.range_pop()
        for m in _METRICS:
            metrics.add(m, stats[m])
        return res

    def compute_agreed(blocks):
        return dist.agreed(what, lambda: compute(blocks))

    return DataFrame(schema, _Derived(df, compute_agreed, streamable=False), nparts)


# ------------------------------------------------------------------ union
def _paired_fields(left, right, by_name: bool, what: str):
    """[(left field, right field)] in the left frame's column order, the types
    checked: equal SQL types (no implicit widening), cell shapes that agree."""
    from .. import core
    from .dataframe import DataFrame
    if not isinstance(right, DataFrame):
        raise TypeError(f"{what}: a DataFrame is expected, got {type(right).__name__}")
    lf, rf = left.schema.fields, right.schema.fields
    if by_name:
        missing = [f.name for f in lf if f.name not in right.schema]
        extra = [f.name for f in rf if f.name not in left.schema]
        if missing or extra:
            raise ValueError(f"{what}: the other frame lacks the columns {missing} and holds the unknown columns "
                             f"{extra}; both frames must hold the same column names")
        rf = [right.schema[f.name] for f in lf]
    elif len(lf) != len(rf):
        raise ValueError(f"{what}: this frame has {len(lf)} columns ({', '.join(left.columns)}), the other "
                         f"{len(rf)} ({', '.join(right.columns)}); columns are resolved by position")
    for a, b in zip(lf, rf):
        sa, sb = ColumnInformation(a).stf, ColumnInformation(b).stf
        if a.dataType != b.dataType or (sa is None) != (sb is None) or \
                (sa is not None and sa.tf_dtype != sb.tf_dtype):
            ta = a.dataType.simpleString() if sa is None else f"{a.dataType.simpleString()} ({D.dtype_name(sa.tf_dtype)})"
            tb = b.dataType.simpleString() if sb is None else f"{b.dataType.simpleString()} ({D.dtype_name(sb.tf_dtype)})"
            raise core.InvalidTypeException(
                f"{what}: column '{a.name}' is {ta} in this frame and {tb} in the other ('{b.name}'); there is no "
                f"implicit widening: .cast() one side to the other's type first")
        if sa is not None:
            ca, cb = sa.shape.tail(), sb.shape.tail()
            if ca.num_dims != cb.num_dims or any(x != y and UNKNOWN not in (x, y) for x, y in zip(ca, cb)):
                raise core.InvalidDimensionException(
                    f"{what}: the cells of column '{a.name}' have shape {ca} in this frame and {cb} in the other "
                    f"('{b.name}'); the cell shapes must agree")
    return list(zip(lf, rf))


def _union_frame(left, right, by_name: bool, what: str):
    """The lazy frame of union / unionByName."""
    from .dataframe import DataFrame, _Union
    pairs = _paired_fields(left, right, by_name, what)
    fields = []
    for a, b in pairs:
        if SHAPE_KEY in a.metadata:
            # the lead dimension (rows of a block) is no longer known; a cell
            # dimension stays where both sides state the same one
            sa, sb = ColumnInformation(a).stf, ColumnInformation(b).stf
            cell = sa.shape.tail().merge(sb.shape.tail())
            a = ColumnInformation.with_info(a, SparkTFColInfo(cell.prepend(UNKNOWN), sa.dataType)).merged()
        fields.append(a)
    rename = [(a.name, b.name) for a, b in pairs]

    def relabel(blk: Block) -> Block:
        return Block(blk.nrows, {ln: blk.columns[rn] for ln, rn in rename})

    return DataFrame(StructType(fields), _Union(left, right, relabel, _device_backed(right)),
                     left.num_partitions + right.num_partitions)


# ------------------------------------------------------------------ intersect / subtract
def _semi_frame(left, right, how: str, what: str):
    """distinct(), then the left-semi / left-anti broadcast join on all columns."""
    _paired_fields(left, right, False, what)
    return _distinct_frame(left, None, what).join(right.toDF(*left.columns), list(left.columns), how)
