"""The holistic aggregates of `GroupedData.agg` / `DataFrame.agg`: median /
percentile, percentile_approx, mode and countDistinct. They need a group's
rows in order, so they do not fold into the mergeable records of group_agg.py.

    scored.groupBy("id").agg(F.median("score"), F.countDistinct("label"), F.avg("score"))

The order aggregates of a call are grouped by their sort (keys..., value
columns). Per sort the frame is projected to those columns and sorted
globally, ascending, with orderBy's sample sort, into the input's number of
partitions. Then

* every partition with rows is summarised on its own from the words of its
  sorted columns (`_C.sort_encode`, or numpy on the host), P key words and W
  in all: per group its start row, its rows, its distinct count (the peer
  heads) and its first longest peer run (`_C.group_order_summary`, or
  `_host_summary`).
* every partition contributes one int64 record (its row count, whether it is
  a single group, the words of its first and of its last row, and rows,
  distinct count, mode length and mode word of its first and of its last
  group) to an [nparts, ...] table that crosses ranks with one host
  all-reduce. Every rank folds the records in ascending partition order,
  skipping empty partitions: rows and distinct counts add, the mode is the
  longer run and on a tie the earlier piece, which holds the smaller word.
* a group wholly inside a partition gets its values from
  `_C.group_order_finish` (or `_host_finish`). A group that spans partitions
  (at most nparts - 1 of them) has its total from the fold; the partition
  whose piece holds a wanted rank reads that word (one small read per
  partition), a second table crosses ranks, and the group's values are
  computed on the host with the same formulas and written into the group's
  row, in the partition where the group starts.

The sample sort cuts its slices at lower bounds of full key tuples, so rows
with an equal full tuple land in one partition: peer runs never span
partitions, groups may. The fold checks this and raises rather than return a
wrong distinct count.

The result holds one row per group in ascending key order, a group's row in
the partition that holds the group's first sorted row. Every output bit is the
same for every partitioning of the same rows and every world size: everything
is an integer or a word except the interpolation of `percentile`, whose
operands do not depend on the partitioning.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ..functions import OrderAggregateExpression
from ..parallel import dist
from ..utils import dtypes as D
from ._scalar_columns import _block_on_device, _decode_sort_word, _ineligible, _scalar_column, _tf_dtype
from .block import Block
from .column import Column

_MAX_OUTPUTS = 16  # kernels.h kMaxPackCols: outputs per _C.group_order_finish call
_MAX_SORT_WORDS = 8  # kernels.h kMaxSortKeys
_LOW32 = 0xFFFFFFFF
_QNAN = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]
_RANKED = ("percentile", "percentile_approx")


# ------------------------------------------------------------------ the formulas
def _approx_rank(p: float, rows: np.ndarray) -> np.ndarray:
    """The 0-based rank max(ceil(p N) - 1, 0) for every N of int64 `rows` (f64 arithmetic)."""
    r = np.ceil(np.float64(p) * rows.astype(np.float64)) - 1.0
    return np.clip(r.astype(np.int64), 0, np.maximum(rows - 1, 0))


def _exact_position(p: float, rows: np.ndarray):
    """(pos, lo, hi) of Spark's Percentile for every N of `rows`: pos = p (N - 1) in f64."""
    pos = np.float64(p) * (rows - 1).astype(np.float64)
    return pos, np.floor(pos), np.ceil(pos)


def _interpolate(pos, lo, hi, v_lo, v_hi) -> np.ndarray:
    """v_lo where lo == hi, otherwise (hi - pos) v_lo + (pos - lo) v_hi: two
    rounded products and one rounded sum (numpy contracts nothing). A NaN
    leaves as the quiet NaN."""
    with np.errstate(all="ignore"):
        v = np.where(lo == hi, v_lo, (hi - pos) * v_lo + (pos - lo) * v_hi)
    return np.where(np.isnan(v), _QNAN, v).astype(np.float64)


def _word_values(words: np.ndarray, np_dt: np.dtype) -> np.ndarray:
    return np.asarray(_decode_sort_word(np.asarray(words, dtype=np.uint64), np_dt)).reshape(-1).astype(np_dt)


# ------------------------------------------------------------------ one partition on the host
def _host_summary(words: np.ndarray, P: int):
    """`_C.group_order_summary` in numpy: (starts [ng + 1], distinct [ng],
    mode_pos [ng], mode_len [ng]) of the uint64 words [W, n], n >= 1."""
    W, n = words.shape
    ghead = np.zeros(n, dtype=bool)
    phead = np.zeros(n, dtype=bool)
    for w in range(W):
        d = words[w, 1:] != words[w, :-1]
        phead[1:] |= d
        if w < P:
            ghead[1:] |= d
    ghead[0] = phead[0] = True
    heads = np.nonzero(ghead)[0].astype(np.int64)
    starts = np.append(heads, np.int64(n))
    distinct = np.add.reduceat(phead.astype(np.int64), heads)
    runs = np.nonzero(phead)[0].astype(np.int64)          # the head row of every peer run
    lens = np.diff(np.append(runs, np.int64(n)))
    # the longer run, then the earlier head (kernels/group_order.hip mode_key)
    key = (lens.astype(np.uint64) << np.uint64(32)) | (np.uint64(_LOW32) - runs.astype(np.uint64))
    best = np.maximum.reduceat(key, np.searchsorted(runs, heads))
    mode_len = (best >> np.uint64(32)).astype(np.int64)
    mode_pos = (np.uint64(_LOW32) - (best & np.uint64(_LOW32))).astype(np.int64)
    return starts, distinct, mode_pos, mode_len


def _host_finish(vwords: np.ndarray, starts: np.ndarray, distinct: np.ndarray, mode_pos: np.ndarray,
                 fns: Sequence[str], pcts: Sequence[Sequence[float]], np_dt: np.dtype) -> List[np.ndarray]:
    """`_C.group_order_finish` in numpy: one [ng] or [ng, Q] array per output."""
    a = starts[:-1]
    rows = np.diff(starts)
    outs = []
    for fn, ps in zip(fns, pcts):
        if fn == "count_distinct":
            outs.append(distinct.astype(np.int64))
        elif fn == "mode":
            outs.append(_word_values(vwords[mode_pos], np_dt))
        elif fn == "percentile_approx":
            outs.append(np.stack([_word_values(vwords[a + _approx_rank(p, rows)], np_dt) for p in ps], 1))
        else:
            cols = []
            for p in ps:
                pos, lo, hi = _exact_position(p, rows)
                v_lo = _word_values(vwords[a + lo.astype(np.int64)], np_dt).astype(np.float64)
                v_hi = _word_values(vwords[a + hi.astype(np.int64)], np_dt).astype(np.float64)
                cols.append(_interpolate(pos, lo, hi, v_lo, v_hi))
            outs.append(np.stack(cols, 1))
    return outs


# ------------------------------------------------------------------ the fold
_REC = 4  # a group's partial: rows, distinct count, mode length, mode word


def _fold(table: np.ndarray, W: int, P: int):
    """table int64 [nparts, 2 + 2 W + 8]: per partition nrows, single group,
    the words of the first and of the last row, (rows, distinct count, mode
    length, mode word) of the first and of the last group.
    -> (continues [nparts] bool: the partition's first group began earlier,
        spans: one dict per group that spans partitions, in order: `pieces`
        [(partition, first local row, rows)], `rows`, `distinct`, `mode_word`).
    The fold runs in ascending partition order over the partitions that hold
    rows."""
    nparts = table.shape[0]
    u = table.view(np.uint64)
    continues = [False] * nparts
    spans: List[dict] = []
    open_key = None   # the first P words of the group that is still open
    last_row = None   # all W words of the last row seen
    cur: Optional[dict] = None

    def close():
        if cur is not None and len(cur["pieces"]) > 1:
            spans.append(cur)

    for p in range(nparts):
        nrows = int(table[p, 0])
        if nrows == 0:
            continue
        single = bool(table[p, 1])
        fw = [int(x) for x in u[p, 2:2 + W]]
        lw = [int(x) for x in u[p, 2 + W:2 + 2 * W]]
        first = [int(x) for x in u[p, 2 + 2 * W:2 + 2 * W + _REC]]
        last = [int(x) for x in u[p, 2 + 2 * W + _REC:2 + 2 * W + 2 * _REC]]
        if last_row is not None and fw == last_row:
            raise RuntimeError(f"agg: internal error: the rows at the end of an earlier partition and at the start "
                               f"of partition {p} have equal (keys, values), so a run of equal tuples spans "
                               f"partitions; the sort is expected to keep equal tuples in one partition")
        goes_on = open_key is not None and fw[:P] == open_key
        if goes_on:
            continues[p] = True
            cur["pieces"].append((p, 0, first[0]))
            cur["rows"] += first[0]
            cur["distinct"] += first[1]
            if first[2] > cur["mode_len"]:  # (a tie: the earlier piece, which holds the smaller word)
                cur["mode_len"], cur["mode_word"] = first[2], first[3]
        if not (goes_on and single):  # the open group ends before this partition's last group
            close()
            cur = dict(pieces=[(p, nrows - last[0], last[0])], rows=last[0], distinct=last[1], mode_len=last[2],
                       mode_word=last[3])
        open_key, last_row = lw[:P], lw
    close()
    return continues, spans


# ------------------------------------------------------------------ one sort
class _Out:
    """One output column of a sort: `fn` over the sort's value columns."""

    def __init__(self, name: str, e: OrderAggregateExpression, value_dtype: torch.dtype):
        self.name, self.fn, self.ps, self.is_list = name, e.fn, list(e.percentages), e.is_list
        self.dtype = torch.int64 if e.fn == "count_distinct" else (torch.float64 if e.fn == "percentile"
                                                                  else value_dtype)
        self.shape = [len(self.ps)] if (e.fn in _RANKED and e.is_list) else []


def _spanning_values(span: dict, outs: Sequence[_Out], words_at: Dict[int, int], np_dt: np.dtype) -> List[np.ndarray]:
    """The outputs of a group that spans partitions, one row: the formulas of
    `_host_finish` over the folded totals and the words read at the wanted
    ranks (`words_at`: rank in the group -> word)."""
    rows = np.array([span["rows"]], dtype=np.int64)
    vals = []
    for o in outs:
        if o.fn == "count_distinct":
            vals.append(np.array([span["distinct"]], dtype=np.int64))
        elif o.fn == "mode":
            vals.append(_word_values(np.array([span["mode_word"]], dtype=np.uint64), np_dt))
        elif o.fn == "percentile_approx":
            w = [words_at[int(_approx_rank(p, rows)[0])] for p in o.ps]
            vals.append(_word_values(np.array(w, dtype=np.uint64), np_dt).reshape(1, -1))
        else:
            got = []
            for p in o.ps:
                pos, lo, hi = _exact_position(p, rows)
                v_lo = _word_values(np.array([words_at[int(lo[0])]], dtype=np.uint64), np_dt).astype(np.float64)
                v_hi = _word_values(np.array([words_at[int(hi[0])]], dtype=np.uint64), np_dt).astype(np.float64)
                got.append(_interpolate(pos, lo, hi, v_lo, v_hi))
            vals.append(np.stack(got, 1))
    return vals


def _wanted_ranks(span: dict, outs: Sequence[_Out]) -> List[int]:
    rows = np.array([span["rows"]], dtype=np.int64)
    want = set()
    for o in outs:
        for p in o.ps:
            if o.fn == "percentile_approx":
                want.add(int(_approx_rank(p, rows)[0]))
            elif o.fn == "percentile":
                _, lo, hi = _exact_position(p, rows)
                want.update((int(lo[0]), int(hi[0])))
    return sorted(want)


def _sort_frame_of(df, keys: Sequence[str], vcols: Sequence[str], members: Sequence[Tuple[str, OrderAggregateExpression]],
                   what: str, keep_on_device: bool):
    """The lazy frame keys + one column per (name, expression) of `members`,
    which all share the sort (keys..., vcols)."""
    from .. import engine
    from ..utils.logging import metrics
    from .dataframe import DataFrame, _Derived, _host_sort_words, _sort_frame, tensor_field
    from .types import StructType
    sort_cols = list(keys) + [v for v in vcols if v not in keys]
    word_cols = list(keys) + list(vcols)
    P, W = len(keys), len(word_cols)
    vdt = D.torch_dtype(_tf_dtype(df, vcols[-1]))
    np_dt = torch.empty(0, dtype=vdt).numpy().dtype
    kdt = [D.torch_dtype(_tf_dtype(df, k)) for k in keys]
    outs = [_Out(name, e, vdt) for name, e in members]
    fns = [o.fn for o in outs]
    pcts = [o.ps if o.fn in _RANKED else [] for o in outs]
    srt = _sort_frame(df.select(*sort_cols), [Column._ref(c).asc() for c in sort_cols], True, True, what)
    nparts = df.num_partitions
    width = 2 + 2 * W + 2 * _REC

    def summarise(b: Block):
        """(on_device, words, (starts, distinct, mode_pos, mode_len), record) of one partition with rows."""
        n = b.nrows
        if n >= (1 << 31):
            raise ValueError(f"{what}: a partition of {n} rows does not fit; the order aggregates index the rows of "
                             f"one partition in 32 bits (repartition into more partitions)")
        cols = [_scalar_column(b, c, what) for c in word_cols]
        on_device = engine.gpu_available() and _block_on_device(b, sort_cols)
        rec = np.zeros(width, dtype=np.int64)
        if on_device:
            from .._native import _C
            words = _C.sort_encode([c.contiguous() for c in cols], [False] * W)
            summ = _C.group_order_summary(words, P)
            starts, distinct, mode_pos, mode_len = summ
            ng = int(starts.shape[0]) - 1
            ends = torch.tensor([0, ng - 1], device=words.device)
            small = torch.cat([words[:, 0], words[:, n - 1], starts[1:2], starts[ng - 1:ng],
                               distinct.index_select(0, ends), mode_len.index_select(0, ends),
                               words[W - 1].index_select(0, mode_pos.index_select(0, ends))]).cpu().numpy()
            metrics.add("order_agg_device_partitions")
        else:
            words = np.stack([_host_sort_words(c, False) for c in cols], 0)
            summ = _host_summary(words, P)
            starts, distinct, mode_pos, mode_len = summ
            ng = len(starts) - 1
            ends = np.array([0, ng - 1])
            small = np.concatenate([words[:, 0].view(np.int64), words[:, n - 1].view(np.int64), starts[1:2],
                                    starts[ng - 1:ng], distinct[ends], mode_len[ends],
                                    words[W - 1][mode_pos[ends]].view(np.int64)])
            metrics.add("order_agg_host_partitions")
        rec[0], rec[1] = n, int(ng == 1)
        rec[2:2 + 2 * W] = small[:2 * W]
        first_rows, last_start, d0, d1, l0, l1, w0, w1 = (int(x) for x in small[2 * W:])
        rec[2 + 2 * W:] = [first_rows, d0, l0, w0, n - last_start, d1, l1, w1]
        return on_device, words, summ, rec

    def read_words(on_device: bool, words, rows: Sequence[int]) -> np.ndarray:
        """The value words of the local rows `rows`: one small read."""
        if on_device:
            at = torch.tensor(list(rows), dtype=torch.int64, device=words.device)
            return words[W - 1].index_select(0, at).cpu().numpy().view(np.uint64)
        return words[W - 1][np.asarray(list(rows), dtype=np.int64)]

    def emit(b: Block, on_device: bool, words, summ, drop_first: bool, patch: Optional[List[np.ndarray]]) -> Block:
        starts, distinct, mode_pos, mode_len = summ
        made: List[Any] = []
        if on_device:
            from .._native import _C
            for a in range(0, len(outs), _MAX_OUTPUTS):
                made.extend(_C.group_order_finish(words, starts, distinct, mode_pos, mode_len, fns[a:a + _MAX_OUTPUTS],
                                                  pcts[a:a + _MAX_OUTPUTS], vdt))
            heads = starts[:-1]
            kcols = [b.columns[k].index_select(0, heads) for k in keys]
        else:
            made = [torch.from_numpy(np.ascontiguousarray(x))
                    for x in _host_finish(words[W - 1], starts, distinct, mode_pos, fns, pcts, np_dt)]
            heads = torch.from_numpy(np.ascontiguousarray(starts[:-1]))
            kcols = [b.columns[k].index_select(0, heads) for k in keys]
        cols: Dict[str, Any] = {}
        lo = 1 if drop_first else 0
        for k, c in zip(keys, kcols):
            cols[k] = c[lo:]
        for i, (o, t) in enumerate(zip(outs, made)):
            if o.fn in _RANKED and not o.is_list:
                t = t.reshape(-1)
            if patch is not None:  # the partition's last group runs on: its values come from the fold
                t[-1] = torch.from_numpy(np.ascontiguousarray(patch[i])).reshape(t.shape[1:]).to(t.device)
            cols[o.name] = t[lo:]
        return Block(int(heads.shape[0]) - lo, cols)

    def compute(blocks: Dict[int, Block]) -> Dict[int, Block]:
        rng = torch.cuda.is_initialized()
        if rng:
            torch.cuda.nvtx.range_push("tfa.order_agg")
        try:
            if keep_on_device and engine.gpu_available():
                # (an exchange between ranks may have staged the sorted rows through the host)
                blocks = {pid: b.to(engine.compute_device()) for pid, b in blocks.items()}
            table = torch.zeros((nparts, width), dtype=torch.int64)
            parts = {}
            rows = 0
            for pid in sorted(blocks):
                b = blocks[pid]
                if b.nrows:
                    parts[pid] = summarise(b)
                    table[pid] = torch.from_numpy(parts[pid][3])
                    rows += b.nrows
            dist.all_reduce_host_(table, "Sum")  # (every rank fills the rows of its own partitions)
            continues, spans = _fold(table.numpy(), W, P)
            # the words at the ranks the spanning groups ask for: [span, rank] in a second table
            wanted = [_wanted_ranks(s, outs) for s in spans]
            words_at: List[Dict[int, int]] = [dict() for _ in spans]
            if any(wanted):
                slots = [(si, r) for si, rs in enumerate(wanted) for r in rs]
                at = {sr: j for j, sr in enumerate(slots)}
                second = torch.zeros(len(slots), dtype=torch.int64)
                reads: Dict[int, List[Tuple[int, int]]] = {}  # partition -> (slot, local row)
                for si, s in enumerate(spans):
                    before = 0
                    for pid, row0, nrows in s["pieces"]:
                        for r in wanted[si]:
                            if before <= r < before + nrows and pid in parts:
                                reads.setdefault(pid, []).append((at[(si, r)], row0 + r - before))
                        before += nrows
                for pid, lst in sorted(reads.items()):
                    got = read_words(parts[pid][0], parts[pid][1], [row for _, row in lst])
                    second[[j for j, _ in lst]] = torch.from_numpy(got.view(np.int64).copy())
                dist.all_reduce_host_(second, "Sum")  # (a slot is read by the one rank that holds its row)
                sw = second.numpy().view(np.uint64)
                for (si, r), j in at.items():
                    words_at[si][r] = int(sw[j])
            patches = {s["pieces"][0][0]: _spanning_values(s, outs, words_at[si], np_dt)
                       for si, s in enumerate(spans)}
            res: Dict[int, Block] = {}
            for pid in sorted(blocks):
                b = blocks[pid]
                if not b.nrows:
                    ref = next((c for c in b.columns.values() if isinstance(c, torch.Tensor)), None)
                    dev = ref.device if ref is not None else torch.device("cpu")
                    cols = {k: torch.empty(0, dtype=t, device=dev) for k, t in zip(keys, kdt)}
                    cols.update({o.name: torch.empty([0] + o.shape, dtype=o.dtype, device=dev) for o in outs})
                    res[pid] = Block(0, cols)
                    continue
                on_device, words, summ, _ = parts[pid]
                res[pid] = emit(b, on_device, words, summ, continues[pid], patches.get(pid))
        finally:
            if rng:
                torch.cuda.nvtx.range_pop()
        metrics.add("order_agg_rows", rows)
        metrics.add("order_agg_sorts")
        return res

    def compute_agreed(blocks):
        return dist.agreed(what, lambda: compute(blocks))

    fields = [df.schema[k] for k in keys] + [tensor_field(o.name, o.dtype, o.shape) for o in outs]
    return DataFrame(StructType(fields), _Derived(srt, compute_agreed, streamable=False), nparts)


# ------------------------------------------------------------------ the call
def _check(df, keys: Sequence[str], e: OrderAggregateExpression, what: str) -> None:
    for c in e.columns:
        if c not in df.schema:
            raise ValueError(f"{what}: Column {c} not found in {df.columns}")
        err = _ineligible(df, c, what)
        if err is not None:
            raise err
    if len(keys) + len(e.columns) > _MAX_SORT_WORDS:
        raise ValueError(f"{what}: '{e.output_name}' sorts by {len(keys)} group keys and {len(e.columns)} value "
                         f"columns, {len(keys) + len(e.columns)} sort words; at most {_MAX_SORT_WORDS} fit")


def _order_frames(df, keys: Sequence[str], members: Sequence[Tuple[str, OrderAggregateExpression]], what: str):
    """One frame (keys + outputs) per distinct sort of the order aggregates, in order of first use."""
    from .window import _device_cached
    sorts: List[Tuple[Tuple[str, ...], List[Tuple[str, OrderAggregateExpression]]]] = []
    for name, e in members:
        for cols, lst in sorts:
            if cols == e.columns:
                lst.append((name, e))
                break
        else:
            sorts.append((e.columns, [(name, e)]))
    keep = _device_cached(df)
    return [_sort_frame_of(df, keys, list(cols), lst, what, keep) for cols, lst in sorts]


def has_order_aggregates(exprs: Sequence[Any]) -> bool:
    return any(isinstance(e, OrderAggregateExpression) for e in exprs)


def agg_with_order(grouped, exprs: Sequence[Any], what: str = "agg"):
    """`GroupedData.agg` / `DataFrame.agg` of a call that holds order
    aggregates, alone or mixed with the moment aggregates of group_agg.py."""
    from .dataframe import from_columns
    from .group_agg import _check_keys, _specs, group_agg
    from .window import refuse_window_expression
    df, keys = grouped.df, list(grouped.keys)
    refuse_window_expression(what, exprs)
    order = [(i, e) for i, e in enumerate(exprs) if isinstance(e, OrderAggregateExpression)]
    moment = [(i, e) for i, e in enumerate(exprs) if not isinstance(e, OrderAggregateExpression)]
    if moment:
        _specs(df, keys, [e for _, e in moment], what)  # (the typed errors of the other expressions, before any work)
    if keys:
        _check_keys(df, keys, what)
    for _, e in order:
        _check(df, keys, e, what)
    names = [getattr(e, "output_name", None) for e in exprs]
    seen = set(keys)
    for nm in names:
        if nm in seen:
            raise ValueError(f"{what}: the output column '{nm}' appears twice (or is a key); use .alias() to rename "
                             f"one")
        seen.add(nm)
    frames = _order_frames(df, keys, [(e.output_name, e) for _, e in order], what)
    left = [group_agg(grouped, [e for _, e in moment], what)] if moment else []
    if not keys:
        # one row each, identical on every rank: side by side, in the order of the call
        cols: Dict[str, np.ndarray] = {}
        for f in left + frames:
            f = f.cache()  # (one evaluation for all of its columns)
            for c in f.columns:
                cols[c] = f.to_numpy(c)
        for nm, a in cols.items():
            if len(a) != 1:
                raise ValueError(f"{what}: '{nm}' of a frame without rows does not exist")
        return from_columns({nm: np.ascontiguousarray(cols[nm]) for nm in names}, num_partitions=1)
    out = (left + frames)[0]
    for f in (left + frames)[1:]:
        out = out.join(f, keys, "inner")
    return out._project([(c, c) for c in keys + names])
