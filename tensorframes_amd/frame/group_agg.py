"""GroupedData.agg / DataFrame.agg: named aggregates over numeric keys.

Per group and value column one record of six 8-byte fields travels as int64
bit patterns: n, mean, M2 (f64; every element converted to f64 first), the sum
(wrapping int64 for integer columns, an f64 running sum for float ones), and
the smallest and largest ascending sort word. `corr`, `covar_samp` and
`covar_pop` have a record of their own per (group, ordered pair of value
columns), seven fields: n, mean_x, mean_y, M2_x, M2_y, the co-moment
C_xy = sum (x - mean_x)(y - mean_y) (f64) and the integer count of rows whose
x or y is NaN or an infinity; the empty record is all zeros. Pair records ride
with the one-column records through both stages (one row per group for the
all-to-all) and are merged by their own merge.

* stage 1: every partition is reduced on its own. Keys are factorised by
  `ops/groupby.group_ids` (the grouping of `groupBy(keys).count()`); device
  partitions go through `_C.segment_csr` + `_C.group_moments`
  (kernels/group_stats.hip), host partitions through numpy (two-pass f64 per
  group). One record per (group of the partition, column); pair records come
  from `_C.group_pair_moments` (the same work items, built once when a call
  needs both kinds), or from `_C.column_pair_moments` for `DataFrame.agg`,
  which reads a device partition densely, without a one-segment gather.
* stage 2: the records of all partitions, tagged with their partition id,
  are routed to the rank their key hashes to (`ops/groupby.route`: one
  all-to-all, the partition id and the record fields riding as ordinary
  columns), ordered by (keys..., partition id) with `group_ids`, and the
  records of equal key are merged in ascending partition id with Chan's
  formula (`_C.merge_group_records`, or `_merge_records` on the host).

For a given partitioning every output bit is the same for every world size
and from run to run: a record depends on its group's rows in row order
alone, and the merge order is the partition order. No float atomics.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ..functions import FUNCTIONS, AggregateExpression, PairAggregateExpression
from ..parallel import dist
from ..utils import dtypes as D
from ._scalar_columns import (_aggregate_dtype, _block_on_device, _decode_sort_word, _ineligible, _scalar_column,
                              _stat_columns, _tf_dtype)
from .block import Block
from .column_info import ColumnInformation
from .types import BinaryType, StringType, StructType

_FIELDS = 6  # kernels.h kGroupRecordFields
_MAX_COLS = 16  # value columns per agg call, outputs per _C.group_results call (kernels.h kMaxPackCols)
_KEY_DTYPES = (D.DT_INT32, D.DT_INT64, D.DT_FLOAT, D.DT_DOUBLE)
_N, _MEAN, _M2, _SUM, _LO, _HI = range(_FIELDS)
_PFIELDS = 7  # kernels.h kPairRecordFields
_PN, _PMX, _PMY, _PM2X, _PM2Y, _PC, _PBAD = range(_PFIELDS)


# ------------------------------------------------------------------ expressions
class _Spec:
    """One output column: statistic `fn` of value column `column` (None: rows),
    or pair statistic `fn` of the ordered pair of value columns `pair`."""

    def __init__(self, fn: str, column: Optional[str], name: str, pair: Optional[Tuple[str, str]] = None):
        self.fn, self.column, self.name, self.pair = fn, column, name, pair


def _specs(df, keys: Sequence[str], exprs: Sequence[Any], what: str) -> List[_Spec]:
    from .window import refuse_window_expression
    refuse_window_expression(what, exprs)
    if len(exprs) == 1 and isinstance(exprs[0], dict):
        made = []
        for col, fn in exprs[0].items():
            if not isinstance(col, str) or not isinstance(fn, str):
                raise TypeError(f"{what}: the dict form maps column names to function names, got {col!r}: {fn!r}")
            if fn.lower() not in FUNCTIONS:
                raise ValueError(f"{what}: '{fn}' is not an aggregate function; expected one of "
                                 f"{', '.join(sorted(FUNCTIONS))}")
            stat = FUNCTIONS[fn.lower()]
            made.append(AggregateExpression(stat, None if (col == "*" and stat == "count") else col))
        exprs = made
    if not exprs:
        raise ValueError(f"{what}: at least one aggregate expression is expected")
    out: List[_Spec] = []
    for e in exprs:
        if isinstance(e, PairAggregateExpression):
            for c in (e.x, e.y):
                if c not in df.schema:
                    raise ValueError(f"{what}: Column {c} not found in {df.columns}")
                err = _ineligible(df, c, what)
                if err is not None:
                    raise err
            out.append(_Spec(e.fn, None, e.output_name, (e.x, e.y)))
            continue
        if not isinstance(e, AggregateExpression):
            hint = " (Column.sum() and friends reduce the cell of one row; use tfs.functions.sum(name))" \
                if type(e).__name__ == "Column" else ""
            raise TypeError(f"{what}: aggregate expressions from tfs.functions are expected, got "
                            f"{type(e).__name__}{hint}")
        if e.column is not None:
            if e.column not in df.schema:
                raise ValueError(f"{what}: Column {e.column} not found in {df.columns}")
            if e.fn != "count":  # (frames hold no nulls: count(x) counts rows, whatever x holds)
                err = _ineligible(df, e.column, what)
                if err is not None:
                    raise err
        out.append(_Spec(e.fn, e.column if e.fn != "count" else None, e.output_name))
    seen = set(keys)
    for s in out:
        if s.name in seen:
            raise ValueError(f"{what}: the output column '{s.name}' appears twice (or is a key); use .alias() to "
                             f"rename one")
        seen.add(s.name)
    return out


def _check_keys(df, keys: Sequence[str], what: str) -> None:
    from .. import core
    for k in keys:
        f = df.schema[k]
        if isinstance(f.dataType, (StringType, BinaryType)):
            raise core.InvalidTypeException(
                f"{what}: the key '{k}' is a {type(f.dataType).__name__[:-4].lower()} column; named aggregates take "
                f"numeric scalar keys (int32, int64, float32, float64). String and binary keys are grouped by "
                f"groupBy(...).aggregate(fetches)")
        stf = ColumnInformation(f).stf
        if stf is None or stf.tf_dtype not in _KEY_DTYPES or stf.shape.num_dims != 1:
            raise core.InvalidTypeException(
                f"{what}: the key '{k}' ({f.dataType}) is not a numeric scalar column of int32, int64, float32 or "
                f"float64")


# ------------------------------------------------------------------ host records
def _f64(a: np.ndarray) -> np.ndarray:
    return a.view(np.float64)


def _host_group_records(vals: Sequence[torch.Tensor], ids: np.ndarray, ng: int) -> np.ndarray:
    """int64 [ng, C, 6]: the records of one host partition (every group has rows).
    Per group the two-pass form of stats._host_record."""
    from .dataframe import _host_sort_words
    out = np.zeros((ng, len(vals), _FIELDS), dtype=np.int64)
    order = np.argsort(ids, kind="stable")
    counts = np.bincount(ids, minlength=ng).astype(np.int64)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    nf = counts.astype(np.float64)
    for c, v in enumerate(vals):
        a = v.detach().contiguous().numpy()[order]
        with np.errstate(all="ignore"):
            x = a.astype(np.float64)
            s = np.add.reduceat(x, starts)
            mean = s / nf
            dev = x - np.repeat(mean, counts)
            # (two passes; the second also takes out what rounding left in the mean)
            mean = mean + np.add.reduceat(dev, starts) / nf
            dev = x - np.repeat(mean, counts)
            m2 = np.add.reduceat(dev * dev, starts)
        w = _host_sort_words(v, False)[order]
        _f64(out[:, c, :3])[:, 0] = nf
        _f64(out[:, c, :3])[:, 1] = mean
        _f64(out[:, c, :3])[:, 2] = m2
        out[:, c, _SUM] = s.view(np.int64) if a.dtype.kind == "f" else np.add.reduceat(a.astype(np.int64), starts)
        out[:, c, _LO] = np.minimum.reduceat(w, starts).view(np.int64)
        out[:, c, _HI] = np.maximum.reduceat(w, starts).view(np.int64)
    return out


def _chan(a: np.ndarray, b: np.ndarray, is_float: Sequence[bool]) -> np.ndarray:
    """Chan's merge of records [s, C, 6], `a` the earlier rows (the arithmetic
    of kernels/group_stats.hip grec_merge)."""
    r = np.empty_like(a)
    fa, fb, fr = _f64(a[..., :3]), _f64(b[..., :3]), _f64(r[..., :3])
    an, bn = fa[..., 0], fb[..., 0]
    with np.errstate(all="ignore"):
        n = an + bn
        delta = fb[..., 1] - fa[..., 1]
        f = np.where(n > 0, bn / np.where(n > 0, n, 1.0), 0.0)
        fr[..., 0] = n
        fr[..., 1] = np.where(an == 0, fb[..., 1], np.where(bn == 0, fa[..., 1], fa[..., 1] + delta * f))
        fr[..., 2] = np.where(an == 0, fb[..., 2],
                              np.where(bn == 0, fa[..., 2], fa[..., 2] + fb[..., 2] + delta * delta * (an * f)))
        fsum = np.where(an == 0, _f64(b[..., _SUM]),
                        np.where(bn == 0, _f64(a[..., _SUM]), _f64(a[..., _SUM]) + _f64(b[..., _SUM])))
        isum = a[..., _SUM] + b[..., _SUM]  # (int64: wraps)
    r[..., _SUM] = np.where(np.asarray(is_float, dtype=bool)[None, :], fsum.view(np.int64), isum)
    r[..., _LO] = np.minimum(a[..., _LO].view(np.uint64), b[..., _LO].view(np.uint64)).view(np.int64)
    r[..., _HI] = np.maximum(a[..., _HI].view(np.uint64), b[..., _HI].view(np.uint64)).view(np.int64)
    return r


def _merge_records(recs: np.ndarray, offsets: np.ndarray, is_float: Sequence[bool]) -> np.ndarray:
    """recs [m, C, 6] ordered by (key, partition), CSR offsets [ng + 1] (every
    group has a record) -> [ng, C, 6]: each group's records merged in order,
    starting from its first."""
    recs = np.ascontiguousarray(recs)
    counts = np.diff(offsets)
    out = recs[offsets[:-1]].copy()
    for j in range(1, int(counts.max()) if len(counts) else 0):
        sel = np.nonzero(counts > j)[0]
        out[sel] = _chan(out[sel], recs[offsets[sel] + j], is_float)
    return out


def _host_results(recs: np.ndarray, cols: Sequence[int], stats: Sequence[str], dtypes: Sequence[np.dtype]):
    """Merged records [ng, C, 6] -> one numpy column per output (the host form
    of `_C.group_results`)."""
    outs = []
    for ci, st, dt in zip(cols, stats, dtypes):
        r = np.ascontiguousarray(recs[:, ci, :])
        n = _f64(r[:, _N]).copy()
        if st == "count":
            outs.append(n.astype(np.int64))
            continue
        lo, hi = r[:, _LO].view(np.uint64), r[:, _HI].view(np.uint64)
        if st in ("min", "max"):
            v = np.asarray(_decode_sort_word(lo if st == "min" else hi, dt)).reshape(-1).copy()
            v[n == 0] = 0
            outs.append(v.astype(dt))
            continue
        fl = dt.kind == "f"
        if st == "sum" and not fl:
            outs.append(r[:, _SUM].copy())
            continue
        with np.errstate(all="ignore"):
            mean = np.where(n > 0, _f64(r[:, _MEAN]), np.nan)
            m2 = np.where(n > 0, _f64(r[:, _M2]), np.nan)
            total = np.where(n > 0, _f64(r[:, _SUM]), 0.0) if fl else None
            if fl:
                # a NaN or an infinity propagates as in a plain sum / n, whatever the
                # order the rows were met in: the extremes tell what is there
                top = np.asarray(_decode_sort_word(hi, dt), dtype=np.float64).reshape(-1)
                bottom = np.asarray(_decode_sort_word(lo, dt), dtype=np.float64).reshape(-1)
                has = n > 0
                bad = has & (np.isnan(top) | ((top == np.inf) & (bottom == -np.inf)))
                one = has & ~bad & ((top == np.inf) | (bottom == -np.inf))
                signed = np.where(top == np.inf, np.inf, -np.inf)
                mean = np.where(bad, np.nan, np.where(one, signed, mean))
                total = np.where(bad, np.nan, np.where(one, signed, total))
                m2 = np.where(bad | one, np.nan, m2)
            if st == "sum":
                v = total
            elif st == "avg":
                v = mean
            elif st in ("var_samp", "stddev_samp"):
                v = np.where(n >= 2, m2 / np.where(n >= 2, n - 1, 1.0), np.nan)
            else:
                v = np.where(n >= 1, m2 / np.where(n >= 1, n, 1.0), np.nan)
            if st.startswith("stddev"):
                v = np.sqrt(v)
        outs.append(np.asarray(v, dtype=np.float64))
    return outs


# ------------------------------------------------------------------ host pair records
def _host_pair_records(xs: Sequence[torch.Tensor], ys: Sequence[torch.Tensor], ids: np.ndarray, ng: int) -> np.ndarray:
    """int64 [ng, Q, 7]: the pair records of one host partition (every group
    has rows). Per group two passes in f64: the means (corrected once, as in
    `_host_group_records`), then the squared deviations and co-deviations."""
    out = np.zeros((ng, len(xs), _PFIELDS), dtype=np.int64)
    order = np.argsort(ids, kind="stable")
    counts = np.bincount(ids, minlength=ng).astype(np.int64)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    nf = counts.astype(np.float64)

    def centred(v):
        x = v.detach().contiguous().numpy()[order].astype(np.float64)
        mean = np.add.reduceat(x, starts) / nf
        mean = mean + np.add.reduceat(x - np.repeat(mean, counts), starts) / nf
        return x, mean, x - np.repeat(mean, counts)

    for q, (vx, vy) in enumerate(zip(xs, ys)):
        with np.errstate(all="ignore"):
            x, mx, dx = centred(vx)
            y, my, dy = centred(vy)
            f = _f64(out[:, q, :_PBAD])
            f[:, _PN], f[:, _PMX], f[:, _PMY] = nf, mx, my
            f[:, _PM2X] = np.add.reduceat(dx * dx, starts)
            f[:, _PM2Y] = np.add.reduceat(dy * dy, starts)
            f[:, _PC] = np.add.reduceat(dx * dy, starts)
        out[:, q, _PBAD] = np.add.reduceat((~(np.isfinite(x) & np.isfinite(y))).astype(np.int64), starts)
    return out


def _pair_chan(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Chan's merge of pair records [s, Q, 7], `a` the earlier rows (the
    arithmetic of kernels/moments.h merge_pairs, without its contractions)."""
    r = np.empty_like(a)
    fa, fb, fr = _f64(a[..., :_PBAD]), _f64(b[..., :_PBAD]), _f64(r[..., :_PBAD])
    an, bn = fa[..., _PN], fb[..., _PN]
    with np.errstate(all="ignore"):
        n = an + bn
        dx, dy = fb[..., _PMX] - fa[..., _PMX], fb[..., _PMY] - fa[..., _PMY]
        f = np.where(n > 0, bn / np.where(n > 0, n, 1.0), 0.0)

        def pick(j, merged):
            return np.where(an == 0, fb[..., j], np.where(bn == 0, fa[..., j], merged))
        fr[..., _PN] = n
        fr[..., _PMX] = pick(_PMX, fa[..., _PMX] + dx * f)
        fr[..., _PMY] = pick(_PMY, fa[..., _PMY] + dy * f)
        fr[..., _PM2X] = pick(_PM2X, fa[..., _PM2X] + fb[..., _PM2X] + dx * dx * (an * f))
        fr[..., _PM2Y] = pick(_PM2Y, fa[..., _PM2Y] + fb[..., _PM2Y] + dy * dy * (an * f))
        fr[..., _PC] = pick(_PC, fa[..., _PC] + fb[..., _PC] + dx * dy * (an * f))
    r[..., _PBAD] = a[..., _PBAD] + b[..., _PBAD]
    return r


def _merge_pair_records(recs: np.ndarray, offsets: np.ndarray) -> np.ndarray:
    """`_merge_records` for pair records [m, Q, 7] (every group has a record)."""
    recs = np.ascontiguousarray(recs)
    counts = np.diff(offsets)
    out = recs[offsets[:-1]].copy()
    for j in range(1, int(counts.max()) if len(counts) else 0):
        sel = np.nonzero(counts > j)[0]
        out[sel] = _pair_chan(out[sel], recs[offsets[sel] + j])
    return out


def _pair_results(recs: np.ndarray, pairs: Sequence[int], stats: Sequence[str]) -> List[np.ndarray]:
    """Merged pair records [ng, Q, 7] -> one float64 column per output (the
    host form of `_C.pair_results`): covar_pop = C / n, covar_samp = C / (n - 1)
    (NaN below two rows), corr = C / sqrt(M2_x * M2_y) (NaN without rows or
    where an M2 is 0; not clamped). A group that counts a row with a NaN or an
    infinity is NaN in all three, whichever row it was."""
    outs = []
    for qi, st in zip(pairs, stats):
        r = np.ascontiguousarray(recs[:, qi, :])
        f = _f64(r[:, :_PBAD])
        n, c = f[:, _PN], f[:, _PC]
        with np.errstate(all="ignore"):
            if st == "covar_pop":
                v = np.where(n >= 1, c / np.where(n >= 1, n, 1.0), np.nan)
            elif st == "covar_samp":
                v = np.where(n >= 2, c / np.where(n >= 2, n - 1, 1.0), np.nan)
            elif st == "corr":
                ok = (n >= 1) & (f[:, _PM2X] != 0) & (f[:, _PM2Y] != 0)
                v = np.where(ok, c / np.sqrt(np.where(ok, f[:, _PM2X] * f[:, _PM2Y], 1.0)), np.nan)
            else:
                raise ValueError(f"'{st}' is not a pair statistic")
        outs.append(np.asarray(np.where(r[:, _PBAD] > 0, np.nan, v), dtype=np.float64))
    return outs


# ------------------------------------------------------------------ stage 1
def _columns_of(specs: Sequence[_Spec], what: str) -> Tuple[List[str], List[Tuple[str, str]]]:
    """(distinct value columns of the one-column outputs, distinct ordered
    pairs of the pair outputs), each in order of first use."""
    vcols: List[str] = []
    pairs: List[Tuple[str, str]] = []
    for s in specs:
        if s.pair is not None:
            if s.pair not in pairs:
                pairs.append(s.pair)
        elif s.column is not None and s.column not in vcols:
            vcols.append(s.column)
    if len(vcols) > _MAX_COLS:
        raise ValueError(f"{what}: at most {_MAX_COLS} distinct value columns per call, got {len(vcols)}; split the "
                         f"call and join the results on the keys")
    if len(pairs) > _MAX_COLS:
        raise ValueError(f"{what}: at most {_MAX_COLS} distinct column pairs per call, got {len(pairs)}; split the "
                         f"call and join the results on the keys")
    return vcols, pairs


def _partition_records(b: Block, keys: Sequence[str], vcols: Sequence[str], on_device: bool, what: str,
                       pairs: Sequence[Tuple[str, str]] = (), single: bool = True):
    """(distinct key columns of the partition, records [ng, C, 6] int64, pair
    records [ng, Q, 7] int64) of one non-empty partition, on the device or on
    the host; a kind the call does not need (`single` False, no `pairs`) is
    None."""
    from .. import core, engine
    from .._native import _C
    from ..ops import groupby as G
    from ..utils.logging import metrics
    dev = engine.compute_device() if on_device else torch.device("cpu")
    vals = [_scalar_column(b, v, what).to(dev) for v in vcols] if single else []
    if single and not vals:  # only rows are counted: a column of zeros carries n
        vals = [engine.device_full(b.nrows, 0, torch.uint8, dev)]
    xs = [_scalar_column(b, x, what).to(dev) for x, _ in pairs]
    ys = [_scalar_column(b, y, what).to(dev) for _, y in pairs]
    if keys:
        K = [b.columns[k] for k in keys]
        if not G.device_keys(K):
            raise core.InvalidDimensionException(
                f"{what}: a key column does not hold one numeric scalar per row in this partition")
        ids, uniq, ng = G.group_ids([k.to(dev).contiguous() for k in K])
    else:
        ids, uniq, ng = engine.device_full(b.nrows, 0, torch.int64, dev), [], 1
    recs = precs = None
    if on_device:
        perm, offsets = _C.segment_csr(ids, ng)
        vals, xs, ys = ([v.contiguous() for v in vs] for vs in (vals, xs, ys))
        if vals and xs:  # (the work items of the segments are built once for both)
            recs, precs = _C.group_both_moments(vals, xs, ys, perm, offsets)
        elif vals:
            recs = _C.group_moments(vals, perm, offsets)
        else:
            precs = _C.group_pair_moments(xs, ys, perm, offsets)
    else:
        if vals:
            recs = torch.from_numpy(_host_group_records(vals, ids.numpy(), ng))
        if xs:
            precs = torch.from_numpy(_host_pair_records(xs, ys, ids.numpy(), ng))
    where = "device" if on_device else "host"
    if vals:
        metrics.add(f"group_agg_{where}_partitions")
        metrics.add("group_agg_rows", b.nrows * len(vals))
    if xs:
        metrics.add(f"pair_agg_{where}_partitions")
        metrics.add("pair_agg_rows", b.nrows * len(xs))
    return uniq, recs, precs


def _needed(keys, vcols, pairs=()):
    out = list(keys)
    for v in list(vcols) + [c for p in pairs for c in p]:
        if v not in out:
            out.append(v)
    return out


def _outputs(specs, scol, spair, vdt, merged, pmerged, on_device: bool) -> List[torch.Tensor]:
    """One column per output from the merged records [ng, C, 6] and pair
    records [ng, Q, 7], in the order of `specs`."""
    from .._native import _C
    one = [i for i, s in enumerate(specs) if s.pair is None]
    two = [i for i, s in enumerate(specs) if s.pair is not None]
    outs: List[Any] = [None] * len(specs)
    for a in range(0, len(one), _MAX_COLS):
        at = one[a:a + _MAX_COLS]
        cols, fns = [scol[i] for i in at], [specs[i].fn for i in at]
        if on_device:
            got = _C.group_results(merged.contiguous(), cols, fns, [vdt[c] for c in cols])
        else:
            np_dt = [torch.empty(0, dtype=vdt[c]).numpy().dtype for c in cols]
            got = [torch.from_numpy(np.ascontiguousarray(o)) for o in _host_results(merged.numpy(), cols, fns, np_dt)]
        for i, o in zip(at, got):
            outs[i] = o
    for a in range(0, len(two), _MAX_COLS):
        at = two[a:a + _MAX_COLS]
        prs, fns = [spair[i] for i in at], [specs[i].fn for i in at]
        if on_device:
            got = _C.pair_results(pmerged.contiguous(), prs, fns)
        else:
            got = [torch.from_numpy(np.ascontiguousarray(o)) for o in _pair_results(pmerged.numpy(), prs, fns)]
        for i, o in zip(at, got):
            outs[i] = o
    return outs


# ------------------------------------------------------------------ both stages
def _merged_records(blocks, keys: Sequence[str], n_route: int, vcols, pairs, single: bool, kdt, is_float,
                    needed: Sequence[str], what: str):
    """Stage 1 and stage 2 of a keyed aggregate over this rank's partitions:
    (on_device, the distinct key columns [ng] in ascending lexicographic
    order, merged records [ng, C, 6], merged pair records [ng, Q, 7]) of the
    keys this rank answers for; a kind the call does not need is None. None
    when no rank has rows, or none arrive here. Collective.

    The first `n_route` keys decide the rank of a record (`GroupedData.agg`:
    all of them; pivot: all but the pivot column, so a key's pivot values meet
    on one rank; none: everything goes to rank 0); the other keys ride as
    columns."""
    from .. import engine
    from .._native import _C
    from ..ops import groupby as G
    C = max(len(vcols), 1) if single else 0
    Q = len(pairs)
    W1, W = C * _FIELDS, C * _FIELDS + Q * _PFIELDS  # a group's row: its records, then its pair records
    parts = [(pid, b) for pid, b in sorted(blocks.items()) if b.nrows]
    # decided together, so every rank takes the same (collective) path:
    # the device path when no rank holds a needed column on the host
    flags = torch.tensor([int(any(not _block_on_device(b, needed) for _, b in parts)), int(bool(parts))],
                         dtype=torch.int64)
    dist.all_reduce_host_(flags, "Max")
    if not int(flags[1]):
        return None
    on_device = engine.gpu_available() and not int(flags[0])
    dev = engine.compute_device() if on_device else torch.device("cpu")
    got = []
    for pid, b in parts:
        u, r, pr = _partition_records(b, keys, vcols, on_device, what, pairs, single)
        ng = int((r if r is not None else pr).shape[0])
        row = [t.reshape(ng, -1) for t in (r, pr) if t is not None]
        got.append((pid, u, row[0] if len(row) == 1 else torch.cat(row, dim=1)))
    if got:
        K = [engine.cat_rows([u[j] for _, u, _ in got]) for j in range(len(keys))]
        R = engine.cat_rows([r for _, _, r in got])
        pids = engine.cat_rows([engine.device_full(r.shape[0], pid, torch.int64, dev) for pid, _, r in got])
    else:
        K = [engine.device_empty(0, t, dev) for t in kdt]
        R = engine.device_empty((0, W), torch.int64, dev)
        pids = engine.device_empty(0, torch.int64, dev)

    def split(rows):
        """rows [m, W] -> (records [m, C, 6], pair records [m, Q, 7]); a kind without columns is None"""
        m = int(rows.shape[0])
        return (rows[:, :W1].contiguous().reshape(m, C, _FIELDS) if C else None,
                rows[:, W1:].contiguous().reshape(m, Q, _PFIELDS) if Q else None)
    if not dist.is_distributed() and len(got) == 1:
        merged, pmerged = split(R)  # one partition: its records are the result
        return on_device, K, merged, pmerged
    if dist.is_distributed():
        recv = G.route(K[:n_route], K[n_route:] + [pids, R])
        K, pids, R = recv[:len(keys)], recv[len(keys)], recv[len(keys) + 1]
    m = int(K[0].shape[0])
    if m == 0:
        return None
    # (keys..., partition id) in lexicographic order: the records of one
    # key are consecutive and in partition order
    ids, uniq, m2 = G.group_ids([k.contiguous() for k in K] + [pids])
    if m2 != m:
        raise RuntimeError(f"{what}: {m} records but {m2} distinct (key, partition) pairs")
    ordered = engine.device_empty((m, W), torch.int64, dev)
    if on_device:
        _C.scatter_rows(ordered, ids, R.contiguous())
    else:
        ordered[ids] = R
    ids2, ukeys, ng = G.group_ids([u.contiguous() for u in uniq[:-1]])
    recs, precs = split(ordered)
    merged = pmerged = None
    if on_device:
        _, offsets = _C.segment_csr(ids2, ng)
        if C:
            merged = _C.merge_group_records(recs, offsets, is_float)
        if Q:
            pmerged = _C.merge_pair_records(precs, offsets)
    else:
        offsets = np.concatenate([[0], np.cumsum(np.bincount(ids2.numpy(), minlength=ng))]).astype(np.int64)
        if C:
            merged = torch.from_numpy(_merge_records(recs.numpy(), offsets, is_float))
        if Q:
            pmerged = torch.from_numpy(_merge_pair_records(precs.numpy(), offsets))
    return on_device, ukeys, merged, pmerged


# ------------------------------------------------------------------ keyed
def group_agg(grouped, exprs: Sequence[Any], what: str = "agg"):
    """`GroupedData.agg`: see there."""
    from .dataframe import DataFrame, _Derived, tensor_field
    from .order_agg import agg_with_order, has_order_aggregates
    if has_order_aggregates(exprs):  # median, percentile, mode, countDistinct: frame/order_agg.py
        return agg_with_order(grouped, exprs, what)
    df, keys = grouped.df, list(grouped.keys)
    specs = _specs(df, keys, exprs, what)
    if not keys:
        return frame_agg(df, specs, what)
    _check_keys(df, keys, what)
    vcols, pairs = _columns_of(specs, what)
    single = any(s.pair is None for s in specs)
    vdt = ([D.torch_dtype(_tf_dtype(df, v)) for v in vcols] or [torch.uint8]) if single else []
    is_float = [t.is_floating_point for t in vdt]
    kdt = [D.torch_dtype(_tf_dtype(df, k)) for k in keys]
    out_dt = [torch.float64 if s.pair is not None else _aggregate_dtype(df, s.fn, s.column) for s in specs]
    scol = [vcols.index(s.column) if s.column is not None else 0 for s in specs]
    spair = [pairs.index(s.pair) if s.pair is not None else 0 for s in specs]
    needed = _needed(keys, vcols, pairs)
    keep_on_device = any(b.columns[n].is_cuda for b in (df._cached or {}).values() if b.nrows for n in needed
                         if isinstance(b.columns[n], torch.Tensor))
    world = max(1, dist.world_size())

    def empty():
        cols: Dict[str, Any] = {k: torch.empty(0, dtype=t) for k, t in zip(keys, kdt)}
        cols.update({s.name: torch.empty(0, dtype=t) for s, t in zip(specs, out_dt)})
        return {p: Block(0, dict(cols)) for p in dist.local_partitions(world)}

    def compute(blocks):
        got = _merged_records(blocks, keys, len(keys), vcols, pairs, single, kdt, is_float, needed, what)
        if got is None:
            return empty()
        on_device, ukeys, merged, pmerged = got
        ng = int((merged if merged is not None else pmerged).shape[0])
        outs = _outputs(specs, scol, spair, vdt, merged, pmerged, on_device)
        keep = on_device and keep_on_device
        cols: Dict[str, Any] = {k: (u if keep else u.cpu()) for k, u in zip(keys, ukeys)}
        cols.update({s.name: (o if keep else o.cpu()) for s, o in zip(specs, outs)})
        return {dist.rank(): Block(ng, cols)}

    def compute_agreed(blocks):
        return dist.agreed(what, lambda: compute(blocks))

    fields = [df.schema[k] for k in keys] + [tensor_field(s.name, t, []) for s, t in zip(specs, out_dt)]
    return DataFrame(StructType(fields), _Derived(df, compute_agreed, streamable=False), world)


# ------------------------------------------------------------------ no keys
def frame_agg(df, specs, what: str = "agg"):
    """`DataFrame.agg`: one row, in one partition, identical on every rank
    (an action, and collective, like `describe`)."""
    from .dataframe import from_columns
    if not isinstance(specs, list) or not all(isinstance(s, _Spec) for s in specs):
        specs = _specs(df, [], list(specs), what)
    vcols, pairs = _columns_of(specs, what)
    single = any(s.pair is None for s in specs)
    C = max(len(vcols), 1) if single else 0
    Q = len(pairs)
    W1, W = C * _FIELDS, C * _FIELDS + Q * _PFIELDS
    vdt = ([D.torch_dtype(_tf_dtype(df, v)) for v in vcols] or [torch.uint8]) if single else []
    is_float = [t.is_floating_point for t in vdt]
    scol = [vcols.index(s.column) if s.column is not None else 0 for s in specs]
    spair = [pairs.index(s.pair) if s.pair is not None else 0 for s in specs]
    pcols = _needed([], [], pairs)

    def run():
        from .. import engine
        from .._native import _C
        from ..utils.logging import metrics
        blocks = df._blocks()
        # a partition's row: its records [C, 6], then its pair records [Q, 7]
        table = torch.zeros((df.num_partitions, W), dtype=torch.int64)
        for pid in sorted(blocks):
            b = blocks[pid]
            if not b.nrows:
                continue
            if single:
                on_device = engine.gpu_available() and _block_on_device(b, vcols) and bool(vcols)
                table[pid, :W1] = _partition_records(b, [], vcols, on_device, what)[1].cpu()[0].reshape(-1)
            if not Q:
                continue
            if engine.gpu_available() and _block_on_device(b, pcols):
                # read where it is, densely: no CSR of one segment, no gather
                xs = [_scalar_column(b, x, what).contiguous() for x, _ in pairs]
                ys = [_scalar_column(b, y, what).contiguous() for _, y in pairs]
                table[pid, W1:] = _C.column_pair_moments(xs, ys).cpu().reshape(-1)
                metrics.add("pair_agg_device_partitions")
                metrics.add("pair_agg_rows", b.nrows * Q)
            else:
                table[pid, W1:] = _partition_records(b, [], [], False, what, pairs, False)[2][0].reshape(-1)
        dist.all_reduce_host_(table, "Sum")  # (every rank fills the rows of its own partitions; the others are zero)
        return table.numpy()
    table = np.ascontiguousarray(dist.agreed(what, run))
    # the partitions with rows, in partition order (n is the first field of both record kinds)
    table = table[_f64(np.ascontiguousarray(table[:, 0])) > 0]
    recs = np.ascontiguousarray(table[:, :W1]).reshape(-1, C, _FIELDS) if C else None
    precs = np.ascontiguousarray(table[:, W1:]).reshape(-1, Q, _PFIELDS) if Q else None
    merged = pmerged = None
    if len(table):
        whole = np.array([0, len(table)], dtype=np.int64)
        if C:
            merged = _merge_records(recs, whole, is_float)
        if Q:
            pmerged = _merge_pair_records(precs, whole)
    else:
        for s in specs:
            if s.fn in ("min", "max"):
                raise ValueError(f"{what}: {s.fn}({s.column}) of a frame without rows does not exist")
        merged = np.zeros((1, C, _FIELDS), dtype=np.int64) if C else None
        pmerged = np.zeros((1, Q, _PFIELDS), dtype=np.int64) if Q else None
    outs = _outputs(specs, scol, spair, vdt, torch.from_numpy(merged) if C else None,
                    torch.from_numpy(pmerged) if Q else None, False)
    return from_columns({s.name: np.ascontiguousarray(o.numpy()) for s, o in zip(specs, outs)}, num_partitions=1)


# ------------------------------------------------------------------ shortcuts
def group_stat(grouped, fn: str, cols: Sequence[Any]):
    """`GroupedData.sum / avg / mean / min / max`: the named columns, or every
    numeric scalar column that is not a key."""
    df = grouped.df
    names = _stat_columns(df, cols, fn)
    if not [c for cs in cols for c in (cs if isinstance(cs, (list, tuple)) else [cs])]:
        names = [n for n in names if n not in grouped.keys]
    if not names:
        raise ValueError(f"{fn}: the frame has no numeric scalar column besides the keys")
    return group_agg(grouped, [AggregateExpression(FUNCTIONS[fn], n) for n in names], fn)
