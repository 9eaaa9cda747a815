"""Random rows and random columns: `DataFrame.sample`, `randomSplit`,
`sampleBy` and `F.rand` / `F.randn`.

Every draw is a pure function of (seed, global row index, purpose), so the
same rows are kept, bit for bit, on the host and on the device, for every
number of ranks, for every partitioning of the same row sequence and on every
recomputation of the lazy frame.

The generator is Philox4x32-10 (Salmon et al., SC'11): multipliers 0xD2511F53
and 0xCD9E8D57, key increments 0x9E3779B9 and 0xBB67AE85, ten rounds.

* key      (seed & 0xffffffff, seed >> 32) of the seed reduced mod 2^64
* counter  (row & 0xffffffff, row >> 32, purpose, 0); `row` is the global row
           index (the index in the partition plus the rows of all earlier
           partitions), purpose 0 uniform, 1 normal, 2 poisson
* one call serves one row and gives the words w0..w3

    uniform  u  = (((w0 << 32) | w1) >> 11) * 2^-53                 in [0, 1)
    normal   u1 = ((((w0 << 32) | w1) >> 11) + 1) * 2^-53           in (0, 1]
             u2 = (((w2 << 32) | w3) >> 11) * 2^-53
             z  = sqrt(-2 ln u1) * cos(2 pi u2)         (Box-Muller, the first)
    poisson  the number of entries <= u of `poisson_cdf(lambda)`

Device-resident partitions run kernels/random.hip and stay on the device;
every other partition runs the vectorised numpy form below (uint64
arithmetic), which is also the CPU oracle. One host all-reduce of the
partitions' row counts gives every partition its first global row index.
"""
from __future__ import annotations

import math
import numbers
import os
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ..parallel import dist
from .block import Block

_MASK32 = np.uint64(0xFFFFFFFF)
_MASK64 = (1 << 64) - 1
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_TWO_POW_MINUS_53 = 2.0 ** -53
PURPOSE_UNIFORM, PURPOSE_NORMAL, PURPOSE_POISSON = 0, 1, 2
MAX_STRATA = 4096         # kernels.h kMaxStrata
MAX_POISSON_TABLE = 64    # kernels.h kMaxPoissonTable
MAX_REPLACEMENT_FRACTION = 16.0  # beyond it 64 entries no longer cover the tail to 2^-53


# ------------------------------------------------------------------ the generator on the host
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of counters (c0..c3) under keys (k0, k1): arrays (or
    scalars) of 32-bit values held as uint64 -> four uint64 arrays of 32-bit
    words."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(x, dtype=np.uint64) for x in (c0, c1, c2, c3, k0, k1))
    for r in range(10):
        p0 = _M0 * c0  # (both factors below 2^32: the product fits 64 bits)
        p1 = _M1 * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _MASK32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _MASK32
        if r < 9:
            k0 = (k0 + _W0) & _MASK32
            k1 = (k1 + _W1) & _MASK32
    return c0, c1, c2, c3


def _row_words(seed: int, row0: int, n: int, purpose: int):
    rows = np.uint64(row0) + np.arange(n, dtype=np.uint64)
    return philox4x32_10(rows & _MASK32, rows >> np.uint64(32), np.uint64(purpose), np.uint64(0),
                         np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF))


def _bits53(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    return ((a << np.uint64(32)) | b) >> np.uint64(11)


def host_uniform(seed: int, row0: int, n: int, purpose: int = PURPOSE_UNIFORM) -> np.ndarray:
    """float64 [n]: u of the rows row0 .. row0 + n (exact)."""
    w0, w1, _, _ = _row_words(seed, row0, n, purpose)
    return _bits53(w0, w1).astype(np.float64) * _TWO_POW_MINUS_53


def host_normal(seed: int, row0: int, n: int) -> np.ndarray:
    w0, w1, w2, w3 = _row_words(seed, row0, n, PURPOSE_NORMAL)
    u1 = (_bits53(w0, w1) + np.uint64(1)).astype(np.float64) * _TWO_POW_MINUS_53
    u2 = _bits53(w2, w3).astype(np.float64) * _TWO_POW_MINUS_53
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def poisson_cdf(lam: float) -> List[float]:
    """cdf[k] = sum_{j <= k} e^-lam lam^j / j! in float64, by the recurrence
    term *= lam / j with a running sum; the table ends at the first
    cdf[k] >= 1 - 2^-53, at most 64 entries are kept."""
    term = math.exp(-lam)
    cdf = [term]
    j = 0
    while cdf[-1] < 1.0 - _TWO_POW_MINUS_53 and len(cdf) < MAX_POISSON_TABLE:
        j += 1
        term *= lam / j
        cdf.append(cdf[-1] + term)
    return cdf


def host_poisson(seed: int, row0: int, n: int, cdf: Sequence[float]) -> np.ndarray:
    """int64 [n]: per row the entries of cdf that are <= u (purpose 2)."""
    u = host_uniform(seed, row0, n, PURPOSE_POISSON)
    return np.searchsorted(np.asarray(cdf, dtype=np.float64), u, side="right").astype(np.int64)


def host_mask_by(seed: int, row0: int, words: np.ndarray, table_words: np.ndarray,
                 table_fractions: np.ndarray) -> np.ndarray:
    """bool [n]: u < the fraction of the row's word (0 for a word the table
    does not hold); table_words ascending (uint64) and distinct."""
    n = len(words)
    u = host_uniform(seed, row0, n)
    S = len(table_words)
    if S == 0:
        return np.zeros(n, dtype=bool)
    at = np.minimum(np.searchsorted(table_words, words), S - 1)
    f = np.where(table_words[at] == words, table_fractions[at], 0.0)
    return u < f


# ------------------------------------------------------------------ arguments
def resolve_seed(seed, what: str) -> int:
    """The 64-bit seed of one call: an int reduced mod 2^64 (negative seeds
    are allowed), or for None eight bytes of os.urandom drawn on rank 0 and
    broadcast. The seed then belongs to the lazy frame: every action on it
    sees the same rows."""
    if seed is None:
        drawn = int.from_bytes(os.urandom(8), "little") if dist.rank() == 0 else None
        return int(dist.broadcast_object(drawn, 0)) & _MASK64
    check_seed(seed, what)
    return int(seed) & _MASK64


def check_seed(seed, what: str) -> None:
    if seed is not None and (isinstance(seed, bool) or not isinstance(seed, numbers.Integral)):
        raise TypeError(f"{what}: the seed must be an int (or None), got {seed!r}")


def _check_fraction(v, what: str, name: str, upper: Optional[float]) -> float:
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, numbers.Real):
        raise ValueError(f"{what}: {name} must be a number, got {v!r}")
    f = float(v)
    if math.isnan(f) or math.isinf(f) or f < 0.0 or (upper is not None and f > upper):
        rng = f"in [0, {upper:g}]" if upper is not None else "positive and finite"
        raise ValueError(f"{what}: {name} must be {rng}, got {v!r}")
    return f


def split_bounds(weights, what: str = "randomSplit") -> List[float]:
    """b_0 = 0 <= b_1 <= ... <= b_k = 1.0: the running float64 sum of the
    weights (left to right) divided by their total; the last bound is forced
    to 1.0."""
    if isinstance(weights, (str, bytes)) or not isinstance(weights, (list, tuple, np.ndarray)):
        raise TypeError(f"{what}: a list of weights is expected, got {type(weights).__name__}")
    if len(weights) == 0:
        raise ValueError(f"{what}: the list of weights is empty")
    ws = []
    for w in weights:
        f = _check_fraction(w, what, "a weight", None)
        if f == 0.0:
            raise ValueError(f"{what}: a weight must be positive and finite, got {w!r}")
        ws.append(f)
    total = 0.0
    for f in ws:
        total += f
    if math.isinf(total):
        raise ValueError(f"{what}: the weights sum to infinity ({list(weights)!r})")
    bounds, run = [0.0], 0.0
    for f in ws:
        run += f
        bounds.append(run / total)
    bounds[-1] = 1.0
    return bounds


# ------------------------------------------------------------------ F.rand / F.randn
class RandomExpression:
    """`F.rand(seed)` / `F.randn(seed)`: one float64 draw per row. It is no
    Column: only `DataFrame.withColumn` and `DataFrame.select` take it."""

    __slots__ = ("fn", "seed", "_alias")

    def __init__(self, fn: str, seed=None, alias: Optional[str] = None):
        check_seed(seed, fn)
        self.fn, self.seed, self._alias = fn, (None if seed is None else int(seed)), alias

    def alias(self, name: str) -> "RandomExpression":
        if not isinstance(name, str) or not name:
            raise TypeError(f"alias: a non-empty column name is expected, got {name!r}")
        return RandomExpression(self.fn, self.seed, name)

    name = alias

    @property
    def has_alias(self) -> bool:
        return self._alias is not None

    @property
    def output_name(self) -> str:
        if self._alias is not None:
            return self._alias
        return f"{self.fn}({'' if self.seed is None else self.seed})"

    def __repr__(self):
        return f"RandomExpression<{self.output_name}>"

    def _refuse(self, *_a, **_k):
        raise TypeError(f"'{self.output_name}' is a random expression: it belongs in DataFrame.withColumn(name, ...) "
                        f"or DataFrame.select(...); add it as a column first, then compute with that column")

    __add__ = __radd__ = __sub__ = __rsub__ = __mul__ = __rmul__ = __truediv__ = __rtruediv__ = _refuse
    __neg__ = __invert__ = __and__ = __rand__ = __or__ = __ror__ = _refuse
    __lt__ = __le__ = __gt__ = __ge__ = _refuse
    __eq__ = __ne__ = _refuse  # type: ignore[assignment]
    __hash__ = None  # type: ignore[assignment]
    __bool__ = _refuse


def refuse_random_expression(what: str, items: Sequence[Any]) -> None:
    """The TypeError of an operator that is given a random expression."""
    for it in items:
        for x in (it if isinstance(it, (list, tuple)) else [it]):
            if isinstance(x, RandomExpression):
                raise TypeError(f"{what}: '{x.output_name}' is a random expression; it belongs in "
                                f"DataFrame.withColumn(name, ...) or DataFrame.select(...). Add it as a column "
                                f"first, then use that column in {what}")


# ------------------------------------------------------------------ the frames
def _dense_device(b: Block, needed: Sequence[str]) -> Optional[torch.device]:
    """The device this partition is sampled on, None for the host path: the
    one device that holds the needed columns, or (none needed) every dense
    column of the partition."""
    from .. import engine
    if not engine.gpu_available():
        return None
    cols = [b.columns[n] for n in needed] if needed else \
        [c for c in b.columns.values() if isinstance(c, torch.Tensor)]
    if not cols or not all(isinstance(c, torch.Tensor) and c.is_cuda for c in cols):
        return None
    devs = {c.device for c in cols}
    return next(iter(devs)) if len(devs) == 1 else None


def _empty_device(b: Block) -> torch.device:
    ref = next((c for c in b.columns.values() if isinstance(c, torch.Tensor)), None)
    return ref.device if ref is not None else torch.device("cpu")


def _derived(df, schema, per_block, what: str, needed: Sequence[str] = ()):
    """The lazy frame whose partition p is per_block(block, row0 of p, device
    or None): one host all-reduce completes the table of row counts, its
    exclusive prefix is every partition's first global row index. Not
    streamable: a partition's draws depend on the rows before it."""
    from ..utils.logging import metrics
    from .dataframe import DataFrame, _Derived
    nparts = df.num_partitions

    def compute(blocks: Dict[int, Block]) -> Dict[int, Block]:
        rng = torch.cuda.is_initialized()
        if rng:
            torch.cuda.nvtx.range_push("tfa.sample")
        rows_in = rows_out = on_dev = on_host = 0
        try:
            table = torch.zeros(nparts, dtype=torch.int64)
            for pid, b in blocks.items():
                table[pid] = b.nrows
            dist.all_reduce_host_(table, "Sum")  # (every rank fills the rows of its own partitions)
            starts = np.concatenate([[0], np.cumsum(table.numpy())[:-1]]) if nparts else np.zeros(0, dtype=np.int64)
            res: Dict[int, Block] = {}
            for pid in sorted(blocks):
                b = blocks[pid]
                dev = _dense_device(b, needed) if b.nrows else None
                res[pid] = per_block(b, int(starts[pid]), dev)
                if b.nrows:
                    rows_in += b.nrows
                    rows_out += res[pid].nrows
                    on_dev += dev is not None
                    on_host += dev is None
        finally:
            if rng:
                torch.cuda.nvtx.range_pop()
        metrics.add("sample_rows_in", rows_in)
        metrics.add("sample_rows_out", rows_out)
        metrics.add("sample_device_partitions", on_dev)
        metrics.add("sample_host_partitions", on_host)
        return res

    def compute_agreed(blocks):
        return dist.agreed(what, lambda: compute(blocks))

    return DataFrame(schema, _Derived(df, compute_agreed, streamable=False), nparts)


def _keep(b: Block, mask) -> Block:
    """The rows of b whose mask entry (a device uint8 tensor or a numpy bool
    array) is set."""
    from .dataframe import _filter_block
    if isinstance(mask, np.ndarray):
        mask = torch.from_numpy(np.ascontiguousarray(mask, dtype=bool))
    else:
        mask = mask.view(torch.bool)  # (bytes 0 / 1: the same storage)
    return _filter_block(b, mask)


def _interval_frame(df, seed: int, lo: float, hi: float, what: str):
    """The rows with lo <= u < hi, in input order and in the input's partitions."""
    def per_block(b: Block, row0: int, dev) -> Block:
        if not b.nrows:
            return b
        if dev is not None:
            from .._native import _C
            return _keep(b, _C.random_mask(seed, row0, b.nrows, lo, hi, dev.index))
        u = host_uniform(seed, row0, b.nrows)
        return _keep(b, (u >= lo) & (u < hi))
    return _derived(df, df.schema, per_block, what)


def _replacement_frame(df, seed: int, lam: float, what: str):
    """Row i count_i times, consecutively and in input order."""
    from .join import _take_block
    cdf = poisson_cdf(lam)
    names = list(df.columns)
    tables: Dict[torch.device, torch.Tensor] = {}

    def per_block(b: Block, row0: int, dev) -> Block:
        if not b.nrows:
            return b
        if dev is not None:
            from .._native import _C
            if dev not in tables:
                tables[dev] = torch.tensor(cdf, dtype=torch.float64).to(dev)
            idx = _C.random_expand(_C.random_poisson(seed, row0, b.nrows, tables[dev]))
        else:
            counts = host_poisson(seed, row0, b.nrows, cdf)
            idx = np.repeat(np.arange(b.nrows, dtype=np.int64), counts)
        cols = _take_block(b, names, idx)
        return Block(int(idx.shape[0]), {n: cols[n] for n in b.columns})
    return _derived(df, df.schema, per_block, what)


def sample_frame(df, withReplacement=None, fraction=None, seed=None):  # noqa: N803
    """`DataFrame.sample` with Spark's call forms: sample(0.1), sample(0.1, 3),
    sample(False, 0.1, 3), sample(fraction=0.1, seed=3)."""
    what = "sample"
    if withReplacement is not None and not isinstance(withReplacement, (bool, np.bool_)):
        # sample(fraction[, seed]) / sample(fraction, seed=...): the arguments move one place
        if fraction is not None and seed is not None:
            raise TypeError(f"sample: withReplacement must be a bool, got {withReplacement!r} (with a fraction and a "
                            f"seed after it)")
        withReplacement, fraction, seed = False, withReplacement, (fraction if seed is None else seed)  # noqa: N806
    if fraction is None:
        raise TypeError("sample: a fraction is expected: sample(0.1), sample(False, 0.1, seed)")
    replace = bool(withReplacement)
    check_seed(seed, what)
    if replace:
        lam = _check_fraction(fraction, what, "the fraction (with replacement: the mean count per row)",
                              MAX_REPLACEMENT_FRACTION)
        return _replacement_frame(df, resolve_seed(seed, what), lam, what)
    f = _check_fraction(fraction, what, "the fraction", 1.0)
    return _interval_frame(df, resolve_seed(seed, what), 0.0, f, what)


def random_split(df, weights, seed=None) -> list:
    """`DataFrame.randomSplit`: split i keeps the rows with b_i <= u < b_{i+1}
    under one seed, so every row lands in exactly one split."""
    what = "randomSplit"
    bounds = split_bounds(weights, what)
    check_seed(seed, what)
    s = resolve_seed(seed, what)
    return [_interval_frame(df, s, bounds[i], bounds[i + 1], what) for i in range(len(bounds) - 1)]


def _strata_table(df, col: str, fractions, what: str) -> Tuple[np.ndarray, np.ndarray]:
    """(words uint64 [S] ascending, fractions float64 [S]) of the dict."""
    from ._scalar_columns import _np_dtype
    from .dataframe import _host_sort_words
    if not isinstance(fractions, dict):
        raise TypeError(f"{what}: fractions must be a dict from key value to fraction, got {type(fractions).__name__}")
    if len(fractions) > MAX_STRATA:
        raise ValueError(f"{what}: at most {MAX_STRATA} strata are supported, got {len(fractions)}")
    np_dt = _np_dtype(df, col)
    entries: Dict[int, Tuple[Any, float]] = {}
    for key, fr in fractions.items():
        f = _check_fraction(fr, what, f"the fraction of key {key!r}", 1.0)
        if not isinstance(key, (numbers.Real, np.bool_)):
            raise TypeError(f"{what}: the key {key!r} is not a value of the {np_dt} column '{col}'")
        with np.errstate(all="ignore"):
            try:
                v = np.array([key]).astype(np_dt)
            except (OverflowError, ValueError) as e:
                raise ValueError(f"{what}: the key {key!r} does not fit the {np_dt} column '{col}'") from e
        fk = float(key)
        if np_dt.kind != "f" and (math.isnan(fk) or math.isinf(fk) or float(v[0]) != fk):
            raise ValueError(f"{what}: the key {key!r} is not a value of the {np_dt} column '{col}'")
        w = int(_host_sort_words(torch.from_numpy(v), False)[0])
        if w in entries:
            raise ValueError(f"{what}: the keys {entries[w][0]!r} and {key!r} are the same value of the {np_dt} "
                             f"column '{col}'")
        entries[w] = (key, f)
    ws = sorted(entries)
    return np.array(ws, dtype=np.uint64), np.array([entries[w][1] for w in ws], dtype=np.float64)


def sample_by(df, col, fractions, seed=None):
    """`DataFrame.sampleBy`: a row of stratum k is kept when u < fractions[k];
    keys not in the dict get fraction 0."""
    from .column import Column
    from .dataframe import _check_sort_key, _host_sort_words
    from ._scalar_columns import _scalar_column
    what = "sampleBy"
    if isinstance(col, Column) and col.is_reference and col.sort_order is None:
        col = col._expr[1]
    if not isinstance(col, str):
        raise TypeError(f"{what}: a column name is expected, got {type(col).__name__}")
    if col not in df.schema:
        raise ValueError(f"{what}: Column {col} not found in {df.columns}")
    _check_sort_key(df.schema[col], col, what)
    tw, tf = _strata_table(df, col, fractions, what)
    check_seed(seed, what)
    s = resolve_seed(seed, what)
    S = len(tw)
    tables: Dict[torch.device, Tuple[torch.Tensor, torch.Tensor]] = {}

    def per_block(b: Block, row0: int, dev) -> Block:
        if not b.nrows:
            return b
        key = _scalar_column(b, col, what)
        if dev is not None:
            from .._native import _C
            if S == 0:
                return _keep(b, _C.random_mask(s, row0, b.nrows, 0.0, 0.0, dev.index))
            if dev not in tables:
                tables[dev] = (torch.from_numpy(tw.view(np.int64).copy()).to(dev), torch.from_numpy(tf.copy()).to(dev))
            words = _C.sort_encode([key.contiguous()], [False])
            return _keep(b, _C.random_mask_by(s, row0, words, *tables[dev]))
        return _keep(b, host_mask_by(s, row0, _host_sort_words(key, False), tw, tf))
    return _derived(df, df.schema, per_block, what, needed=[col])


def apply_randoms(df, items: Sequence[Tuple[str, Any]], what: str):
    """`items`: (output name, column name | RandomExpression) in output order;
    every expression becomes one float64 column, drawn in one pass."""
    from .dataframe import tensor_field
    from .types import StructType
    tmp: Dict[int, str] = {}
    taken = set(df.columns) | {n for n, _ in items}
    draws: List[Tuple[str, str, int]] = []  # (temporary column, fn, seed)
    k = 0
    for i, (_, it) in enumerate(items):
        if not isinstance(it, RandomExpression):
            continue
        while f"tfa_random_{k}" in taken:
            k += 1
        tmp[i] = f"tfa_random_{k}"
        taken.add(tmp[i])
        draws.append((tmp[i], it.fn, resolve_seed(it.seed, it.fn)))

    def per_block(b: Block, row0: int, dev) -> Block:
        cols = dict(b.columns)
        n = b.nrows
        for name, fn, seed in draws:
            if not n:
                cols[name] = torch.empty(0, dtype=torch.float64, device=_empty_device(b))
            elif dev is not None:
                from .._native import _C
                cols[name] = (_C.random_uniform if fn == "rand" else _C.random_normal)(seed, row0, n, dev.index)
            else:
                cols[name] = torch.from_numpy(host_uniform(seed, row0, n) if fn == "rand" else
                                              host_normal(seed, row0, n))
        return Block(n, cols)

    fields = list(df.schema.fields) + [tensor_field(name, torch.float64, []) for name, _, _ in draws]
    out = _derived(df, StructType(fields), per_block, what)
    return out._project([(tmp[i] if i in tmp else it, name) for i, (name, it) in enumerate(items)])
