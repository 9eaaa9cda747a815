"""What describe / summary / approxQuantile (stats.py), groupBy().agg
(group_agg.py) and Window / .over() (window.py) share about their value
columns: which columns are numeric scalars with statistics, how one is read
from a partition, its dtypes, and the decoding of an order-preserving word."""
from __future__ import annotations

from typing import Any, List, Optional, Sequence

import numpy as np
import torch

from ..utils import dtypes as D
from .block import Block
from .column_info import ColumnInformation
from .types import BinaryType, BooleanType, StringType

_STAT_DTYPES = (D.DT_UINT8, D.DT_INT8, D.DT_INT16, D.DT_INT32, D.DT_INT64, D.DT_FLOAT, D.DT_DOUBLE)
_SIGN = 1 << 63


# ------------------------------------------------------------------ words
def _decode_sort_word(word, dtype):
    """The value whose ascending order-preserving word is `word` (an unsigned
    64-bit integer or an array of them), as `dtype`: the inverse of
    `_host_sort_words(.., False)`. Words canonicalise, so -0.0 comes back as
    0.0 and every NaN as the quiet NaN."""
    if isinstance(dtype, torch.dtype):
        dtype = torch.empty(0, dtype=dtype).numpy().dtype
    dt = np.dtype(dtype)
    w = np.asarray(word, dtype=np.uint64)
    if dt == np.float32:
        e = w.astype(np.uint32)
        b = np.where(e & np.uint32(0x80000000), e ^ np.uint32(0x80000000), ~e).astype(np.uint32)
        out = b.view(np.float32)
    elif dt == np.float64:
        b = np.where(w & np.uint64(_SIGN), w ^ np.uint64(_SIGN), ~w).astype(np.uint64)
        out = b.view(np.float64)
    elif dt in (np.dtype(np.uint8), np.dtype(np.bool_)):
        out = w.astype(dt)
    elif dt.kind == "i":
        out = (w ^ np.uint64(_SIGN)).view(np.int64).astype(dt)
    else:
        raise TypeError(f"_decode_sort_word: {dt} has no order-preserving word")
    return out[()] if out.ndim == 0 else out


# ------------------------------------------------------------------ columns
def _flatten(items: Sequence[Any]) -> List[Any]:
    return [c for cs in items for c in (cs if isinstance(cs, (list, tuple)) else [cs])]


def _ineligible(df, name: str, what: str) -> Optional[BaseException]:
    """The typed error for a column that cannot be described, None if it can."""
    from .. import core
    f = df.schema[name]
    if isinstance(f.dataType, (StringType, BinaryType)):
        return core.InvalidTypeException(
            f"{what}: '{name}' is a {type(f.dataType).__name__[:-4].lower()} column; only numeric scalar columns "
            f"have statistics")
    stf = ColumnInformation(f).stf
    if isinstance(f.dataType, BooleanType) or (stf is not None and stf.tf_dtype == D.DT_BOOL):
        return core.InvalidTypeException(f"{what}: '{name}' is a bool column; cast it to a numeric type first")
    if stf is None:
        return core.InvalidTypeException(f"{what}: the type of '{name}' ({f.dataType}) has no statistics")
    if stf.tf_dtype not in _STAT_DTYPES:
        return core.InvalidTypeException(
            f"{what}: '{name}' is {D.dtype_name(stf.tf_dtype)}, which has no statistics here (cast to float)")
    if stf.shape.num_dims != 1:
        return core.InvalidDimensionException(
            f"{what}: '{name}' holds a cell of rank {max(stf.shape.num_dims - 1, 0)} per row, not a scalar; reduce "
            f"the cell first (.sum(), .max(), ...)")
    return None


def _stat_columns(df, names: Sequence[Any], what: str) -> List[str]:
    """The columns to describe: the named ones (validated, typed errors), or
    every numeric scalar column in schema order."""
    names = _flatten(names)
    if not names:
        return [n for n in df.columns if _ineligible(df, n, what) is None]
    for n in names:
        if not isinstance(n, str):
            raise TypeError(f"{what}: column names are expected, got {type(n).__name__}")
        if n not in df.schema:
            raise ValueError(f"{what}: Column {n} not found in {df.columns}")
        err = _ineligible(df, n, what)
        if err is not None:
            raise err
    return list(names)


def _tf_dtype(df, name: str) -> int:
    return ColumnInformation(df.schema[name]).stf.tf_dtype


def _np_dtype(df, name: str) -> np.dtype:
    return np.dtype(D.numpy_dtype(_tf_dtype(df, name)))


def _aggregate_dtype(df, fn: str, column: Optional[str]) -> torch.dtype:
    """What count / sum / avg / min / max / a variance of `column` comes out as."""
    if fn == "count":
        return torch.int64
    vt = D.torch_dtype(_tf_dtype(df, column))
    if fn == "sum":
        return torch.float64 if vt.is_floating_point else torch.int64
    return vt if fn in ("min", "max") else torch.float64


def _scalar_column(b: Block, name: str, what: str) -> torch.Tensor:
    from .. import core
    c = b.columns[name]
    if not isinstance(c, torch.Tensor) or c.dim() != 1:
        raise core.InvalidDimensionException(
            f"{what}: the column '{name}' does not hold one scalar per row in this partition; reduce the cell first "
            f"(.sum(), .max(), ...)")
    return c


def _block_on_device(b: Block, names: Sequence[str]) -> bool:
    """The named columns (at least one) of the partition all live on one device."""
    cols = [b.columns[n] for n in names]
    return bool(cols) and all(isinstance(c, torch.Tensor) and c.is_cuda for c in cols) and \
        len({c.device for c in cols}) == 1
