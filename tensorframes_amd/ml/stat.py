"""`Correlation`: the correlation / covariance matrix of a vector column
(`pyspark.ml.stat.Correlation`; `cov` is this project's addition, the
counterpart of `RowMatrix.computeCovariance`).

Every partition is reduced on its own to one float64 record (n, mean[d],
C[d, d]) with C = sum_r (x_r - mean)(x_r - mean)^T: device-resident partitions
through `_C.vector_moments` (kernels/vector_moments.hip: column means, a centred
SYRK on the f64 MFMA, a fold in slice order), host partitions through numpy
(shift by the partition mean, then xc.T @ xc). The records travel as one
zero-filled [nparts, 1 + d + d * d] table (one host all-reduce; every rank
fills the rows of its own partitions) and every rank merges them in ascending
partition order with Chan's formula

    C = C_a + C_b + delta delta^T * n_a n_b / n

skipping empty partitions: never sum(x x^T) - n mean mean^T, and for a given
partitioning the same bits on every rank and for every world size.
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np
import torch

from ..frame.block import Block
from ..frame.column_info import ColumnInformation
from ..frame.types import BinaryType, StringType, StructType
from ..parallel import dist
from ..utils import dtypes as D

MAX_COMPONENTS = 512  # a partition's record is 1 + d + d * d doubles: about 2 MB at the limit


def _vector_column(df, column, what: str) -> int:
    """The number of components d of the vector column, or the typed error."""
    from .. import core
    if not isinstance(column, str):
        raise TypeError(f"{what}: a column name is expected, got {type(column).__name__}")
    if column not in df.schema:
        raise ValueError(f"{what}: Column {column} not found in {df.columns}")
    f = df.schema[column]
    stf = ColumnInformation(f).stf
    if isinstance(f.dataType, (StringType, BinaryType)) or stf is None:
        raise core.InvalidTypeException(
            f"{what}: '{column}' ({f.dataType}) is not a dense vector column of float32 or float64")
    if stf.tf_dtype not in (D.DT_FLOAT, D.DT_DOUBLE):
        raise core.InvalidTypeException(
            f"{what}: '{column}' holds {D.dtype_name(stf.tf_dtype)} cells; cast them to float32 or float64 first")
    if stf.shape.num_dims == 1:
        raise core.InvalidDimensionException(
            f"{what}: '{column}' is a scalar column; a vector column (one cell [d] per row) is expected (F.corr and "
            f"df.stat.corr take two scalar columns)")
    if stf.shape.num_dims != 2:
        raise core.InvalidDimensionException(
            f"{what}: '{column}' holds a cell of rank {stf.shape.num_dims - 1} per row, not a vector [d]")
    d = stf.shape[1]
    if d is None or int(d) < 0:
        raise core.InvalidDimensionException(
            f"{what}: the cells of '{column}' have no fixed length in the schema; run analyze() first")
    if not 1 <= int(d) <= MAX_COMPONENTS:
        raise ValueError(f"{what}: '{column}' has cells of {int(d)} components; 1 to {MAX_COMPONENTS} are supported")
    return int(d)


def _host_record(x: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(mean [d], C [d, d]) of the rows x [n, d] (n >= 1), float64."""
    with np.errstate(all="ignore"):
        x = x.astype(np.float64)
        n = x.shape[0]
        mean = x.sum(0) / n
        xc = x - mean
        mean = mean + xc.sum(0) / n  # (the second pass takes out what rounding left in the mean)
        xc = x - mean
        c = np.triu(xc.T @ xc)
    return mean, c + np.triu(c, 1).T  # (the lower triangle is a copy of the upper)


def _merge(a, b):
    """Chan's merge of (n, mean, C), `a` the earlier rows."""
    if a is None:
        return b
    n = a[0] + b[0]
    with np.errstate(all="ignore"):
        delta = b[1] - a[1]
        f = b[0] / n
        return n, a[1] + delta * f, a[2] + b[2] + np.outer(delta, delta) * (a[0] * f)


def _moments(df, blocks: Dict[int, Block], column: str, d: int, what: str):
    """The merged (n, mean, C) of the column over all ranks, None without rows (collective)."""
    from .. import core, engine
    from .._native import _C
    from ..utils.logging import metrics
    table = torch.zeros((df.num_partitions, 1 + d + d * d), dtype=torch.float64)
    rows = 0
    rng = torch.cuda.is_initialized()
    if rng:
        torch.cuda.nvtx.range_push("tfa.vector_moments")
    try:
        for pid in sorted(blocks):
            b = blocks[pid]
            if not b.nrows:
                continue
            c = b.columns[column]
            if not isinstance(c, torch.Tensor) or c.dim() != 2 or c.shape[1] != d:
                raise core.InvalidDimensionException(
                    f"{what}: the column '{column}' does not hold one dense vector [{d}] per row in partition {pid}")
            table[pid, 0] = b.nrows
            if c.is_cuda and engine.gpu_available():
                mean, cm = _C.vector_moments(c.contiguous())
                table[pid, 1:] = torch.cat([mean, cm.reshape(-1)]).cpu()  # (the partition's one D2H)
                metrics.add("vector_moments_device_partitions")
            else:
                mean, cm = _host_record(c.detach().cpu().numpy())
                table[pid, 1:1 + d] = torch.from_numpy(mean)
                table[pid, 1 + d:] = torch.from_numpy(cm.reshape(-1))
                metrics.add("vector_moments_host_partitions")
            rows += b.nrows
    finally:
        if rng:
            torch.cuda.nvtx.range_pop()
    metrics.add("vector_moments_rows", rows)
    dist.all_reduce_host_(table, "Sum")  # (every rank fills the rows of its own partitions; the others are zero)
    tab = table.numpy()
    acc = None
    for p in range(tab.shape[0]):  # (partition order: the same on every rank)
        if tab[p, 0] > 0:
            acc = _merge(acc, (float(tab[p, 0]), tab[p, 1:1 + d].copy(), tab[p, 1 + d:].reshape(d, d).copy()))
    return acc


def _covariance(acc, d: int) -> np.ndarray:
    if acc is None or acc[0] < 2:
        return np.full((d, d), np.nan)
    with np.errstate(all="ignore"):
        cov = acc[2] / (acc[0] - 1.0)
    bad = ~np.isfinite(np.diagonal(cov))  # a NaN or an infinity among the component's values
    cov[bad, :] = np.nan
    cov[:, bad] = np.nan
    return cov


def _correlation(acc, d: int) -> np.ndarray:
    cov = _covariance(acc, d)
    var = np.diagonal(cov).copy()
    with np.errstate(all="ignore"):
        r = cov / np.sqrt(np.outer(var, var))  # (unclamped, as F.corr)
    bad = ~(np.isfinite(var) & (var > 0))  # constant components: NaN where Spark gives null
    r[bad, :] = np.nan
    r[:, bad] = np.nan
    r[np.diag_indices(d)] = np.where(bad, np.nan, 1.0)
    return r


def _matrix_frame(df, column: str, name: str, finish, what: str):
    from ..frame.dataframe import DataFrame, _Derived, tensor_field
    d = _vector_column(df, column, what)

    def compute(blocks):
        acc = dist.agreed(what, lambda: _moments(df, blocks, column, d, what))
        if dist.rank() != 0:  # (partition 0 lives on rank 0)
            return {}
        return {0: Block(1, {name: torch.from_numpy(finish(acc, d)).reshape(1, d, d)})}
    schema = StructType([tensor_field(name, torch.float64, [d, d])])
    return DataFrame(schema, _Derived(df, compute, streamable=False), 1)


class Correlation:
    """`pyspark.ml.stat.Correlation` for a dense vector column of float32 or
    float64 cells `[d]`, 1 <= d <= 512. The results are lazy frames of one
    partition and one row; evaluating them is collective."""

    @staticmethod
    def corr(df, column, method="pearson"):
        """The Pearson correlation matrix as one `double[d, d]` cell in a column
        `pearson(<column>)`: r_ij = C_ij / sqrt(C_ii C_jj), the diagonal exactly
        1.0, exactly symmetric. A constant component, or one that holds a NaN
        or an infinity, has a NaN row and column."""
        if method != "pearson":
            raise NotImplementedError(f"Correlation.corr: the method {method!r} is not implemented; only 'pearson' is")
        return _matrix_frame(df, column, f"pearson({column})", _correlation, "Correlation.corr")

    @staticmethod
    def cov(df, column):
        """The sample covariance matrix (divisor n - 1) as one `double[d, d]`
        cell in a column `cov(<column>)`; all NaN below two rows. Not part of
        Spark's class: the counterpart of `RowMatrix.computeCovariance`."""
        return _matrix_frame(df, column, f"cov({column})", _covariance, "Correlation.cov")
