"""`KMeans` / `KMeansModel` (`pyspark.ml.clustering.KMeans`): Lloyd's algorithm
over a dense vector column.

Per iteration every partition is reduced on its own to one float64 record
(count [k], sums [k, d], cost, bad): device-resident partitions through
`_C.kmeans_step` (kernels/kmeans.hip: the assignment on the f64 MFMA without
an [n, k] distance matrix, the per-centre sums as a one-hot GEMM over row
slices, folds in a fixed order), host partitions through numpy. Both shift the
rows and the centres by o, the mean of the centres (`_shift`: f64, index
order, the same bits as the binding's), score a centre by ||c'||^2 - 2 x'.c'
with x' = x - o, c' = c - o, give a tie to the smallest index and sum x', not
x: a partition far from the origin loses no digits. The records travel as one
zero-filled [nparts, k + k d + 2] table (one host all-reduce per iteration;
every rank fills the rows of its own partitions) and every rank adds them in
ascending partition order: for a given partitioning the same centre bits on
every rank and for every world size. The new centre is o + S_c / count_c; a
centre without rows keeps its place.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from ..frame.block import Block
from ..frame.types import StructType
from ..parallel import dist
from .stat import _vector_column

MAX_K, MAX_COMPONENTS, MAX_CELLS = 1024, 2048, 262144  # kernels.h: kKMeansMaxK, kKMeansMaxD, kKMeansMaxKD
_HOST_CHUNK_CELLS = 1 << 22  # host path: rows x k scores alive at a time


def _shift(centers: np.ndarray) -> np.ndarray:
    """The mean of the centres, added in index order (the expression of `_C.kmeans_step`)."""
    o = np.zeros(centers.shape[1])
    for c in centers:
        o = o + c
    return o / centers.shape[0]


def _host_assign(x: np.ndarray, centers: np.ndarray, o: np.ndarray):
    """(assign int32 [n], dist f64 [n]) of the rows x [n, d]: -1 and 0.0 for a row with a NaN or an infinity."""
    n, k = x.shape[0], centers.shape[0]
    assign, dist_ = np.full(n, -1, dtype=np.int32), np.zeros(n)
    cs = centers - o
    cn = (cs * cs).sum(1)
    step = max(1, _HOST_CHUNK_CELLS // k)
    with np.errstate(all="ignore"):
        for a in range(0, n, step):
            xs = x[a:a + step].astype(np.float64) - o
            xn = (xs * xs).sum(1)
            ok = np.isfinite(xn)
            score = cn[None, :] - 2.0 * (xs[ok] @ cs.T)
            best = score.argmin(1)  # (the first of equal scores)
            assign[a:a + step][ok] = best
            dist_[a:a + step][ok] = np.maximum(xn[ok] + score[np.arange(best.size), best], 0.0)
    return assign, dist_


def _host_step(x: np.ndarray, centers: np.ndarray, o: np.ndarray):
    """The record (counts [k], sums of x - o [k, d], cost, bad) of the rows x [n, d]."""
    k = centers.shape[0]
    assign, dist_ = _host_assign(x, centers, o)
    sums = np.zeros(centers.shape)
    for c in np.unique(assign[assign >= 0]):
        sums[c] = (x[assign == c].astype(np.float64) - o).sum(0)
    return np.bincount(assign[assign >= 0], minlength=k), sums, dist_.sum(), int((assign < 0).sum())


def _column(b: Block, pid: int, column: str, d: int, what: str):
    from .. import core
    c = b.columns[column]
    if not isinstance(c, torch.Tensor) or c.dim() != 2 or c.shape[1] != d:
        raise core.InvalidDimensionException(
            f"{what}: the column '{column}' does not hold one dense vector [{d}] per row in partition {pid}")
    return c


def _lloyd_step(df, blocks: Dict[int, Block], column: str, centers: np.ndarray, what: str):
    """(counts [k], sums [k, d], cost, bad) over all ranks against `centers` (collective)."""
    from .. import engine
    from .._native import _C
    from ..utils.logging import metrics
    k, d = centers.shape
    o = _shift(centers)
    table = torch.zeros((df.num_partitions, k + k * d + 2), dtype=torch.float64)
    cdev = {}  # the centres per device
    for pid in sorted(blocks):
        b = blocks[pid]
        if not b.nrows:
            continue
        c = _column(b, pid, column, d, what)
        if c.is_cuda and engine.gpu_available():
            if c.device not in cdev:
                cdev[c.device] = torch.from_numpy(centers).to(c.device)
            counts, sums, cost, bad = _C.kmeans_step(c.contiguous(), cdev[c.device])
            table[pid] = torch.cat([counts.double(), sums.reshape(-1), cost, bad.double()]).cpu()  # (the one D2H)
            metrics.add("kmeans_device_partitions")
        else:
            counts, sums, cost, bad = _host_step(c.detach().cpu().numpy(), centers, o)
            table[pid] = torch.from_numpy(np.concatenate([counts, sums.reshape(-1), [cost, bad]]))
            metrics.add("kmeans_host_partitions")
    dist.all_reduce_host_(table, "Sum")  # (every rank fills the rows of its own partitions; the others are zero)
    acc = np.zeros(k + k * d + 2)
    for row in table.numpy():  # (partition order: the same on every rank)
        acc = acc + row
    return acc[:k], acc[k:k + k * d].reshape(k, d), float(acc[-2]), int(acc[-1])


def _random_start(df, blocks: Dict[int, Block], column: str, k: int, d: int, seed: int, what: str) -> np.ndarray:
    """k distinct rows of the frame, a function of (seed, row sequence) alone (collective)."""
    rows = torch.zeros(df.num_partitions, dtype=torch.int64)
    for pid, b in blocks.items():
        rows[pid] = b.nrows
    dist.all_reduce_host_(rows, "Sum")
    starts = np.concatenate([[0], np.cumsum(rows.numpy())])
    if starts[-1] < k:
        raise ValueError(f"{what}: the frame has {int(starts[-1])} rows, fewer than k = {k}")
    picks = np.sort(np.random.default_rng(seed).choice(int(starts[-1]), k, replace=False))
    table = torch.zeros((k, d), dtype=torch.float64)
    for j, g in enumerate(picks):
        pid = int(np.searchsorted(starts, g, side="right")) - 1
        if pid in blocks:
            table[j] = _column(blocks[pid], pid, column, d, what)[int(g - starts[pid])].double().cpu()
    dist.all_reduce_host_(table, "Sum")
    return table.numpy()


class KMeansSummary:
    """`trainingCost` (the sum of squared distances measured by the last
    iteration run, against the centres that iteration started from: Spark's
    definition), `clusterSizes` (of that same iteration), `numIter` and `k`."""

    def __init__(self, training_cost: float, cluster_sizes: List[int], num_iter: int):
        self.trainingCost = training_cost  # noqa: N815
        self.clusterSizes = cluster_sizes  # noqa: N815
        self.numIter = num_iter  # noqa: N815
        self.k = len(cluster_sizes)


class KMeansModel:
    """The fitted centres. `transform` is lazy and works partition by
    partition: device-resident partitions through `_C.kmeans_assign` (the
    column stays on the device), host partitions through numpy. A row that
    holds a NaN or an infinity is predicted -1 (Spark gives it a cluster)."""

    def __init__(self, centers: np.ndarray, featuresCol: str, predictionCol: str,  # noqa: N803
                 summary: Optional[KMeansSummary] = None):
        self._centers = np.ascontiguousarray(centers, dtype=np.float64)
        self._features, self._prediction, self._summary = featuresCol, predictionCol, summary

    def clusterCenters(self) -> List[np.ndarray]:  # noqa: N802
        """The k centres, one float64 array [d] each."""
        return [c.copy() for c in self._centers]

    @property
    def hasSummary(self) -> bool:  # noqa: N802
        return self._summary is not None

    @property
    def summary(self) -> KMeansSummary:
        if self._summary is None:
            raise RuntimeError("KMeansModel.summary: this model has no training summary")
        return self._summary

    def predict(self, vector) -> int:
        """The index of the nearest centre of one vector [d], on the host; -1 with a NaN or an infinity."""
        v = np.asarray(vector, dtype=np.float64).reshape(1, -1)
        if v.shape[1] != self._centers.shape[1]:
            raise ValueError(f"KMeansModel.predict: a vector of {self._centers.shape[1]} components is expected, got "
                             f"{v.shape[1]}")
        return int(_host_assign(v, self._centers, _shift(self._centers))[0][0])

    def transform(self, df):
        """`df` with the int32 column `predictionCol` appended: the index of the nearest centre (a tie to the
        smallest), -1 for a row with a NaN or an infinity. Lazy and partition-local."""
        from .. import engine
        from .._native import _C
        from ..frame.dataframe import DataFrame, _Derived, tensor_field
        what = "KMeansModel.transform"
        column, name, centers = self._features, self._prediction, self._centers
        d = _vector_column(df, column, what, MAX_COMPONENTS)
        if d != centers.shape[1]:
            raise ValueError(f"{what}: '{column}' has cells of {d} components, the centres of {centers.shape[1]}")
        if name in df.schema:
            raise ValueError(f"{what}: the frame already has a column '{name}'; choose another predictionCol")
        o = _shift(centers)

        def compute(blocks):
            out = {}
            for pid, b in blocks.items():
                c = _column(b, pid, column, d, what) if b.nrows else None
                if c is None:
                    pred = torch.empty(0, dtype=torch.int32)
                elif c.is_cuda and engine.gpu_available():
                    pred = _C.kmeans_assign(c.contiguous(), torch.from_numpy(centers))[0]
                else:
                    pred = torch.from_numpy(_host_assign(c.detach().cpu().numpy(), centers, o)[0])
                out[pid] = Block(b.nrows, {**b.columns, name: pred})
            return out
        schema = StructType(list(df.schema.fields) + [tensor_field(name, torch.int32, [])])
        return DataFrame(schema, _Derived(df, compute), df.num_partitions)


_PARAMS = ("featuresCol", "predictionCol", "k", "maxIter", "tol", "seed", "initMode", "distanceMeasure", "weightCol")


class KMeans:
    """`pyspark.ml.clustering.KMeans` for a dense vector column of float32 or
    float64 cells `[d]`: 1 <= k <= 1024, 1 <= d <= 2048, k d <= 262144, Euclidean
    distance, unweighted, `initMode="random"` (k distinct rows chosen by
    `np.random.default_rng(seed)` over the global row sequence) or the centres
    given to `setInitialCenters` (this project's addition). `fit` is
    collective; rows with a NaN or an infinity are a ValueError."""

    def __init__(self, featuresCol="features", predictionCol="prediction", k=2, maxIter=20, tol=1e-4,  # noqa: N803
                 seed=None, initMode="random", distanceMeasure="euclidean", weightCol=None):
        self._initial = None
        for p in _PARAMS:
            getattr(self, "set" + p[0].upper() + p[1:])(locals()[p])

    def _set(self, name: str, v):
        what = f"KMeans.set{name[0].upper()}{name[1:]}"
        if name in ("featuresCol", "predictionCol") and (not isinstance(v, str) or not v):
            raise TypeError(f"{what}: a non-empty column name is expected, got {v!r}")
        if name in ("k", "maxIter") and (isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1):
            raise ValueError(f"{what}: a positive int is expected, got {v!r}")
        if name == "k" and v > MAX_K:
            raise ValueError(f"{what}: 1 to {MAX_K} clusters are supported, got {v}")
        if name == "tol" and not (isinstance(v, (int, float)) and v >= 0):
            raise ValueError(f"{what}: a number >= 0 is expected, got {v!r}")
        if name == "seed" and v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0):
            raise ValueError(f"{what}: a non-negative int or None is expected, got {v!r}")
        if name == "initMode" and v != "random":
            raise NotImplementedError(f"{what}: the initMode {v!r} is not implemented; only 'random' and "
                                      f"setInitialCenters are")
        if name == "distanceMeasure" and v != "euclidean":
            raise NotImplementedError(f"{what}: the distanceMeasure {v!r} is not implemented; only 'euclidean' is")
        if name == "weightCol" and v is not None:
            raise NotImplementedError(f"{what}: weighted rows are not implemented; only weightCol=None is")
        setattr(self, "_" + name, v)
        return self

    def setInitialCenters(self, centers) -> "KMeans":  # noqa: N802
        """Start from these centres [k, d] instead of a random draw (not part of Spark's class)."""
        c = np.array(centers, dtype=np.float64)
        if c.ndim != 2 or not np.isfinite(c).all():
            raise ValueError("KMeans.setInitialCenters: a finite array [k, d] is expected")
        self._initial = c
        return self

    def fit(self, df) -> KMeansModel:
        """Lloyd iterations from the start until every centre moved by at most `tol` or `maxIter` is reached
        (collective). A row with a NaN or an infinity is a ValueError on every rank."""
        from ..utils.logging import metrics
        what = "KMeans.fit"
        column, k = self._featuresCol, self._k
        d = _vector_column(df, column, what, MAX_COMPONENTS)
        if k * d > MAX_CELLS:
            raise ValueError(f"{what}: k d = {k} x {d} centre cells; up to {MAX_CELLS} are supported")
        if self._initial is not None and self._initial.shape != (k, d):
            raise ValueError(f"{what}: the initial centres are {list(self._initial.shape)}, [k, d] = [{k}, {d}] expected")
        seed = self._seed
        if self._initial is None and seed is None:  # (drawn once, the same on every rank)
            seed = dist.broadcast_object(int(np.random.SeedSequence().generate_state(1)[0]), 0) \
                if dist.is_distributed() else int(np.random.SeedSequence().generate_state(1)[0])

        def run():
            blocks = df._blocks()
            centers = self._initial.copy() if self._initial is not None else \
                _random_start(df, blocks, column, k, d, seed, what)
            if not np.isfinite(centers).all():
                raise ValueError(f"{what}: a row chosen as a starting centre holds a NaN or an infinity")
            for it in range(self._maxIter):
                counts, sums, cost, bad = _lloyd_step(df, blocks, column, centers, what)
                if bad:
                    raise ValueError(f"{what}: '{column}' holds {bad} rows with a NaN or an infinity")
                new, full = centers.copy(), counts > 0  # (a centre without rows keeps its place)
                new[full] = _shift(centers) + sums[full] / counts[full, None]
                moved = np.sqrt(((new - centers) ** 2).sum(1)).max()
                centers = new
                if moved <= self._tol:
                    break
            metrics.add("kmeans_iterations", it + 1)
            return centers, KMeansSummary(cost, [int(c) for c in counts], it + 1)
        rng = torch.cuda.is_initialized()
        if rng:
            torch.cuda.nvtx.range_push("tfa.kmeans")
        try:
            centers, summary = dist.agreed(what, run)
        finally:
            if rng:
                torch.cuda.nvtx.range_pop()
        return KMeansModel(centers, column, self._predictionCol, summary)


def _accessors(name: str):
    cap = name[0].upper() + name[1:]

    def setter(self, value):
        return self._set(name, value)

    def getter(self):
        return getattr(self, "_" + name)
    setter.__name__, getter.__name__ = "set" + cap, "get" + cap
    setter.__doc__ = f"Sets `{name}` and returns the estimator, as pyspark's setter does."
    getter.__doc__ = f"The value of `{name}`."
    setattr(KMeans, "set" + cap, setter)
    setattr(KMeans, "get" + cap, getter)


for _p in _PARAMS:
    _accessors(_p)
