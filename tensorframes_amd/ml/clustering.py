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

`GaussianMixture` / `GaussianMixtureModel` (`pyspark.ml.clustering.GaussianMixture`):
EM over the same kind of column, in the same frame form. Per iteration the
host takes the Cholesky factor L_j of every covariance, T_j = L_j^-1 and c_j =
log w_j - (d / 2) log 2 pi - sum_i log L_j,ii; every partition gives one float64
record (N [k], S [k, d], C [k, d, d], loglik, bad) with S and C centred at the
current means: device-resident partitions through `_C.gmm_step`
(kernels/gmm.hip), host partitions through numpy in the same form. The records
travel as one zero-filled [nparts, k + k d + k d^2 + 2] table and are added in
ascending partition order. Then w_j = N_j / sum N, mu_j += S_j / N_j, Sigma_j =
C_j / N_j - (S_j / N_j)(S_j / N_j)^T.
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


# ------------------------------------------------------------------ GaussianMixture
GMM_MAX_K, GMM_MAX_COMPONENTS, GMM_MAX_CELLS = 64, 128, 262144  # kernels.h: kGmmMaxK, kGmmMaxD, kGmmMaxKDD


def _gmm_params(weights: np.ndarray, covs: np.ndarray, what: str, produced_by: int):
    """(transforms [k, d, d], logconst [k]) of a mixture: T_j = L_j^-1 (lower triangular, zeros above the
    diagonal) with Sigma_j = L_j L_j^T, c_j = log w_j - (d / 2) log 2 pi - sum_i log L_j,ii. A covariance that numpy's
    Cholesky refuses is a ValueError that names the component and the iteration that produced it (0: the start)."""
    k, d = covs.shape[0], covs.shape[1]
    transforms, logconst = np.zeros((k, d, d)), np.zeros(k)
    for j in range(k):
        try:
            if not (np.isfinite(covs[j]).all() and weights[j] > 0):
                raise np.linalg.LinAlgError
            low = np.linalg.cholesky(covs[j])
        except np.linalg.LinAlgError:
            where = "of the start" if produced_by == 0 else f"after iteration {produced_by}"
            raise ValueError(f"{what}: the covariance of component {j} {where} is not positive definite (or the "
                             f"component has no weight); Spark falls back to a pseudo-determinant, this project "
                             f"refuses") from None
        transforms[j] = np.tril(np.linalg.solve(low, np.eye(d)))
        logconst[j] = np.log(weights[j]) - 0.5 * d * np.log(2.0 * np.pi) - np.log(np.diagonal(low)).sum()
    return transforms, logconst


def _host_estep(x: np.ndarray, means: np.ndarray, transforms: np.ndarray, logconst: np.ndarray):
    """(r [n, k], lse [n], ok [n]) of the rows x [n, d]: log p_ij = c_j - ||T_j (x_i - mu_j)||^2 / 2, the safe
    log-sum-exp, r_ij = exp(log p_ij - lse_i); a row with a NaN or an infinity (or an lse that is not finite) has
    r = 0, lse = 0 and ok False. The expression of `_C.gmm_step`; no [n, k, d] array."""
    n, k = x.shape[0], means.shape[0]
    xd = x.astype(np.float64)
    logp = np.empty((n, k))
    with np.errstate(all="ignore"):
        for j in range(k):
            z = (xd - means[j]) @ transforms[j].T
            logp[:, j] = logconst[j] - 0.5 * (z * z).sum(1)
        top = logp.max(1)
        lse = top + np.log(np.exp(logp - top[:, None]).sum(1))
        ok = np.isfinite(xd).all(1) & np.isfinite(lse)
        r = np.where(ok[:, None], np.exp(logp - lse[:, None]), 0.0)
    return r, np.where(ok, lse, 0.0), ok


def _host_em_step(x: np.ndarray, means: np.ndarray, transforms: np.ndarray, logconst: np.ndarray):
    """The record (N [k], S [k, d], C [k, d, d], loglik, bad) of the rows x [n, d], centred at the current means."""
    k, d = means.shape
    r, lse, ok = _host_estep(x, means, transforms, logconst)
    xd = np.where(ok[:, None], x.astype(np.float64), 0.0)
    N, S, C = r.sum(0), np.zeros((k, d)), np.zeros((k, d, d))
    for j in range(k):
        xc = xd - means[j]
        S[j] = r[:, j] @ xc
        up = np.triu((xc * r[:, j, None]).T @ xc)
        C[j] = up + np.triu(up, 1).T  # (exactly symmetric)
    return N, S, C, lse.sum(), int((~ok).sum())


def _em_step(df, blocks: Dict[int, Block], column: str, means: np.ndarray, transforms: np.ndarray,
             logconst: np.ndarray, what: str):
    """(N [k], S [k, d], C [k, d, d], loglik, bad) over all ranks (collective)."""
    from .. import engine
    from .._native import _C
    from ..utils.logging import metrics
    k, d = means.shape
    table = torch.zeros((df.num_partitions, k + k * d + k * d * d + 2), dtype=torch.float64)
    pdev = {}  # the parameters per device
    for pid in sorted(blocks):
        b = blocks[pid]
        if not b.nrows:
            continue
        c = _column(b, pid, column, d, what)
        if c.is_cuda and engine.gpu_available():
            if c.device not in pdev:
                pdev[c.device] = [torch.from_numpy(a).to(c.device) for a in (means, transforms, logconst)]
            N, S, C, ll, bad = _C.gmm_step(c.contiguous(), *pdev[c.device])
            table[pid] = torch.cat([N, S.reshape(-1), C.reshape(-1), ll, bad.double()]).cpu()  # (the one D2H)
            metrics.add("gmm_device_partitions")
        else:
            N, S, C, ll, bad = _host_em_step(c.detach().cpu().numpy(), means, transforms, logconst)
            table[pid] = torch.from_numpy(np.concatenate([N, S.reshape(-1), C.reshape(-1), [ll, bad]]))
            metrics.add("gmm_host_partitions")
    dist.all_reduce_host_(table, "Sum")  # (every rank fills the rows of its own partitions; the others are zero)
    acc = np.zeros(table.shape[1])
    for row in table.numpy():  # (partition order: the same on every rank)
        acc = acc + row
    a, b = k + k * d, k + k * d + k * d * d
    return acc[:k], acc[k:a].reshape(k, d), acc[a:b].reshape(k, d, d), float(acc[-2]), int(acc[-1])


def _gmm_assign(c: torch.Tensor, params, pdev: dict):
    """(prob f64 [n, k], pred int32 [n]) of one partition's column, on the column's device."""
    from .. import engine
    from .._native import _C
    if c.is_cuda and engine.gpu_available():
        if c.device not in pdev:  # (one parameter upload per device)
            pdev[c.device] = [torch.from_numpy(a).to(c.device) for a in params]
        return _C.gmm_predict(c.contiguous(), *pdev[c.device])
    r, _, ok = _host_estep(c.detach().cpu().numpy(), *params)
    return torch.from_numpy(r), torch.from_numpy(np.where(ok, r.argmax(1), -1).astype(np.int32))


def _cluster_sizes(df, blocks: Dict[int, Block], column: str, params, what: str) -> List[int]:
    """The rows per component by the largest responsibility under `params` (collective)."""
    k, d = params[0].shape
    table, pdev = torch.zeros((df.num_partitions, k), dtype=torch.int64), {}
    for pid in sorted(blocks):
        if blocks[pid].nrows:
            pred = _gmm_assign(_column(blocks[pid], pid, column, d, what), params, pdev)[1]
            table[pid] = torch.bincount(pred[pred >= 0].long(), minlength=k).cpu()
    dist.all_reduce_host_(table, "Sum")
    return [int(v) for v in table.sum(0)]


class MultivariateGaussian:
    """One component: `.mean` float64 [d] and `.cov` float64 [d, d]."""

    def __init__(self, mean: np.ndarray, cov: np.ndarray):
        self.mean, self.cov = mean, cov


class GaussianMixtureSummary:
    """`logLikelihood` (of the last E step run, under the parameters that step
    started from), `clusterSizes` (the rows per component by the largest
    responsibility of that step), `numIter` and `k`."""

    def __init__(self, log_likelihood: float, cluster_sizes: List[int], num_iter: int):
        self.logLikelihood = log_likelihood  # noqa: N815
        self.clusterSizes = cluster_sizes  # noqa: N815
        self.numIter = num_iter  # noqa: N815
        self.k = len(cluster_sizes)


class GaussianMixtureModel:
    """The fitted mixture. `transform` is lazy and works partition by partition:
    device-resident partitions through `_C.gmm_predict` (the column stays on
    the device, one parameter upload per device), host partitions through
    numpy. A row that holds a NaN or an infinity gets the prediction -1 and a
    zero probability vector."""

    def __init__(self, weights, means, covs, featuresCol: str, predictionCol: str, probabilityCol: str,  # noqa: N803
                 summary: Optional[GaussianMixtureSummary] = None):
        self._weights = np.ascontiguousarray(weights, dtype=np.float64)
        self._means = np.ascontiguousarray(means, dtype=np.float64)
        self._covs = np.ascontiguousarray(covs, dtype=np.float64)
        self._features, self._prediction, self._probability = featuresCol, predictionCol, probabilityCol
        self._summary = summary
        self._params = (self._means,) + _gmm_params(self._weights, self._covs, "GaussianMixtureModel",
                                                    summary.numIter if summary is not None else 0)

    @property
    def weights(self) -> List[float]:
        return [float(w) for w in self._weights]

    @property
    def gaussians(self) -> List[MultivariateGaussian]:
        return [MultivariateGaussian(m.copy(), c.copy()) for m, c in zip(self._means, self._covs)]

    @property
    def gaussiansDF(self):  # noqa: N802
        """A frame of k rows with the columns `mean` double[d] and `cov` double[d, d]."""
        from ..frame.dataframe import from_columns
        return from_columns({"mean": self._means.copy(), "cov": self._covs.copy()}, num_partitions=1)

    @property
    def hasSummary(self) -> bool:  # noqa: N802
        return self._summary is not None

    @property
    def summary(self) -> GaussianMixtureSummary:
        if self._summary is None:
            raise RuntimeError("GaussianMixtureModel.summary: this model has no training summary")
        return self._summary

    def predictProbability(self, vector) -> np.ndarray:  # noqa: N802
        """The responsibilities [k] of one vector [d], on the host; zeros with a NaN or an infinity."""
        v = np.asarray(vector, dtype=np.float64).reshape(1, -1)
        if v.shape[1] != self._means.shape[1]:
            raise ValueError(f"GaussianMixtureModel.predictProbability: a vector of {self._means.shape[1]} components "
                             f"is expected, got {v.shape[1]}")
        return _host_estep(v, *self._params)[0][0]

    def predict(self, vector) -> int:
        """The component of the first largest responsibility of one vector [d], on the host; -1 with a NaN or an
        infinity."""
        p = self.predictProbability(vector)
        return int(p.argmax()) if p.any() else -1

    def transform(self, df):
        """`df` with `probabilityCol` (double[k], the responsibilities) and `predictionCol` (int32, the first
        largest of them; -1 and zeros for a row with a NaN or an infinity) appended. Lazy and partition-local."""
        from ..frame.dataframe import DataFrame, _Derived, tensor_field
        what = "GaussianMixtureModel.transform"
        column, params = self._features, self._params
        k, dm = self._means.shape
        d = _vector_column(df, column, what, GMM_MAX_COMPONENTS)
        if d != dm:
            raise ValueError(f"{what}: '{column}' has cells of {d} components, the means of {dm}")
        for name in (self._probability, self._prediction):
            if name in df.schema:
                raise ValueError(f"{what}: the frame already has a column '{name}'; choose another name")
        pdev = {}

        def compute(blocks):
            out = {}
            for pid, b in blocks.items():
                if b.nrows:
                    prob, pred = _gmm_assign(_column(b, pid, column, d, what), params, pdev)
                else:
                    prob, pred = torch.empty((0, k), dtype=torch.float64), torch.empty(0, dtype=torch.int32)
                out[pid] = Block(b.nrows, {**b.columns, self._probability: prob, self._prediction: pred})
            return out
        schema = StructType(list(df.schema.fields) + [tensor_field(self._probability, torch.float64, [k]),
                                                      tensor_field(self._prediction, torch.int32, [])])
        return DataFrame(schema, _Derived(df, compute), df.num_partitions)


_GMM_PARAMS = ("featuresCol", "predictionCol", "probabilityCol", "k", "maxIter", "tol", "seed", "aggregationDepth",
               "weightCol")


class GaussianMixture:
    """`pyspark.ml.clustering.GaussianMixture` for a dense vector column of
    float32 or float64 cells `[d]`: 1 <= k <= 64, 1 <= d <= 128, k d^2 <= 262144,
    full covariances, unweighted. The start is the model given to
    `setInitialModel` (this project's addition) or k distinct rows chosen by
    `np.random.default_rng(seed)` as the means, the diagonal of the column's
    variances as every covariance and the weights 1 / k (Spark samples its
    start). `fit` is collective; rows with a NaN or an infinity and a
    covariance that is not positive definite are a ValueError."""

    def __init__(self, featuresCol="features", predictionCol="prediction", probabilityCol="probability",  # noqa: N803
                 k=2, maxIter=100, tol=0.01, seed=None, aggregationDepth=2, weightCol=None):
        self._initial = None
        for p in _GMM_PARAMS:
            getattr(self, "set" + p[0].upper() + p[1:])(locals()[p])

    def _set(self, name: str, v):
        what = f"GaussianMixture.set{name[0].upper()}{name[1:]}"
        if name.endswith("Col") and name != "weightCol" and (not isinstance(v, str) or not v):
            raise TypeError(f"{what}: a non-empty column name is expected, got {v!r}")
        if name in ("k", "maxIter", "aggregationDepth") and \
                (isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1):
            raise ValueError(f"{what}: a positive int is expected, got {v!r}")
        if name == "aggregationDepth" and v < 2:  # (validated as Spark does, then ignored: one all-reduce)
            raise ValueError(f"{what}: a depth >= 2 is expected, got {v}")
        if name == "k" and v > GMM_MAX_K:
            raise ValueError(f"{what}: 1 to {GMM_MAX_K} components are supported, got {v}")
        if name == "tol" and not (isinstance(v, (int, float)) and v >= 0):
            raise ValueError(f"{what}: a number >= 0 is expected, got {v!r}")
        if name == "seed" and v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0):
            raise ValueError(f"{what}: a non-negative int or None is expected, got {v!r}")
        if name == "weightCol" and v is not None:
            raise NotImplementedError(f"{what}: weighted rows are not implemented; only weightCol=None is")
        setattr(self, "_" + name, v)
        return self

    def setInitialModel(self, weights, means, covs) -> "GaussianMixture":  # noqa: N802
        """Start from weights [k], means [k, d] and covariances [k, d, d] (not part of Spark's class)."""
        w, m, c = [np.array(a, dtype=np.float64) for a in (weights, means, covs)]
        if w.ndim != 1 or m.ndim != 2 or c.ndim != 3 or m.shape[0] != w.shape[0] or \
                c.shape != (m.shape[0], m.shape[1], m.shape[1]):
            raise ValueError(f"GaussianMixture.setInitialModel: weights [k], means [k, d] and covs [k, d, d] are "
                             f"expected, got {list(w.shape)}, {list(m.shape)} and {list(c.shape)}")
        if not (np.isfinite(w).all() and np.isfinite(m).all() and np.isfinite(c).all() and (w > 0).all()):
            raise ValueError("GaussianMixture.setInitialModel: finite values and positive weights are expected")
        self._initial = (w / w.sum(), m, c)
        return self

    def fit(self, df) -> GaussianMixtureModel:
        """EM iterations from the start until the log-likelihood changed by less than `tol` or `maxIter` is
        reached (collective). A row with a NaN or an infinity, and a covariance that is not positive definite, are
        a ValueError on every rank."""
        from . import stat
        from ..utils.logging import metrics
        what = "GaussianMixture.fit"
        column, k = self._featuresCol, self._k
        d = _vector_column(df, column, what, GMM_MAX_COMPONENTS)
        if k * d * d > GMM_MAX_CELLS:
            raise ValueError(f"{what}: k d^2 = {k} x {d}^2 covariance cells; up to {GMM_MAX_CELLS} are supported")
        if self._initial is not None and self._initial[1].shape != (k, d):
            raise ValueError(f"{what}: the initial means are {list(self._initial[1].shape)}, [k, d] = [{k}, {d}] "
                             f"expected")
        seed = self._seed
        if self._initial is None and seed is None:  # (drawn once, the same on every rank)
            seed = dist.broadcast_object(int(np.random.SeedSequence().generate_state(1)[0]), 0) \
                if dist.is_distributed() else int(np.random.SeedSequence().generate_state(1)[0])

        def run():
            blocks = df._blocks()
            if self._initial is not None:
                weights, means, covs = [a.copy() for a in self._initial]
            else:
                means = _random_start(df, blocks, column, k, d, seed, what)
                count, q, acc = stat._summary(df, blocks, column, None, d, ("variance",), what)
                var = stat._metric("variance", count, q, acc, d).numpy().reshape(d)
                if not (np.isfinite(means).all() and np.isfinite(var).all()):
                    raise ValueError(f"{what}: '{column}' holds rows with a NaN or an infinity")
                weights, covs = np.full(k, 1.0 / k), np.tile(np.diag(var), (k, 1, 1))
            prev = None
            for it in range(self._maxIter):
                transforms, logconst = _gmm_params(weights, covs, what, it)
                last = (means, transforms, logconst)
                N, S, C, loglik, bad = _em_step(df, blocks, column, means, transforms, logconst, what)
                if bad:
                    raise ValueError(f"{what}: '{column}' holds {bad} rows with a NaN or an infinity")
                with np.errstate(all="ignore"):  # (a component without weight is refused by _gmm_params)
                    step = S / N[:, None]
                    weights, means = N / N.sum(), means + step
                    covs = C / N[:, None, None] - step[:, :, None] * step[:, None, :]
                done = prev is not None and abs(loglik - prev) < self._tol
                prev = loglik
                if done:
                    break
            _gmm_params(weights, covs, what, it + 1)  # (the model's own covariances are checked too)
            metrics.add("gmm_iterations", it + 1)
            sizes = _cluster_sizes(df, blocks, column, last, what)
            return weights, means, covs, GaussianMixtureSummary(loglik, sizes, it + 1)
        rng = torch.cuda.is_initialized()
        if rng:
            torch.cuda.nvtx.range_push("tfa.gmm")
        try:
            weights, means, covs, summary = dist.agreed(what, run)
        finally:
            if rng:
                torch.cuda.nvtx.range_pop()
        return GaussianMixtureModel(weights, means, covs, column, self._predictionCol, self._probabilityCol, summary)


def _accessors(cls, name: str):
    cap = name[0].upper() + name[1:]

    def setter(self, value):
        return self._set(name, value)

    def getter(self):
        return getattr(self, "_" + name)
    setter.__name__, getter.__name__ = "set" + cap, "get" + cap
    setter.__doc__ = f"Sets `{name}` and returns the estimator, as pyspark's setter does."
    getter.__doc__ = f"The value of `{name}`."
    setattr(cls, "set" + cap, setter)
    setattr(cls, "get" + cap, getter)


for _p in _PARAMS:
    _accessors(KMeans, _p)
for _p in _GMM_PARAMS:
    _accessors(GaussianMixture, _p)
