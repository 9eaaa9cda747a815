"""`LogisticRegression` / `LogisticRegressionModel`
(`pyspark.ml.classification.LogisticRegression`): binomial and multinomial
logistic regression with an L2 penalty over a dense vector column.

One objective evaluation reduces every partition on its own to one float64
record (grad [R, d + 1], loss, wsum, bad [3]): device-resident partitions
through `_C.logreg_step` (kernels/logreg.hip: the margins of a stripe of rows
in f64 MFMA accumulators, a safe softmax / softplus row epilogue, the gradient
q^T [x, 1] as a dense GEMM over row slices, folds in a fixed order), host
partitions through numpy with the same expressions. The records travel as one
zero-filled [nparts, R (d + 1) + 5] table (one host all-reduce per evaluation;
every rank fills the rows of its own partitions) and every rank adds them in
ascending partition order: for a given partitioning the same bits on every
rank and for every world size, so the optimiser (L-BFGS in numpy, a pure
function of those bits) takes the same branches everywhere.

The unknown is u = beta * sigma, sigma the weighted sample standard deviation
of a feature (the Summarizer record); the kernel is handed beta = u / sigma and
the chain rule is applied on the host. The objective is loss / wsum + regParam
/ 2 * P with P = sum u^2 (`standardization`) or sum (u / sigma)^2; intercepts
are never penalised. A feature with sigma == 0 keeps the coefficient 0.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from ..frame.block import Block
from ..frame.types import StructType
from ..parallel import dist
from . import stat
from .clustering import _column

MAX_CLASSES, MAX_FEATURES, MAX_CELLS = 128, 4096, 262144  # kernels.h: kLogRegMaxK, kLogRegMaxD, kLogRegMaxRD
_HISTORY, _ARMIJO, _MAX_HALVINGS = 10, 1e-4, 40


def _host_margins(x: np.ndarray, coef: np.ndarray, icpt: np.ndarray):
    """(rows without a NaN or an infinity, margins [those rows, R]) of x [n, d]."""
    x = x.astype(np.float64)
    ok = np.isfinite(x).all(1)
    return ok, x[ok], x[ok] @ coef.T + icpt


def _softmax(m: np.ndarray):
    """(M, S, p) of the margins [n, R]: the safe form of `lr_forward`."""
    M = m.max(1)
    e = np.exp(m - M[:, None])
    S = e.sum(1)
    return M, S, e / S[:, None]


def _sigmoid(m: np.ndarray):
    """(exp(-|m|), sigma(m)) without overflow for any m."""
    e = np.exp(-np.abs(m))
    return e, np.where(m >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _host_eval(x: np.ndarray, y: np.ndarray, w, coef: np.ndarray, icpt: np.ndarray, binomial: bool):
    """The record (loss, grad [R, d + 1], wsum, bad [3]) of the rows x [n, d] (the contract of `_C.logreg_step`)."""
    k = 2 if binomial else coef.shape[0]
    with np.errstate(all="ignore"):
        y = y.astype(np.float64)
        w = np.ones(x.shape[0]) if w is None else w.astype(np.float64)
        okx, xs, m = _host_margins(x, coef, icpt)
        oky = (y >= 0) & (y < k) & (y == np.floor(y))
        okw = (w >= 0) & np.isfinite(w)
        bad = [int((~okx).sum()), int((okx & ~oky).sum()), int((okx & oky & ~okw).sum())]
        use = (oky & okw)[okx]
        xs, m, y, w = xs[use], m[use], y[okx][use], w[okx][use]
        if binomial:
            m = m[:, 0]
            e, sig = _sigmoid(m)
            loss = w * ((np.maximum(m, 0.0) + np.log1p(e)) - y * m)
            q = (w * (sig - y))[:, None]
        else:
            M, S, p = _softmax(m)
            yi = y.astype(np.int64)
            loss = w * ((M + np.log(S)) - m[np.arange(len(yi)), yi])
            p[np.arange(len(yi)), yi] -= 1.0
            q = w[:, None] * p
        live = w != 0  # (a row of weight 0 contributes exact zeros)
        grad = q[live].T @ np.concatenate([xs[live], np.ones((int(live.sum()), 1))], 1)
    return float(loss[live].sum()), grad, float(w.sum()), bad


def _host_predict(x: np.ndarray, coef: np.ndarray, icpt: np.ndarray, binomial: bool, threshold: float):
    """(pred int32 [n], raw [n, K], prob [n, K]) of x [n, d] (the contract of `_C.logreg_predict`)."""
    n, k = x.shape[0], 2 if binomial else coef.shape[0]
    pred, raw, prob = np.full(n, -1, dtype=np.int32), np.zeros((n, k)), np.zeros((n, k))
    with np.errstate(all="ignore"):
        ok, _, m = _host_margins(x, coef, icpt)
        if binomial:
            m = m[:, 0]
            _, sig = _sigmoid(m)
            raw[ok], prob[ok] = np.stack([-m, m], 1), np.stack([_sigmoid(-m)[1], sig], 1)
            pred[ok] = m > np.log(np.float64(threshold) / (1.0 - np.float64(threshold)))
        elif m.shape[0]:
            raw[ok], prob[ok] = m, _softmax(m)[2]
            pred[ok] = prob[ok].argmax(1)  # (the first of equal ones)
    return pred, raw, prob


def _evaluate(df, blocks: Dict[int, Block], features: str, label: str, weight, coef: np.ndarray, icpt: np.ndarray,
              binomial: bool, what: str):
    """(loss, grad [R, d + 1], wsum) over all ranks at (coef, icpt) (collective); a left-out row is a ValueError."""
    from .. import engine
    from .._native import _C
    from ..frame._scalar_columns import _scalar_column
    from ..utils.logging import metrics
    r, d = coef.shape
    cells = r * (d + 1)
    table = torch.zeros((df.num_partitions, cells + 5), dtype=torch.float64)
    dev = {}  # the coefficients per device
    for pid in sorted(blocks):
        b = blocks[pid]
        if not b.nrows:
            continue
        c = _column(b, pid, features, d, what)
        y = _scalar_column(b, label, what)
        w = None if weight is None else _scalar_column(b, weight, what)
        if c.is_cuda and engine.gpu_available():
            if c.device not in dev:
                dev[c.device] = (torch.from_numpy(coef).to(c.device), torch.from_numpy(icpt).to(c.device))
            loss, grad, wsum, bad = _C.logreg_step(c.contiguous(), y.to(c.device).contiguous(),
                                                   None if w is None else w.to(c.device).contiguous(),
                                                   dev[c.device][0], dev[c.device][1], binomial)
            table[pid] = torch.cat([grad.reshape(-1), loss, wsum, bad.double()]).cpu()  # (the one D2H)
            metrics.add("logreg_device_partitions")
        else:
            loss, grad, wsum, bad = _host_eval(c.detach().cpu().numpy(), y.detach().cpu().numpy(),
                                               None if w is None else w.detach().cpu().numpy(), coef, icpt, binomial)
            table[pid] = torch.from_numpy(np.concatenate([grad.reshape(-1), [loss, wsum], bad]))
            metrics.add("logreg_host_partitions")
    dist.all_reduce_host_(table, "Sum")  # (every rank fills the rows of its own partitions; the others are zero)
    acc = np.zeros(cells + 5)
    for row in table.numpy():  # (partition order: the same on every rank)
        acc = acc + row
    metrics.add("logreg_evaluations")
    for count, column, why in zip(acc[cells + 2:], (features, label, weight),
                                  ("rows with a NaN or an infinity",
                                   "labels that are not an integer in [0, numClasses)",
                                   "negative, NaN or infinite weights")):
        if count:
            raise ValueError(f"{what}: '{column}' holds {int(count)} {why}")
    if not acc[cells + 1] > 0:
        raise ValueError(f"{what}: the frame has no row of positive weight")
    return float(acc[cells]), acc[:cells].reshape(r, d + 1), float(acc[cells + 1])


def _lbfgs(fun, theta: np.ndarray, max_iter: int, tol: float):
    """L-BFGS (history 10) with a backtracking Armijo search on fun(theta) -> (f, g): (theta, [f per iteration, the
    start included], iterations). A trial point is taken when f_new <= f + 1e-4 t g.p and s.y > 0; the loop ends when
    ||g||_inf <= tol max(1, |f|), at max_iter, or when no trial point is taken."""
    f, g = fun(theta)
    hist, ss, ys, it = [f], [], [], 0
    while it < max_iter and np.abs(g).max(initial=0.0) > tol * max(1.0, abs(f)):
        p, alpha = -g, []
        for s, y in zip(reversed(ss), reversed(ys)):  # (the two-loop recursion)
            alpha.append(s.dot(p) / s.dot(y))
            p = p - alpha[-1] * y
        if ss:
            p = p * (ss[-1].dot(ys[-1]) / ys[-1].dot(ys[-1]))
        for (s, y), a in zip(zip(ss, ys), reversed(alpha)):
            p = p + (a - y.dot(p) / s.dot(y)) * s
        slope = g.dot(p)
        if not slope < 0:
            p, slope, ss, ys = -g, -g.dot(g), [], []
        t = 1.0 if ss else 1.0 / max(1.0, float(np.sqrt(g.dot(g))))
        for _ in range(_MAX_HALVINGS):
            f_new, g_new = fun(theta + t * p)
            if f_new <= f + _ARMIJO * t * slope and (t * p).dot(g_new - g) > 0:
                break
            t *= 0.5
        else:
            break
        ss, ys = (ss + [t * p])[-_HISTORY:], (ys + [g_new - g])[-_HISTORY:]
        theta, f, g, it = theta + t * p, f_new, g_new, it + 1
        hist.append(f)
    return theta, hist, it


class LogisticRegressionTrainingSummary:
    """`objectiveHistory` (the objective at the start and after every iteration) and `totalIterations`."""

    def __init__(self, objective_history: List[float], total_iterations: int):
        self.objectiveHistory = objective_history  # noqa: N815
        self.totalIterations = total_iterations  # noqa: N815


class LogisticRegressionModel:
    """The fitted coefficients. `transform` is lazy and works partition by
    partition: device-resident partitions through `_C.logreg_predict` (the
    columns stay on the device), host partitions through numpy. A row that
    holds a NaN or an infinity is predicted -1 with zero raw prediction and
    probability (Spark gives it NaN probabilities and a class)."""

    def __init__(self, coefficient_matrix: np.ndarray, intercept_vector: np.ndarray, binomial: bool, params: dict,
                 summary: Optional[LogisticRegressionTrainingSummary] = None):
        self._coef = np.ascontiguousarray(coefficient_matrix, dtype=np.float64)
        self._icpt = np.ascontiguousarray(intercept_vector, dtype=np.float64)
        self._binomial, self._params, self._summary = binomial, dict(params), summary

    @property
    def coefficientMatrix(self) -> np.ndarray:  # noqa: N802
        """[R, d]: one row in a binomial model, one per class in a multinomial one."""
        return self._coef.copy()

    @property
    def interceptVector(self) -> np.ndarray:  # noqa: N802
        return self._icpt.copy()

    @property
    def coefficients(self) -> np.ndarray:
        if not self._binomial:
            raise RuntimeError("LogisticRegressionModel.coefficients: a multinomial model has a coefficientMatrix")
        return self._coef[0].copy()

    @property
    def intercept(self) -> float:
        if not self._binomial:
            raise RuntimeError("LogisticRegressionModel.intercept: a multinomial model has an interceptVector")
        return float(self._icpt[0])

    @property
    def numClasses(self) -> int:  # noqa: N802
        return 2 if self._binomial else self._coef.shape[0]

    @property
    def numFeatures(self) -> int:  # noqa: N802
        return self._coef.shape[1]

    @property
    def hasSummary(self) -> bool:  # noqa: N802
        return self._summary is not None

    @property
    def summary(self) -> LogisticRegressionTrainingSummary:
        if self._summary is None:
            raise RuntimeError("LogisticRegressionModel.summary: this model has no training summary")
        return self._summary

    def _host(self, vector):
        v = np.asarray(vector, dtype=np.float64).reshape(1, -1)
        if v.shape[1] != self.numFeatures:
            raise ValueError(f"LogisticRegressionModel.predict: a vector of {self.numFeatures} components is expected, "
                             f"got {v.shape[1]}")
        return _host_predict(v, self._coef, self._icpt, self._binomial, self._params["threshold"])

    def predict(self, vector) -> float:
        """The class of one vector [d], on the host; -1.0 with a NaN or an infinity."""
        return float(self._host(vector)[0][0])

    def predictRaw(self, vector) -> np.ndarray:  # noqa: N802
        """The margins [K] of one vector (binomial: [-m, m]), on the host; zeros with a NaN or an infinity."""
        return self._host(vector)[1][0]

    def predictProbability(self, vector) -> np.ndarray:  # noqa: N802
        """The class probabilities [K] of one vector, on the host; zeros with a NaN or an infinity."""
        return self._host(vector)[2][0]

    def transform(self, df):
        """`df` with `rawPredictionCol` (double[K]), `probabilityCol` (double[K]) and `predictionCol` (float64)
        appended. Lazy and partition-local."""
        from .. import engine
        from .._native import _C
        from ..frame.dataframe import DataFrame, _Derived, tensor_field
        what = "LogisticRegressionModel.transform"
        column, coef, icpt, binomial = self._params["featuresCol"], self._coef, self._icpt, self._binomial
        threshold, k = self._params["threshold"], self.numClasses
        names = [self._params[p] for p in ("rawPredictionCol", "probabilityCol", "predictionCol")]
        d = stat._vector_column(df, column, what, MAX_FEATURES)
        if d != coef.shape[1]:
            raise ValueError(f"{what}: '{column}' has cells of {d} components, the model {coef.shape[1]} features")
        for i, name in enumerate(names):
            if name in df.schema or name in names[:i]:
                raise ValueError(f"{what}: the frame already has a column '{name}'; choose another output column name")

        def compute(blocks):
            out, dev = {}, {}  # (the coefficients per device, uploaded once)
            for pid, b in blocks.items():
                c = _column(b, pid, column, d, what) if b.nrows else b.columns.get(column)
                on_device = isinstance(c, torch.Tensor) and c.is_cuda and engine.gpu_available()
                if not b.nrows:  # (empty columns on the device of the partition's features)
                    where = c.device if on_device else torch.device("cpu")
                    pred, raw, prob = torch.empty(0, dtype=torch.float64, device=where), \
                        torch.empty((0, k), dtype=torch.float64, device=where), \
                        torch.empty((0, k), dtype=torch.float64, device=where)
                elif on_device:
                    if c.device not in dev:
                        dev[c.device] = (torch.from_numpy(coef).to(c.device), torch.from_numpy(icpt).to(c.device))
                    pred, raw, prob = _C.logreg_predict(c.contiguous(), *dev[c.device], binomial, threshold)
                    pred = pred.double()
                else:
                    pred, raw, prob = [torch.from_numpy(a) for a in
                                       _host_predict(c.detach().cpu().numpy(), coef, icpt, binomial, threshold)]
                    pred = pred.double()
                out[pid] = Block(b.nrows, {**b.columns, names[0]: raw, names[1]: prob, names[2]: pred})
            return out
        schema = StructType(list(df.schema.fields) + [tensor_field(names[0], torch.float64, [k]),
                                                      tensor_field(names[1], torch.float64, [k]),
                                                      tensor_field(names[2], torch.float64, [])])
        return DataFrame(schema, _Derived(df, compute), df.num_partitions)


_PARAMS = ("featuresCol", "labelCol", "predictionCol", "probabilityCol", "rawPredictionCol", "maxIter", "regParam",
           "elasticNetParam", "tol", "fitIntercept", "threshold", "standardization", "weightCol", "family")
_REFUSED = ("thresholds", "aggregationDepth", "lowerBoundsOnCoefficients", "upperBoundsOnCoefficients",
            "lowerBoundsOnIntercepts", "upperBoundsOnIntercepts")


class LogisticRegression:
    """`pyspark.ml.classification.LogisticRegression` for a dense vector column
    of float32 or float64 cells `[d]`, a numeric label column with the classes
    0 .. K - 1 and an optional numeric weight column: 1 <= d <= 4096, K <= 128,
    R d <= 262144 (R = 1 binomial, R = K multinomial), an L2 penalty
    (`elasticNetParam=0`), no bounds, no per-class `thresholds`. `fit` is
    collective; a row with a NaN or an infinity, a label outside the classes
    or a negative, NaN or infinite weight is a ValueError."""

    def __init__(self, featuresCol="features", labelCol="label", predictionCol="prediction",  # noqa: N803
                 probabilityCol="probability", rawPredictionCol="rawPrediction", maxIter=100, regParam=0.0,
                 elasticNetParam=0.0, tol=1e-6, fitIntercept=True, threshold=0.5, standardization=True,
                 weightCol=None, family="auto"):
        for p in _PARAMS:
            getattr(self, "set" + p[0].upper() + p[1:])(locals()[p])

    def _set(self, name: str, v):
        what = f"LogisticRegression.set{name[0].upper()}{name[1:]}"
        if name in _REFUSED:
            raise NotImplementedError(f"{what}: {name} is not implemented")
        if name.endswith("Col") and not (isinstance(v, str) and v) and not (name == "weightCol" and v is None):
            raise TypeError(f"{what}: a non-empty column name is expected, got {v!r}")
        if name == "maxIter" and (isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0):
            raise ValueError(f"{what}: a non-negative int is expected, got {v!r}")
        if name in ("regParam", "tol", "elasticNetParam", "threshold") and \
                (isinstance(v, bool) or not isinstance(v, (int, float)) or not v >= 0):
            raise ValueError(f"{what}: a number >= 0 is expected, got {v!r}")
        if name == "elasticNetParam" and v != 0:
            raise NotImplementedError(f"{what}: the L1 part of the elastic net is not implemented; only "
                                      f"elasticNetParam=0 is")
        if name == "threshold" and v > 1:
            raise ValueError(f"{what}: a threshold in [0, 1] is expected, got {v!r}")
        if name in ("fitIntercept", "standardization") and not isinstance(v, bool):
            raise TypeError(f"{what}: a bool is expected, got {v!r}")
        if name == "family" and v not in ("auto", "binomial", "multinomial"):
            raise ValueError(f"{what}: 'auto', 'binomial' or 'multinomial' is expected, got {v!r}")
        setattr(self, "_" + name, v)
        return self

    def fit(self, df) -> LogisticRegressionModel:
        """L-BFGS from zero coefficients (and the intercepts of the class priors) until ||gradient||_inf <= tol
        max(1, |objective|) or `maxIter` (collective)."""
        from .. import functions as F
        from ..frame._scalar_columns import _ineligible
        from ..utils.logging import metrics
        what = "LogisticRegression.fit"
        features, label, weight = self._featuresCol, self._labelCol, self._weightCol
        d = stat._vector_column(df, features, what, MAX_FEATURES)
        for name in (label,) if weight is None else (label, weight):
            if name not in df.schema:
                raise ValueError(f"{what}: Column {name} not found in {df.columns}")
            err = _ineligible(df, name, what)
            if err is not None:
                raise err
        top = float(df.agg(F.max(label)).to_numpy(f"max({label})")[0])
        if not (top >= 0 and top == np.floor(top)):
            raise ValueError(f"{what}: '{label}' must hold the classes 0 .. K - 1, its largest value is {top}")
        k = int(top) + 1
        if k > MAX_CLASSES:
            raise ValueError(f"{what}: '{label}' has {k} classes; up to {MAX_CLASSES} are supported")
        if self._family == "binomial" and k > 2:
            raise ValueError(f"{what}: family='binomial' with {k} classes in '{label}'")
        binomial = self._family == "binomial" or (self._family == "auto" and k <= 2)
        r = 1 if binomial else max(k, 2)
        if r * d > MAX_CELLS:
            raise ValueError(f"{what}: R d = {r} x {d} coefficients; up to {MAX_CELLS} are supported")
        reg, fit_icpt = float(self._regParam), self._fitIntercept

        def run():
            blocks = df._blocks()
            count, q, acc = stat._summary(df, blocks, features, weight, d, ("std",), what)
            sigma = stat._metric("std", count, q, acc, d).numpy().reshape(d)
            active = sigma > 0  # (a constant feature keeps u = 0, as Spark)
            inv = np.where(active, 1.0 / np.where(active, sigma, 1.0), 0.0)
            scale = np.ones(d) if self._standardization else inv * inv  # (d P / d u = 2 scale u)
            na = int(active.sum())

            def split(theta):
                u = np.zeros((r, d))
                u[:, active] = theta[:r * na].reshape(r, na)
                return u, theta[r * na:] if fit_icpt else np.zeros(r)

            def fun(theta):
                u, b = split(theta)
                loss, grad, wsum = _evaluate(df, blocks, features, label, weight, u * inv, b, binomial, what)
                f = loss / wsum + 0.5 * reg * float((scale * u * u).sum())
                g = grad[:, :d] / wsum * inv + reg * scale * u
                return f, np.concatenate([g[:, active].reshape(-1), grad[:, d] / wsum if fit_icpt else []])

            theta = np.zeros(r * na + (r if fit_icpt else 0))
            if fit_icpt:  # the class weights from the intercepts' gradient at zero: sum w (1 / K - [y == c])
                _, grad, wsum = _evaluate(df, blocks, features, label, weight, np.zeros((r, d)), np.zeros(r),
                                          binomial, what)
                if binomial:
                    ones = 0.5 * wsum - grad[0, d]
                    prior = np.array([np.log(ones / (wsum - ones))]) if 0 < ones < wsum else np.zeros(1)
                else:
                    logs = np.log(np.maximum(wsum / r - grad[:, d], 0.0)) if (wsum / r - grad[:, d] > 0).all() else \
                        np.zeros(r)
                    prior = logs - logs.mean()
                theta[r * na:] = prior
            theta, history, iters = _lbfgs(fun, theta, self._maxIter, float(self._tol))
            metrics.add("logreg_iterations", iters)
            u, b = split(theta)
            if fit_icpt and not binomial:
                b = b - b.mean()  # (the softmax does not see a common shift; Spark centres them too)
            return u * inv, np.asarray(b, dtype=np.float64), LogisticRegressionTrainingSummary(history, iters)
        rng = torch.cuda.is_initialized()
        if rng:
            torch.cuda.nvtx.range_push("tfa.logreg")
        try:
            coef, icpt, summary = dist.agreed(what, run)
        finally:
            if rng:
                torch.cuda.nvtx.range_pop()
        return LogisticRegressionModel(coef, icpt, binomial, {p: getattr(self, "_" + p) for p in _PARAMS}, summary)


def _accessors(name: str):
    cap = name[0].upper() + name[1:]

    def setter(self, value):
        return self._set(name, value)

    def getter(self):
        return getattr(self, "_" + name)
    setter.__name__, getter.__name__ = "set" + cap, "get" + cap
    setter.__doc__ = f"Sets `{name}` and returns the estimator, as pyspark's setter does."
    getter.__doc__ = f"The value of `{name}`."
    setattr(LogisticRegression, "set" + cap, setter)
    if name not in _REFUSED:
        setattr(LogisticRegression, "get" + cap, getter)


for _p in _PARAMS + _REFUSED:
    _accessors(_p)
