"""`ml.classification.LogisticRegression` on the host path
(tensorframes_amd/ml/classification.py): records per partition in numpy float64,
added in partition order, L-BFGS on the host.

The reference and the bounds are in tests/logreg_cases.py. numpy adds the n
rows of a partition in an order of its own: an element of grad and the loss are
held to n + 1 terms."""
import numpy as np
import pytest

import tensorframes_amd as tfs
from tensorframes_amd.ml import classification
from tensorframes_amd.ml.classification import LogisticRegression

from logreg_cases import check_eval, check_fit, check_predict, data, frame, reference
from vector_moments_cases import SIZES

RNG = np.random.default_rng(11)
X = np.concatenate([(RNG.standard_normal((sum(SIZES), 4)) * [1, 10, 0.1, 3]), np.ones((sum(SIZES), 1))], 1) \
    .astype(np.float32)  # (unequal scales and a constant feature)
W = RNG.uniform(0.5, 2.0, len(X))
Y = {k: RNG.integers(0, k, len(X)).astype(np.int32) for k in (2, 3)}


def fit(k, **kw):
    df = frame({"features": X, "label": Y[k], "w": W}, SIZES)
    return LogisticRegression(fitIntercept=False, regParam=0.1, weightCol="w", tol=1e-8, **kw).fit(df)


@pytest.mark.parametrize("dtype,d,n,k,weighted", [(np.float32, 1, 1, 0, False), (np.float64, 17, 65, 3, True),
                                                  (np.float32, 33, 70, 128, True), (np.float64, 33, 64, 0, True)])
def test_host_evaluation_against_reference(dtype, d, n, k, weighted):
    x, y, w, coef, icpt = data(dtype, n, d, k, weighted)
    ref = reference(x, y, w, coef, icpt, k == 0)
    check_eval(classification._host_eval(x, y, w, coef, icpt, k == 0), ref, n + 1, n + 1)
    check_predict(classification._host_predict(x, coef, icpt, k == 0, 0.5), ref)


@pytest.mark.parametrize("k", [2, 3])
def test_fit_reaches_the_optimum_of_the_strongly_convex_objective(k):
    model = fit(k)
    check_fit(model, X, Y[k], W, 0.1, 1e-8)
    s = model.summary
    assert model.hasSummary and len(s.objectiveHistory) == s.totalIterations + 1
    assert (np.diff(s.objectiveHistory) <= 0).all()
    assert (model.coefficientMatrix[:, 4] == 0.0).all()  # (the constant feature)
    assert model.numClasses == k and model.numFeatures == 5 and model.coefficientMatrix.shape == (k - (k == 2), 5)


def test_standardization_false_penalises_the_coefficients_themselves():
    a, b = fit(2), fit(2, standardization=False)
    check_fit(b, X, Y[2], W, 0.1, 1e-8, standardization=False)
    assert np.abs(a.coefficients - b.coefficients).max() > 1e-3


def test_intercepts_transform_and_threshold():
    df = frame({"features": X, "label": Y[2], "w": W}, SIZES)
    model = LogisticRegression(maxIter=30).fit(df)
    out = model.transform(df)
    assert out.columns == ["features", "label", "w", "rawPrediction", "probability", "prediction"]
    prob, pred = out.to_numpy("probability"), out.to_numpy("prediction")
    assert pred.dtype == np.float64 and prob.shape == (len(X), 2) and (out.to_numpy("rawPrediction")[:, 0] < 0).any()
    assert (pred == (prob[:, 1] > 0.5)).all() and 0 < pred.sum() < len(X)
    assert pred[3] == model.predict(X[3]) and (prob[3] == model.predictProbability(X[3])).all()
    high = LogisticRegression(maxIter=30, threshold=0.9).fit(df).transform(df)
    assert (high.to_numpy("prediction") == (high.to_numpy("probability")[:, 1] > 0.9)).all()
    with pytest.raises(RuntimeError, match="multinomial"):
        LogisticRegression(maxIter=2, labelCol="label").fit(frame({"features": X, "label": Y[3]}, SIZES)).intercept
    multi = LogisticRegression(maxIter=30).fit(frame({"features": X, "label": Y[3]}, SIZES))
    assert abs(multi.interceptVector.sum()) < 1e-12 and multi.interceptVector.shape == (3,)


def _df(**cols):
    return tfs.from_columns({"features": X[:8], "label": Y[3][:8], **cols}, num_partitions=1)


REFUSALS = [
    (lambda: LogisticRegression(elasticNetParam=0.5), NotImplementedError, "elastic"),
    (lambda: LogisticRegression().setThresholds([0.5, 0.5]), NotImplementedError, "thresholds"),
    (lambda: LogisticRegression().setAggregationDepth(3), NotImplementedError, "aggregationDepth"),
    (lambda: LogisticRegression().setLowerBoundsOnCoefficients(np.zeros((1, 5))), NotImplementedError, "lowerBounds"),
    (lambda: LogisticRegression().setUpperBoundsOnIntercepts(np.zeros(1)), NotImplementedError, "upperBounds"),
    (lambda: LogisticRegression(family="binomial").fit(_df()), ValueError, "binomial"),
    (lambda: LogisticRegression().fit(_df(label=np.arange(8, dtype=np.int32) * 20)), ValueError, "141 classes"),
    (lambda: LogisticRegression().fit(_df(label=np.full(8, 0.5))), ValueError, "largest value"),
    (lambda: LogisticRegression().fit(_df(label=np.array([0, 1, -1, 1, 0, 1, 0, 1]))), ValueError, "'label' holds 1"),
    (lambda: LogisticRegression().fit(_df(features=np.where(np.arange(8)[:, None] == 2, np.nan, X[:8]))), ValueError,
     "'features' holds 1 rows"),
    (lambda: LogisticRegression(weightCol="w").fit(_df(w=-np.ones(8))), ValueError, "'w' holds 8 negative"),
    (lambda: LogisticRegression().fit(_df()).transform(_df(prediction=np.zeros(8))), ValueError, "already has"),
]


@pytest.mark.parametrize("call,exc,word", REFUSALS, ids=[r[2] for r in REFUSALS])
def test_refusals(call, exc, word):
    with pytest.raises(exc, match=word):
        call()
