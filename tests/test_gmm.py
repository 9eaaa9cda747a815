"""`ml.clustering.GaussianMixture` on the host path (tensorframes_amd/ml/clustering.py):
records per partition in numpy float64, added in partition order.

The reference and the bounds are in tests/gmm_cases.py. numpy adds the rows of
a partition in an order of its own: at most rows - 1 additions that are not
additions of an exact zero, so `terms` is the rows of the largest partition,
plus one addition per partition; exp and log of the host are within the 2 ulp
allowed there."""
import numpy as np
import pytest

import tensorframes_amd as tfs
from tensorframes_amd.ml import clustering
from tensorframes_amd.ml.clustering import GaussianMixture

from gmm_cases import case, check_fit, check_step, data, mixture
from vector_moments_cases import SIZES, frame_of

Y = data(np.float32, sum(SIZES), 5)
INIT = mixture(Y, 3)
TERMS = max(SIZES) + len(SIZES)


@pytest.mark.parametrize("dtype,d,n,k", [(np.float32, 1, 1, 1), (np.float64, 3, 2, 2), (np.float32, 17, 33, 5)])
def test_host_step_against_reference(dtype, d, n, k):
    x, params, ref = case(dtype, d, n, k)
    check_step(clustering._host_em_step(x, *params), ref, n)
    r, _, ok = clustering._host_estep(x, *params)
    assert ok.all() and (np.abs(r - ref.r) <= ref.b_r).all() and (r.argmax(1) == ref.pred).all()


def test_three_partitions_on_the_host():
    model, _, _ = check_fit(frame_of(Y, SIZES), Y, INIT, 3, TERMS)
    out = model.transform(frame_of(Y, SIZES))
    assert out.columns == ["y", "probability", "prediction"] and out.to_numpy("prediction").dtype == np.int32
    assert (out.to_numpy("prediction") == [model.predict(v) for v in Y]).all()
    assert (out.to_numpy("probability")[4] == model.predictProbability(Y[4])).all()
    assert model.gaussiansDF.to_numpy("cov").shape == (3, 5, 5) and model.hasSummary


def test_loglik_does_not_decrease():
    """EM never lowers the log-likelihood; each of two values is off by at most its own bound."""
    lls = check_fit(frame_of(Y, SIZES), Y, INIT, 5, TERMS)[2]
    assert all(b + tb >= a - ta for (a, ta), (b, tb) in zip(lls, lls[1:])) and lls[-1][0] > lls[0][0]


def test_seeded_start_gives_the_same_model_twice():
    a, b = [GaussianMixture(featuresCol="y", k=2, seed=3, maxIter=4).fit(frame_of(Y, SIZES)) for _ in range(2)]
    assert a.weights == b.weights and a.summary.logLikelihood == b.summary.logLikelihood
    assert all((g.mean == h.mean).all() and (g.cov == h.cov).all() for g, h in zip(a.gaussians, b.gaussians))


REFUSALS = [
    (lambda: GaussianMixture().setWeightCol("w"), NotImplementedError, "weightCol=None"),
    (lambda: GaussianMixture(k=65), ValueError, "64"),
    (lambda: GaussianMixture(featuresCol="y").fit(tfs.from_columns({"y": np.ones((2, 129), dtype=np.float32)})),
     ValueError, "128"),
    (lambda: GaussianMixture(featuresCol="y", k=17).fit(tfs.from_columns({"y": np.ones((2, 128), dtype=np.float32)})),
     ValueError, "262144"),
    (lambda: GaussianMixture(featuresCol="y", k=3).setInitialModel(*INIT).fit(
        frame_of(np.where(np.arange(70)[:, None] == 4, np.nan, Y), SIZES)), ValueError, "1 rows with a NaN"),
    (lambda: GaussianMixture(featuresCol="y", k=1, seed=0).fit(frame_of(np.ones((2, 3), dtype=np.float32), [2])),
     ValueError, "component 0 of the start is not positive definite"),
    (lambda: GaussianMixture().setInitialModel(INIT[0], INIT[1], INIT[2][:2]), ValueError, r"covs \[k, d, d\]"),
    (lambda: GaussianMixture(featuresCol="y", k=2).setInitialModel(*INIT).fit(frame_of(Y, SIZES)),
     ValueError, "initial means"),
]


@pytest.mark.parametrize("call,exc,word", REFUSALS, ids=[r[2] for r in REFUSALS])
def test_refusals(call, exc, word):
    with pytest.raises(exc, match=word):
        call()
