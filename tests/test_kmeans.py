"""`ml.clustering.KMeans` on the host path (tensorframes_amd/ml/clustering.py):
records per partition in numpy float64, added in partition order.

The reference and the bound of a distance are in tests/kmeans_cases.py. An
element of a cluster's sum of x' is held to terms * 2^-52 * sum |x'_rf| with
  the rows of the cluster added in a partition                       rows of the largest partition
  the rounded subtraction of the shift                               1
  one addition per partition and iteration                           nparts * iterations"""
import numpy as np
import pytest

import tensorframes_amd as tfs
from tensorframes_amd import core
from tensorframes_amd.ml import clustering
from tensorframes_amd.ml.clustering import KMeans

from kmeans_cases import EPS, check_fit, data, reference, rows_as_centres
from vector_moments_cases import SIZES, far_apart, frame_of

Y = data(np.float32, sum(SIZES), 17)
INIT = rows_as_centres(Y, 4)
TERMS = max(SIZES) + 1 + 3 * len(SIZES)


def test_three_partitions_on_the_host():
    check_fit(frame_of(Y, SIZES), Y, INIT, 3, TERMS)


def test_two_partitionings_agree():
    a = check_fit(frame_of(Y, SIZES), Y, INIT, 3, TERMS)
    b = check_fit(frame_of(Y, [35, 35]), Y, INIT, 3, 35 + 1 + 3 * 2)
    ref = reference(Y, np.array(a.clusterCenters()))
    tol = (TERMS + 35 + 1 + 3 * 2 + 4) * EPS * (ref.sums_mag / np.maximum(ref.counts, 1)[:, None] + np.abs(Y).max())
    assert (np.abs(np.array(a.clusterCenters()) - np.array(b.clusterCenters())) <= tol).all()


def test_seeded_start_and_equal_bits():
    df = frame_of(Y, SIZES)
    start = clustering._random_start(df, df.local_blocks(), "y", 4, 17, 3, "t")
    assert (start == Y[np.sort(np.random.default_rng(3).choice(len(Y), 4, replace=False))]).all()
    a, b = [KMeans(featuresCol="y", k=4, seed=3).fit(df) for _ in range(2)]
    assert (np.array(a.clusterCenters()) == np.array(b.clusterCenters())).all()
    assert a.summary.trainingCost == b.summary.trainingCost and a.hasSummary


def test_blobs_converge_and_an_empty_cluster_keeps_its_centre():
    y = far_apart(SIZES, 5, np.float64)  # blobs of 5 and 65 rows, 1e3 apart
    init = np.stack([y[0], y[-1], np.full(5, 1e6)])
    model = KMeans(featuresCol="y", k=3, maxIter=20).setInitialCenters(init).fit(frame_of(y, SIZES))
    s = model.summary
    assert s.numIter == 2 and s.k == 3 and s.clusterSizes == [5, 65, 0]
    got = np.array(model.clusterCenters())
    assert (got[2] == init[2]).all()
    assert np.allclose(got[0], y[:5].mean(0), rtol=0, atol=1e-9) and np.allclose(got[1], y[5:].mean(0), rtol=0, atol=1e-9)


def test_training_cost_is_that_of_the_centres_the_last_iteration_started_from():
    s = KMeans(featuresCol="y", k=4, maxIter=1).setInitialCenters(INIT).fit(frame_of(Y, SIZES)).summary
    ref = reference(Y, INIT)
    assert abs(s.trainingCost - ref.dist.sum()) <= (17 + 8 + len(Y)) * EPS * ref.mag.sum()
    assert s.clusterSizes == list(ref.counts) and s.numIter == 1


def test_predict_equals_transform_and_a_bad_row_gets_minus_one():
    y = Y.copy()
    y[7, 2] = np.inf
    model = KMeans(featuresCol="y", k=4, maxIter=1).setInitialCenters(INIT).fit(frame_of(Y, SIZES))
    out = model.transform(frame_of(y, SIZES))
    pred = out.to_numpy("prediction")
    assert out.columns == ["y", "prediction"] and pred.dtype == np.int32
    assert pred[7] == -1 and (pred == [model.predict(v) for v in y]).all()
    keep = np.arange(len(y)) != 7
    assert (pred[keep] == reference(Y, np.array(model.clusterCenters())).assign[keep]).all()


REFUSALS = [
    (lambda: KMeans(featuresCol="y", k=9).fit(frame_of(Y[:5], [5])), ValueError, "fewer than k"),
    (lambda: KMeans(featuresCol="y", k=2).fit(frame_of(np.where(np.arange(70)[:, None] == 4, np.nan, Y), SIZES)),
     ValueError, "1 rows with a NaN"),
    (lambda: KMeans(featuresCol="y").fit(tfs.from_columns({"y": np.ones(4, dtype=np.float32)}, num_partitions=1)),
     core.InvalidDimensionException, "scalar"),
    (lambda: KMeans(featuresCol="y").fit(tfs.create_dataframe([([1.0, 2.0],), ([3.0],)], schema=["y"])),
     core.InvalidDimensionException, "analyze"),
    (lambda: KMeans(k=1025), ValueError, "1024"),
    (lambda: KMeans(featuresCol="y").fit(tfs.from_columns({"y": np.ones((2, 2049), dtype=np.float32)})),
     ValueError, "2048"),
    (lambda: KMeans(featuresCol="y", k=200).fit(tfs.from_columns({"y": np.ones((2, 2048), dtype=np.float32)})),
     ValueError, "262144"),
    (lambda: KMeans(initMode="k-means||"), NotImplementedError, "'random'"),
    (lambda: KMeans(distanceMeasure="cosine"), NotImplementedError, "'euclidean'"),
    (lambda: KMeans().setWeightCol("w"), NotImplementedError, "weightCol=None"),
]


@pytest.mark.parametrize("call,exc,word", REFUSALS, ids=[r[2] for r in REFUSALS])
def test_refusals(call, exc, word):
    with pytest.raises(exc, match=word):
        call()
