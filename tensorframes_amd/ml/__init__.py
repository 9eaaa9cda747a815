"""Counterparts of `pyspark.ml`: `tensorframes_amd.ml.stat.Correlation`, `tensorframes_amd.ml.stat.Summarizer`,
`tensorframes_amd.ml.clustering.KMeans`, `tensorframes_amd.ml.clustering.GaussianMixture` and
`tensorframes_amd.ml.classification.LogisticRegression`."""
from . import classification, clustering, stat  # noqa: F401
