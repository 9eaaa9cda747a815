"""Counterparts of `pyspark.ml`: `tensorframes_amd.ml.stat.Correlation`, `tensorframes_amd.ml.stat.Summarizer` and
`tensorframes_amd.ml.clustering.KMeans`."""
from . import clustering, stat  # noqa: F401
