"""Counterparts of `pyspark.ml`: `tensorframes_amd.ml.stat.Correlation` and `tensorframes_amd.ml.stat.Summarizer`."""
