"""Counterparts of `pyspark.ml`: `tensorframes_amd.ml.stat.Correlation`."""
