"""`Summarizer` on the host path (tensorframes_amd/ml/stat.py): one numpy
record per partition (two passes), Chan's weighted merge in partition order.

The reference and the bounds are in tests/vector_summary_cases.py. The terms
of the host path:
  the products one component adds in a partition, each after its        3 * rows of the largest partition
  own rounded weight product and rounded deviation
  the second pass over the mean                                         2
  one merge per partition (delta, the factor, two products, the sums)   5 * nparts
  the end (the product for sum, the quotient, the root)                 4"""
import numpy as np
import pytest

import tensorframes_amd as tfs
from tensorframes_amd import core
from tensorframes_amd.frame.column_info import ColumnInformation
from tensorframes_amd.ml.stat import METRICS, Summarizer
from tensorframes_amd.utils import dtypes as D

from vector_moments_cases import SIZES, far_apart, frame_of
from vector_summary_cases import CONST, EPS, MERGE, ROW, check, frame_metrics, reference, weights


def host_terms(sizes):
    return ROW * max(sizes) + 2 + MERGE * len(sizes) + CONST


def test_three_partitions_on_the_host():
    y = far_apart(SIZES, 17)
    check(frame_metrics(frame_of(y, SIZES)), y, None, host_terms(SIZES))


def test_weighted_with_zero_weights():
    y, w = far_apart([70], 5, np.float64), weights(70, np.float32)
    df = tfs.from_columns({"y": y, "w": w}, num_partitions=3)
    check(frame_metrics(df, "y", "w"), y, w, host_terms([24, 24, 24]))


def test_two_partitionings_agree():
    y = far_apart(SIZES, 5, np.float64)
    _, tol = reference(y)
    a, b = frame_metrics(frame_of(y, SIZES)), frame_metrics(frame_of(y, [35, 35]))
    terms = host_terms(SIZES) + host_terms([35, 35])
    for m in ("mean", "sum", "variance", "std", "normL1", "normL2"):
        assert (np.abs(a[m] - b[m]) <= terms * EPS * tol[m] + 8 * EPS * np.abs(a[m])).all(), m
    for m in ("count", "numNonZeros", "min", "max"):
        assert np.array_equal(a[m], b[m]), m


def test_names_types_order_alias_and_agg():
    df = tfs.from_columns({"y": far_apart([9], 3), "w": np.ones(9)}, num_partitions=2)
    exprs = [Summarizer.metrics("variance", "count", "max").summary(df["y"], "w"), Summarizer.mean("y").alias("mu")]
    out = df.select(*exprs)
    assert out.columns == ["variance(y)", "count(y)", "max(y)", "mu"] and out.num_partitions == 1
    for name in out.columns:
        stf = ColumnInformation(out.schema[name]).stf
        scalar = name == "count(y)"
        assert stf.tf_dtype == (D.DT_INT64 if scalar else D.DT_DOUBLE)
        assert list(stf.shape.dims) == ([-1] if scalar else [-1, 3])
        assert np.array_equal(out.to_numpy(name), df.agg(exprs).to_numpy(name))
    assert out.to_numpy("count(y)").tolist() == [9] and out.to_numpy("mu").shape == (1, 3)
    assert [getattr(Summarizer, m)("y").output_names for m in METRICS] == [[f"{m}(y)"] for m in METRICS]


def test_one_row_has_variance_zero_and_an_empty_frame_counts_zero():
    one = tfs.from_columns({"y": np.full((1, 2), 3.0, dtype=np.float32)}, num_partitions=1)
    check(frame_metrics(one), np.full((1, 2), 3.0, dtype=np.float32), None, CONST)
    empty = tfs.from_columns({"y": np.ones((0, 2), dtype=np.float32)}, num_partitions=1)
    assert empty.agg(Summarizer.count("y")).to_numpy("count(y)").tolist() == [0]


VEC, W4 = np.ones((4, 3), dtype=np.float32), np.ones(4)
REFUSALS = [
    ({"y": VEC}, lambda df: Summarizer.metrics("mean", "median"), ValueError, "median"),
    ({"y": VEC}, lambda df: Summarizer.metrics("mean", "min", "mean"), ValueError, "repeated"),
    ({"y": VEC}, lambda df: Summarizer.metrics("mean", "min").summary("y").alias("m"), ValueError, "single"),
    ({"y": VEC}, lambda df: df.select(Summarizer.mean("y"), df["y"]), TypeError, "mixed"),
    ({"y": VEC}, lambda df: df.select(Summarizer.mean("y"), Summarizer.mean("y")), ValueError, "duplicate"),
    ({"y": W4}, lambda df: df.select(Summarizer.mean("y")), core.InvalidDimensionException, "scalar"),
    ({"y": VEC.astype(np.int32)}, lambda df: df.agg(Summarizer.mean("y")), core.InvalidTypeException, "int32"),
    ({"y": VEC, "w": VEC}, lambda df: df.select(Summarizer.mean("y", "w")), core.InvalidDimensionException, "rank 1"),
    ({"y": np.ones((1, 65537), dtype=np.float32)}, lambda df: df.select(Summarizer.mean("y")), ValueError, "65536"),
    ({"y": VEC, "w": -W4}, lambda df: df.select(Summarizer.mean("y", "w")).collect(), ValueError, "negative"),
    ({"y": VEC[:0]}, lambda df: df.select(Summarizer.mean("y")).collect(), ValueError, "no row"),
]


@pytest.mark.parametrize("cols,call,exc,word", REFUSALS, ids=[r[3] for r in REFUSALS])
def test_refusals(cols, call, exc, word):
    with pytest.raises(exc, match=word):
        call(tfs.from_columns(cols, num_partitions=1))
