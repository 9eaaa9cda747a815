"""`_C.vector_summary` (csrc/kernels/vector_summary.hip) and the device path of
`Summarizer`, on the GPU.

The reference and the bounds are in tests/vector_summary_cases.py. The terms
follow the kernel as built, with rows per pass = 256 / (the power of two at or
above ceil(min(d, 256) / 4)):
  the rows a thread takes in sequence, three roundings each       3 * ceil(min(slice_rows, n) / rows per pass)
  (the deviation, the factor w / (W + w), the fused update)
  the levels of the lane tree, one merge each (delta, the         5 * log2(rows per pass)
  factor, two products, the sums)
  the slices folded in slice order, one merge each                5 * slices
  the end (the product for sum, the quotient, the root)           4
  frame level: one merge per partition                            5 * nparts
The default slice is 4096 rows or more, so every default-sliced case here is
one slice of n rows. Every shape handed to the binding is valid."""
import numpy as np
import pytest
import torch

from tensorframes_amd._native import _C
from tensorframes_amd.utils.logging import metrics

from vector_moments_cases import SIZES, far_apart, frame_of
from vector_summary_cases import CONST, MERGE, ROW, check, data, frame_metrics, record_metrics, weights

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]

DEV = "cuda:0"


def kernel_terms(n, d, slice_rows=None):
    per_pass = 256 // (1 << (-(-min(d, 256) // 4) - 1).bit_length())
    rows = n if slice_rows is None else min(slice_rows, n)
    return ROW * -(-rows // per_pass) + MERGE * (per_pass.bit_length() - 1) + MERGE * -(-n // rows) + CONST


def summary(x, w=None, slice_rows=None):
    return _C.vector_summary(x, None if w is None else torch.from_numpy(w).to(DEV), slice_rows)


# d: the quad tail (1, 3, 5), a full quad (4), a full group and its edges (255, 256), a second component group (257,
# 260); n: 1, 2, rows per pass - 1 and + 1, a few passes, past the four passes a thread loads ahead (4 * rows per
# pass) and past a tile of 1024 weights; slice_rows: three slices with a ragged last one
CASES = [(np.float32, 1, 1, None), (np.float64, 3, 2, None), (np.float32, 4, 255, None), (np.float64, 1, 257, None),
         (np.float32, 5, 127, None), (np.float64, 5, 129, None), (np.float32, 255, 3, None), (np.float64, 256, 5, None),
         (np.float32, 257, 17, None), (np.float64, 260, 18, None), (np.float32, 5, 1030, None),
         (np.float64, 4, 1100, None), (np.float32, 260, 11, 4), (np.float64, 3, 700, 256), (np.float32, 255, 2500, 1024)]


@pytest.mark.parametrize("dtype,d,n,slice_rows", CASES)
def test_kernel_against_reference(dtype, d, n, slice_rows):
    x = data(dtype, n, d)
    rec = summary(torch.from_numpy(x).to(DEV), None, slice_rows).cpu().numpy()
    assert rec.shape == (4 + 8 * d,) and rec[0] == n and rec[3] == 0
    check(record_metrics(rec, d), x, None, kernel_terms(n, d, slice_rows))


@pytest.mark.parametrize("wdtype", [np.float32, np.float64, np.int32])
@pytest.mark.parametrize("dtype,d,n,slice_rows", [(np.float32, 5, 300, None), (np.float64, 260, 21, 8)])
def test_weighted_with_zero_weights(dtype, d, n, slice_rows, wdtype):
    x, w = data(dtype, n, d), weights(n, wdtype)
    rec = summary(torch.from_numpy(x).to(DEV), w, slice_rows).cpu().numpy()
    check(record_metrics(rec, d), x, w, kernel_terms(n, d, slice_rows))


@pytest.mark.parametrize("d,n,slice_rows", [(5, 131, None), (257, 19, 8)])
def test_four_byte_aligned_view_and_weights_of_ones_give_the_same_bits(d, n, slice_rows):
    x = torch.from_numpy(data(np.float32, n + 1, d)).to(DEV)
    view = x[1:]  # (odd d: the base is 4-byte aligned)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    want = summary(view.clone(), None, slice_rows)
    assert torch.equal(summary(view, None, slice_rows), want)
    assert torch.equal(summary(view.clone(), np.ones(n, dtype=np.float32), slice_rows), want)
    y = torch.from_numpy(data(np.float32, n, 8)).to(DEV)  # (d % 4 == 0: 16-byte loads, scalar loads one element on)
    shifted = torch.cat([y.reshape(-1)[:1], y.reshape(-1)])[1:].reshape(n, 8)
    assert y.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4
    assert torch.equal(summary(y, None, slice_rows), summary(shifted, None, slice_rows))


@pytest.mark.parametrize("dtype,d,n", [(np.float32, 6, 40), (np.float64, 258, 9)])
def test_nan_infinity_and_negative_zero_stay_in_their_components(dtype, d, n):
    clean = data(dtype, n, d)
    x = clean.copy()
    x[3, 1], x[n - 1, d - 2], x[2, 0] = np.nan, np.inf, -0.0
    rec = summary(torch.from_numpy(x).to(DEV)).cpu().numpy()
    got = record_metrics(rec, d)
    check(got, x, None, kernel_terms(n, d), skip=(1, d - 2))
    assert np.isnan(got["normL1"][1]) and np.isnan(got["normL2"][1]) and np.isnan(got["max"][1])
    assert got["normL1"][d - 2] == np.inf and got["normL2"][d - 2] == np.inf and got["max"][d - 2] == np.inf
    assert got["numNonZeros"][0] == n - 1 and got["numNonZeros"][1] == n
    untouched = [j for j in range(d) if j not in (0, 1, d - 2)]
    base = summary(torch.from_numpy(clean).to(DEV)).cpu().numpy()
    assert np.array_equal(rec[4:].reshape(8, d)[:, untouched], base[4:].reshape(8, d)[:, untouched])


def test_bad_weights_are_counted_in_the_header():
    x, w = data(np.float32, 20, 3), np.ones(20)
    w[4], w[11], w[12] = -1.0, np.nan, 0.0
    rec = summary(torch.from_numpy(x).to(DEV), w).cpu().numpy()
    assert rec[0] == 17 and rec[3] == 2


def test_frame_on_the_device():
    y = far_apart(SIZES, 17)
    df = frame_of(y, SIZES).cache_on_device(DEV)
    before = metrics.snapshot().get("vector_summary_device_partitions", 0)
    got = frame_metrics(df)
    assert metrics.snapshot()["vector_summary_device_partitions"] - before == 2  # (the third partition is empty)
    check(got, y, None, kernel_terms(max(SIZES), 17) + MERGE * len(SIZES))
