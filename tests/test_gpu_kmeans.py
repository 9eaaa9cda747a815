"""`_C.kmeans_step` / `_C.kmeans_assign` (csrc/kernels/kmeans.hip) and the device
path of `ml.clustering.KMeans`, on the GPU.

The reference and the bound of a distance are in tests/kmeans_cases.py. An
element of `sums` is held to terms * 2^-52 * sum over the cluster's rows of
|x'_rf|; the terms follow the kernel as built:
  the rows one MFMA accumulator adds in sequence in a slice          min(slice_rows, n)
  the slice partials folded in slice order                           slices
  the rounded subtraction of the shift                               1
  frame level: one addition per partition and iteration              nparts * iterations
The default slice is 256 rows or more, so every default-sliced case here is one
slice of n rows. `cost` adds n distances (64 of a block in row order, a lane's
blocks in block order, 64 lanes in lane order: at most n - 1 additions that
are not additions of an exact zero), so it is held to (d + 8 + n) * 2^-52 * sum
M_r. Every shape handed to the binding is valid."""
import numpy as np
import pytest
import torch

from tensorframes_amd._native import _C
from tensorframes_amd.utils.logging import metrics

from kmeans_cases import EPS, check_fit, data, reference, rows_as_centres
from vector_moments_cases import SIZES, frame_of

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]

DEV = "cuda:0"


def check(x_dev, x, centers, slice_rows=None):
    """Both bindings on x_dev against the reference of x."""
    n, d = x.shape
    c_dev = torch.from_numpy(centers).to(DEV)
    counts, sums, cost, bad = [t.cpu().numpy() for t in _C.kmeans_step(x_dev, c_dev, slice_rows=slice_rows)]
    assign, dist = [t.cpu().numpy() for t in _C.kmeans_assign(x_dev, c_dev)]
    ref = reference(x, centers)
    assert assign.dtype == np.int32 and (assign == ref.assign).all()
    assert counts.dtype == np.int64 and (counts == ref.counts).all() and bad[0] == 0
    assert slice_rows is not None or n <= 256
    rows = n if slice_rows is None else min(slice_rows, n)
    assert (np.abs(sums - ref.sums) <= (rows + -(-n // rows) + 1) * EPS * ref.sums_mag).all()
    assert (np.abs(dist - ref.dist) <= (d + 8) * EPS * ref.mag).all()
    assert abs(cost[0] - ref.dist.sum()) <= (d + 8 + n) * EPS * ref.mag.sum()


CASES = [(np.float32, 1, 1, 1, None), (np.float64, 3, 2, 2, None), (np.float32, 4, 15, 3, None),
         (np.float64, 5, 16, 16, None), (np.float32, 31, 17, 17, None), (np.float64, 32, 33, 5, None),
         (np.float32, 33, 65, 18, None), (np.float64, 33, 130, 65, None), (np.float32, 67, 130, 10, 32),
         (np.float64, 67, 70, 64, 32), (np.float32, 200, 64, 7, None), (np.float64, 100, 300, 130, 64)]


@pytest.mark.parametrize("dtype,d,n,k,slice_rows", CASES)
def test_kernel_against_reference(dtype, d, n, k, slice_rows):
    x = data(dtype, n, d)
    check(torch.from_numpy(x).to(DEV), x, rows_as_centres(x, k), slice_rows)


@pytest.mark.parametrize("apart", [2, 64])
def test_ties_go_to_the_smallest_index(apart):
    """Centres [c0, c1, ..., c0, c1] with the duplicates `apart` places on (64: in another centre tile)."""
    x = data(np.float32, 70, 9)
    two = rows_as_centres(x, 2)
    centers = np.concatenate([two, 1e4 + 50 + np.arange((apart - 2) * 9.0).reshape(apart - 2, 9), two])
    assign = _C.kmeans_assign(torch.from_numpy(x).to(DEV), torch.from_numpy(centers).to(DEV))[0].cpu().numpy()
    assert set(assign) <= {0, 1} and (assign == reference(x, two).assign).all()


@pytest.mark.parametrize("d,n,slice_rows", [(17, 33, None), (65, 2 * 32 + 3, 32)])
def test_four_byte_aligned_view(d, n, slice_rows):
    x = data(np.float32, n + 1, d)
    view = torch.from_numpy(x).to(DEV)[1:]  # (odd d: the base is 4-byte aligned, the scalar-load path)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    check(view, x[1:], rows_as_centres(x[1:], 5), slice_rows)


@pytest.mark.parametrize("dtype,d,n", [(np.float32, 33, 50), (np.float64, 130, 40)])
def test_nan_and_infinity_rows_are_left_out(dtype, d, n):
    clean = data(dtype, n, d)
    centers = rows_as_centres(clean, 6)
    x = np.insert(clean, [3, n], 0.0, axis=0)  # two more rows: at 3 and at the end
    x[3, 5], x[n + 1, d - 2] = np.nan, np.inf
    c_dev = torch.from_numpy(centers).to(DEV)
    got = _C.kmeans_step(torch.from_numpy(x).to(DEV), c_dev)
    want = _C.kmeans_step(torch.from_numpy(clean).to(DEV), c_dev)
    for g, w in zip(got[:3], want[:3]):  # (one block, one slice: the same rows added in the same order)
        assert torch.equal(g, w)
    assert got[3].item() == 2 and want[3].item() == 0
    assign, dist = [t.cpu().numpy() for t in _C.kmeans_assign(torch.from_numpy(x).to(DEV), c_dev)]
    keep = np.ones(n + 2, dtype=bool)
    keep[[3, n + 1]] = False
    assert (assign[~keep] == -1).all() and (dist[~keep] == 0.0).all()
    assert (assign[keep] == reference(clean, centers).assign).all()


def test_frame_on_the_device():
    y = data(np.float32, sum(SIZES), 17)
    df = frame_of(y, SIZES).cache_on_device(DEV)
    before = metrics.snapshot().get("kmeans_device_partitions", 0)
    model = check_fit(df, y, rows_as_centres(y, 4), 3, max(SIZES) + 1 + 1 + 3 * len(SIZES))
    assert metrics.snapshot()["kmeans_device_partitions"] - before == 2 * 3  # (the first partition is empty)
    blocks = model.transform(df).local_blocks()
    pred = torch.cat([blocks[p].columns["prediction"] for p in (1, 2)])
    assert pred.is_cuda and pred.dtype == torch.int32
    assert (pred.cpu().numpy() == reference(y, np.array(model.clusterCenters())).assign).all()
