"""`_C.gmm_step` / `_C.gmm_predict` (csrc/kernels/gmm.hip) and the device path of
`ml.clustering.GaussianMixture`, on the GPU.

The reference and the bounds are in tests/gmm_cases.py. The `terms` of N, S and
C follow the kernel as built:
  the rows one MFMA accumulator adds in sequence in a slice          min(slice_rows, n)
  the slice partials folded in slice order                           slices
  frame level: one addition per partition                            nparts
(the roundings of x - mu and of r (x - mu) are added by gmm_cases.tolerances).
The default slice is 256 rows or more, so every default-sliced case here is one
slice of n rows. `loglik` adds n values of lse (64 of a block in row order, a
lane's blocks in block order, 64 lanes in lane order: at most n - 1 additions
that are not additions of an exact zero). exp and log on the device are given
2 ulp each. Every shape handed to the binding is valid."""
import numpy as np
import pytest
import torch

from tensorframes_amd._native import _C
from tensorframes_amd.ml.clustering import _gmm_params
from tensorframes_amd.utils.logging import metrics

from gmm_cases import case, check_fit, check_step, data, mixture, reference
from vector_moments_cases import SIZES, frame_of

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]

DEV = "cuda:0"


def on_device(params):
    return [torch.from_numpy(a).to(DEV) for a in params]


def step(x_dev, params, slice_rows=None):
    N, S, C, loglik, bad = [t.cpu().numpy() for t in _C.gmm_step(x_dev, *on_device(params), slice_rows=slice_rows)]
    return N, S, C, loglik[0], bad[0]


def check(x_dev, params, ref, slice_rows=None):
    """Both bindings on x_dev against the reference of its rows."""
    n = ref.n
    assert slice_rows is not None or n <= 256
    rows = n if slice_rows is None else min(slice_rows, n)
    check_step(step(x_dev, params, slice_rows), ref, rows + -(-n // rows))
    prob, pred = [t.cpu().numpy() for t in _C.gmm_predict(x_dev, *on_device(params))]
    assert prob.dtype == np.float64 and (np.abs(prob - ref.r) <= ref.b_r).all()
    assert pred.dtype == np.int32 and (pred == ref.pred).all()


CASES = [(np.float32, 1, 1, 1, None), (np.float64, 3, 2, 2, None), (np.float32, 4, 15, 3, None),
         (np.float64, 16, 65, 5, None), (np.float32, 17, 33, 17, None), (np.float64, 33, 130, 4, None),
         (np.float32, 64, 67, 64, 32), (np.float64, 65, 70, 3, 32), (np.float64, 128, 130, 16, 64),
         (np.float32, 128, 200, 2, None)]


@pytest.mark.parametrize("dtype,d,n,k,slice_rows", CASES)
def test_kernel_against_reference(dtype, d, n, k, slice_rows):
    x, params, ref = case(dtype, d, n, k)
    check(torch.from_numpy(x).to(DEV), params, ref, slice_rows)


def test_four_byte_aligned_view():
    x = data(np.float32, 33 + 1, 17)
    view = torch.from_numpy(x).to(DEV)[1:]  # (odd d: the base is 4-byte aligned, the scalar-load path)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    weights, means, covs = mixture(x[1:], 5)
    params = (means,) + _gmm_params(weights, covs, "t", 0)
    check(view, params, reference(x[1:], *params))


def test_nan_and_infinity_rows_are_left_out():
    clean, params, ref = case(np.float32, 33, 50, 6)
    x = np.insert(clean, [3, 50], 0.0, axis=0)  # two more rows: at 3 and at the end
    x[3, 5], x[51, 31] = np.nan, np.inf
    got, want = step(torch.from_numpy(x).to(DEV), params), step(torch.from_numpy(clean).to(DEV), params)
    for g, w in zip(got[:4], want[:4]):  # (one block, one slice: the same rows added in the same order)
        assert (np.asarray(g).view(np.int64) == np.asarray(w).view(np.int64)).all()
    assert got[4] == 2 and want[4] == 0
    prob, pred = [t.cpu().numpy() for t in _C.gmm_predict(torch.from_numpy(x).to(DEV), *on_device(params))]
    keep = np.ones(52, dtype=bool)
    keep[[3, 51]] = False
    assert (pred[~keep] == -1).all() and (prob[~keep] == 0.0).all() and (pred[keep] == ref.pred).all()


def test_two_calls_give_equal_bits():
    x, params, _ = case(np.float64, 65, 70, 3)
    x_dev, p_dev = torch.from_numpy(x).to(DEV), on_device(params)
    for a, b in zip(_C.gmm_step(x_dev, *p_dev, slice_rows=32), _C.gmm_step(x_dev, *p_dev, slice_rows=32)):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))


def test_frame_on_the_device():
    y = data(np.float32, sum(SIZES), 5)
    df = frame_of(y, SIZES).cache_on_device(DEV)
    before = metrics.snapshot().get("gmm_device_partitions", 0)
    model, _, _ = check_fit(df, y, mixture(y, 3), 3, max(SIZES) + 1 + len(SIZES))
    assert metrics.snapshot()["gmm_device_partitions"] - before == 2 * (1 + 2 + 3)  # (the first partition is empty)
    blocks = model.transform(df).local_blocks()
    prob = torch.cat([blocks[p].columns["probability"] for p in (1, 2)])
    pred = torch.cat([blocks[p].columns["prediction"] for p in (1, 2)])
    assert prob.is_cuda and prob.dtype == torch.float64 and pred.is_cuda and pred.dtype == torch.int32
    want = reference(y, *model._params)
    assert (pred.cpu().numpy() == want.pred).all() and (np.abs(prob.cpu().numpy() - want.r) <= want.b_r).all()
