"""`_C.logreg_step` / `_C.logreg_predict` (csrc/kernels/logreg.hip) and the device
path of `ml.classification.LogisticRegression`, on the GPU.

The reference and the bounds are in tests/logreg_cases.py. The terms of a sum
follow the kernel as built:
  grad  the rows one MFMA accumulator adds in sequence in a slice    min(slice_rows, n)
        the slice partials folded in slice order                     slices
        the rounded product q x                                      1
  loss  64 rows of a block in row order, a lane's blocks in block
        order, 64 lanes in lane order                                128 + blocks
The default slice is 256 rows wherever (n, d, R) here leave the choice to the
plan (n / 512 is below 256 in every case): one slice of n rows up to n = 256,
18 slices and 71 blocks at n = 4500. Every shape handed to the binding is valid."""
import numpy as np
import pytest
import torch

from tensorframes_amd._native import _C
from tensorframes_amd.ml.classification import LogisticRegression
from tensorframes_amd.utils.logging import metrics

from logreg_cases import EPS, check_eval, check_fit, check_predict, data, frame, reference
from vector_moments_cases import SIZES

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]

DEV = "cuda:0"


def dev(a):
    return None if a is None else torch.from_numpy(a).to(DEV)


def step(x_dev, y, w, coef, icpt, binomial, slice_rows=None):
    return [t.cpu().numpy() for t in _C.logreg_step(x_dev, dev(y), dev(w), dev(coef), dev(icpt), binomial,
                                                    slice_rows=slice_rows)]


def check(x_dev, x, y, w, coef, icpt, binomial, slice_rows=None):
    """Both bindings on x_dev against the reference of x."""
    n = x.shape[0]
    ref = reference(x, y, w, coef, icpt, binomial)
    assert slice_rows is not None or n <= 256 * 512
    rows = min(slice_rows or 256, n)
    check_eval(step(x_dev, y, w, coef, icpt, binomial, slice_rows), ref, rows + -(-n // rows) + 1, 128 + -(-n // 64))
    got = [t.cpu().numpy() for t in _C.logreg_predict(x_dev, dev(coef), dev(icpt), binomial, 0.5)]
    assert got[0].dtype == np.int32
    check_predict(got, ref)


# (dtype, d, n, K (0: binomial), slice_rows, weighted, label dtype)
CASES = [(np.float32, 1, 1, 0, None, False, np.int32), (np.float64, 15, 63, 2, None, True, np.int64),
         (np.float32, 16, 64, 3, None, False, np.float64), (np.float64, 17, 65, 16, None, True, np.int32),
         (np.float32, 33, 130, 17, None, True, np.int64), (np.float64, 65, 64, 64, None, False, np.int32),
         (np.float32, 130, 65, 65, 32, True, np.float64), (np.float64, 33, 70, 128, 32, False, np.int32),
         (np.float32, 130, 130, 0, None, True, np.int64), (np.float64, 64, 67, 0, 32, True, np.float64),
         (np.float32, 128, 130, 33, 64, False, np.int32), (np.float64, 16, 65, 3, 32, False, np.int64),
         (np.float32, 17, 63, 128, None, True, np.int32), (np.float32, 17, 4500, 3, None, True, np.int32),
         (np.float64, 9, 4500, 0, None, False, np.int64)]


@pytest.mark.parametrize("dtype,d,n,k,slice_rows,weighted,ydtype", CASES)
def test_kernel_against_reference(dtype, d, n, k, slice_rows, weighted, ydtype):
    x, y, w, coef, icpt = data(dtype, n, d, k, weighted, ydtype)
    check(dev(x), x, y, w, coef, icpt, k == 0, slice_rows)


@pytest.mark.parametrize("threshold", [0.0, 0.8, 0.95, 1.0])
def test_binomial_threshold(threshold):
    """pred is m > logit(threshold); the data keep every margin further than delta_r (and the
    roundings of the logit in f64) from it."""
    x, y, w, coef, icpt = data(np.float32, 130, 17, 0)
    ref = reference(x, y, w, coef, icpt, True)
    with np.errstate(divide="ignore"):
        cut = np.log(np.longdouble(threshold) / (1 - np.longdouble(threshold)))
    assert (np.abs(ref.raw[:, 1] - cut) > ref.delta + (0 if np.isinf(cut) else 4 * EPS * abs(cut))).all()
    pred = _C.logreg_predict(dev(x), dev(coef), dev(icpt), True, threshold)[0].cpu().numpy()
    assert (pred == (ref.raw[:, 1] > cut)).all() and (0 < pred.sum() < 130) == (0 < threshold < 1)


@pytest.mark.parametrize("d,n,k,slice_rows", [(17, 33, 0, None), (65, 2 * 32 + 3, 5, 32)])
def test_four_byte_aligned_view(d, n, k, slice_rows):
    x, y, w, coef, icpt = data(np.float32, n + 1, d, k, True)
    view = dev(x)[1:]  # (odd d: the base is 4-byte aligned, the scalar-load path)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    check(view, x[1:], y[1:], w[1:], coef, icpt, k == 0, slice_rows)


@pytest.mark.parametrize("k", [0, 5])
def test_margins_of_eight_hundred(k):
    """|m| of about 800: exp(800) is an infinity in f64, so a softmax or a sigmoid without the shift is not finite."""
    x, y, w, coef, icpt = data(np.float64, 40, 15, k, True, scale=800.0)
    assert np.abs(reference(x, y, w, coef, icpt, k == 0).raw).max() > 800
    check(dev(x), x, y, w, coef, icpt, k == 0)


@pytest.mark.parametrize("dtype,d,n,k", [(np.float32, 33, 50, 0), (np.float64, 20, 40, 6)])
def test_left_out_rows_are_counted_and_change_no_bit(dtype, d, n, k):
    clean = data(dtype, n, d, k, True, np.float64)
    at = [3, 9, 20, 31, n]  # five more rows (the indices of the clean rows they go before)
    x, y, w = [np.insert(a, at, a[0], axis=0) for a in clean[:3]]
    new = np.array(at) + np.arange(5)
    x[new[0], 5], x[new[1], d - 2] = np.nan, np.inf
    y[new[2]], y[new[3]], w[new[4]] = (k if k else 2), 0.5, -1.0
    got = step(dev(x), y, w, *clean[3:], k == 0)
    want = step(dev(clean[0]), *clean[1:], k == 0)
    for g, t in zip(got[:3], want[:3]):  # (one block, one slice: the same rows added in the same order)
        assert (g == t).all()
    assert list(got[3]) == [2, 2, 1] and list(want[3]) == [0, 0, 0]
    pred, raw, prob = [t.cpu().numpy() for t in _C.logreg_predict(dev(x), dev(clean[3]), dev(clean[4]), k == 0, 0.5)]
    keep = np.ones(n + 5, dtype=bool)
    keep[new[:2]] = False
    assert (pred[~keep] == -1).all() and (raw[~keep] == 0).all() and (prob[~keep] == 0).all()
    assert (pred[keep] == reference(x[keep], y[keep] % 2, None, *clean[3:], k == 0).pred).all()


@pytest.mark.parametrize("k", [0, 4])
def test_zero_and_unit_weights(k):
    x, y, _, coef, icpt = data(np.float32, 60, 9, k)
    w = np.ones(60)
    for g, t in zip(step(dev(x), y, w, coef, icpt, k == 0), step(dev(x), y, None, coef, icpt, k == 0)):
        assert (g == t).all()
    w[[4, 59]] = 0.0
    keep = w > 0  # (one block, one slice: the other rows are added in the same order)
    for g, t in zip(step(dev(x), y, w, coef, icpt, k == 0), step(dev(x[keep]), y[keep], w[keep], coef, icpt, k == 0)):
        assert (g == t).all()
    check_eval(step(dev(x), y, w, coef, icpt, k == 0), reference(x, y, w, coef, icpt, k == 0), 62, 129)


@pytest.mark.parametrize("k", [2, 3])
def test_frame_on_the_device(k):
    rng = np.random.default_rng(k)
    x = (rng.standard_normal((sum(SIZES), 5)) * [1, 10, 0.1, 3, 1]).astype(np.float32)
    y, w = rng.integers(0, k, len(x)).astype(np.int32), rng.uniform(0.5, 2, len(x))
    df = frame({"features": x, "label": y, "w": w}, SIZES).cache_on_device(DEV)
    before = metrics.snapshot()
    model = LogisticRegression(fitIntercept=False, regParam=0.1, weightCol="w", tol=1e-8).fit(df)
    after = metrics.snapshot()
    evals = after["logreg_evaluations"] - before.get("logreg_evaluations", 0)
    assert after["logreg_device_partitions"] - before.get("logreg_device_partitions", 0) == 2 * evals  # (one is empty)
    assert after.get("logreg_host_partitions", 0) == before.get("logreg_host_partitions", 0)
    u = check_fit(model, x, y, w, 0.1, 1e-8)
    blocks = model.transform(df).local_blocks()
    cols = {c: torch.cat([blocks[p].columns[c] for p in (1, 2)])
            for c in ("rawPrediction", "probability", "prediction")}
    assert all(c.is_cuda and c.dtype == torch.float64 for c in cols.values())
    empty = blocks[0].columns["probability"]
    assert empty.is_cuda and empty.shape == (0, k) and cols["rawPrediction"].shape == (len(x), k)
    ref = reference(x, y, w, model.coefficientMatrix, model.interceptVector, k == 2)
    check_predict([cols[c].cpu().numpy() for c in ("prediction", "rawPrediction", "probability")], ref)
    assert u.shape == (1 if k == 2 else k, 5)
