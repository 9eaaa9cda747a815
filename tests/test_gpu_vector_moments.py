"""`_C.vector_moments` (csrc/kernels/vector_moments.hip) and the device path of
`Correlation.corr` / `Correlation.cov`, on the GPU.

The reference (tests/vector_moments_cases.py) is a plain two-pass computation
in np.longdouble: the exact mean, then xc.T @ xc. An element of C is held to
terms * 2^-52 * sum_r |xc_ri| |xc_rj| (the sum in longdouble). The terms
follow the kernel as built:
  the products one element adds in sequence in a slice (the MFMA
  accumulator runs over the slice's rows in row order)               min(slice_rows, n)
  the slice partials folded in slice order                           slices
  the two rounded subtractions of the shift                          2
  the correction n m_i m_j and the mirror                            2
  frame level: one merge per partition                               nparts
The default slice is 256 rows or more, so every default-sliced case here is
one slice of n rows. A mean is held to terms * 2^-52 * sum |x| / n with
  the rows a thread adds in sequence                                 ceil(n / rows per pass)
  the row lanes folded in lane order                                 rows per pass
  the chunk fold, the division, the centred mean added               3
where rows per pass = 256 / min(64, d rounded up to a power of two).
Every shape handed to the binding is valid."""
import numpy as np
import pytest
import torch

from tensorframes_amd._native import _C
from tensorframes_amd.ml.stat import Correlation
from tensorframes_amd.utils.logging import metrics

from vector_moments_cases import EPS, SIZES, check_cov_corr, far_apart, frame_of, reference

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]

DEV = "cuda:0"


def data(dtype, n, d, seed=0):
    """f32: 1e4 + N(0, 1); f64: N(0, 1) scaled per component by powers of ten."""
    z = np.random.default_rng(seed + 1000 * n + d).standard_normal((n, d))
    if dtype == np.float32:
        return (1e4 + z).astype(np.float32)
    return z * 10.0 ** (np.arange(d) % 9 - 4)


def c_terms(n, slice_rows=None):
    assert slice_rows is not None or n <= 256
    rows = n if slice_rows is None else min(slice_rows, n)
    return rows + -(-n // rows) + 2 + 2


def check(x_dev, x, slice_rows=None, skip=()):
    """The binding on x_dev against the reference of x; the components in `skip` are left out."""
    mean, c = _C.vector_moments(x_dev) if slice_rows is None else _C.vector_moments(x_dev, slice_rows=slice_rows)
    mean, c = mean.cpu().numpy(), c.cpu().numpy()
    n, d = x.shape
    keep = [j for j in range(d) if j not in skip]
    want_mean, want, mag = reference(x)
    per_pass = 256 // min(64, 1 << (d - 1).bit_length())
    mean_tol = (-(-n // per_pass) + per_pass + 3) * EPS * np.abs(x.astype(np.longdouble)).sum(0) / n
    assert (np.abs(mean - want_mean) <= mean_tol)[keep].all()
    assert (np.abs(c - want) <= c_terms(n, slice_rows) * EPS * mag)[np.ix_(keep, keep)].all()
    assert c.shape == (d, d) and (c == c.T)[np.ix_(keep, keep)].all()
    return c


CASES = [(np.float32, 1, 1, None), (np.float64, 2, 3, None), (np.float32, 15, 4, None), (np.float64, 16, 5, None),
         (np.float32, 17, 31, None), (np.float64, 33, 32, None), (np.float32, 65, 33, None),
         (np.float64, 130, 33, None), (np.float32, 16, 32, None), (np.float64, 65, 1, None),
         (np.float32, 130, 2 * 32 + 3, 32), (np.float64, 17, 2 * 32 + 3, 32), (np.float32, 64, 200, 64)]


@pytest.mark.parametrize("dtype,d,n,slice_rows", CASES)
def test_kernel_against_reference(dtype, d, n, slice_rows):
    x = data(dtype, n, d)
    check(torch.from_numpy(x).to(DEV), x, slice_rows)


@pytest.mark.parametrize("d,n,slice_rows", [(17, 33, None), (65, 2 * 32 + 3, 32)])
def test_four_byte_aligned_view(d, n, slice_rows):
    x = data(np.float32, n + 1, d)
    view = torch.from_numpy(x).to(DEV)[1:]  # (odd d: the base is 4-byte aligned, the scalar-load path)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    check(view, x[1:], slice_rows)


@pytest.mark.parametrize("dtype,d,n", [(np.float32, 33, 33), (np.float64, 130, 40)])
def test_nan_and_infinity_stay_in_their_components(dtype, d, n):
    clean = data(dtype, n, d)
    x = clean.copy()
    x[3, 5], x[n - 1, d - 2] = np.nan, np.inf
    c = check(torch.from_numpy(x).to(DEV), clean, skip=(5, d - 2))
    bad = np.zeros((d, d), dtype=bool)
    bad[[5, d - 2], :] = True
    bad[:, [5, d - 2]] = True
    assert (np.isnan(c) == bad).all()


def test_frame_on_the_device():
    y = far_apart(SIZES, 17)
    df = frame_of(y, SIZES).cache_on_device(DEV)
    before = metrics.snapshot().get("vector_moments_device_partitions", 0)
    Correlation.cov(df, "y").to_numpy("cov(y)")
    assert metrics.snapshot()["vector_moments_device_partitions"] - before == 2  # (the third partition is empty)
    check_cov_corr(df, y, c_terms(max(SIZES)) + len(SIZES))
