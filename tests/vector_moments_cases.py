"""What tests/test_vector_moments.py and tests/test_gpu_vector_moments.py
share: the longdouble reference, the three-partition frame whose partition
means lie far apart, and the check of `Correlation.cov` / `Correlation.corr`
against the reference."""
import numpy as np
import torch

import tensorframes_amd as tfs
from tensorframes_amd.ml.stat import Correlation

EPS = 2.0 ** -52
SIZES = [0, 5, 2 * 32 + 1]


def reference(x):
    """(mean, C, sum |xc_i| |xc_j|) of the rows x in longdouble: the exact mean, then xc.T @ xc."""
    xl = np.asarray(x).astype(np.longdouble)
    mean = xl.sum(0) / xl.shape[0]
    xc = xl - mean
    return mean, xc.T @ xc, np.abs(xc).T @ np.abs(xc)


def frame_of(y, sizes):
    """A one-column frame whose partition p holds sizes[p] rows of y (zero allowed)."""
    from tensorframes_amd.frame.block import Block
    from tensorframes_amd.frame.dataframe import DataFrame, _Materialized
    schema = tfs.from_columns({"y": y[:1]}, num_partitions=1).schema
    starts = np.concatenate([[0], np.cumsum(sizes)])
    blocks = {p: Block(int(s), {"y": torch.from_numpy(np.ascontiguousarray(y[starts[p]:starts[p + 1]]))})
              for p, s in enumerate(sizes)}
    return DataFrame(schema, _Materialized(blocks), len(sizes))


def far_apart(sizes, d, dtype=np.float32, seed=3):
    """Rows whose partition means lie 1e3 apart: the merge's delta delta^T term dominates."""
    rng = np.random.default_rng(seed)
    parts = [1e3 * p + rng.standard_normal((s, d)) for p, s in enumerate(sizes)]
    return np.concatenate(parts, 0).astype(dtype)


def cell(df, name):
    return df.to_numpy(name)[0]


def check_cov_corr(df, y, terms):
    """cov and corr of column y of df against the reference of the rows y, an element of C held to `terms`."""
    n = y.shape[0]
    _, want, mag = reference(y)
    tol = terms * EPS * mag / (n - 1)
    want = want / (n - 1)
    cov = cell(Correlation.cov(df, "y"), "cov(y)")
    assert (np.abs(cov - want) <= tol).all()
    assert (cov == cov.T).all()
    var = np.diagonal(want)
    r_want = want / np.sqrt(np.outer(var, var))
    # first-order propagation of tol through C_ij / sqrt(C_ii C_jj), and four roundings of the quotient
    rel = tol / np.sqrt(np.outer(var, var))
    r_tol = rel + np.abs(r_want) * (0.5 * (np.diagonal(rel)[:, None] + np.diagonal(rel)[None, :]) + 4 * EPS)
    r = cell(Correlation.corr(df, "y"), "pearson(y)")
    assert (np.abs(r - r_want) <= r_tol).all()
    assert (np.diagonal(r) == 1.0).all() and (r == r.T).all()
