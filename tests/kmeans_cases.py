"""What tests/test_kmeans.py and tests/test_gpu_kmeans.py share: the data, the
plain np.longdouble Lloyd step and the check of `KMeans.fit` against it.

With x' = x - o, c' = c - o (o the mean of the centres) a squared distance is
held to (d + 8) * 2^-52 * M, M = sum x'^2 + 2 |x'|.|c'| + sum c'^2: per sum d
products of two once-rounded operands and at most d - 1 additions that are not
additions of an exact zero, whatever their order, then the two roundings of
||c'||^2 - 2 x'.c' and of + ||x'||^2 (d + 4 roundings of 2^-53 each). The
reference asserts that its gap between the best and the second-best centre is
at least twice that bound for every row, so `assign` is compared for every row."""
from types import SimpleNamespace

import numpy as np

from tensorframes_amd.ml.clustering import KMeans, _shift

EPS = 2.0 ** -52


def data(dtype, n, d, seed=0):
    """f32: 1e4 + N(0, 1); f64: N(0, 1) scaled per component by powers of ten."""
    z = np.random.default_rng(seed + 1000 * n + d).standard_normal((n, d))
    if dtype == np.float32:
        return (1e4 + z).astype(np.float32)
    return z * 10.0 ** (np.arange(d) % 9 - 4)


def rows_as_centres(x, k):
    return x[np.sort(np.random.default_rng(7).choice(x.shape[0], k, replace=False))].astype(np.float64)


def reference(x, centers):
    """One Lloyd step in longdouble: distances by the definition sum_f (x - c)^2, argmin, per-cluster sums of x - o."""
    k, d = centers.shape
    xl, cl = np.asarray(x).astype(np.longdouble), centers.astype(np.longdouble)
    d2 = ((xl[:, None, :] - cl[None, :, :]) ** 2).sum(2)
    xs, cs = xl - _shift(centers), cl - _shift(centers)
    mag = (xs ** 2).sum(1)[:, None] + 2 * np.abs(xs) @ np.abs(cs).T + (cs ** 2).sum(1)[None, :]
    if k > 1:
        two = np.sort(d2, 1)[:, :2]
        assert (two[:, 1] - two[:, 0] >= 2 * (d + 8) * EPS * mag.max(1)).all()
    assign = d2.argmin(1)
    member = assign[:, None] == np.arange(k)[None, :]
    return SimpleNamespace(assign=assign, dist=d2.min(1), mag=mag[np.arange(len(xl)), assign],
                           counts=member.sum(0), sums=member.T.astype(np.longdouble) @ xs,
                           sums_mag=member.T.astype(np.longdouble) @ np.abs(xs))


def check_fit(df, y, init, iters, terms):
    """`fit` from `init` with maxIter = iters on column y against `iters` reference steps; returns the model.
    A centre o + S / count: S held to `terms`, two more roundings on |o| + |S| / count."""
    model = KMeans(featuresCol="y", k=len(init), maxIter=iters, tol=0.0).setInitialCenters(init).fit(df)
    want = init.astype(np.longdouble)
    for _ in range(iters):
        ref = reference(y, want.astype(np.float64))
        o = _shift(want.astype(np.float64))
        start, want = want, o + ref.sums / np.maximum(ref.counts, 1)[:, None]
        want[ref.counts == 0] = start[ref.counts == 0]
    tol = (terms + 2) * EPS * (ref.sums_mag / np.maximum(ref.counts, 1)[:, None] + np.abs(o))
    assert (np.abs(np.array(model.clusterCenters()) - want) <= tol).all()
    assert model.summary.numIter == iters and model.summary.clusterSizes == list(ref.counts)
    return model
