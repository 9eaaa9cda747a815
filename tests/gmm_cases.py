"""What tests/test_gmm.py and tests/test_gpu_gmm.py share: the data, the plain
np.longdouble EM step with its bounds, and the check of `GaussianMixture.fit`.

The reference takes the same means, transforms T and logconst c as the code
under test, so no bound involves a condition number. A rounding is 2^-53; every
count below is multiplied by EPS = 2^-52, twice that. With xc = x - mu_j, z = T_j
xc and A_i = sum_f |T_if| |xc_f|:
  log p = c - ||z||^2 / 2   z_i: one rounding of xc and <= d of the sum, 2 (d + 1) A_i^2 on z_i^2, one more
                            for the square, <= d additions of squares, one for c - s / 2:
                            (3 d + 4) * EPS * (|c| + sum_i A_i^2 / 2) =: B_j, B = max_j B_j
  lse = M + log S           lse is 1-Lipschitz in max_j |error of log p_j|: B; S = sum exp(log p - M) >= 1: the
                            subtraction, 2 ulp of exp and k - 1 additions, (k + 4) * EPS; 2 ulp of log, 2 EPS
                            |log S|; the last addition, EPS |lse|
  r = exp(log p - lse)      the argument is off by B_j + b_lse + EPS |log p - lse|; exp adds 2 ulp; a result under
                            the normal range is held absolutely to the smallest normal number
The table of ulp errors of the HIP device math functions is not at hand here:
2 ulp per call of exp and log are allowed. A sum over rows is held to
terms * EPS * (sum of |what is added|) plus what the errors of r contribute;
`terms` is counted by the caller from the order of additions of its path, + 2
(S: the roundings of xc and of r xc) or + 3 (C: one more xc). The reference
asserts that its gap between the best and the second-best log p is at least
2 (B + 4 EPS) for every row, so `pred` is compared for every row."""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

from tensorframes_amd.ml.clustering import GaussianMixture, _gmm_params

EPS = 2.0 ** -52
TINY = float(np.finfo(np.float64).tiny)
L = np.longdouble


def scale(dtype, d):
    return np.ones(d) if dtype == np.float32 else 10.0 ** (np.arange(d) % 3 - 1)


def data(dtype, n, d, seed=0):
    """f32: 1e3 + N(0, 1); f64: N(0, 1) scaled per component by 0.1, 1, 10."""
    z = np.random.default_rng(seed + 1000 * n + d).standard_normal((n, d))
    return (1e3 + z).astype(np.float32) if dtype == np.float32 else z * scale(dtype, d)


def mixture(x, k):
    """(weights, means, covs): k rows of x as the means, unequal weights, full covariances D (W W^T / d + a I) D."""
    n, d = x.shape
    rng = np.random.default_rng(7)
    means = x[np.sort(rng.choice(n, k, replace=False))].astype(np.float64)
    s = scale(x.dtype.type, d)
    covs = np.empty((k, d, d))
    for j in range(k):
        w = rng.standard_normal((d, d))
        covs[j] = 4.0 * (w @ w.T / d + (0.5 + j / k) * np.eye(d)) * np.outer(s, s)
    weights = 1.0 + np.arange(k)
    return weights / weights.sum(), means, covs


def reference(x, means, transforms, logconst):
    """One EM step in longdouble by the definitions, with the bounds of the module docstring."""
    n, d = x.shape
    k = means.shape[0]
    xc = np.asarray(x).astype(L)[:, None, :] - means.astype(L)[None]  # [n, k, d]
    s, a2 = np.empty((n, k), dtype=L), np.empty((n, k), dtype=L)
    for j in range(k):
        z = xc[:, j] @ transforms[j].astype(L).T
        s[:, j] = (z * z).sum(1)
        a2[:, j] = ((np.abs(xc[:, j]) @ np.abs(transforms[j]).astype(L).T) ** 2).sum(1)
    lp = logconst.astype(L) - s / 2
    b_lp = (3 * d + 4) * EPS * (np.abs(logconst) + a2 / 2)
    if k > 1:
        two = np.sort(lp, 1)[:, -2:]
        assert (two[:, 1] - two[:, 0] >= 2 * (b_lp.max(1) + 4 * EPS)).all()
    top = lp.max(1)
    S = np.exp(lp - top[:, None]).sum(1)
    lse = top + np.log(S)
    b_lse = b_lp.max(1) + EPS * (k + 4 + 2 * np.abs(np.log(S)) + np.abs(lse))
    r = np.exp(lp - lse[:, None])
    arg = b_lp + b_lse[:, None] + EPS * np.abs(lp - lse[:, None])
    b_r = r * (np.expm1(arg) * (1 + 2 * EPS) + 2 * EPS) + TINY
    ref = SimpleNamespace(n=n, r=r, b_r=b_r, pred=lp.argmax(1), lse=lse, b_lse=b_lse, N=r.sum(0), N_err=b_r.sum(0))
    ax = np.abs(xc)
    ref.S = np.einsum("nj,njf->jf", r, xc)
    ref.S_mag, ref.S_err = np.einsum("nj,njf->jf", r, ax), np.einsum("nj,njf->jf", b_r, ax)
    ref.C, ref.C_mag, ref.C_err = [np.stack([(m[:, j] * w[:, j, None]).T @ m[:, j] for j in range(k)])
                                   for w, m in ((r, xc), (r, ax), (b_r, ax))]
    return ref


@lru_cache(maxsize=None)
def case(dtype, d, n, k):
    """(x, (means, transforms, logconst), reference) of one kernel case, computed once."""
    x = data(dtype, n, d)
    weights, means, covs = mixture(x, k)
    params = (means,) + _gmm_params(weights, covs, "case", 0)
    return x, params, reference(x, *params)


def tolerances(ref, terms):
    """The bounds of (N, S, C, loglik) for sums whose path adds `terms` times in sequence."""
    return (ref.N_err + terms * EPS * ref.N, ref.S_err + (terms + 2) * EPS * ref.S_mag,
            ref.C_err + (terms + 3) * EPS * ref.C_mag, ref.b_lse.sum() + ref.n * EPS * np.abs(ref.lse).sum())


def check_step(got, ref, terms):
    N, S, C, loglik, bad = got
    tn, ts, tc, tl = tolerances(ref, terms)
    assert bad == 0 and (np.abs(N - ref.N) <= tn).all() and (np.abs(S - ref.S) <= ts).all()
    assert (np.abs(C - ref.C) <= tc).all() and (C == C.transpose(0, 2, 1)).all()
    assert abs(loglik - ref.lse.sum()) <= tl


def check_fit(df, y, init, iters, terms):
    """`fit` from `init` with maxIter = 1 .. iters on column y: the model after m iterations against one reference
    EM step from the model after m - 1 (fit repeats its bits, so that is the state it came from). The update is
    w = N / sum N, mu += S / N, Sigma = C / N - (S / N)(S / N)^T; the bounds of N, S, C are carried through it to
    first order with one EPS per rounded operation. Returns the last model, its reference step and per iteration
    (the summary's logLikelihood, its bound)."""
    est = GaussianMixture(featuresCol="y", k=len(init[0]), tol=0.0)
    weights, means, covs = est.setInitialModel(*init)._initial
    lls = []
    for m in range(1, iters + 1):
        model = est.setMaxIter(m).setInitialModel(*init).fit(df)
        ref = reference(y, means, *_gmm_params(weights, covs, "check", m - 1))
        tn, ts, tc, tl = tolerances(ref, terms)
        N, tot = ref.N, ref.N.sum()
        step, t_step = ref.S / N[:, None], (ts + np.abs(ref.S) * (tn / N)[:, None]) / N[:, None]
        t_step = t_step + EPS * np.abs(step)
        assert (np.abs(np.array(model.weights) - N / tot) <= tn / tot + N * tn.sum() / tot ** 2 + 2 * EPS * N / tot).all()
        got_means = np.array([g.mean for g in model.gaussians])
        assert (np.abs(got_means - (means + step)) <= t_step + EPS * (np.abs(means) + np.abs(step))).all()
        outer = np.abs(step)[:, :, None] * np.abs(step)[:, None, :]
        t_cov = (tc + np.abs(ref.C) * (tn / N)[:, None, None]) / N[:, None, None] + \
            np.abs(step)[:, :, None] * t_step[:, None, :] + t_step[:, :, None] * np.abs(step)[:, None, :] + \
            3 * EPS * (np.abs(ref.C) / N[:, None, None] + outer)
        want = ref.C / N[:, None, None] - step[:, :, None] * step[:, None, :]
        got_covs = np.array([g.cov for g in model.gaussians])
        assert (np.abs(got_covs - want) <= t_cov).all()
        s = model.summary
        assert s.numIter == m and s.k == len(N) and abs(s.logLikelihood - ref.lse.sum()) <= tl
        assert s.clusterSizes == list(np.bincount(ref.pred, minlength=len(N)))
        lls.append((s.logLikelihood, tl))
        weights, means, covs = np.array(model.weights), got_means, got_covs
    return model, ref, lls
