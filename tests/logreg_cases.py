"""What tests/test_logreg.py and tests/test_gpu_logreg.py share: the data, one
objective evaluation in np.longdouble straight from the definitions, the
bounds, and the strong-convexity check of `LogisticRegression.fit`.

A binomial model is the two-class softmax of the margins [0, m]. With eps =
2^-52, K classes and A_r = max_c (|icpt_c| + sum_f |x_rf| |coef_cf|):

  margin  d products and d additions (the intercept included) of 2^-53 each, in
          any order, and the rounded m - M (|m - M| <= 2 A_r, another 2^-53 of
          it): delta_r = (d + 2) eps A_r.
  p, q    the softmax moves by at most e^(2 delta_r) - 1 relative when every
          margin moves by delta_r (numerator and denominator e^(+-delta_r)
          each; not linearised). The roundings: exp of the numerator and of
          the terms of S (1 ulp = eps each), K - 1 additions of positive terms
          and one division (2^-53 each): (K / 2 + 2) eps; p - [c == y] and the
          product with w: 2 * 2^-53 more on |p - [c == y]| <= 1. The binomial
          sigma = 1 / (1 + e) or e / (1 + e) has fewer. Together
          dq_r = w_r (expm1(2 delta_r) + (K + 4) eps), so c = 4, and dp_r is
          dq_r / w_r.
  loss    logsumexp is 1-Lipschitz in the largest margin error and m_y moves by
          delta_r: 2 delta_r. The roundings of log (eps log K), of S inside it
          ((K / 2 + 2) eps), of M + log S, of - m_y and of the product with w
          (2^-53 each on at most 2 A_r + log K) stay below (K + 8) eps (1 + A_r):
          dL_r = w_r (2 delta_r + (K + 8) eps (1 + A_r)).
  sums    an element of grad: sum_r dq_r |x_rf| + terms eps sum_r |q_rc| |x_rf|,
          terms = the rows one accumulator adds in sequence + the partials
          folded + 1 (the caller's); loss and wsum: sum dL_r + terms eps sum L_r.

The reference asserts for every row that its largest and second largest
probability are at least 2 dp_r apart, so `pred` is compared for every row."""
from types import SimpleNamespace

import numpy as np

EPS = 2.0 ** -52
LD = np.longdouble


def data(dtype, n, d, k, weighted=False, ydtype=np.int32, scale=1.0, seed=0):
    """(x [n, d], y [n] in [0, k), w [n] or None, coef [R, d], icpt [R]); k = 0 is the binomial model (R = 1)."""
    rng = np.random.default_rng(seed + 1000 * n + 10 * d + k)
    r = k if k else 1
    x = rng.standard_normal((n, d)).astype(dtype)
    y = rng.integers(0, k if k else 2, n).astype(ydtype)
    w = rng.uniform(0.5, 2.0, n).astype(np.float32) if weighted else None
    return x, y, w, scale * rng.standard_normal((r, d)) / np.sqrt(d), scale * rng.standard_normal(r)


def reference(x, y, w, coef, icpt, binomial):
    n, d = x.shape
    xl, wl = x.astype(LD), (np.ones(n) if w is None else w).astype(LD)
    m = xl @ coef.astype(LD).T + icpt.astype(LD)
    amp = (np.abs(xl) @ np.abs(coef).astype(LD).T + np.abs(icpt).astype(LD)).max(1)
    if binomial:
        m = np.concatenate([np.zeros((n, 1), dtype=LD), m], 1)
    k = m.shape[1]
    big = m.max(1)
    e = np.exp(m - big[:, None])
    p = e / e.sum(1)[:, None]
    rows = wl * (big + np.log(e.sum(1)) - m[np.arange(n), y.astype(np.int64)])
    q = wl[:, None] * (p - (y.astype(np.int64)[:, None] == np.arange(k)[None, :]))
    q = q[:, 1:] if binomial else q
    delta = (d + 2) * EPS * amp
    dp = np.expm1(2 * delta) + (k + 4) * EPS
    two = np.sort(p, 1)[:, -2:]
    assert (two[:, 1] - two[:, 0] >= 2 * dp).all()
    x1 = np.concatenate([np.abs(xl), np.ones((n, 1), dtype=LD)], 1)
    return SimpleNamespace(
        raw=np.concatenate([-m[:, 1:], m[:, 1:]], 1) if binomial else m, prob=p, pred=p.argmax(1), amp=amp, dp=dp,
        delta=delta,
        loss=rows.sum(), loss_mag=np.abs(rows).sum(), dloss=(wl * (2 * delta + (k + 8) * EPS * (1 + amp))).sum(),
        wsum=wl.sum(), grad=q.T @ np.concatenate([xl, np.ones((n, 1), dtype=LD)], 1),
        grad_mag=np.abs(q).T @ x1, dgrad=np.repeat((wl * dp)[None, :], q.shape[1], 0) @ x1)


def check_eval(got, ref, grad_terms, sum_terms):
    """(loss, grad, wsum, bad) of one evaluation against the reference."""
    loss, grad, wsum, bad = [np.asarray(g) for g in got]
    assert (np.asarray(bad) == 0).all() and np.isfinite(grad).all()
    assert (np.abs(grad - ref.grad) <= ref.dgrad + grad_terms * EPS * ref.grad_mag).all()
    assert abs(loss.reshape(-1)[0] - ref.loss) <= ref.dloss + sum_terms * EPS * ref.loss_mag
    assert abs(wsum.reshape(-1)[0] - ref.wsum) <= sum_terms * EPS * ref.wsum


def check_predict(got, ref):
    pred, raw, prob = [np.asarray(g) for g in got]
    assert (pred == ref.pred).all()
    assert (np.abs(raw - ref.raw) <= ref.delta[:, None]).all() and (np.abs(prob - ref.prob) <= ref.dp[:, None]).all()


def objective(u, x, y, w, sigma, reg, standardization, binomial):
    """(f, g, H) in longdouble of f(u) = sum w (logsumexp m - m_y) / sum w + reg / 2 P at u [R, d], no intercept."""
    n, d = x.shape
    r = u.shape[0]
    z = x.astype(LD) / sigma
    wl = (np.ones(n) if w is None else w).astype(LD)
    scale = np.ones(d, dtype=LD) if standardization else 1 / sigma ** 2
    m = z @ u.T
    if binomial:
        m = np.concatenate([np.zeros((n, 1), dtype=LD), m], 1)
    big = m.max(1)
    e = np.exp(m - big[:, None])
    p = e / e.sum(1)[:, None]
    f = (wl * (big + np.log(e.sum(1)) - m[np.arange(n), y])).sum() / wl.sum() + reg / 2 * (scale * u * u).sum()
    own = (p - (y[:, None] == np.arange(m.shape[1])[None, :]))[:, -r:]
    g = (wl[:, None] * own).T @ z / wl.sum() + reg * scale * u
    pr = p[:, -r:]
    v = (pr[:, :, None] * np.eye(r)[None] - pr[:, :, None] * pr[:, None, :]) * wl[:, None, None]
    h = np.einsum("nce,ni,nj->ciej", v, z, z) / wl.sum() + np.einsum("ce,ij->ciej", np.eye(r), np.diag(scale)) * reg
    return f, g, h.reshape(r * d, r * d)


def check_fit(model, x, y, w, reg, tol, standardization=True):
    """The fitted u = beta * sigma of a fit with fitIntercept=False against the optimum of a Newton iteration on the
    longdouble objective (its linear solves in float64; it ends at a gradient below 1e-17): the objective is
    reg-strongly convex in u, so ||u - u*||_2 <= ||g(u)||_2 / reg, and fit stopped at ||g||_inf <= tol max(1, |f|)
    of its own gradient, which the bounds above put far below tol from g: twice that is asserted."""
    n, d = x.shape
    wl = (np.ones(n) if w is None else w).astype(LD)
    big_w = wl.sum()
    mean = (wl[:, None] * x.astype(LD)).sum(0) / big_w
    sigma = np.sqrt((wl[:, None] * (x.astype(LD) - mean) ** 2).sum(0) / (big_w - (wl * wl).sum() / big_w))
    binomial = model.numClasses == 2 and model.coefficientMatrix.shape[0] == 1
    act = sigma > 0  # (a constant feature is no unknown)
    assert (model.coefficientMatrix[:, ~act] == 0.0).all()
    args = (x[:, act], y.astype(np.int64), w, sigma[act], LD(reg), standardization, binomial)
    u = model.coefficientMatrix[:, act].astype(LD) * sigma[act]
    f, g, _ = objective(u, *args)
    assert np.abs(g).max() <= 2 * tol * max(1.0, abs(f))
    best = np.zeros_like(u)
    for _ in range(50):
        _, gb, hb = objective(best, *args)
        if np.abs(gb).max() < 1e-17:
            break
        best = best - np.linalg.solve(hb.astype(np.float64), gb.reshape(-1).astype(np.float64)).reshape(u.shape)
    assert np.abs(gb).max() < 1e-17
    assert np.sqrt(((u - best) ** 2).sum()) <= np.sqrt((g ** 2).sum()) / reg
    return u


def frame(columns, sizes):
    """A frame whose partition p holds sizes[p] rows of every column (zero allowed): `frame_of` of
    vector_moments_cases.py for several columns."""
    import torch

    import tensorframes_amd as tfs
    from tensorframes_amd.frame.block import Block
    from tensorframes_amd.frame.dataframe import DataFrame, _Materialized
    schema = tfs.from_columns({c: v[:1] for c, v in columns.items()}, num_partitions=1).schema
    starts = np.concatenate([[0], np.cumsum(sizes)])
    blocks = {p: Block(int(s), {c: torch.from_numpy(np.ascontiguousarray(v[starts[p]:starts[p + 1]]))
                                for c, v in columns.items()}) for p, s in enumerate(sizes)}
    return DataFrame(schema, _Materialized(blocks), len(sizes))
