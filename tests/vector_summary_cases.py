"""What tests/test_vector_summary.py and tests/test_gpu_vector_summary.py share:
the longdouble reference of `Summarizer`, the test data, and the comparison of
all ten metrics against it.

The reference is plain numpy in np.longdouble, two passes per component over
the rows of positive weight. count, numNonZeros, min, max and the positions of
NaN are compared exactly; a rounded metric is held to terms * 2^-52 * mag with
  mean                 mag = sum w |x| / W
  sum, normL1          mag = sum w |x|
  normL2               mag = sum w x^2 under the root: tol / (2 normL2), one more rounding for the root
  variance, std        mag = sum w |x - m| (|x - m| + |m|) for M2, over the divisor W - Q / W (three more
                       roundings: Q / W, the difference, the quotient), for std through the root as normL2
`terms` is the caller's count of the roundings a value passes through in
sequence. The weights of every test are small multiples of 1/2, so W, Q and
the divisor are exact and add no terms."""
import numpy as np

from tensorframes_amd.ml.stat import METRICS, Summarizer, _metric, _unpack

EPS = 2.0 ** -52
ROW, MERGE, CONST = 3, 5, 4  # roundings of one row's update (delta, the factor, the fused add), of one merge, of the end


def data(dtype, n, d, seed=0):
    """f32: 1e4 + N(0, 1); f64: N(0, 1) scaled per component by powers of ten (a power-sum variance fails on both)."""
    z = np.random.default_rng(seed + 1000 * n + d).standard_normal((n, d))
    if dtype == np.float32:
        return (1e4 + z).astype(np.float32)
    return z * 10.0 ** (np.arange(d) % 9 - 4)


def weights(n, dtype, seed=7):
    """Zeros among small multiples of 1/2 (integers for an integer dtype)."""
    pool = [0, 1, 2, 3] if np.dtype(dtype).kind == "i" else [0.0, 0.5, 1.0, 2.0, 3.0]
    return np.random.default_rng(seed + n).choice(pool, n).astype(dtype)


def reference(x, w=None):
    """({metric: value}, {metric: tolerance per term}) of the rows x with weights w (None: ones)."""
    wl = np.ones(x.shape[0], np.longdouble) if w is None else w.astype(np.longdouble)
    x, wl = x[wl > 0].astype(np.float64), wl[wl > 0][:, None]
    xl = x.astype(np.longdouble)
    with np.errstate(all="ignore"):
        W, Q = wl.sum(), (wl * wl).sum()
        m = (wl * xl).sum(0) / W
        xc = xl - m
        m2, l1, s2 = (wl * xc * xc).sum(0), (wl * np.abs(xl)).sum(0), (wl * xl * xl).sum(0)
        den = W - Q / W
        var = np.maximum(m2 / den, 0) if den > 0 else np.zeros(x.shape[1], np.longdouble)
        nan = np.isnan(x).any(0)
        lo = np.where(np.isnan(x).all(0), np.nan, np.nanmin(np.where(np.isnan(x), np.inf, x), 0)) + 0.0
        hi = np.where(nan, np.nan, np.max(np.where(np.isnan(x), -np.inf, x), 0)) + 0.0  # (NaN is the largest)
        want = {"count": x.shape[0], "mean": m, "sum": m * W, "variance": var, "std": np.sqrt(var),
                "numNonZeros": (x != 0).sum(0).astype(np.float64), "min": lo, "max": hi, "normL1": l1,
                "normL2": np.sqrt(s2)}
        t_var = (wl * np.abs(xc) * (np.abs(xc) + np.abs(m))).sum(0) / den if den > 0 else 0 * m
        tol = {"mean": l1 / W, "sum": l1, "normL1": l1, "normL2": s2 / (2 * np.sqrt(s2)), "variance": t_var,
               "std": t_var / (2 * np.sqrt(var))}
    return want, tol


def check(got, x, w, terms, skip=()):
    """The ten metrics `got` against the reference; the rounded metrics of the components in `skip`
    (those that hold a NaN or an infinity) must be NaN or follow IEEE and are compared by position only."""
    want, tol = reference(x, w)
    keep = np.array([j not in skip for j in range(x.shape[1])])
    assert got["count"] == want["count"]
    for m in ("numNonZeros", "min", "max"):
        assert np.array_equal(got[m], want[m].astype(np.float64), equal_nan=True), m
    for m in ("min", "max"):
        assert not np.signbit(got[m][got[m] == 0]).any(), m
    extra = {"mean": 0, "sum": 1, "normL1": 0, "normL2": 1, "variance": 3, "std": 4}
    for m, more in extra.items():
        if m in ("mean", "sum", "variance", "std"):
            assert (np.isnan(got[m]) == ~keep).all(), m
        if want["count"] == 1 and m in ("variance", "std"):
            assert (got[m][keep] == 0.0).all(), m
            continue
        with np.errstate(all="ignore"):  # (the components in `skip` hold NaN and infinities)
            bound = terms * EPS * tol[m] + more * EPS * np.abs(want[m])
            err = np.abs(got[m] - want[m])
        print(m, "worst error / bound:", float(np.max((err / bound)[keep], initial=0)))
        assert (err <= bound)[keep].all(), m


def record_metrics(rec, d):
    """The ten metrics of one record of `_C.vector_summary` / `_host_summary` (int64 numpy [4 + 8 d])."""
    count, q = int(rec[0]), float(rec[2:3].view(np.float64)[0])
    acc = _unpack(rec, d) if count else None
    return {m: _metric(m, count, q, acc, d).numpy()[0] for m in METRICS}


def frame_metrics(df, column="y", weight=None):
    out = df.select(Summarizer.metrics(*METRICS).summary(column, weight)).cache()  # (one evaluation for the ten)
    return {m: out.to_numpy(f"{m}({column})")[0] for m in METRICS}
