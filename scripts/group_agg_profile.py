"""groupBy(k).agg over 10M rows / 100k int32 keys on a device-cached frame,
next to the monoid `aggregate` of the same frame (the shape of
scripts/groupby_profile.py). Prints one JSON line per case.

Frame level: milliseconds per call as the median of REPEATS timed calls after
WARMUP warm-up calls (a host clock around a call that ends in a device
synchronise). Kernel level: hipEvents around `_C.factorize`,
`_C.segment_csr` and `_C.group_moments` on the whole column, with the bytes
group_moments reads (perm + values) per second, and the alternative that
gathers the value columns into segment order first (`_C.take_rows`) and reads
them contiguously."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import tensorframes_amd as tfs  # noqa: E402
from tensorframes_amd import functions as F  # noqa: E402
from tensorframes_amd import tf  # noqa: E402
from tensorframes_amd._native import _C  # noqa: E402

WARMUP, REPEATS = 3, 20
N, NK, PARTS = 10_000_000, 100_000, 4
dev = torch.device("cuda", 0)


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def events(fn):
    """Median device milliseconds of fn (hipEvents), and its last result."""
    out = None
    for _ in range(WARMUP):
        out = fn()
    ms = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return round(statistics.median(ms), 4), out


def five(cols):
    return [F.count("*")] + [f(c) for c in cols for f in (F.avg, F.stddev, F.min, F.max)]


def frame_cases(label, keys, x):
    cols = {"k": keys}
    cols.update({f"x{j}": x[:, j].contiguous() for j in range(4)})
    df = tfs.from_columns(cols, num_partitions=PARTS).cache_on_device(dev)
    with tf.Graph().as_default():
        xi = tf.placeholder(tf.double, [None], name="x0_input")
        s = tf.reduce_sum(xi, [0], name="x0")
        res = timed(lambda: tfs.aggregate(s, df.groupBy("k")).local_blocks())
    print(json.dumps({"case": f"{label}: aggregate(Sum x0), the monoid yardstick", **res}), flush=True)
    for name, exprs in (("agg(sum(x0))", [F.sum("x0")]), ("agg(count, avg, stddev, min, max of x0)", five(["x0"])),
                        ("agg(the five statistics of x0..x3)", five(["x0", "x1", "x2", "x3"]))):
        res = timed(lambda: df.groupBy("k").agg(*exprs).local_blocks())
        print(json.dumps({"case": f"{label}: {name}", **res}), flush=True)


def kernel_cases(label, keys, x):
    n = keys.shape[0]
    t_fact, (ids, uniq) = events(lambda: _C.factorize(keys))
    ng = int(uniq.shape[0])
    t_csr, (perm, offsets) = events(lambda: _C.segment_csr(ids, ng))
    for ncols in (1, 4):
        cols = [x[:, j].contiguous() for j in range(ncols)]
        t_mom, _ = events(lambda: _C.group_moments(cols, perm, offsets))
        nbytes = 8 * n + 8 * n * ncols
        print(json.dumps({"case": f"{label}: kernels, {ncols} f64 column(s)", "groups": ng, "factorize_ms": t_fact,
                          "segment_csr_ms": t_csr, "group_moments_ms": t_mom,
                          "group_moments_TBps": round(nbytes / (t_mom * 1e-3) / 1e12, 3)}), flush=True)
        ident = torch.arange(n, device=dev, dtype=torch.int64)
        t_take, taken = events(lambda: _C.take_rows(perm, cols))
        t_cont, _ = events(lambda: _C.group_moments(taken, ident, offsets))
        print(json.dumps({"case": f"{label}: take_rows first, {ncols} f64 column(s)", "take_rows_ms": t_take,
                          "group_moments_contiguous_ms": t_cont, "sum_ms": round(t_take + t_cont, 4)}), flush=True)


def main():
    g = torch.Generator(device=dev).manual_seed(5)
    keys = torch.randint(0, NK, (N,), device=dev, generator=g, dtype=torch.int32)
    x = torch.rand((N, 4), device=dev, generator=g, dtype=torch.float64)
    skew = keys.clone()
    skew[torch.rand(N, device=dev, generator=g) < 0.5] = 7       # half the rows in one key
    frame_cases("uniform", keys, x)
    frame_cases("skewed", skew, x)
    kernel_cases("uniform", keys, x)
    kernel_cases("skewed", skew, x)
    single = torch.randperm(1_000_000, device=dev, generator=g).to(torch.int32)
    kernel_cases("1M singletons", single, x[:1_000_000])


if __name__ == "__main__":
    main()
