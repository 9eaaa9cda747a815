"""sample / randomSplit / sampleBy / F.rand on a device-cached frame: 10M
rows, an int32 key and one float32 column, 4 partitions (the shape of
scripts/distinct_profile.py). Prints one JSON line per case.

Frame level: milliseconds per call as the median of REPEATS timed calls after
WARMUP warm-up calls (a host clock around a call that ends in a device
synchronise): `sample(0.1).count()`, both counts of `randomSplit([0.8, 0.2])`,
`sampleBy` over 100 strata (every stratum at 0.1), `withColumn("r",
F.rand(1))`, and with replacement at a mean of 0.1; each next to
`filter(x < c).count()` at the `c` that keeps the same share of the same
frame in the same run (x is uniform in [0, 1), so c is the share).
Kernel level: hipEvents around `_C.random_mask` and `_C.random_uniform` over
the 10M rows as one partition, next to `_C.compact_rows` of the two columns
under that mask, with the bytes each writes per second: random_mask writes 1
byte per row and reads nothing, random_uniform writes 8 bytes per row;
compact_rows reads the mask twice and reads and writes 8 bytes per kept row."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import tensorframes_amd as tfs  # noqa: E402
from tensorframes_amd import functions as F  # noqa: E402
from tensorframes_amd._native import _C  # noqa: E402

WARMUP, REPEATS = 2, 7
N, NK, PARTS = 10_000_000, 100, 4
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


def against_filter(df, label, fn, share):
    kept = fn()
    got = timed(fn)
    flt = timed(lambda: df.filter(df.x < share).count())
    print(json.dumps({"case": f"frame: {label}", "rows_out": int(kept), "ms": got,
                      f"filter(x < {share}).count()_ms": flt, "rows_out_filter": int(df.filter(df.x < share).count()),
                      "over_filter": round(got["ms"] / flt["ms"], 3)}), flush=True)


def frame_cases(keys, x):
    df = tfs.from_columns({"k": keys, "x": x}, num_partitions=PARTS).cache_on_device(dev)
    against_filter(df, "sample(0.1, 1).count()", lambda: df.sample(0.1, 1).count(), 0.1)

    def both():
        a, b = df.randomSplit([0.8, 0.2], 1)
        return a.count() + b.count()
    against_filter(df, "randomSplit([0.8, 0.2], 1): both counts (all rows leave)", both, 0.8)
    against_filter(df, "randomSplit([0.8, 0.2], 1)[1].count()", lambda: df.randomSplit([0.8, 0.2], 1)[1].count(), 0.2)
    strata = {k: 0.1 for k in range(NK)}
    against_filter(df, "sampleBy(k, 100 strata at 0.1, 1).count()", lambda: df.sampleBy("k", strata, 1).count(), 0.1)
    against_filter(df, "sample(True, 0.1, 1).count()", lambda: df.sample(True, 0.1, 1).count(), 0.1)
    rand = timed(lambda: df.withColumn("r", F.rand(1)).local_blocks())
    randn = timed(lambda: df.withColumn("z", F.randn(1)).local_blocks())
    plain = timed(lambda: df.withColumn("y", df.x * 2.0).local_blocks())
    print(json.dumps({"case": "frame: withColumn", "rand(1)_ms": rand, "randn(1)_ms": randn,
                      "withColumn(y, x * 2)_ms": plain}), flush=True)
    before = tfs.metrics.snapshot()
    df.sample(0.1, 1).count()
    after = tfs.metrics.snapshot()
    print(json.dumps({"case": "frame: metrics of one sample(0.1, 1).count()",
                      **{m: int(after.get(m, 0) - before.get(m, 0)) for m in
                         ("sample_rows_in", "sample_rows_out", "sample_device_partitions", "sample_host_partitions")}}),
          flush=True)


def kernel_cases(keys, x):
    n = keys.shape[0]
    t_mask, mask = events(lambda: _C.random_mask(1, 0, n, 0.0, 0.1))
    t_uni, _ = events(lambda: _C.random_uniform(1, 0, n))
    t_nor, _ = events(lambda: _C.random_normal(1, 0, n))
    words = _C.sort_encode([keys], [False])
    # the words of the keys 0..99: the sign bit flipped, as int64 bit patterns
    tw = torch.arange(NK, dtype=torch.int64, device=dev) + (-(1 << 63))
    tf = torch.full((NK,), 0.1, dtype=torch.float64, device=dev)
    t_by, by = events(lambda: _C.random_mask_by(1, 0, words, tw, tf))
    assert int(by.sum()) == int(mask.sum())                            # every stratum at 0.1: the same rows
    cdf = torch.tensor([0.9048374180359595, 0.9953211598395555, 0.9998453469297354, 1.0], dtype=torch.float64,
                       device=dev)
    t_poi, _ = events(lambda: _C.random_poisson(1, 0, n, cdf))
    t_compact, got = events(lambda: _C.compact_rows(mask.view(torch.bool), [keys, x], False))
    m = int(got[1])
    print(json.dumps({"case": f"kernels, one partition of {n} rows", "tile_rows": int(_C.random_tile_rows()),
                      "kept_rows": m, "random_mask_ms": t_mask, "random_mask_Grows_per_s": round(n / t_mask / 1e6, 1),
                      "random_uniform_ms": t_uni, "random_uniform_GBps": round(8 * n / t_uni / 1e6, 1),
                      "random_normal_ms": t_nor, "random_mask_by_100_strata_ms": t_by, "random_poisson_ms": t_poi,
                      "compact_rows_k_x_ms": t_compact,
                      "compact_rows_GBps": round((2 * n + 2 * 8 * m) / t_compact / 1e6, 1)}), flush=True)


def main():
    g = torch.Generator(device=dev).manual_seed(5)
    keys = torch.randint(0, NK, (N,), device=dev, generator=g, dtype=torch.int32)
    x = torch.rand(N, device=dev, generator=g, dtype=torch.float32)
    frame_cases(keys, x)
    kernel_cases(keys, x)


if __name__ == "__main__":
    main()
