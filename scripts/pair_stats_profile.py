"""corr / covar on a device-cached frame of 10M rows in 4 partitions, next to
the one-column passes over the same columns (unchanged code: they stand for
the parent commit on the same GPU in the same run). Prints one JSON line per
case.

Dense: `df.stat.corr` of two f32 columns and of an f32 / f64 pair, and the
kernel pair under it (`_C.column_pair_moments`) against `_C.column_moments` of
the same two columns: the same bytes read, about two thirds of the arithmetic.
Grouped: `groupBy(k).agg(F.corr(a, b))` at 100k int32 keys, balanced and with
half of the rows in one key, against `groupBy(k).agg(F.stddev(a),
F.stddev(b))` on the same frame, and `_C.group_pair_moments` against
`_C.group_moments` of the two columns on the whole column.

Frame level: milliseconds per call as the median of REPEATS timed calls after
WARMUP warm-up calls (a host clock around a call that ends in a device
synchronise), with the fastest and the slowest as the spread. Kernel level:
hipEvents around the binding call (launches and pool allocations inside), the
same median and spread, and the bytes the kernel reads per second. The dense
kernel and its yardstick alternate call by call over KERNEL_REPEATS pairs of
calls. One 10M-row pair is 80 to 160 MB and stays in the last-level cache from
call to call, so the dense pair is also timed "cold": COLD_SETS copies of the
columns taken in rotation, more bytes between two reads of a copy than the
cache holds."""
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

WARMUP, REPEATS, KERNEL_REPEATS, COLD_SETS = 3, 20, 100, 6
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
    """Device milliseconds of fn (hipEvents): median, fastest, slowest; and its last result."""
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
    return {"ms": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}, out


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def spread(ms):
    return {"ms": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def alternating(fa, fb):
    """Device milliseconds of fa and fb, one call of each in turn."""
    for _ in range(WARMUP):
        fa(), fb()
    ta, tb = [], []
    for _ in range(KERNEL_REPEATS):
        ta.append(device_ms(fa))
        tb.append(device_ms(fb))
    return spread(ta), spread(tb)


def rotating(fn, sets):
    """Device milliseconds of fn(set) over the sets in rotation (every call reads a copy that has left the cache)."""
    for j in range(len(sets)):
        fn(sets[j])
    return spread([device_ms(lambda: fn(sets[j % len(sets)])) for j in range(KERNEL_REPEATS)])


def dense_cases(cols, bufs):
    df = tfs.from_columns(cols, num_partitions=PARTS).cache_on_device(dev)
    for a, b in (("a", "b"), ("a", "d")):
        res = timed(lambda: df.stat.corr(a, b))
        print(json.dumps({"case": f"dense frame: stat.corr({a}, {b})", **res}), flush=True)
        print(json.dumps({"case": f"dense frame: agg(stddev({a}), stddev({b})), the one-column yardstick",
                          **timed(lambda: df.agg(F.stddev(a), F.stddev(b)))}), flush=True)
    for label, x, y in (("f32 / f32", cols["a"], cols["b"]), ("f32 / f64", cols["a"], cols["d"]),
                        ("f64 / f64", cols["d"], cols["e"]), ("f32 / f32, both one element into their buffers",
                                                              bufs["a"][1:], bufs["b"][1:]),
                        ("u8 / i32", cols["u"], cols["i"])):
        nbytes = x.numel() * (x.element_size() + y.element_size())
        pair, one = alternating(lambda: _C.column_pair_moments([x], [y]), lambda: _C.column_moments([x, y]))
        print(json.dumps({"case": f"dense kernels, 10M rows, {label}", "column_pair_moments": pair,
                          "column_moments_of_both": one, "ratio": round(pair["ms"] / one["ms"], 3),
                          "MB_read": round(nbytes / 1e6, 1),
                          "pair_TBps": round(nbytes / (pair["ms"] * 1e-3) / 1e12, 3),
                          "moments_TBps": round(nbytes / (one["ms"] * 1e-3) / 1e12, 3)}), flush=True)


    for label, x, y in (("f32 / f32", cols["a"], cols["b"]), ("f32 / f64", cols["a"], cols["d"])):
        sets = [(x + j, y + j) for j in range(COLD_SETS)]
        nbytes = x.numel() * (x.element_size() + y.element_size())
        pair = rotating(lambda xy: _C.column_pair_moments([xy[0]], [xy[1]]), sets)
        one = rotating(lambda xy: _C.column_moments([xy[0], xy[1]]), sets)
        print(json.dumps({"case": f"dense kernels, cold, 10M rows, {label}, {COLD_SETS} copies in rotation",
                          "column_pair_moments": pair, "column_moments_of_both": one,
                          "ratio": round(pair["ms"] / one["ms"], 3), "MB_read": round(nbytes / 1e6, 1),
                          "pair_TBps": round(nbytes / (pair["ms"] * 1e-3) / 1e12, 3),
                          "moments_TBps": round(nbytes / (one["ms"] * 1e-3) / 1e12, 3)}), flush=True)


def grouped_cases(label, keys, cols):
    df = tfs.from_columns({"k": keys, "a": cols["a"], "d": cols["d"]}, num_partitions=PARTS).cache_on_device(dev)
    res = timed(lambda: df.groupBy("k").agg(F.corr("a", "d")).local_blocks())
    print(json.dumps({"case": f"{label}: groupBy(k).agg(corr(a, d))", **res}), flush=True)
    res = timed(lambda: df.groupBy("k").agg(F.stddev("a"), F.stddev("d")).local_blocks())
    print(json.dumps({"case": f"{label}: groupBy(k).agg(stddev(a), stddev(d)), the one-column yardstick", **res}),
          flush=True)
    res = timed(lambda: df.groupBy("k").agg(F.corr("a", "d"), F.stddev("a"), F.stddev("d")).local_blocks())
    print(json.dumps({"case": f"{label}: groupBy(k).agg(corr(a, d), stddev(a), stddev(d)), work items built once",
                      **res}), flush=True)
    n = keys.shape[0]
    fact, (ids, uniq) = events(lambda: _C.factorize(keys))
    ng = int(uniq.shape[0])
    csr, (perm, offsets) = events(lambda: _C.segment_csr(ids, ng))
    x, y = cols["a"], cols["d"]
    nbytes = n * (8 + x.element_size() + y.element_size())
    pair, _ = events(lambda: _C.group_pair_moments([x], [y], perm, offsets))
    one, _ = events(lambda: _C.group_moments([x, y], perm, offsets))
    both, _ = events(lambda: _C.group_both_moments([x, y], [x], [y], perm, offsets))
    print(json.dumps({"case": f"{label}: kernels, 10M rows, f32 / f64", "groups": ng, "factorize": fact,
                      "segment_csr": csr, "group_pair_moments": pair, "group_moments_of_both": one,
                      "group_both_moments": both, "ratio": round(pair["ms"] / one["ms"], 3),
                      "pair_TBps": round(nbytes / (pair["ms"] * 1e-3) / 1e12, 3)}), flush=True)


def main():
    g = torch.Generator(device=dev).manual_seed(5)
    z, w = (torch.randn(N + 1, device=dev, generator=g, dtype=torch.float64) for _ in range(2))
    cols = {"a": (1e4 + z).to(torch.float32), "b": (1e4 + 0.6 * z + 0.8 * w).to(torch.float32),
            "d": 1e4 + 0.6 * z + 0.8 * w, "e": 1e4 + w, "u": (100 + 5 * z).clamp(0, 255).to(torch.uint8),
            "i": (1e4 + 100 * w).to(torch.int32)}
    whole = {k: v[:N] for k, v in cols.items()}
    dense_cases(whole, cols)
    keys = torch.randint(0, NK, (N,), device=dev, generator=g, dtype=torch.int32)
    skew = keys.clone()
    skew[torch.rand(N, device=dev, generator=g) < 0.5] = 7       # half the rows in one key
    grouped_cases("balanced", keys, whole)
    grouped_cases("skewed", skew, whole)


if __name__ == "__main__":
    main()
