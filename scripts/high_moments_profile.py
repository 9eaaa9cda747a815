"""skewness / kurtosis on a device-cached frame of 10M rows in 4 partitions,
next to stddev over the same column (unchanged code: it stands for the parent
commit on the same GPU in the same run). Prints one JSON line per case.

Dense: `df.agg(F.skewness(a), F.kurtosis(a))` against `df.agg(F.stddev(a))`,
and the kernel pair under it (`_C.column_high_moments`) against
`_C.column_moments` of the same column: the same bytes read, more arithmetic
per row. Grouped: `groupBy(k).agg(F.skewness(a), F.kurtosis(a))` at 100k int32
keys, balanced and with half of the rows in one key, against
`groupBy(k).agg(F.stddev(a))`, and `_C.group_high_moments` against
`_C.group_moments` on the whole column.

Frame level: milliseconds per call as the median of REPEATS timed calls after
WARMUP warm-up calls (a host clock around a call that ends in a device
synchronise), with the fastest and the slowest as the spread. Kernel level:
hipEvents around the binding call (launches and pool allocations inside), the
kernel and its yardstick alternating call by call over KERNEL_REPEATS pairs of
calls. One 10M-row column is 10 to 80 MB and stays in the last-level cache
from call to call, so the dense kernels are also timed "cold": COLD_SETS
copies of the column taken in rotation."""
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

WARMUP, REPEATS, KERNEL_REPEATS, COLD_SETS = 3, 20, 100, 8
N, NK, PARTS = 10_000_000, 100_000, 4
dev = torch.device("cuda", 0)


def spread(ms):
    return {"ms": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


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
    return spread(ms)


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternating(fa, fb, sets):
    """Device milliseconds of fa(set) and fb(set), one call of each in turn, the sets in rotation."""
    for s in sets:
        fa(s), fb(s)
    ta, tb = [], []
    for j in range(KERNEL_REPEATS):
        ta.append(device_ms(lambda: fa(sets[j % len(sets)])))
        tb.append(device_ms(lambda: fb(sets[j % len(sets)])))
    return spread(ta), spread(tb)


def report(case, name, high, one, nbytes, **more):
    print(json.dumps({"case": case, name: high, name.replace("high_", ""): one,
                      "ratio": round(high["ms"] / one["ms"], 3), "MB_read": round(nbytes / 1e6, 1),
                      "high_TBps": round(nbytes / (high["ms"] * 1e-3) / 1e12, 3),
                      "moments_TBps": round(nbytes / (one["ms"] * 1e-3) / 1e12, 3), **more}), flush=True)


def dense_cases(cols):
    df = tfs.from_columns({"a": cols["a"]}, num_partitions=PARTS).cache_on_device(dev)
    print(json.dumps({"case": "dense frame: agg(skewness(a), kurtosis(a))",
                      **timed(lambda: df.agg(F.skewness("a"), F.kurtosis("a")))}), flush=True)
    print(json.dumps({"case": "dense frame: agg(stddev(a)), the yardstick",
                      **timed(lambda: df.agg(F.stddev("a")))}), flush=True)
    for label, x in (("f32", cols["a"]), ("f64", cols["d"]), ("u8", cols["u"]), ("i32", cols["i"])):
        for how, sets in (("warm", [x]), (f"cold, {COLD_SETS} copies in rotation", [x + j for j in range(COLD_SETS)])):
            high, one = alternating(lambda c: _C.column_high_moments([c]), lambda c: _C.column_moments([c]), sets)
            report(f"dense kernels, {how}, 10M rows, {label}", "column_high_moments", high, one,
                   x.numel() * x.element_size())


def grouped_cases(label, keys, cols):
    df = tfs.from_columns({"k": keys, "a": cols["a"]}, num_partitions=PARTS).cache_on_device(dev)
    print(json.dumps({"case": f"{label}: groupBy(k).agg(skewness(a), kurtosis(a))",
                      **timed(lambda: df.groupBy("k").agg(F.skewness("a"), F.kurtosis("a")).local_blocks())}),
          flush=True)
    print(json.dumps({"case": f"{label}: groupBy(k).agg(stddev(a)), the yardstick",
                      **timed(lambda: df.groupBy("k").agg(F.stddev("a")).local_blocks())}), flush=True)
    ids, uniq = _C.factorize(keys)
    perm, offsets = _C.segment_csr(ids, int(uniq.shape[0]))
    x = cols["a"]
    high, one = alternating(lambda c: _C.group_high_moments([c], perm, offsets),
                            lambda c: _C.group_moments([c], perm, offsets), [x])
    report(f"{label}: kernels, 10M rows, f32", "group_high_moments", high, one,
           keys.shape[0] * (8 + x.element_size()), groups=int(uniq.shape[0]))


def main():
    g = torch.Generator(device=dev).manual_seed(5)
    z = torch.randn(N, device=dev, generator=g, dtype=torch.float64)
    cols = {"a": (1e4 + z).to(torch.float32), "d": 1e4 + z, "u": (100 + 5 * z).clamp(0, 255).to(torch.uint8),
            "i": (1e4 + 100 * z).to(torch.int32)}
    dense_cases(cols)
    keys = torch.randint(0, NK, (N,), device=dev, generator=g, dtype=torch.int32)
    skew = keys.clone()
    skew[torch.rand(N, device=dev, generator=g) < 0.5] = 7       # half the rows in one key
    grouped_cases("balanced", keys, cols)
    grouped_cases("skewed", skew, cols)


if __name__ == "__main__":
    main()
