"""median + mode + countDistinct + percentile_approx of one value column per
key on a device-cached frame: 10M rows, 100k int32 keys, 4 partitions, one
float32 value column (the shape of scripts/group_agg_profile.py and
scripts/window_profile.py), and the same with half of the rows in one key.
Prints one JSON line per case.

Frame level: milliseconds per call as the median of REPEATS timed calls after
WARMUP warm-up calls (a host clock around a call that ends in a device
synchronise): the order aggregates, `orderBy` alone on the same columns, and
the moment aggregates `agg(avg, max)` of the same frame for scale.
Kernel level: hipEvents around `_C.group_order_summary` (the head list of
unique.hip, the peer-head scan of window_scan.hip, the chunk and fold kernels
of group_order.hip; it synchronises twice) and `_C.group_order_finish` on the
whole sorted column as one partition."""
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

WARMUP, REPEATS = 2, 10
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


def frame_case(label, keys, x):
    df = tfs.from_columns({"k": keys, "x": x}, num_partitions=PARTS).cache_on_device(dev)
    exprs = [F.median("x"), F.mode("x"), F.countDistinct("x"), F.percentile_approx("x", [0.25, 0.75])]
    order = timed(lambda: df.orderBy("k", "x").local_blocks())
    agg = timed(lambda: df.groupBy("k").agg(*exprs).local_blocks())
    moments = timed(lambda: df.groupBy("k").agg(F.avg("x"), F.max("x")).local_blocks())
    out = df.groupBy("k").agg(*exprs)
    sizes = [b.nrows for _, b in sorted(out.local_blocks().items())]
    print(json.dumps({"case": f"{label}: frame", "orderBy_ms": order, "order_agg_ms": agg, "moment_agg_ms": moments,
                      "summary_and_finish_ms": round(agg["ms"] - order["ms"], 3), "groups_per_partition": sizes}),
          flush=True)


def kernel_case(label, keys, x):
    n = keys.shape[0]
    perm = _C.sort_argsort(_C.sort_encode([keys, x], [False, False]))
    ks, xs = _C.permute_rows(perm, [keys, x])
    sw = _C.sort_encode([ks, xs], [False, False])
    t_enc, _ = events(lambda: _C.sort_encode([ks, xs], [False, False]))
    t_sum, summ = events(lambda: _C.group_order_summary(sw, 1))
    fns = ["percentile", "mode", "count_distinct", "percentile_approx"]
    t_fin, _ = events(lambda: _C.group_order_finish(sw, *summ, fns, [[0.5], [], [], [0.25, 0.75]], torch.float32))
    print(json.dumps({"case": f"{label}: kernels, one partition of {n} rows",
                      "chunk_rows": int(_C.group_order_chunk_rows()), "groups": int(summ[1].shape[0]),
                      "encode_sorted_ms": t_enc, "summary_ms": t_sum, "finish_ms": t_fin,
                      "summary_and_finish_ms": round(t_sum + t_fin, 4),
                      "summary_Grows_per_s": round(n / (t_sum * 1e-3) / 1e9, 3)}), flush=True)


def main():
    g = torch.Generator(device=dev).manual_seed(5)
    keys = torch.randint(0, NK, (N,), device=dev, generator=g, dtype=torch.int32)
    x = torch.rand(N, device=dev, generator=g, dtype=torch.float32)
    skew = keys.clone()
    skew[torch.rand(N, device=dev, generator=g) < 0.5] = 7       # half the rows in one key
    frame_case("uniform", keys, x)
    frame_case("skewed", skew, x)
    kernel_case("uniform", keys, x)
    kernel_case("skewed", skew, x)


if __name__ == "__main__":
    main()
