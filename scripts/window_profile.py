"""row_number + rank + a running sum over one window spec on a device-cached
frame: 10M rows, 100k int32 keys, 4 partitions, one float32 value column
(the shape of scripts/group_agg_profile.py), and the same with half of the
rows in one key. Prints one JSON line per case.

Frame level: milliseconds per call as the median of REPEATS timed calls after
WARMUP warm-up calls (a host clock around a call that ends in a device
synchronise): the window expressions, and `orderBy` alone on the same keys.
Kernel level: hipEvents around `_C.window_scan` (forwards over all channels,
in reverse over the two index channels) and `_C.window_finish` on the whole
sorted column as one partition, with the bytes the forward scan moves per
second: two reads of the words and of the value column, one write of its
outputs."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import tensorframes_amd as tfs  # noqa: E402
from tensorframes_amd import Window  # noqa: E402
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
    w = Window.partitionBy("k").orderBy("x")
    order = timed(lambda: df.orderBy("k", "x").local_blocks())
    win = timed(lambda: df.select("k", "x", F.row_number().over(w).alias("rn"), F.rank().over(w).alias("r"),
                                  F.sum("x").over(w).alias("running")).local_blocks())
    out = df.withColumn("rn", F.row_number().over(w))
    sizes = [b.nrows for _, b in sorted(out.local_blocks().items())]
    print(json.dumps({"case": f"{label}: frame", "orderBy_ms": order, "window_ms": win,
                      "scan_and_finish_ms": round(win["ms"] - order["ms"], 3), "partition_rows": sizes}), flush=True)


def kernel_case(label, keys, x):
    n = keys.shape[0]
    words = _C.sort_encode([keys, x], [False, False])
    perm = _C.sort_argsort(words)
    ks, xs = _C.permute_rows(perm, [keys, x])
    t_sort, _ = events(lambda: _C.permute_rows(_C.sort_argsort(_C.sort_encode([keys, x], [False, False])), [keys, x]))
    sw = _C.sort_encode([ks, xs], [False, False])
    kinds = ["group_head", "peer_head", "sum_f64"]
    t_enc, _ = events(lambda: _C.sort_encode([ks, xs], [False, False]))
    t_fwd, fwd = events(lambda: _C.window_scan(sw, 1, False, kinds, [xs]))
    t_rev, rev = events(lambda: _C.window_scan(sw, 1, True, kinds[:2], []))
    t_fin, _ = events(lambda: _C.window_finish(fwd, rev, kinds, [0] * 3, [0] * 3, False, False, 0, 0,
                                               ["row_number", "rank", "sum"], ["rows", "rows", "range"], [0, 0, 2],
                                               [torch.float32] * 3))
    fwd_bytes = 2 * (2 * 8 + 4) * n + 3 * 8 * n
    rev_bytes = 2 * (2 * 8) * n + 2 * 8 * n
    print(json.dumps({"case": f"{label}: kernels, one partition of {n} rows", "tile_rows": int(_C.window_tile_rows()),
                      "encode_argsort_permute_ms": t_sort, "encode_sorted_ms": t_enc, "scan_forward_ms": t_fwd,
                      "scan_reverse_ms": t_rev, "finish_ms": t_fin,
                      "scan_and_finish_ms": round(t_fwd + t_rev + t_fin, 4),
                      "scan_forward_TBps": round(fwd_bytes / (t_fwd * 1e-3) / 1e12, 3),
                      "scan_reverse_TBps": round(rev_bytes / (t_rev * 1e-3) / 1e12, 3)}), flush=True)


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
