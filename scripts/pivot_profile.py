"""groupBy(k).pivot(p).agg(sum, avg) over 10M rows / 100k int32 keys / 8 int32
pivot values / one f32 column on a device-cached frame of 4 partitions, next
to groupBy(k, p).agg(sum, avg) of the same frame in the same run (the
composite-key aggregate: the yardstick, the long table pivot starts from).
The whole set is repeated with half of the rows in one key. Prints one JSON
line per case (the shape of scripts/group_agg_profile.py).

Frame level: milliseconds per call as the median of REPEATS timed calls after
WARMUP warm-up calls (a host clock around a call that ends in a device
synchronise). Kernel level: hipEvents around the steps pivot adds to the
composite-key aggregate, on the long table of the same data: `group_ids` on
the key column, `_C.segment_csr`, `_C.sort_encode` of the pivot column, and
`_C.pivot_spread` alone with the bytes it moves per second (offsets 8 (G + 1),
the words a binary search touches counted once, 8 m, the hit records' values
and every output cell)."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import tensorframes_amd as tfs  # noqa: E402
from tensorframes_amd import functions as F  # noqa: E402
from tensorframes_amd._native import _C  # noqa: E402
from tensorframes_amd.ops import groupby as G  # noqa: E402

WARMUP, REPEATS = 3, 20
N, NK, NV, PARTS = 10_000_000, 100_000, 8, 4
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


def exprs():
    return [F.sum("x"), F.avg("x")]


def cases(label, keys, pivot, x):
    df = tfs.from_columns({"k": keys, "p": pivot, "x": x}, num_partitions=PARTS).cache_on_device(dev)
    agg = timed(lambda: df.groupBy("k", "p").agg(*exprs()).local_blocks())
    print(json.dumps({"case": f"{label}: groupBy(k, p).agg(sum, avg), the yardstick", **agg}), flush=True)
    values = list(range(NV))
    piv = timed(lambda: df.groupBy("k").pivot("p", values).agg(*exprs()).local_blocks())
    print(json.dumps({"case": f"{label}: groupBy(k).pivot(p, values).agg(sum, avg)", **piv,
                      "ratio_to_agg": round(piv["ms"] / agg["ms"], 3)}), flush=True)
    found = timed(lambda: df.groupBy("k").pivot("p").agg(*exprs()).local_blocks())
    print(json.dumps({"case": f"{label}: the same with the values discovered (select(p).distinct(), collected)",
                      **found, "ratio_to_agg": round(found["ms"] / agg["ms"], 3)}), flush=True)
    # the steps pivot adds, on the long table of this frame
    long = df.groupBy("k", "p").agg(*exprs()).local_blocks()[0]
    lk, lp = long.columns["k"].contiguous(), long.columns["p"].contiguous()
    outs = [long.columns["sum(x)"].contiguous(), long.columns["avg(x)"].contiguous()]
    m = int(lk.shape[0])
    t_ids, (ids, _, ng) = events(lambda: G.group_ids([lk]))
    t_csr, (_, offsets) = events(lambda: _C.segment_csr(ids, ng))
    t_enc, words = events(lambda: _C.sort_encode([lp], [False]))
    pw = words[0].contiguous()
    vw = torch.from_numpy((np.arange(NV, dtype=np.int64).view(np.uint64) ^ np.uint64(1 << 63)).view(np.int64)).to(dev)
    nan = 0x7FF8000000000000
    t_spread, wide = events(lambda: _C.pivot_spread(offsets, pw, vw, outs, [nan, nan]))
    cells = ng * NV
    hits = int(sum(int((~torch.isnan(w)).sum()) for w in wide[:1]))
    nbytes = 8 * (ng + 1) + 8 * m + 8 * hits * len(outs) + 8 * cells * len(outs)
    print(json.dumps({"case": f"{label}: the steps pivot adds (long table of {m} records, {ng} keys)",
                      "group_ids_ms": t_ids, "segment_csr_ms": t_csr, "sort_encode_ms": t_enc,
                      "pivot_spread_ms": t_spread, "pivot_spread_cells": cells * len(outs),
                      "pivot_spread_GBps": round(nbytes / (t_spread * 1e-3) / 1e9, 1),
                      "added_steps_sum_ms": round(t_ids + t_csr + t_enc + t_spread, 4),
                      "pivot_minus_agg_ms": round(piv["ms"] - agg["ms"], 3)}), flush=True)


def main():
    g = torch.Generator(device=dev).manual_seed(5)
    keys = torch.randint(0, NK, (N,), device=dev, generator=g, dtype=torch.int32)
    pivot = torch.randint(0, NV, (N,), device=dev, generator=g, dtype=torch.int32)
    x = torch.rand((N,), device=dev, generator=g, dtype=torch.float32)
    skew = keys.clone()
    skew[torch.rand(N, device=dev, generator=g) < 0.5] = 7       # half the rows in one key
    cases("uniform", keys, pivot, x)
    cases("skewed", skew, pivot, x)


if __name__ == "__main__":
    main()
