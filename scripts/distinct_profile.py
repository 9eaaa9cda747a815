"""dropDuplicates(["k"]) on a device-cached frame: 10M rows, int32 keys,
4 partitions, one float32 value column (the shape of
scripts/window_profile.py), with 100k distinct keys and with every key
distinct. Prints one JSON line per case.

Frame level: milliseconds per call as the median of REPEATS timed calls after
WARMUP warm-up calls (a host clock around a call that ends in a device
synchronise): `dropDuplicates(["k"])`, and `orderBy("k")` and
`groupBy("k").count()` of the same frame, with the rows that crossed the
exchange (the metric distinct_rows_exchanged).
Kernel level: hipEvents around `_C.unique_rows` on the 10M sorted rows as one
partition (in order already, and through the order of the radix argsort),
next to `_C.compact_rows` of one int64 column with a mask of the same
density, with the bytes each moves per second. In between, the steps of
one partition on both sides of the exchange (host clock), next to
`orderBy`'s steps on the same rows. unique_rows reads the words
(and the order) once, writes and reads n / 8 bytes of head bits, and reads
and writes 8 bytes per kept row; compact_rows reads the mask twice and reads
and writes 8 bytes per kept row (the index output is not asked for)."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import tensorframes_amd as tfs  # noqa: E402
from tensorframes_amd._native import _C  # noqa: E402

WARMUP, REPEATS = 2, 7
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
    before = tfs.metrics.snapshot()
    out = df.dropDuplicates(["k"])
    sizes = [b.nrows for _, b in sorted(out.local_blocks().items())]
    after = tfs.metrics.snapshot()
    moved = {m: int(after.get(m, 0) - before.get(m, 0)) for m in ("distinct_rows_in", "distinct_rows_exchanged",
                                                                   "distinct_rows_kept", "distinct_device_partitions")}
    distinct = timed(lambda: df.dropDuplicates(["k"]).local_blocks())
    order = timed(lambda: df.orderBy("k").local_blocks())
    count = timed(lambda: df.groupBy("k").count().local_blocks())
    print(json.dumps({"case": f"{label}: frame", "dropDuplicates_ms": distinct, "orderBy_ms": order,
                      "groupBy_count_ms": count, "dropDuplicates_over_orderBy": round(distinct["ms"] / order["ms"], 3),
                      "dropDuplicates_over_groupBy_count": round(distinct["ms"] / count["ms"], 3),
                      **moved, "partition_rows": sizes}), flush=True)


def phase_case(label, keys, x):
    """Where a dropDuplicates call spends its time against orderBy, per
    partition-level step (host clock around a device synchronise; one of the 4
    partitions, then what one output partition receives)."""
    from tensorframes_amd.frame.block import concat_blocks
    from tensorframes_amd.frame.dataframe import _lower_bounds, _sort_block, _sort_order_of
    from tensorframes_amd.frame.setops import _distinct_block, _heads, _words_of_rows
    df = tfs.from_columns({"k": keys, "x": x}, num_partitions=PARTS).cache_on_device(dev)
    blocks = df.local_blocks()
    names = ["k", "x"]
    b0 = blocks[0]
    words, perm, _ = _sort_order_of(b0, ["k"], [False])
    kept = _heads(words, perm)
    first = {
        "rows": b0.nrows,
        "encode_argsort_ms": timed(lambda: _sort_order_of(b0, ["k"], [False]))["ms"],
        "unique_rows_ms": timed(lambda: _heads(words, perm))["ms"],
        "gather_kept_words_ms": timed(lambda: _words_of_rows(words, kept))["ms"],
        "distinct_block_ms": timed(lambda: _distinct_block(b0, names, ["k"]))["ms"],    # (the three above + the row gather)
        "orderBy_sort_block_ms": timed(lambda: _sort_block(b0, ["k"], [False], [0, 0]))["ms"],
    }
    surv = {p: _distinct_block(blocks[p], names, ["k"]) for p in sorted(blocks)}
    # what output partition 0 receives: the lowest quarter of every partition's sorted rows
    got_d = concat_blocks([surv[p][0].slice(0, surv[p][0].nrows // PARTS) for p in sorted(surv)], names).to(dev)
    srt = {p: _sort_block(blocks[p], ["k"], [False], [0, 0])[0] for p in sorted(blocks)}
    got_o = concat_blocks([srt[p].slice(0, srt[p].nrows // PARTS) for p in sorted(srt)], names).to(dev)
    sw = surv[0][1]
    m = int(sw.shape[1])
    ident = torch.arange(m, dtype=torch.int64, device=dev)
    sp = sw[:, [m // 4, m // 2, 3 * m // 4]].cpu().numpy().view(np.uint64).T
    second = {
        "received_rows_dropDuplicates": got_d.nrows, "received_rows_orderBy": got_o.nrows,
        "distinct_block_ms": timed(lambda: _distinct_block(got_d, names, ["k"]))["ms"],
        "orderBy_sort_block_ms": timed(lambda: _sort_block(got_o, ["k"], [False], [0, 0]))["ms"],
        "cut_survivors_at_splitters_ms": timed(lambda: _lower_bounds(sw, ident, sp))["ms"],
        "cut_sorted_partition_at_splitters_ms": timed(lambda: _lower_bounds(words, perm, sp))["ms"],
    }
    print(json.dumps({"case": f"{label}: steps of one partition", "before_the_exchange": first,
                      "after_the_exchange": second}), flush=True)


def kernel_case(label, keys):
    n = keys.shape[0]
    words = _C.sort_encode([keys], [False])
    perm = _C.sort_argsort(words)
    (ks,) = _C.permute_rows(perm, [keys])
    sw = _C.sort_encode([ks], [False])
    t_sort, _ = events(lambda: _C.sort_argsort(_C.sort_encode([keys], [False])))
    t_sorted, kept = events(lambda: _C.unique_rows(sw, None))
    t_perm, kept_p = events(lambda: _C.unique_rows(words, perm))
    m = int(kept.shape[0])
    assert int(kept_p.shape[0]) == m
    mask = torch.zeros(n, dtype=torch.bool, device=dev)
    mask[kept] = True                                             # the same rows kept: the same density
    col = torch.arange(n, dtype=torch.int64, device=dev)
    t_compact, got = events(lambda: _C.compact_rows(mask, [col], False))
    assert int(got[1]) == m
    t_take, _ = events(lambda: _C.take_rows(kept_p, [keys]))
    unique_bytes = 8 * n + 2 * (n // 8) + 2 * 8 * m
    unique_perm_bytes = unique_bytes + 8 * n                      # the order as well
    compact_bytes = 2 * n + 2 * 8 * m
    print(json.dumps({"case": f"{label}: kernels, one partition of {n} rows", "tile_rows": int(_C.unique_tile_rows()),
                      "kept_rows": m, "encode_argsort_ms": t_sort,
                      "unique_rows_sorted_ms": t_sorted, "unique_rows_sorted_GBps": round(unique_bytes / t_sorted / 1e6, 1),
                      "unique_rows_through_perm_ms": t_perm,
                      "unique_rows_through_perm_GBps": round(unique_perm_bytes / t_perm / 1e6, 1),
                      "compact_rows_int64_ms": t_compact, "compact_rows_GBps": round(compact_bytes / t_compact / 1e6, 1),
                      "take_rows_of_the_kept_keys_ms": t_take}), flush=True)


def main():
    g = torch.Generator(device=dev).manual_seed(5)
    keys = torch.randint(0, NK, (N,), device=dev, generator=g, dtype=torch.int32)
    every = torch.randperm(N, device=dev, generator=g).to(torch.int32)
    x = torch.rand(N, device=dev, generator=g, dtype=torch.float32)
    frame_case("100k distinct keys", keys, x)
    frame_case("every key distinct", every, x)
    phase_case("100k distinct keys", keys, x)
    phase_case("every key distinct", every, x)
    kernel_case("100k distinct keys", keys)
    kernel_case("every key distinct", every)


if __name__ == "__main__":
    main()
