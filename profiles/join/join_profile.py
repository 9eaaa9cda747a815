"""Times DataFrame.join's device path against a torch baseline on one GPU.

    python profiles/join/join_profile.py [log file]

Stages of the new path: (a) _C.join_probe, (b) _C.join_expand (scan, the one
synchronisation that reads the total, expand), (c) _C.take_rows of the right
payload, (d) the whole inner join of two device-resident frames (build side
sorted inside). The baseline is what a user would write with torch on a single
int64 key: torch.sort of the right key, torch.searchsorted left / right,
repeat_interleave plus index arithmetic, one index_select per column.

Every series is warmed up, timed with device events around each repetition
and reported as the median; the baseline is measured twice (the difference of
the two is the run-to-run spread)."""
import os
import statistics
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.getcwd(), os.path.dirname(os.path.dirname(HERE))):
    if os.path.isdir(os.path.join(p, "tensorframes_amd")) and p not in sys.path:
        sys.path.insert(0, p)

import tensorframes_amd as tfs  # noqa: E402
from tensorframes_amd._native import _C  # noqa: E402

DEV = "cuda:0"


def timed(fn, min_reps=10, min_seconds=0.5, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms, t0 = [], time.perf_counter()
    while len(ms) < min_reps or time.perf_counter() - t0 < min_seconds:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
        if len(ms) >= 200:
            break
    return statistics.median(ms), len(ms)


def shape(name, n, keys, per_key, seed):
    rng = np.random.default_rng(seed)
    rk = np.repeat(np.arange(keys, dtype=np.int64), per_key)
    rng.shuffle(rk)
    m = len(rk)
    lk = rng.integers(0, keys, n).astype(np.int64)
    left = {"k": torch.from_numpy(lk), "i": torch.arange(n, dtype=torch.int64)}
    right = {"k": torch.from_numpy(rk), "j": torch.arange(m, dtype=torch.int64),
             "v": torch.from_numpy(rng.standard_normal((m, 17)).astype(np.float32))}      # 8 + 68 = 76 B payload rows
    return name, left, right


def run(name, left, right, out):
    n, m = left["k"].shape[0], right["k"].shape[0]
    L = {c: t.to(DEV) for c, t in left.items()}
    R = {c: t.to(DEV) for c, t in right.items()}
    payload = [R["j"], R["v"]]
    # ---- new path, stage by stage
    rw = _C.sort_encode([R["k"]], [False])
    perm = _C.sort_argsort(rw)
    sw = _C.join_gather_words(rw, perm)
    lw = _C.sort_encode([L["k"]], [False])
    lo, cnt, _ = _C.join_probe(lw, sw, 0)
    li, ri, _ = _C.join_expand(lo, cnt, perm)
    total = li.shape[0]
    res = {}
    res["a join_probe"] = timed(lambda: _C.join_probe(lw, sw, 0))
    res["b join_expand"] = timed(lambda: _C.join_expand(lo, cnt, perm))
    res["c take_rows"] = timed(lambda: _C.take_rows(ri, payload))
    lf = tfs.from_columns(L, num_partitions=1).cache_on_device(DEV)
    rf = tfs.from_columns(R, num_partitions=1).cache_on_device(DEV)
    res["d inner join"] = timed(lambda: lf.join(rf, "k").local_blocks(), min_reps=5)

    # ---- torch baseline
    def t_sort():
        return torch.sort(R["k"], stable=True)

    srt, tperm = t_sort()

    def t_probe():
        a = torch.searchsorted(srt, L["k"], right=False)
        return a, torch.searchsorted(srt, L["k"], right=True) - a

    tlo, tcnt = t_probe()

    def t_expand():
        offs = torch.cumsum(tcnt, 0) - tcnt
        rows = torch.repeat_interleave(torch.arange(n, device=DEV), tcnt)
        pos = tlo[rows] + (torch.arange(rows.shape[0], device=DEV) - offs[rows])
        return rows, tperm[pos]

    tli, tri = t_expand()

    def t_take():
        return [c.index_select(0, tri) for c in payload]

    def t_whole():
        nonlocal srt, tperm, tlo, tcnt
        srt, tperm = t_sort()
        tlo, tcnt = t_probe()
        rows, rr = t_expand()
        return [c.index_select(0, rows) for c in (L["k"], L["i"])] + [c.index_select(0, rr) for c in payload]

    assert torch.equal(tli, li) and torch.equal(tri, ri)            # the same rows in the same order
    for rep in (1, 2):
        res[f"a torch searchsorted x2 #{rep}"] = timed(t_probe)
        res[f"b torch repeat_interleave + index #{rep}"] = timed(t_expand)
        res[f"c torch index_select per column #{rep}"] = timed(t_take)
        res[f"d torch whole #{rep}"] = timed(t_whole, min_reps=5)
    out.write(f"## {name}: {n} left rows, {m} right rows, {total} output rows\n")
    for k in sorted(res):
        out.write(f"{k:48s} {res[k][0]:10.3f} ms   (median of {res[k][1]})\n")
    out.flush()


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "join_profile.log")
    with open(path, "w") as out:
        out.write(f"device: {torch.cuda.get_device_name(0)}; join tile {_C.join_tile_rows()} rows\n")
        run(*shape("foreign key", 10_000_000, 1_000_000, 1, 0), out)
        run(*shape("duplicates", 1_000_000, 100_000, 4, 1), out)
    print(open(path).read())


if __name__ == "__main__":
    main()
