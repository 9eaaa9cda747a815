"""`_C.vector_summary` on 10M rows x f32, d = 16, 64, 512, next to the
project's own column Sum (`reduce_blocks` of `reduce_sum(x, [0])`) on the same
device-cached frame in the same process, as the yardstick: the summary reads
every element once and leaves ten metrics, the Sum reads it once and leaves
one. Prints one JSON line per measurement.

Run once, without arguments: every d runs in a child process of its own under
`timeout`, and nothing more is started after a child that did not end cleanly.
  --case d   device events around windows of CALLS calls of `_C.vector_summary`
             of the whole column (two launches and the pool allocations each):
             the median window of REPEATS after WARMUP, per call, with the
             fastest and the slowest, and the bytes of the column over that
             time; then a host clock around `reduce_blocks` (it ends in a
             device-to-host copy) and around `Summarizer` end to end, both on
             the frame of PARTS partitions."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

WARMUP, REPEATS, CALLS = 2, 7, 10
N, PARTS, DIMS = 10_000_000, 4, (16, 64, 512)


def spread(ms):
    return {"ms": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def case(d):
    import torch

    import tensorframes_amd as tfs
    from tensorframes_amd import tf
    from tensorframes_amd._native import _C
    from tensorframes_amd.ml.stat import Summarizer
    x = torch.empty((N, d), dtype=torch.float32, device="cuda:0")
    x.normal_(1e4, 1.0, generator=torch.Generator(device="cuda:0").manual_seed(5))
    nbytes = N * d * 4

    for _ in range(WARMUP):
        _C.vector_summary(x)
    ms = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            _C.vector_summary(x)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / CALLS)
    res = spread(ms)
    print(json.dumps({"case": f"d={d}: _C.vector_summary, 10M rows in one call (device events, per call)", **res,
                      "column_MB": round(nbytes / 1e6, 1), "column_TBps": round(nbytes / (res["ms"] * 1e-3) / 1e12, 3)}),
          flush=True)

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

    df = tfs.from_columns({"y": x}, num_partitions=PARTS).cache_on_device("cuda:0")

    def column_sum():
        with tf.Graph().as_default():
            xi = tf.placeholder(tf.float32, shape=[None, d], name="y_input")
            return tfs.reduce_blocks(tf.reduce_sum(xi, [0], name="y"), df)
    res = timed(column_sum)
    print(json.dumps({"case": f"d={d}: reduce_blocks(reduce_sum(y, [0])), {PARTS} partitions, end to end (host clock)",
                      **res, "column_TBps": round(nbytes / (res["ms"] * 1e-3) / 1e12, 3)}), flush=True)
    expr = Summarizer.metrics("mean", "variance", "min", "max", "normL2", "count").summary("y")
    res = timed(lambda: df.select(expr).collect())
    print(json.dumps({"case": f"d={d}: Summarizer, six metrics, {PARTS} partitions, end to end (host clock)", **res,
                      "column_TBps": round(nbytes / (res["ms"] * 1e-3) / 1e12, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", type=int)
    a = ap.parse_args()
    if a.case:
        return case(a.case)
    for d in DIMS:
        cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--case", str(d)]
        r = subprocess.run(cmd, cwd=REPO)
        if r.returncode != 0:  # (a device fault can surface as a plain Python error: any failure ends the run)
            raise SystemExit(f"--case {d} ended with status {r.returncode}: nothing more is started")


if __name__ == "__main__":
    main()
