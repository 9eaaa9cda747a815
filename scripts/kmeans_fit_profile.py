"""`_C.kmeans_step` on 100k x 100 f64, k = 10 (the shape of the K-Means
benchmark configuration) and on 10M x 64 f32, k = 64, next to one iteration of
the graph path `models.kmeans.run_one_step2` on the same device-cached frame in
the same process, as the baseline. Prints one JSON line per measurement.

Run once, without arguments: every case runs in a child process of its own
under `timeout`, and nothing more is started after a child that did not end
cleanly.
  --case i   device events around windows of CALLS calls of `_C.kmeans_step` of
             the whole column (four launches, the shift on the host, the pool
             allocations): the median window of REPEATS after WARMUP, per call,
             with the fastest and the slowest, and the bytes the step has to
             move (x twice per centre tile, the assignment and the distances
             once each way). Then, on a frame of PARTS partitions, a host clock
             around one iteration of `KMeans.fit` and around `run_one_step2`
             (both end in a device-to-host copy). The graph path takes float64
             points only, so the f32 case has no baseline; its bytes are those
             of its [n, k] f64 distance matrix written and read once, on top of
             x read three times."""
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

WARMUP, REPEATS, CALLS, PARTS = 2, 7, 10, 4
CASES = [(100_000, 100, 10, "float64"), (10_000_000, 64, 64, "float32")]


def spread(ms):
    return {"ms": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def case(i):
    import numpy as np
    import torch

    import tensorframes_amd as tfs
    from tensorframes_amd._native import _C
    from tensorframes_amd.ml.clustering import KMeans
    from tensorframes_amd.models import kmeans
    n, d, k, dtype = CASES[i]
    tdtype = getattr(torch, dtype)
    x = torch.empty((n, d), dtype=tdtype, device="cuda:0")
    x.uniform_(0.0, 1.0, generator=torch.Generator(device="cuda:0").manual_seed(2))
    c0 = np.random.default_rng(2).standard_normal((k, d))
    cdev = torch.from_numpy(c0).to("cuda:0")
    shape = f"{n} x {d} {dtype}, k={k}"
    ctiles = -(-k // 64)
    step_bytes = n * d * x.element_size() * (ctiles + ctiles) + n * (4 + 8) + n * 4 * ctiles * -(-d // 64)
    graph_bytes = 3 * n * d * 8 + 2 * n * k * 8

    for _ in range(WARMUP):
        _C.kmeans_step(x, cdev)
    ms = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            _C.kmeans_step(x, cdev)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / CALLS)
    res = spread(ms)
    print(json.dumps({"case": f"{shape}: _C.kmeans_step, one call (device events, per call)", **res,
                      "moved_MB": round(step_bytes / 1e6, 1),
                      "moved_TBps": round(step_bytes / (res["ms"] * 1e-3) / 1e12, 3)}), flush=True)

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

    df = tfs.from_columns({"features": x}, num_partitions=PARTS).cache_on_device("cuda:0")
    est = KMeans(k=k, maxIter=1).setInitialCenters(c0)
    print(json.dumps({"case": f"{shape}: KMeans.fit, one iteration, {PARTS} partitions, end to end (host clock)",
                      **timed(lambda: est.fit(df)), "moved_MB": round(step_bytes / 1e6, 1)}), flush=True)
    if dtype == "float64":
        print(json.dumps({"case": f"{shape}: models.kmeans.run_one_step2, {PARTS} partitions, end to end (host clock)",
                          **timed(lambda: kmeans.run_one_step2(df, c0)), "moved_MB": round(graph_bytes / 1e6, 1)}),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", type=int)
    a = ap.parse_args()
    if a.case is not None:
        return case(a.case)
    for i in range(len(CASES)):
        cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--case", str(i)]
        r = subprocess.run(cmd, cwd=REPO)
        if r.returncode != 0:  # (a device fault can surface as a plain Python error: any failure ends the run)
            raise SystemExit(f"--case {i} ended with status {r.returncode}: nothing more is started")


if __name__ == "__main__":
    main()
