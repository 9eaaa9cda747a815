"""`_C.logreg_step` on 10M x 64 and 2M x 512 f32, binomial and K = 10, next to
two yardsticks in the same process on the same column: the same evaluation
written with torch ops on the device (f64 matmul, logsumexp, matmul), and the
project's column Sum (`reduce_blocks` of `reduce_sum(x, [0])` on the column as a
device-cached frame of PARTS partitions), whose time taken twice is the cost of
reading the column twice. Then a whole `LogisticRegression.fit` of 20
iterations over PARTS partitions. Prints one JSON line per measurement.

Run once, without arguments: every case runs in a child process of its own
under `timeout`, and nothing more is started after a child that did not end
cleanly.
  --case i   device events around windows of CALLS calls, the median window of
             REPEATS after WARMUP, per call, with the fastest and the slowest;
             the frame calls under a host clock (they end in a device-to-host
             copy). Bytes are what the step has to move, computed from the
             shapes: x twice, q [n, R] f64 written and read once."""
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

WARMUP, REPEATS, CALLS, PARTS, FIT_ITERS = 2, 7, 5, 4, 20
CASES = [(10_000_000, 64, 0), (10_000_000, 64, 10), (2_000_000, 512, 0), (2_000_000, 512, 10)]  # K = 0: binomial


def spread(ms):
    return {"ms": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def case(i):
    import numpy as np
    import torch

    import tensorframes_amd as tfs
    from tensorframes_amd import tf
    from tensorframes_amd._native import _C
    from tensorframes_amd.ml.classification import LogisticRegression
    n, d, k = CASES[i]
    r, classes = (k, k) if k else (1, 2)
    gen = torch.Generator(device="cuda:0").manual_seed(2)
    x = torch.empty((n, d), dtype=torch.float32, device="cuda:0").normal_(generator=gen)
    y = torch.randint(0, classes, (n,), dtype=torch.int32, device="cuda:0", generator=gen)
    rng = np.random.default_rng(2)
    coef = torch.from_numpy(rng.standard_normal((r, d)) / np.sqrt(d)).to("cuda:0")
    icpt = torch.from_numpy(rng.standard_normal(r)).to("cuda:0")
    shape = f"{n} x {d} float32, {'binomial' if not k else f'K={k}'}"
    two_reads = 2 * n * d * 4
    step_bytes = two_reads + 2 * n * r * 8 + n * 4

    def events(fn):
        for _ in range(WARMUP):
            fn()
        ms = []
        for _ in range(REPEATS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(CALLS):
                fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b) / CALLS)
        return spread(ms)

    def clock(fn):
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

    def torch_eval():
        xd = x.double()
        m = xd @ coef.T + icpt
        if not k:
            m = torch.cat([torch.zeros_like(m), m], 1)
        lse = torch.logsumexp(m, 1)
        loss = (lse - m.gather(1, y.long()[:, None])[:, 0]).sum()
        q = torch.exp(m - lse[:, None])
        q.scatter_add_(1, y.long()[:, None], torch.full((n, 1), -1.0, dtype=torch.float64, device=x.device))
        q = q[:, -r:]
        return loss, q.T @ xd, q.sum(0)

    res = events(lambda: _C.logreg_step(x, y, None, coef, icpt, not k))
    print(json.dumps({"case": f"{shape}: _C.logreg_step, one call (device events, per call)", **res,
                      "moved_MB": round(step_bytes / 1e6, 1),
                      "moved_TBps": round(step_bytes / (res["ms"] * 1e-3) / 1e12, 3)}), flush=True)
    print(json.dumps({"case": f"{shape}: the evaluation in torch ops, f64 (device events, per call)",
                      **events(torch_eval)}), flush=True)
    df = tfs.from_columns({"features": x, "label": y}, num_partitions=PARTS).cache_on_device("cuda:0")

    def column_sum():
        with tf.Graph().as_default():
            xi = tf.placeholder(tf.float32, shape=[None, d], name="features_input")
            return tfs.reduce_blocks(tf.reduce_sum(xi, [0], name="features"), df)

    s = clock(column_sum)
    print(json.dumps({"case": f"{shape}: reduce_blocks column Sum, {PARTS} partitions, one read (host clock)", **s,
                      "two_reads_ms": round(2 * s["ms"], 3),
                      "step_over_two_reads": round(res["ms"] / (2 * s["ms"]), 3)}),
          flush=True)
    est = LogisticRegression(maxIter=FIT_ITERS, regParam=0.01, tol=0.0)
    t0 = time.perf_counter()
    model = est.fit(df)
    torch.cuda.synchronize()
    print(json.dumps({"case": f"{shape}: LogisticRegression.fit, {PARTS} partitions, end to end (host clock, one run)",
                      "ms": round((time.perf_counter() - t0) * 1e3, 1), "iterations": model.summary.totalIterations,
                      "objective": [round(model.summary.objectiveHistory[0], 6),
                                    round(model.summary.objectiveHistory[-1], 6)]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", type=int)
    a = ap.parse_args()
    if a.case is not None:
        return case(a.case)
    for i in range(len(CASES)):
        cmd = ["timeout", "-k", "10", "280", sys.executable, os.path.abspath(__file__), "--case", str(i)]
        r = subprocess.run(cmd, cwd=REPO)
        if r.returncode != 0:  # (a device fault can surface as a plain Python error: any failure ends the run)
            raise SystemExit(f"--case {i} ended with status {r.returncode}: nothing more is started")


if __name__ == "__main__":
    main()
