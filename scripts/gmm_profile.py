"""`_C.gmm_step` on 10M x 16 f32, k = 8 and on 2M x 64 f32, k = 16, next to two
yardsticks in the same process on the same column, neither of them the code
under test: the same EM step written with torch ops on the device (per
component an f64 matmul for z, `logsumexp`, and a weighted Gram by matmul), and
a floor, the larger of one read of the column at the rate of the project's
column Sum (`reduce_blocks` of `reduce_sum(x, [0])` on the column as a
device-cached frame of PARTS partitions, host clock) and 4 n k d^2 flops at
GEMM_TF, the rate docs/PERFORMANCE.md records for the project's own f64 GEMM.
Prints one JSON line per measurement.

Run once, without arguments: every case runs in a child process of its own
under `timeout`, and nothing more is started after a child that did not end
cleanly."""
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

WARMUP, REPEATS, CALLS, PARTS = 2, 7, 5, 4
GEMM_TF = 65.2  # docs/PERFORMANCE.md, round 4: f64 GEMM 10M x 512 x 512
CASES = [(10_000_000, 16, 8), (2_000_000, 64, 16)]


def spread(ms):
    return {"ms": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def case(i):
    import numpy as np
    import torch

    import tensorframes_amd as tfs
    from tensorframes_amd import tf
    from tensorframes_amd._native import _C
    from tensorframes_amd.ml.clustering import _gmm_params
    n, d, k = CASES[i]
    gen = torch.Generator(device="cuda:0").manual_seed(2)
    x = torch.empty((n, d), dtype=torch.float32, device="cuda:0").normal_(generator=gen)
    rng = np.random.default_rng(2)
    means = rng.standard_normal((k, d))
    w = rng.standard_normal((k, d, d))
    covs = w @ w.transpose(0, 2, 1) / d + np.eye(d)
    transforms, logconst = _gmm_params(np.full(k, 1.0 / k), covs, "gmm_profile", 0)
    mu, tr, lc = [torch.from_numpy(a).to("cuda:0") for a in (means, transforms, logconst)]
    shape = f"{n} x {d} float32, k={k}"

    def events(fn, calls=CALLS):
        for _ in range(WARMUP):
            fn()
        ms = []
        for _ in range(REPEATS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b) / calls)
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

    def torch_step():
        xd = x.double()
        logp = torch.empty((n, k), dtype=torch.float64, device=x.device)
        for j in range(k):
            z = (xd - mu[j]) @ tr[j].T
            logp[:, j] = lc[j] - 0.5 * (z * z).sum(1)
        lse = torch.logsumexp(logp, 1)
        r = torch.exp(logp - lse[:, None])
        S, C = [], []
        for j in range(k):
            xc = xd - mu[j]
            S.append(r[:, j] @ xc)
            C.append((xc * r[:, j, None]).T @ xc)
        return r.sum(0), torch.stack(S), torch.stack(C), lse.sum()

    res = events(lambda: _C.gmm_step(x, mu, tr, lc))
    flops = 4.0 * n * k * d * d
    print(json.dumps({"case": f"{shape}: _C.gmm_step, one call (device events, per call)", **res,
                      "TF_of_4nkd2": round(flops / (res["ms"] * 1e-3) / 1e12, 2)}), flush=True)
    pred = events(lambda: _C.gmm_predict(x, mu, tr, lc))
    print(json.dumps({"case": f"{shape}: _C.gmm_predict, the E step alone (device events, per call)", **pred}),
          flush=True)
    t = events(torch_step, 1)
    print(json.dumps({"case": f"{shape}: the EM step in torch ops, f64 (device events, per call)", **t,
                      "torch_over_step": round(t["ms"] / res["ms"], 2)}), flush=True)
    df = tfs.from_columns({"features": x}, num_partitions=PARTS).cache_on_device("cuda:0")

    def column_sum():
        with tf.Graph().as_default():
            xi = tf.placeholder(tf.float32, shape=[None, d], name="features_input")
            return tfs.reduce_blocks(tf.reduce_sum(xi, [0], name="features"), df)

    s = clock(column_sum)
    gemm_ms = flops / (GEMM_TF * 1e12) * 1e3
    floor = max(s["ms"], gemm_ms)
    print(json.dumps({"case": f"{shape}: floor = max(column Sum, {PARTS} partitions, one read (host clock); 4 n k d^2 "
                              f"flops at {GEMM_TF} TF)", "sum": s, "gemm_ms": round(gemm_ms, 3),
                      "floor_ms": round(floor, 3), "step_over_floor": round(res["ms"] / floor, 2)}), flush=True)


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
