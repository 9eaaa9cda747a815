"""Correlation.corr of a vector column on a device-cached frame of 10M rows x
f32 in 4 partitions, d = 16, 128, 512, next to the route that existed before
it on the same frame in the same run: the f64 cast and centring, then
MatMul(transpose_a=True) on gemm_f64.hip, through map_blocks(trim=True), one
[d, d] Gram per partition. Prints one JSON line per case.

Run once, without arguments: every d runs in two child processes, each under
its own `timeout`, and nothing more is started after a child that did not end
cleanly.
  --case d   hipEvents around `_C.vector_moments` of the whole column (three
             launches and the pool allocations), a host clock around
             `Correlation.corr(...)` and around the GEMM route (both end in a
             device-to-host copy): the median of REPEATS calls after WARMUP,
             with the fastest and the slowest; and the largest difference
             between the two covariance matrices, relative to sqrt(C_ii C_jj).
  --trace d  under `rocprofv3 --kernel-trace`, in a run of its own: the three
             launches by kernel name, the median of REPEATS dispatches; the
             bytes of the column over the SYRK launch's time."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

WARMUP, REPEATS = 2, 7
N, PARTS, DIMS = 10_000_000, 4, (16, 128, 512)


def spread(ms):
    return {"ms": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def column(d):
    import torch
    x = torch.empty((N, d), dtype=torch.float32, device="cuda:0")
    x.normal_(1e4, 1.0, generator=torch.Generator(device="cuda:0").manual_seed(5))
    return x


def case(d):
    import numpy as np
    import torch

    import tensorframes_amd as tfs
    from tensorframes_amd import tf
    from tensorframes_amd._native import _C
    from tensorframes_amd.ml.stat import Correlation
    x = column(d)

    def timed(fn):
        out = None
        for _ in range(WARMUP):
            out = fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return spread(ms), out

    def events(fn):
        for _ in range(WARMUP):
            fn()
        ms = []
        for _ in range(REPEATS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return spread(ms)

    print(json.dumps({"case": f"d={d}: _C.vector_moments, 10M rows in one call (hipEvents)",
                      **events(lambda: _C.vector_moments(x))}), flush=True)
    df = tfs.from_columns({"y": x}, num_partitions=PARTS).cache_on_device("cuda:0")
    res, _ = timed(lambda: Correlation.corr(df, "y").to_numpy("pearson(y)"))
    print(json.dumps({"case": f"d={d}: Correlation.corr, {PARTS} partitions, end to end", **res}), flush=True)
    _, cov = timed(lambda: Correlation.cov(df, "y").to_numpy("cov(y)")[0])
    mean = _C.vector_moments(x)[0].cpu().numpy()

    def gemm_route():
        with tf.Graph().as_default():
            xc = tf.cast(tfs.block(df, "y"), tf.float64) - tf.constant(mean)
            g = tf.matmul(xc, xc, transpose_a=True, name="g")
            return tfs.map_blocks(g, df, trim=True).to_numpy("g")
    res, parts = timed(gemm_route)
    old = parts.reshape(PARTS, d, d).sum(0) / (N - 1)
    scale = np.sqrt(np.outer(np.diagonal(cov), np.diagonal(cov)))
    print(json.dumps({"case": f"d={d}: cast + centre + MatMul(transpose_a) on gemm_f64, {PARTS} partitions, given the "
                              f"mean", **res, "max_rel_difference_of_cov": float(np.abs(old - cov).max() / scale.max())}),
          flush=True)


def trace(d):
    from tensorframes_amd._native import _C
    import torch
    x = column(d)
    for _ in range(WARMUP + REPEATS):
        _C.vector_moments(x)
    torch.cuda.synchronize()


def trace_summary(d, out_dir):
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel trace under {out_dir}")
    with open(files[0], newline="") as f:
        rows = list(csv.DictReader(f))
    key = {k.lower(): k for k in rows[0]}
    name, t0, t1 = key["kernel_name"], key["start_timestamp"], key["end_timestamp"]
    out = {"case": f"d={d}: the three launches, 10M rows in one call (kernel trace)"}
    for kern in ("vm_means", "vm_syrk", "vm_finish"):
        ns = [int(r[t1]) - int(r[t0]) for r in rows if kern in r[name]][WARMUP:]
        out[kern] = spread([v / 1e6 for v in ns])
    out["column_MB"] = round(N * d * 4 / 1e6, 1)
    out["syrk_column_TBps"] = round(N * d * 4 / (out["vm_syrk"]["ms"] * 1e-3) / 1e12, 3)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", type=int)
    ap.add_argument("--trace", type=int)
    ap.add_argument("--out", help="where the kernel traces go (default: a temporary directory)")
    a = ap.parse_args()
    if a.case:
        return case(a.case)
    if a.trace:
        return trace(a.trace)
    me = [sys.executable, os.path.abspath(__file__)]
    out = a.out or tempfile.mkdtemp(prefix="vector_moments_trace_")
    for d in DIMS:
        out_dir = os.path.join(out, f"d{d}")
        for cmd in (["timeout", "-k", "10", "400", *me, "--case", str(d)],
                    ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", out_dir,
                     "--", *me, "--trace", str(d)]):
            traced = "rocprofv3" in cmd
            r = subprocess.run(cmd, cwd=REPO, stdout=subprocess.DEVNULL if traced else None)
            if r.returncode != 0:  # (a device fault can surface as a plain Python error: any failure ends the run)
                raise SystemExit(f"{' '.join(cmd[4:])} ended with status {r.returncode}: nothing more is started")
            if traced:
                trace_summary(d, out_dir)


if __name__ == "__main__":
    main()
