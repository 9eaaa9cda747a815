"""describe / approxQuantile on a 10 M-row device-cached frame (an f32 score, an
int32 key in [0, 1000) and six more f32 feature columns) against what a user
would otherwise write:

* `torch.std_mean` + `torch.aminmax` per column, the four numbers read back;
* `torch.sort` of the score column and three reads of the sorted values;
* this project's `orderBy("score")` of the whole frame (the route the parent
  commit offers for a median).

Also the two kernels alone (`_C.column_moments`, `_C.select_hist` on the score
column, device events) with their read rates. Every variant is warmed; the
variants alternate round after round in one process until each has at least
`--window-s` seconds of samples (and five repeats); the median is reported
with the fastest and slowest repeat as the spread. Frame calls end in a D2H
of their result, so they are timed with the host clock around a device
synchronise. Prints one JSON line per variant and a markdown table. Needs a
GPU.

    python scripts/stats_profile.py              # 10 M rows
    python scripts/stats_profile.py --rows 1000000
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def host_timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def event_timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--window-s", type=float, default=1.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("stats_profile: needs a GPU")
    import tensorframes_amd as tfs
    from tensorframes_amd._native import _C
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n = args.rows
    g = torch.Generator(device=dev).manual_seed(11)
    cols = {"score": torch.randn(n, device=dev, generator=g),
            "key": torch.randint(0, 1000, (n,), device=dev, generator=g).to(torch.int32)}
    for j in range(6):
        cols[f"f{j}"] = torch.randn(n, device=dev, generator=g) + float(j)
    df = tfs.from_columns(cols, num_partitions=1).cache_on_device(dev)
    score = cols["score"]
    probs = [0.25, 0.5, 0.75]
    pos = torch.tensor([max(math.ceil(p * n) - 1, 0) for p in probs], device=dev)
    zero = torch.zeros(1, dtype=torch.int64)

    def torch_moments(ts):
        out = []
        for t in ts:
            sd, mean = torch.std_mean(t.double() if t.dtype != torch.float32 else t)
            lo, hi = torch.aminmax(t)
            out.append(torch.stack([sd.double(), mean.double(), lo.double(), hi.double()]))
        return torch.stack(out).cpu()

    variants = {
        "describe(score): 1 column": (host_timed, lambda: df.describe("score").local_blocks()),
        "describe(): 8 columns": (host_timed, lambda: df.describe().local_blocks()),
        "approxQuantile(score, 3 probabilities)": (host_timed, lambda: df.approxQuantile("score", probs, 0.0)),
        "torch.std_mean + aminmax: 1 column": (host_timed, lambda: torch_moments([score])),
        "torch.std_mean + aminmax: 8 columns": (host_timed, lambda: torch_moments(list(cols.values()))),
        "torch.sort(score) + 3 reads": (host_timed, lambda: torch.sort(score).values[pos].cpu()),
        "orderBy(score) of the frame (8 columns)": (host_timed, lambda: df.orderBy("score").local_blocks()),
        "kernel: column_moments(score)": (event_timed, lambda: _C.column_moments([score])),
        "kernel: column_moments(8 columns)": (event_timed, lambda: _C.column_moments(list(cols.values()))),
        "kernel: select_hist(score, 1 prefix)": (event_timed, lambda: _C.select_hist(score, zero, 0)),
    }
    # the answers agree before anything is timed
    q = df.approxQuantile("score", probs, 0.0)
    want = torch.sort(score).values[pos].cpu().tolist()
    assert q == [float(v) for v in want], (q, want)
    d = df.describe("score")
    got = dict(zip(d.to_numpy("summary").tolist(), d.to_numpy("score").tolist()))
    ref = torch_moments([score])[0].tolist()
    assert abs(got["stddev"] - ref[0]) <= 1e-4 * ref[0] and got["min"] == ref[2] and got["max"] == ref[3], (got, ref)
    before = tfs.metrics.snapshot().get("quantile_passes", 0)
    df.approxQuantile("score", probs, 0.0)
    passes = int(tfs.metrics.snapshot().get("quantile_passes", 0) - before)

    for _ in range(2):  # warm every variant at this shape
        for timer, fn in variants.values():
            timer(fn)
    t = {k: [] for k in variants}

    def wanted(v):  # a window of samples, five repeats at least, 200 at most (the kernels alone are short)
        return len(v) < 5 or (sum(v) < args.window_s * 1e3 and len(v) < 200)
    while any(wanted(v) for v in t.values()):
        for k, (timer, fn) in variants.items():
            if wanted(t[k]):
                ms, out = timer(fn)
                t[k].append(ms)
                del out
    read_bytes = {"kernel: column_moments(score)": n * 4, "kernel: column_moments(8 columns)": n * 4 * 8,
                  "kernel: select_hist(score, 1 prefix)": n * 4}
    recs = []
    for k, v in t.items():
        rec = {"variant": k, "rows": n, "repeats": len(v), "median_ms": round(statistics.median(v), 4),
               "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
        if k in read_bytes:
            rec["read_gbs"] = round(read_bytes[k] / statistics.median(v) / 1e6, 1)
        if k.startswith("approxQuantile"):
            rec["quantile_passes"] = passes
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    print("\n| variant | median ms | fastest .. slowest ms | repeats | read GB/s |")
    print("|---|---|---|---|---|")
    for r in recs:
        print(f"| {r['variant']} | {r['median_ms']:.3f} | {r['min_ms']:.3f} .. {r['max_ms']:.3f} | {r['repeats']} | "
              f"{r.get('read_gbs', '')} |")


if __name__ == "__main__":
    main()
