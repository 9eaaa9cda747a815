"""Row compaction of device-resident columns (DataFrame.filter's device path,
`_C.compact_rows`) against what dropping rows cost before it existed:
`torch.nonzero(mask)` plus one `index_select` per column (block.col_take).

Two partitions -- 10 M rows of (f32, i64, f32[16]) and 2.5 M rows of f32[512]
-- at 1 %, 50 % and 99 % selectivity. Every shape is warmed, the two paths
alternate in one process and each call is timed with device events (both
paths synchronise once inside, to read the kept count) until each has at
least a second of samples. Prints one JSON line per case (median ms,
effective GB/s with bytes = mask + 2 x kept bytes, share of the 8.0 TB/s HBM
peak) and a markdown table. Needs a GPU.

    python scripts/filter_profile.py            # all cases
    python scripts/filter_profile.py --quick    # a tenth of the rows (a smoke run)
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak (6.29 TB/s is what a float4 copy reaches)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--window-s", type=float, default=1.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("filter_profile: needs a GPU")
    from tensorframes_amd._native import _C
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    scale = 10 if args.quick else 1
    g = torch.Generator(device=dev).manual_seed(7)
    frames = {
        "10M x (f32, i64, f32[16])": lambda n=10_000_000 // scale: [
            torch.rand(n, device=dev, generator=g), torch.randint(0, 1 << 40, (n,), device=dev, generator=g),
            torch.rand((n, 16), device=dev, generator=g)],
        "2.5M x f32[512]": lambda n=2_500_000 // scale: [torch.rand((n, 512), device=dev, generator=g)],
    }
    rows_out = []
    for fname, make in frames.items():
        cols = make()
        n = cols[0].shape[0]
        row_bytes = sum(c[0].numel() * c.element_size() for c in cols)
        r = torch.rand(n, device=dev, generator=g)
        for pct in (1, 50, 99):
            mask = r < pct / 100.0

            def new():
                return _C.compact_rows(mask, cols, False)[0]

            def base():
                idx = torch.nonzero(mask).reshape(-1)
                return [c.index_select(0, idx) for c in cols]
            for _ in range(2):  # warm both paths at this shape
                a, b = new(), base()
            assert all(torch.equal(x, y) for x, y in zip(a, b)), "the two paths disagree"
            kept = int(a[0].shape[0])
            del a, b
            tn, tb = [], []
            while sum(tn) < args.window_s * 1e3 or sum(tb) < args.window_s * 1e3 or len(tn) < 5:
                tn.append(timed(new)[0])
                tb.append(timed(base)[0])
            nbytes = n + 2 * kept * row_bytes
            rec = {"frame": fname, "rows": n, "row_bytes": row_bytes, "selectivity_pct": pct, "kept": kept,
                   "repeats": len(tn), "bytes": nbytes}
            for name, ts in (("compact", tn), ("index_select", tb)):
                ms = statistics.median(ts)
                rec[f"{name}_ms"] = round(ms, 4)
                rec[f"{name}_gbs"] = round(nbytes / ms / 1e6, 1)
                rec[f"{name}_hbm_share"] = round(nbytes / ms / 1e6 / HBM_PEAK_GBS, 4)
            rec["verdict"] = "no slower" if rec["compact_ms"] <= rec["index_select_ms"] else "LOSES"
            print(json.dumps(rec), flush=True)
            rows_out.append(rec)
        del cols, r
        torch.cuda.empty_cache()
    print("\n| partition | kept | compact_rows ms | GB/s | % of HBM peak | nonzero + index_select ms | GB/s | "
          "% of HBM peak | verdict |")
    print("|---|---|---|---|---|---|---|---|---|")
    for q in rows_out:
        print(f"| {q['frame']} | {q['selectivity_pct']} % | {q['compact_ms']:.3f} | {q['compact_gbs']:.0f} | "
              f"{100 * q['compact_hbm_share']:.1f} | {q['index_select_ms']:.3f} | {q['index_select_gbs']:.0f} | "
              f"{100 * q['index_select_hbm_share']:.1f} | {q['verdict']} |")


if __name__ == "__main__":
    main()
