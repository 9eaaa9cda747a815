"""Sorting a device-resident partition (DataFrame.orderBy's device path:
`_C.sort_encode` + `_C.sort_argsort`, then `_C.permute_rows`) against what a
user would write with torch on the same device: `torch.argsort(stable=True)`
on the key (LSD over the keys for two keys) plus one `index_select` per
column.

Shapes: 10 M rows of (f32 key, i64, f32[16]) with a uniform float key, the
same with an int32 key in [0, 1000) (digit skipping), two keys (int32 in
[0, 100) ascending, f32 descending), and 2.5 M rows of f32[512] with an f32
key (the permute dominates). Every shape is warmed; the new path, the
baseline and the baseline AGAIN alternate in one process, and each stage
(argsort, permute) is timed with its own device-event pair until each has at
least a second of samples. The second baseline series gives the run-to-run
spread: the difference between two measurements of the same code. Prints one
JSON line per shape and a markdown table. Needs a GPU.

    python scripts/sort_profile.py            # all shapes
    python scripts/sort_profile.py --quick    # a tenth of the rows (a smoke run)
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


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
        sys.exit("sort_profile: needs a GPU")
    from tensorframes_amd._native import _C
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    scale = 10 if args.quick else 1
    g = torch.Generator(device=dev).manual_seed(7)

    def payload(n):
        return [torch.randint(0, 1 << 40, (n,), device=dev, generator=g), torch.rand((n, 16), device=dev, generator=g)]

    def f32_key(n):
        return torch.rand(n, device=dev, generator=g)

    def small_key(n, hi):
        return torch.randint(0, hi, (n,), device=dev, generator=g).to(torch.int32)

    n10, n25 = 10_000_000 // scale, 2_500_000 // scale
    # name -> (keys, descending flags, the other columns)
    shapes = {
        "10M x (f32 key uniform, i64, f32[16])": lambda: ([f32_key(n10)], [False], payload(n10)),
        "10M x (i32 key in [0,1000), i64, f32[16])": lambda: ([small_key(n10, 1000)], [False], payload(n10)),
        "10M x (i32 key in [0,100) asc, f32 key desc, i64, f32[16])":
            lambda: ([small_key(n10, 100), f32_key(n10)], [False, True], payload(n10)),
        "2.5M x (f32 key, f32[512])":
            lambda: ([f32_key(n25)], [False], [torch.rand((n25, 512), device=dev, generator=g)]),
    }
    rows_out = []
    for sname, make in shapes.items():
        keys, desc, rest = make()
        cols = keys + rest
        n = keys[0].shape[0]
        row_bytes = sum(c[0].numel() * c.element_size() for c in cols)

        def new_argsort():
            return _C.sort_argsort(_C.sort_encode(keys, desc))

        def base_argsort():
            perm = None  # LSD over the keys: the last key first, each pass stable
            for k, d in reversed(list(zip(keys, desc))):
                kk = k if perm is None else k.index_select(0, perm)
                p = torch.argsort(kk, stable=True, descending=d)
                perm = p if perm is None else perm.index_select(0, p)
            return perm

        def new_permute(perm):
            return _C.permute_rows(perm, cols)

        def base_permute(perm):
            return [c.index_select(0, perm) for c in cols]

        for _ in range(2):  # warm both paths at this shape
            pn, pb = new_argsort(), base_argsort()
            a, b = new_permute(pn), base_permute(pb)
        # uniform float keys have (almost) no ties and the other shapes' ties are stable in both paths
        assert torch.equal(pn, pb), "the two argsorts disagree"
        assert all(torch.equal(x, y) for x, y in zip(a, b)), "the two permutes disagree"
        passes = int(_C.sort_last_passes())  # (of the warm-up's last new_argsort: nothing sorted since)
        del a, b, pb
        t = {k: [] for k in ("new_argsort", "new_permute", "base_argsort", "base_permute", "again_argsort",
                             "again_permute")}
        while min(sum(v) for v in t.values()) < args.window_s * 1e3 or len(t["new_argsort"]) < 5:
            for tag, fa, fp in (("new", new_argsort, new_permute), ("base", base_argsort, base_permute),
                                ("again", base_argsort, base_permute)):
                ms, perm = timed(fa)
                t[f"{tag}_argsort"].append(ms)
                ms, out = timed(lambda: fp(perm))
                t[f"{tag}_permute"].append(ms)
                del out, perm
        rec = {"shape": sname, "rows": n, "row_bytes": row_bytes, "keys": len(keys), "radix_passes": passes,
               "repeats": len(t["new_argsort"])}
        for k, v in t.items():
            rec[f"{k}_ms"] = round(statistics.median(v), 4)
        for stage in ("argsort", "permute"):
            base, again, new = rec[f"base_{stage}_ms"], rec[f"again_{stage}_ms"], rec[f"new_{stage}_ms"]
            spread = abs(base - again)
            rec[f"{stage}_spread_ms"] = round(spread, 4)
            ref = min(base, again)
            rec[f"{stage}_verdict"] = "LOSES" if new > ref + spread else ("faster" if new < ref - spread else "same")
        rec["permute_gbs"] = round(2 * n * row_bytes / rec["new_permute_ms"] / 1e6, 1)
        best = min(rec["base_permute_ms"], rec["again_permute_ms"])
        rec["base_permute_gbs"] = round(2 * n * row_bytes / best / 1e6, 1)
        print(json.dumps(rec), flush=True)
        rows_out.append(rec)
        del keys, rest, cols, pn
        torch.cuda.empty_cache()
    print("\n| partition | radix passes | argsort ms | torch.argsort ms (twice) | verdict | permute_rows ms | GB/s | "
          "index_select ms (twice) | GB/s | verdict |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for q in rows_out:
        print(f"| {q['shape']} | {q['radix_passes']} | {q['new_argsort_ms']:.3f} | {q['base_argsort_ms']:.3f} / "
              f"{q['again_argsort_ms']:.3f} | {q['argsort_verdict']} | {q['new_permute_ms']:.3f} | "
              f"{q['permute_gbs']:.0f} | {q['base_permute_ms']:.3f} / {q['again_permute_ms']:.3f} | "
              f"{q['base_permute_gbs']:.0f} | {q['permute_verdict']} |")


if __name__ == "__main__":
    main()
