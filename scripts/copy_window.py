"""Memory-copy summary of ONE timed window of a rocprofv3 run
(`--memory-copy-trace --marker-trace --output-format csv`), the companion of
scripts/trace_window.py: per copy direction the number of copies, their bytes
(when the trace has a size column), the summed copy time and the time at least
one copy of that direction was in flight.

    python scripts/copy_window.py traces/headline --out profiles/pack_d2h/copies_after.md
"""
import argparse
import glob
import json
import os

from trace_window import _col, _rows, window


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--marker", default="tfa.timed_steps")
    ap.add_argument("--out", required=True)
    ap.add_argument("--title", default="")
    a = ap.parse_args()
    ccsv = glob.glob(os.path.join(a.dir, "**", "*memory_copy_trace.csv"), recursive=True)
    mcsv = glob.glob(os.path.join(a.dir, "**", "*marker_api_trace.csv"), recursive=True)
    if not ccsv or not mcsv:
        raise SystemExit(f"memory-copy / marker trace CSVs not found under {a.dir}")
    t0, t1 = window(mcsv[0], a.marker)
    rows = _rows(ccsv[0])
    sk, ek, dk = _col(rows[0], "start_timestamp"), _col(rows[0], "end_timestamp"), _col(rows[0], "direction")
    try:
        bk = _col(rows[0], "bytes", "size")
    except KeyError:
        bk = None
    by = {}
    for r in rows:
        s, e = int(r[sk]), int(r[ek])
        if s < t0 or e > t1:
            continue
        d = by.setdefault(r[dk], {"direction": r[dk], "copies": 0, "bytes": 0, "ns": 0, "iv": []})
        d["copies"] += 1
        d["ns"] += e - s
        d["iv"].append((s, e))
        if bk:
            d["bytes"] += int(r[bk])
    win = t1 - t0
    out = []
    for d in by.values():
        busy, cs, ce = 0, None, None
        for s, e in sorted(d.pop("iv")):
            if ce is None or s > ce:
                if ce is not None:
                    busy += ce - cs
                cs, ce = s, e
            else:
                ce = max(ce, e)
        if ce is not None:
            busy += ce - cs
        d["copy_ms"] = d.pop("ns") / 1e6
        d["in_flight_ms"] = busy / 1e6
        d["in_flight_pct"] = 100.0 * busy / win if win else 0.0
        d["GBps_in_flight"] = d["bytes"] / busy if busy and bk else None
        out.append(d)
    out.sort(key=lambda d: -d["copy_ms"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(os.path.splitext(a.out)[0] + ".json", "w") as f:
        json.dump({"window_ms": win / 1e6, "copies": out}, f, indent=1)
    lines = [f"# {a.title or 'memory copies of one timed window'}\n",
             f"Window (roctx `{a.marker}`): {win / 1e6:.2f} ms.\n",
             "| direction | copies | GB | copy ms (sum) | in flight ms | in flight | GB/s while in flight |",
             "|---|---:|---:|---:|---:|---:|---:|"]
    for d in out:
        gb = f"{d['bytes'] / 1e9:.3f}" if bk else "n/a"
        rate = f"{d['GBps_in_flight']:.1f}" if d["GBps_in_flight"] else "n/a"
        lines.append(f"| {d['direction']} | {d['copies']} | {gb} | {d['copy_ms']:.1f} | {d['in_flight_ms']:.1f} | "
                     f"{d['in_flight_pct']:.1f}% | {rate} |")
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps({"window_ms": win / 1e6, "copies": out}))


if __name__ == "__main__":
    main()
