"""Packed against dense D2H on a synthetic graph whose output has a chosen
share of zero words (docs/PERFORMANCE.md, "Packed D2H": the threshold t).

y = abs(x) over host-resident float32[512] rows whose words are zero with
probability z (the mask is applied to x once, outside the timed region), so
the H2D side is the headline's and only the D2H payload changes. For every z
the pass is timed with plain copies and with packing forced on (the dense
switch is lifted for the sweep), `--reps` times each, alternating. Prints one
JSON line per z: ms per pass of each run, the packed share of the dense bytes
(from the d2h_bytes counter) and whether packing wins by more than the spread.

    python scripts/pack_threshold_sweep.py --rows 2500000 --steps 8 --warmup 2
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tensorframes_amd import engine, tf  # noqa: E402
from tensorframes_amd._native import _C  # noqa: E402
from tensorframes_amd.config import set_config  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2_500_000)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--zeros", default="0,25,50,75,100")
    a = ap.parse_args()
    g = tf.Graph()
    with g.as_default():
        x = tf.placeholder(tf.float32, [None, 512], name="x")
        tf.abs(x, name="y")
    prog = engine.program(g.serialize(), ["y"], ["x"])
    rng = np.random.default_rng(0)
    base = engine.pin(torch.from_numpy(rng.standard_normal((a.rows, 512), dtype=np.float32)))
    base[base == 0] = 1.0
    xin = _C.empty_pinned([a.rows, 512], torch.float32)
    spec = [[((a.rows, 512), torch.float32)]]

    def timed(pack):
        set_config(pack_outputs=pack)
        for _ in range(a.warmup):
            engine.run_segments_pipelined(prog, [[xin]], spec)
        before = prog.stats()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            out = engine.run_segments_pipelined(prog, [[xin]], spec)
        dt = (time.perf_counter() - t0) / a.steps * 1e3
        st = prog.stats()
        frac = (st["d2h_bytes"] - before["d2h_bytes"]) / max(1, st["d2h_dense_bytes"] - before["d2h_dense_bytes"])
        packed_chunks = st["chunks_packed"] - before["chunks_packed"]
        return dt, frac, packed_chunks, out[0][0]

    _C.set_pack_dense_fraction(2.0)  # never switch to dense by itself
    for z in [int(v) for v in a.zeros.split(",")]:
        xin.copy_(base)
        if z >= 100:
            xin.zero_()
        elif z > 0:
            keep = torch.from_numpy(rng.random((a.rows, 512), dtype=np.float32) >= z / 100.0)
            xin.mul_(keep)
        want = xin.abs()
        dense_ms, packed_ms, frac, chunks = [], [], 0.0, 0
        for _ in range(a.reps):
            d, _, _, od = timed(False)
            assert torch.equal(od.view(torch.int32), want.view(torch.int32))
            p, frac, chunks, op = timed(True)
            assert torch.equal(op.view(torch.int32), want.view(torch.int32))
            dense_ms.append(d)
            packed_ms.append(p)
        spread = max(max(dense_ms) - min(dense_ms), max(packed_ms) - min(packed_ms))
        print(json.dumps({"zero_pct": z, "packed_fraction": round(frac, 4), "chunks_packed_per_pass": chunks // a.steps,
                          "dense_ms": [round(v, 2) for v in dense_ms], "packed_ms": [round(v, 2) for v in packed_ms],
                          "spread_ms": round(spread, 2),
                          "packing_wins": max(packed_ms) < min(dense_ms) - spread}), flush=True)
    _C.set_pack_dense_fraction(0.0)


if __name__ == "__main__":
    main()
