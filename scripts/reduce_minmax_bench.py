"""Sum / Min / Max on HBM-bound shapes, one route each (column, wave per row,
row split): the median of 30 timed calls per op, each call synchronised.

    python scripts/reduce_minmax_bench.py

The three ops stream the same bytes, so Min / Max against Sum shows what the
NaN-propagating compare costs on each route (docs/PERFORMANCE.md)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tensorframes_amd import engine, tf  # noqa: E402

DEV = torch.device("cuda", 0)
FN = {"Sum": tf.reduce_sum, "Min": tf.reduce_min, "Max": tf.reduce_max}
for shape, axes in (((2_000_000, 256), [0]), ((500_000, 1024), [1]), ((64, 8_000_000), [1])):
    x = torch.randn(shape, device=DEV)
    for op in ("Sum", "Min", "Max"):
        g = tf.Graph()
        with g.as_default():
            FN[op](tf.placeholder(np.float32, [None, None], name="x"), axes, name="y")
        prog = engine.program(g.serialize(), ["y"], ["x"])
        for _ in range(5):
            engine.run_program(prog, [x], DEV)
        torch.cuda.synchronize()
        ts = []
        for _ in range(30):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            engine.run_program(prog, [x], DEV)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        gb = x.numel() * 4 / 1e9
        print("minmax %s %s axes=%s median %.3f ms (min %.3f) %.0f GB/s" % (op, shape, axes, ts[15], ts[0], gb / ts[15] * 1e3), flush=True)
