"""Case table for the reductions of csrc/kernels/reduce.hip (a data module).

Every case names the kernel route it was written for. tests/test_reduce_routes.py
checks on the host that each case lands on that route and that every route the
dispatch can take is named here; tests/test_gpu_reduce_routes.py runs the same
cases on the device.

The shapes are the smallest that reach each route. The row and column shapes
are written for 4-byte elements; where the route depends on the element size
(`VEC = 16 / sizeof(T)` elements per 16-byte load, 256 KB rows for the
one-block route) the 8-byte and bool rows give the equivalent.
"""
from collections import namedtuple

import numpy as np

WIDTH = {"float32": 4, "float64": 8, "int32": 4, "int64": 8, "bool": 1}
DTYPES_BY_WIDTH = {4: ("float32", "int32"), 8: ("float64", "int64"), 1: ("bool",)}

ReduceCase = namedtuple("ReduceCase", "id dtype shape axes keep_dims route")


def canonical(shape, axes):
    """(outer, r, inner) as the executor hands a reduction to the kernel:
    adjacent axes reduce in place, others are permuted to the back first."""
    axes = sorted(a % len(shape) for a in axes)
    if all(b == a + 1 for a, b in zip(axes, axes[1:])):
        outer = int(np.prod(shape[:axes[0]], dtype=np.int64))
        r = int(np.prod([shape[a] for a in axes], dtype=np.int64))
        inner = int(np.prod(shape[axes[-1] + 1:], dtype=np.int64))
        return outer, r, inner, True
    kept = [d for i, d in enumerate(shape) if i not in axes]
    return (int(np.prod(kept, dtype=np.int64)), int(np.prod([shape[a] for a in axes], dtype=np.int64)), 1, False)


# (shape, axes, keep_dims, route) for 4-byte elements
_ROWS4 = [
    # one wave per row
    ((1024, 8), [1], False, "row_wave_vec"),
    ((1024, 7), [1], False, "row_wave"),
    ((3, 4096), [1], False, "row_wave_vec"),
    ((1, 1), [1], False, "row_wave"),
    ((5, 63), [1], False, "row_wave"),
    ((5, 64), [1], False, "row_wave_vec"),
    ((5, 65), [1], False, "row_wave"),
    ((16389, 5), [1], False, "row_wave"),          # past the 4096-block x 4-wave grid: the row loop runs twice
    # one 1024-thread block per row
    ((1, 4097), [1], False, "row_block"),
    ((64, 8191), [1], False, "row_block"),         # around the 8 x 1024 unroll
    ((64, 8192), [1], False, "row_block"),
    ((64, 8193), [1], False, "row_block"),
    ((1, 65536), [1], False, "row_block"),         # exactly 256 KB
    # row split over S blocks
    ((1, 65537), [1], False, "row_split"),         # one element past 256 KB
    ((65, 4097), [1], False, "row_split"),         # one row past 64
    ((2, 70001), [1], False, "row_split_fold"),    # S = 68 > 64
    # column kernels
    ((2048, 3, 5), [1], False, "col"),
    ((2048, 3, 8), [1], False, "col_vec"),
    ((1, 200, 33), [1], False, "col_split"),       # S = 3
    ((4, 130, 8), [1], False, "col_vec_split"),    # S = 2, ragged last slice
    ((1, 4161, 3), [1], False, "col_split_fold"),  # S = 65
    ((1, 4161, 8), [1], False, "col_vec_split_fold"),
    ((2, 130, 255), [1], False, "col_split"),      # around one 256-thread column block
    ((2, 130, 256), [1], False, "col_vec_split"),
    ((2, 130, 257), [1], False, "col_split"),
    ((2, 130, 1028), [1], False, "col_vec_split"),
    ((65535, 2, 3), [1], False, "col"),            # the last outer that fits one grid dimension
    ((65536, 2, 3), [1], False, "col"),            # the first that does not
    ((70000, 2, 3), [1], False, "col"),
    # several axes
    ((6, 5, 4), [0, 2], False, "row_wave_vec"),    # permuted to [5, 24]
    ((20, 30), [0, 1], False, "row_wave_vec"),     # full reduction
    ((33, 100), [1], True, "row_wave_vec"),
    ((130, 9, 11), [0], True, "col_split"),
]

# what differs for 8-byte elements: VEC = 2 and half as many elements in 256 KB
_ROWS8 = [row for row in _ROWS4 if row[0] not in ((1, 65536), (1, 65537))] + [
    ((1, 32768), [1], False, "row_block"),
    ((1, 32769), [1], False, "row_split"),
    ((1, 65537), [1], False, "row_split"),
]

# bool (All / Any): VEC = 16, 262144 elements in 256 KB
_ROWS1 = [
    ((1024, 16), [1], False, "row_wave_vec"),
    ((1024, 7), [1], False, "row_wave"),
    ((16389, 5), [1], False, "row_wave"),
    ((1, 4097), [1], False, "row_block"),
    ((64, 8193), [1], False, "row_block"),
    ((1, 262144), [1], False, "row_block"),
    ((65, 4097), [1], False, "row_split"),
    ((1, 262145), [1], False, "row_split_fold"),
    ((2048, 3, 5), [1], False, "col"),
    ((2048, 3, 16), [1], False, "col_vec"),
    ((1, 200, 33), [1], False, "col_split"),
    ((4, 130, 16), [1], False, "col_vec_split"),
    ((1, 4161, 3), [1], False, "col_split_fold"),
    ((1, 4161, 16), [1], False, "col_vec_split_fold"),
    ((70000, 2, 3), [1], False, "col"),
    ((6, 5, 4), [0, 2], False, "row_wave"),
    ((20, 30), [0, 1], False, "row_wave"),
]


def _build():
    out = []
    for width, rows in ((4, _ROWS4), (8, _ROWS8), (1, _ROWS1)):
        for dtype in DTYPES_BY_WIDTH[width]:
            for shape, axes, keep, route in rows:
                cid = "%s-%s-ax%s%s" % (dtype, "x".join(map(str, shape)), "_".join(map(str, axes)), "-keep" if keep else "")
                out.append(ReduceCase(cid, dtype, shape, axes, keep, route))
    return out


REDUCE_CASES = _build()

# ------------------------------------------------------------------ unsorted segment reductions
# op family: Sum / Min / Max / Prod. `route` as _C.unsorted_segment_route names it:
# tiny_int, small_int, private_g<G> (G lanes per output in the final pass, the
# next power of two >= the block count B, at most 64), sorted_perm_p<inner_pad>,
# sorted_perm_wide (inner > 64). `blocks`: B of the private route, else None.
UsegCase = namedtuple("UsegCase", "id op dtype ids_dtype n inner nseg route blocks")


def _useg(op, dtype, ids_dtype, n, inner, nseg, route, blocks=None):
    cid = "%s-%s-%s-n%d-i%d-s%d" % (op, dtype, ids_dtype, n, inner, nseg)
    return UsegCase(cid, op, dtype, ids_dtype, n, inner, nseg, route, blocks)


def _build_useg():
    c = []
    # integer data, inner == 1: the register and LDS-atomic routes and their limits
    for dtype in ("int32", "int64"):
        for op in ("Sum", "Min", "Max"):
            c.append(_useg(op, dtype, "int64", 1023, 1, 16, "tiny_int"))
            c.append(_useg(op, dtype, "int32", 1024, 1, 16, "tiny_int"))
            c.append(_useg(op, dtype, "int64", 1025, 1, 16, "tiny_int"))
            c.append(_useg(op, dtype, "int64", 1025, 1, 17, "small_int"))
            c.append(_useg(op, dtype, "int32", 262144, 1, 16, "tiny_int"))
            c.append(_useg(op, dtype, "int64", 262144, 1, 128, "small_int"))
            # one row more: the slab route (64 rows per block)
            c.append(_useg(op, dtype, "int64", 262145, 1, 16, "private_g64", 4097))
            # the LDS table ends at 128 segments of one column: above it the sorted route
            c.append(_useg(op, dtype, "int64", 5000, 1, 129, "sorted_perm_p1"))
            c.append(_useg(op, dtype, "int32", 5000, 1, 4096, "sorted_perm_p1"))
            c.append(_useg(op, dtype, "int64", 5000, 1, 4097, "sorted_perm_p1"))
        # Prod has no integer fast route
        c.append(_useg("Prod", dtype, "int64", 1024, 1, 16, "private_g16", 16))
        c.append(_useg("Prod", dtype, "int32", 3000, 3, 200, "sorted_perm_p4"))
    # float data: every G of the slab route (block counts 1, 2, 63, 64, 65) and every inner class
    for dtype in ("float32", "float64"):
        for op in ("Sum", "Min", "Max", "Prod"):
            c.append(_useg(op, dtype, "int32", 1, 1, 5, "private_g1", 1))
            c.append(_useg(op, dtype, "int64", 32, 3, 5, "private_g1", 1))
            c.append(_useg(op, dtype, "int32", 33, 3, 5, "private_g2", 2))
            c.append(_useg(op, dtype, "int64", 96, 64, 5, "private_g4", 3))
            c.append(_useg(op, dtype, "int64", 160, 65, 5, "private_g8", 5))
            c.append(_useg(op, dtype, "int32", 416, 257, 5, "private_g16", 13))
            c.append(_useg(op, dtype, "int64", 800, 1, 5, "private_g32", 25))
            c.append(_useg(op, dtype, "int64", 2016, 3, 5, "private_g64", 63))
            c.append(_useg(op, dtype, "int32", 2048, 3, 5, "private_g64", 64))
            c.append(_useg(op, dtype, "int64", 2049, 3, 5, "private_g64", 65))
            # the LDS / sorted boundary at inner <= 64
            c.append(_useg(op, dtype, "int64", 3000, 3, 128, "private_g8", 6))
            c.append(_useg(op, dtype, "int64", 3000, 3, 129, "sorted_perm_p4"))
            c.append(_useg(op, dtype, "int32", 3000, 64, 128, "private_g8", 6))
            c.append(_useg(op, dtype, "int32", 3000, 64, 129, "sorted_perm_p64"))
            # the sorted route at every inner class
            c.append(_useg(op, dtype, "int64", 3000, 1, 200, "sorted_perm_p1"))
            c.append(_useg(op, dtype, "int32", 3000, 2, 200, "sorted_perm_p2"))
            c.append(_useg(op, dtype, "int64", 3000, 5, 200, "sorted_perm_p8"))
            c.append(_useg(op, dtype, "int64", 3000, 16, 200, "sorted_perm_p16"))
            c.append(_useg(op, dtype, "int32", 3000, 17, 200, "sorted_perm_p32"))
            c.append(_useg(op, dtype, "int64", 3000, 65, 70, "sorted_perm_wide"))
            c.append(_useg(op, dtype, "int64", 1000, 257, 40, "sorted_perm_wide"))
    return c


USEG_CASES = _build_useg()
