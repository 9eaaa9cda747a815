"""Shared by test_unpack_words.py and test_gpu_pack_outputs.py: a numpy
reference for the zero-word packed format (csrc/kernels/pack_layout.h) and the
shapes / contents both sides are checked on."""
import numpy as np

from tensorframes_amd._native import _C

TILE = _C.pack_layout(1, 1)["tile_rows"]
ROWS = [1, TILE - 1, TILE, TILE + 1, 3 * TILE + 7]
WPRS = [1, 15, 16, 17, 31, 32, 33, 512]
CONTENTS = ["all_zero", "no_zero", "half_zero", "float_specials", "int32"]


def make_words(kind, rows, wpr, seed=0):
    """uint32 [rows, wpr] of the given content class."""
    rng = np.random.default_rng(seed + 1000 * rows + wpr)
    n = rows * wpr
    if kind == "all_zero":
        w = np.zeros(n, np.uint32)
    elif kind == "no_zero":
        w = rng.integers(1, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    elif kind == "half_zero":
        w = rng.integers(1, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
        w[rng.random(n) < 0.5] = 0
    elif kind == "float_specials":
        # relu-like floats with -0.0, NaN, +-inf and a denormal sprinkled in:
        # only +0.0 is a zero word
        f = np.maximum(rng.standard_normal(n).astype(np.float32), 0)
        special = np.array([-0.0, np.nan, np.inf, -np.inf, 1e-45], np.float32)
        idx = rng.integers(0, n, max(1, n // 7))
        f[idx] = special[rng.integers(0, special.size, idx.size)]
        w = f.view(np.uint32).copy()
        if n >= 5:
            w[:5] = special.view(np.uint32)  # every one of them present
    elif kind == "int32":
        v = rng.integers(-3, 4, n).astype(np.int32)
        w = v.view(np.uint32).copy()
    else:
        raise ValueError(kind)
    return w.reshape(rows, wpr)


def tile_bounds(rows, wpr, t):
    return t * TILE * wpr, min(rows, (t + 1) * TILE) * wpr


def np_pack(words, shuffle_seed=None):
    """The packed buffer (uint8) of uint32 words [rows, wpr]; with
    shuffle_seed the tiles' value runs lie in a shuffled order."""
    rows, wpr = words.shape
    L = _C.pack_layout(rows, wpr)
    flat = np.ascontiguousarray(words).reshape(-1)
    nz = flat != 0
    bits = np.zeros(L["mask_words"] * 32, np.uint8)
    bits[:flat.size] = nz
    mask = np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").reshape(-1).view("<u4")
    tiles = L["tiles"]
    counts = [int(nz[slice(*tile_bounds(rows, wpr, t))].sum()) for t in range(tiles)]
    order = list(range(tiles))
    if shuffle_seed is not None:
        np.random.default_rng(shuffle_seed).shuffle(order)
    offs, cur = {}, 0
    for t in order:
        offs[t] = cur
        cur += counts[t]
    buf = np.zeros(L["values_off"] + 4 * cur, np.uint8)
    header = buf[:8 * (1 + 2 * tiles)].view("<u8")
    header[0] = cur
    values = buf[L["values_off"]:].view("<u4")
    for t in range(tiles):
        header[1 + 2 * t] = offs[t]
        header[2 + 2 * t] = counts[t]
        a, b = tile_bounds(rows, wpr, t)
        tile = flat[a:b]
        values[offs[t]:offs[t] + counts[t]] = tile[tile != 0]
    buf[L["mask_off"]:L["mask_off"] + 4 * L["mask_words"]].view("<u4")[:] = mask
    return buf


def split_packed(buf, rows, wpr):
    """(header uint64 [1 + 2 * tiles], mask uint32, values uint32 [total]) of a packed buffer."""
    L = _C.pack_layout(rows, wpr)
    buf = np.ascontiguousarray(buf)
    header = buf[:8 * (1 + 2 * L["tiles"])].view("<u8")
    mask = buf[L["mask_off"]:L["mask_off"] + 4 * L["mask_words"]].view("<u4")
    total = int(header[0])
    values = buf[L["values_off"]:L["values_off"] + 4 * total].view("<u4")
    return header, mask, values
