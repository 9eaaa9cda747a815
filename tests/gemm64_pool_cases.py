"""Case table for the three kernel families of csrc/kernels/gemm_f64.hip: the
float64 MFMA GEMM, the integer GEMM and NHWC pooling (a data module).

Every case names the route it was written for. tests/test_gemm64_pool_routes.py
checks on the host that each case lands on that route and that every route the
dispatch can take is named here; tests/test_gpu_gemm64_pool_routes.py runs the
same cases on the device against exact references.

The shapes are the smallest that reach each route. For the f64 GEMM the route
is the kernel (`<tile>_<N|T><N|T>`: tile x transpose_a x transpose_b) plus the
kinds of block its grid holds, which the device decides per block:

    I  A and B loaded in unchecked 16-byte pairs (an interior block)
    M  A checked, B in pairs (the block holds the M edge, or A cannot pair)
    N  A in pairs, B checked
    C  both checked (the corner block, or neither operand can pair)

An operand can pair when it is 16-byte aligned and its leading dimension is
even; an I block runs the interleaved FAST loop when K is a multiple of 16.
"""
from collections import namedtuple

KS = (1, 3, 15, 16, 17, 32, 33, 48)
TRANS = ((False, False), (False, True), (True, False), (True, True))
EPILOGUES = ("none", "bias", "bias_relu", "bias_relu6", "bias_tanh", "chain")

F64Case = namedtuple("F64Case", "id tile ta tb batch M N K epi kinds fast bcast_b")


def f64_kernel(c):
    return "%s_%s%s" % (c.tile, "T" if c.ta else "N", "T" if c.tb else "N")


def f64_block_kinds(M, N, K, batch, ta, tb, BM, BN, bcast_b=False):
    """The kinds of block (see the module docstring) in the grid of a GEMM over
    contiguous, 16-byte aligned operands, and whether any runs the FAST loop."""
    lda, ldb = (M if ta else K), (K if tb else N)
    kinds = set()
    for b in range(min(batch, 2)):      # an odd batch stride moves every other matrix off the pairs
        a_pairs = lda % 2 == 0 and (b * M * K) % 2 == 0
        b_pairs = ldb % 2 == 0 and (bcast_b or (b * N * K) % 2 == 0)
        for i in range(-(-M // BM)):
            for j in range(-(-N // BN)):
                a_fast = a_pairs and (i + 1) * BM <= M
                b_fast = b_pairs and (j + 1) * BN <= N
                kinds.add("I" if a_fast and b_fast else "M" if b_fast else "N" if a_fast else "C")
    order = "IMNC"
    return "".join(k for k in order if k in kinds)


_TILE_DIMS = {"64x16": (64, 16), "64x64": (64, 64), "128x128": (128, 128)}


def _f64(tile, ta, tb, batch, M, N, K, epi="none", bcast_b=False):
    BM, BN = _TILE_DIMS[tile]
    kinds = f64_block_kinds(M, N, K, batch, ta, tb, BM, BN, bcast_b)
    fast = "I" in kinds and K % 16 == 0
    cid = "%s-%s%s-b%d%s-%dx%dx%d-%s" % (tile, "T" if ta else "N", "T" if tb else "N", batch, "bc" if bcast_b else "",
                                        M, N, K, epi)
    return F64Case(cid, tile, ta, tb, batch, M, N, K, epi, kinds, fast, bcast_b)


def _build_f64():
    c = []
    for ta, tb in TRANS:
        for K in KS:
            # 64x16 (N <= 16): B never fills a tile below N = 16; at 16 the grid has I and M blocks
            c.append(_f64("64x16", ta, tb, 1, 200, 10, K))
            c.append(_f64("64x16", ta, tb, 1, 200, 16, K))
            # 64x64: 3 x 2 blocks, every kind at once where both operands pair (N = 78), odd ldb at 77
            c.append(_f64("64x64", ta, tb, 1, 130, 78, K))
        for K in (18, 34):
            # an even K off the k-tile: full k-tiles load in pairs whatever the layout, the tail is checked
            c.append(_f64("64x16", ta, tb, 1, 200, 16, K))
            c.append(_f64("64x64", ta, tb, 1, 130, 78, K))
            c.append(_f64("128x128", ta, tb, 52, 514, 130, K))
        for K in (16, 17, 48):
            c.append(_f64("64x64", ta, tb, 1, 130, 77, K))
            # 128x128 through batch: 5 x 2 x 52 = 520 blocks
            c.append(_f64("128x128", ta, tb, 52, 514, 130, K))
        c.append(_f64("128x128", ta, tb, 52, 513, 129, 33))        # the issue's shape: odd N
        for M in (1, 63, 64, 65):
            for N in (1, 10, 16):
                c.append(_f64("64x16", ta, tb, 1, M, N, 32))
        # block counts 1, 3 and 13 (no multiple of 8: the XCD remap's remainder path), N around the tile
        for M, N in ((64, 64), (1, 17), (130, 64), (832, 64), (800, 17), (128, 78), (63, 65), (64, 128)):
            c.append(_f64("64x64", ta, tb, 1, M, N, 32))
        # batches and a batch-broadcast B (stride 0); odd M * K: every other batch is off the pairs
        c.append(_f64("64x16", ta, tb, 3, 65, 16, 16))
        c.append(_f64("64x64", ta, tb, 3, 65, 66, 17))
        c.append(_f64("64x64", ta, tb, 3, 64, 64, 32, bcast_b=True))
        c.append(_f64("64x16", ta, tb, 3, 130, 10, 33, bcast_b=True))
    # the K sweep on the 128x128 tile and the non-batched way to it
    for K in KS:
        c.append(_f64("128x128", False, False, 52, 514, 130, K))
    c.append(_f64("128x128", False, True, 1, 32768, 256, 16))
    # epilogues on an interior + edge grid of every tile
    for epi in EPILOGUES[1:]:
        c.append(_f64("64x16", False, False, 1, 200, 16, 32, epi))
        c.append(_f64("64x16", False, True, 1, 130, 10, 17, epi))
        c.append(_f64("64x64", False, False, 1, 130, 78, 32, epi))
        c.append(_f64("64x64", True, True, 1, 130, 78, 33, epi))
        c.append(_f64("128x128", False, False, 1, 32642, 130, 16, epi))    # 256 x 2 blocks, the last of each partial
    seen, out = set(), []
    for x in c:
        if x.id not in seen:
            seen.add(x.id)
            out.append(x)
    return out


F64_CASES = _build_f64()

# special values: (tile, ta, tb, M, N, K) grids with an interior and an edge block in M and N
F64_SPECIAL_GRIDS = [
    ("64x16", False, False, 130, 16, 33),
    ("64x16", True, True, 130, 10, 32),
    ("64x64", False, True, 130, 78, 33),
    ("64x64", True, False, 130, 78, 48),
]

# ------------------------------------------------------------------ integer GEMM
IntCase = namedtuple("IntCase", "id dtype ta tb batch M N K epi")
INT_LIMIT_M = 1048561          # one row past 16 * 65535: grid.y could not hold it
INT_LIMIT_BATCH = 65536        # one batch past grid.z


def _int(dtype, ta, tb, batch, M, N, K, epi="none"):
    cid = "%s-%s%s-b%d-%dx%dx%d-%s" % (dtype, "T" if ta else "N", "T" if tb else "N", batch, M, N, K, epi)
    return IntCase(cid, dtype, ta, tb, batch, M, N, K, epi)


def _build_int():
    c = []
    for dtype in ("int32", "int64"):
        for M in (1, 15, 16, 17, 33):
            for N in (1, 15, 16, 17, 33):
                c.append(_int(dtype, False, False, 1, M, N, 17))
        for ta, tb in TRANS:
            for K in (1, 16, 17, 40):
                c.append(_int(dtype, ta, tb, 1, 17, 33, K))
            c.append(_int(dtype, ta, tb, 3, 33, 17, 40))
        for epi in ("bias", "bias_relu", "bias_relu6"):
            c.append(_int(dtype, False, False, 1, 33, 17, 40, epi))
            c.append(_int(dtype, False, True, 3, 17, 33, 17, epi))
    return c


INT_CASES = _build_int()

# ------------------------------------------------------------------ pooling
# slice: None, or (offset, ldc): the pool writes channels [offset, offset + C) of a concat output ldc wide.
# force: the route set with _C.set_pool_route for the case (None: automatic).
PoolCase = namedtuple("PoolCase", "id is_max N H W C KH KW sh sw pad epi slice force route")
POOL_ROUTES = ("pool3x3_v4_xcd", "pool3x3_v4", "generic_v4_u32", "generic_v4_i64", "generic_v1_u32", "generic_v1_i64")


def pool_out(size, k, s, pad):
    """(output size, leading pad) of one dimension, TF semantics."""
    if pad == "SAME":
        o = -(-size // s)
        return o, max((o - 1) * s + k - size, 0) // 2
    return (size - k) // s + 1, 0


def pool_auto_route(C, KH, KW, slice_):
    v4 = C % 4 == 0 and (slice_ is None or (slice_[0] % 4 == 0 and slice_[1] % 4 == 0))
    if v4 and KH == 3 and KW == 3:
        return "pool3x3_v4_xcd"
    return "generic_v4_u32" if v4 else "generic_v1_u32"


def _pool(is_max, N, H, W, C, KH, KW, sh, sw, pad, epi="none", slice_=None, force=None):
    route = force or pool_auto_route(C, KH, KW, slice_)
    cid = "%s-n%d-%dx%dx%d-k%dx%d-s%dx%d-%s-%s%s%s" % (
        "max" if is_max else "avg", N, H, W, C, KH, KW, sh, sw, pad, epi,
        "-slice%d_%d" % slice_ if slice_ else "", "-" + force if force else "")
    return PoolCase(cid, is_max, N, H, W, C, KH, KW, sh, sw, pad, epi, slice_, force, route)


IMAGES = ((1, 1), (2, 2), (3, 3), (5, 5), (8, 8), (1, 5), (5, 2), (3, 8), (13, 11))
WINDOWS = ((1, 1), (2, 2), (3, 3), (3, 2), (5, 5))
STRIDES = ((1, 1), (2, 2), (3, 3), (1, 2))
CHANNELS = (1, 3, 4, 7, 8, 36)


def _build_pool():
    c = []
    i = 0
    for is_max in (True, False):
        for H, W in IMAGES:
            for KH, KW in WINDOWS:
                for pad in ("SAME", "VALID"):
                    if pad == "VALID" and (H < KH or W < KW):
                        continue
                    # strides, channels and batch cycle with different periods: every pair meets
                    sh, sw = STRIDES[i % 4]
                    c.append(_pool(is_max, (1, 3)[i % 2], H, W, CHANNELS[(i // 2) % 6], KH, KW, sh, sw, pad))
                    i += 1
        # Inception's last pool, every stride on the 3x3 kernel, and both channel classes of the odd image
        c.append(_pool(is_max, 3, 8, 8, 8, 8, 8, 1, 1, "VALID"))
        c.append(_pool(is_max, 1, 8, 8, 36, 8, 8, 2, 2, "SAME"))
        for sh, sw in STRIDES:
            for pad in ("SAME", "VALID"):
                for C in CHANNELS:
                    c.append(_pool(is_max, 3, 13, 11, C, 3, 3, sh, sw, pad))
                c.append(_pool(is_max, 1, 2, 2, 4, 3, 3, sh, sw, "SAME"))      # W < 3 on the unrolled taps
                c.append(_pool(is_max, 3, 1, 5, 8, 3, 3, sh, sw, "SAME"))
        # more than 256 items, block counts 4 and 11: the XCD remap's remainder path
        c.append(_pool(is_max, 3, 13, 11, 8, 3, 3, 1, 1, "SAME"))
        c.append(_pool(is_max, 2, 13, 11, 36, 3, 3, 1, 1, "SAME"))
        # fused epilogues
        for epi in ("bias", "bias_relu", "bias_relu6"):
            c.append(_pool(is_max, 3, 13, 11, 36, 3, 3, 1, 1, "SAME", epi))
            c.append(_pool(is_max, 3, 13, 11, 8, 3, 2, 2, 2, "VALID", epi))
            c.append(_pool(is_max, 1, 5, 5, 7, 2, 2, 1, 2, "SAME", epi))
        # concat slices: offsets that keep the float4 stores, and one that does not (C = 4 at offset 2)
        for KH, KW in ((3, 3), (2, 2)):
            c.append(_pool(is_max, 3, 5, 5, 4, KH, KW, 1, 1, "SAME", "none", (0, 12)))
            c.append(_pool(is_max, 3, 5, 5, 8, KH, KW, 1, 1, "SAME", "none", (4, 12)))
            c.append(_pool(is_max, 3, 5, 5, 4, KH, KW, 1, 1, "SAME", "none", (2, 8)))
            c.append(_pool(is_max, 3, 5, 5, 3, KH, KW, 1, 1, "SAME", "none", (4, 7)))
            c.append(_pool(is_max, 3, 5, 5, 8, KH, KW, 2, 2, "SAME", "bias_relu", (4, 12)))
        # every route the setter reaches, on shapes whose automatic route is more specialised
        for force in POOL_ROUTES[1:]:
            for N, H, W, C, KH, KW, sh, sw, pad in ((3, 13, 11, 8, 3, 3, 1, 1, "SAME"), (2, 13, 11, 36, 3, 3, 2, 2, "VALID"),
                                                    (1, 2, 2, 4, 3, 3, 1, 1, "SAME")):
                c.append(_pool(is_max, N, H, W, C, KH, KW, sh, sw, pad, "none", None, force))
            c.append(_pool(is_max, 3, 13, 11, 36, 3, 3, 1, 2, "SAME", "bias_relu6", None, force))
            c.append(_pool(is_max, 3, 5, 5, 8, 3, 3, 1, 1, "SAME", "none", (4, 12), force))
        for force in ("generic_v4_i64", "generic_v1_u32", "generic_v1_i64"):
            c.append(_pool(is_max, 3, 8, 8, 8, 5, 5, 2, 2, "SAME", "none", None, force))
            c.append(_pool(is_max, 3, 5, 2, 36, 3, 2, 1, 2, "VALID", "bias", None, force))
        c.append(_pool(is_max, 3, 5, 5, 7, 3, 3, 1, 1, "SAME", "none", None, "generic_v1_i64"))
    seen, out = set(), []
    for x in c:
        if x.id not in seen:
            seen.add(x.id)
            out.append(x)
    return out


POOL_CASES = _build_pool()
