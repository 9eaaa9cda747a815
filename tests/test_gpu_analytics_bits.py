"""The exact output bits of the analytics kernels (stats.hip, group_stats.hip,
window_scan.hip, sort.hip's encode), held against recorded digests.

The value tests of these kernels compare moments with an exact reference
within a tolerance, so they cannot see a reordered sum or a differently fused
multiply-add. Here fixed inputs go through the `_C` entry points and the
SHA-256 of every output's bytes must equal tests/golden/analytics_bits.json
(case name, shapes, dtypes and digest only). The README promises the same bits
for every number of ranks; that rests on these kernels giving the same bits
for the same rows, build after build.

Inputs come from `numpy.random.default_rng(seed).integers` alone (floats are
integers over a power of two with -0.0 and subnormals planted, NaN and
infinities in the cases marked so), so they do not depend on a sampling
algorithm.

Re-recording: `python tests/test_gpu_analytics_bits.py record` on a GPU, from a
build of the commit whose bits are the reference, rewrites the golden file.
The only reasons to do that are a deliberate change of a summation order (say
so in the commit) or a compiler upgrade that moves the bits of an unchanged
source; a refactor that moves a digest is a failed refactor."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "analytics_bits.json")
DTYPES = [np.float32, np.float64, np.int64, np.int32, np.int16, np.int8, np.uint8]
MOMENT_ROWS = [1, 63, 65, 4097, 3 * 4096 + 7]          # 4097: past one moments block
SEGMENTS = [0, 1, 64, 65, 512, 513, 4097, 35840]       # chunks of 512 rows: 1, 2, 9 (the wide fold), 70 (> 64 lanes)
WINDOW_ROWS = [1, 2047, 2048, 2049, 65 * 2048 + 3]     # tiles of 2048 rows; the last crosses the 64-tile scan step
STATS = ["count", "sum", "avg", "min", "max", "var_samp", "var_pop", "stddev_samp", "stddev_pop"]
KINDS = ["group_head", "peer_head", "peer_count", "sum_i64", "sum_f64", "min_word", "max_word"]
FRAMES = ["rows", "range", "whole"]
FNS = [("row_number", 0), ("rank", 0), ("dense_rank", 2), ("count", 0), ("sum", 3), ("sum", 4), ("avg", 4),
       ("min", 5), ("max", 6)]


def name_of(dt) -> str:
    return np.dtype(dt).name


def column(dt, n: int, seed: int, odd_rows=()) -> np.ndarray:
    """n values of dtype dt. Floats: k / 256 with -0.0 and two subnormals planted
    (16 rows on), then NaN, +inf, -inf, +inf at odd_rows (as many as given)."""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dt)
    if dt.kind != "f":
        ii = np.iinfo(dt)
        lo, hi = (-(1 << 62), 1 << 62) if dt == np.int64 else (int(ii.min), int(ii.max) + 1)
        return rng.integers(lo, hi, n).astype(dt)
    x = (rng.integers(-(1 << 20), 1 << 20, n) / 256.0).astype(dt)
    fi = np.finfo(dt)
    if n >= 16:
        x[3], x[8], x[13] = -0.0, fi.smallest_subnormal, -fi.tiny / 8
    for r, v in zip(odd_rows, (np.nan, np.inf, -np.inf, np.inf)):
        x[r] = v
    return x


def dev(a: np.ndarray, off: int = 0) -> torch.Tensor:
    """a on the device; off = 1: the same values in a view one element into its buffer."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not off:
        return t.to(DEV)
    buf = torch.zeros(t.shape[0] + off, dtype=t.dtype, device=DEV)
    buf[off:] = t.to(DEV)
    return buf[off:]


def host_words(a: np.ndarray) -> np.ndarray:
    """The ascending order-preserving words (the table in kernels.h), uint64."""
    if a.dtype.kind == "f":
        bits, ubits = (32, np.uint32) if a.dtype == np.float32 else (64, np.uint64)
        b = a.view(ubits).astype(np.uint64)
        sign, full = np.uint64(1 << (bits - 1)), np.uint64((1 << bits) - 1)
        b = np.where(np.isnan(a), np.uint64(0x7FC00000 if bits == 32 else 0x7FF8000000000000), b)
        b = np.where(b == sign, np.uint64(0), b)
        return np.where(b & sign != 0, ~b & full, b | sign)
    if a.dtype.kind == "u":
        return a.astype(np.uint64)
    return a.astype(np.int64).view(np.uint64) ^ np.uint64(1 << 63)


def entry(*tensors) -> dict:
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return {"shape": [list(t.shape) for t in tensors], "dtype": [str(t.dtype) for t in tensors],
            "sha256": h.hexdigest()}


# ------------------------------------------------------------------ the cases
def moments_and_hist(_C, out):
    for di, dt in enumerate(DTYPES):
        for n in MOMENT_ROWS:
            x = column(dt, n, 100 + di)
            w = host_words(x)
            top = np.array([w[0], w[n // 2], w[n - 1]], dtype=np.uint64) & np.uint64(0xFF << 56)
            pre8 = torch.from_numpy(top.view(np.int64).copy())
            for off in (0, 1):
                t = dev(x, off)
                out[f"column_moments/{name_of(dt)}/n{n}/off{off}"] = entry(*_C.column_moments([t]))
                out[f"select_hist/{name_of(dt)}/n{n}/off{off}"] = entry(
                    _C.select_hist(t, torch.zeros(1, dtype=torch.int64), 0), _C.select_hist(t, pre8, 8))
    n = MOMENT_ROWS[-1]
    for dt in (np.float32, np.float64):   # NaN and both infinities among the rows
        t = dev(column(dt, n, 200, odd_rows=(100, 5000, 9000)))
        out[f"column_moments/{name_of(dt)}/odd/n{n}"] = entry(*_C.column_moments([t]))
    mixed = [column(DTYPES[c % 7], n, 300 + c, odd_rows=(7 * c, 4100) if c >= 14 else ()) for c in range(16)]
    out[f"column_moments/mixed16/n{n}"] = entry(*_C.column_moments([dev(x, c % 2) for c, x in enumerate(mixed)]))


def grouped(_C, out):
    offsets = np.concatenate([[0], np.cumsum(SEGMENTS)]).astype(np.int64)
    n = int(offsets[-1])
    recs = []
    for part in range(3):
        rng = np.random.default_rng(400 + part)
        perm = np.argsort(rng.integers(0, 1 << 40, n), kind="stable").astype(np.int64)
        seg = lambda s, j: int(perm[offsets[s] + j])  # noqa: E731  (the row behind position j of segment s)
        # a NaN in the 64-row segment, +inf in the 65-row one, both infinities in the 513-row one
        odd = (seg(2, 2), seg(3, 60), seg(5, 400), seg(5, 7))
        cols = [dev(column(dt, n, 500 + 10 * part + c, odd_rows=odd)) for c, dt in enumerate(DTYPES)]
        recs.append(_C.group_moments(cols, dev(perm), dev(offsets)))
        out[f"group_moments/part{part}"] = entry(recs[-1])
    # ordered by (group, partition): three records per group
    stacked = torch.stack(recs, 1).reshape(len(SEGMENTS) * 3, len(DTYPES), 6).contiguous()
    merged = _C.merge_group_records(stacked, dev(np.arange(0, 3 * len(SEGMENTS) + 1, 3, dtype=np.int64)),
                                    [np.dtype(dt).kind == "f" for dt in DTYPES])
    out["merge_group_records/3_per_group"] = entry(merged)
    asked = [(c, st) for c in range(len(DTYPES)) for st in STATS]
    for k in range(0, len(asked), 16):
        part = asked[k:k + 16]
        res = _C.group_results(merged, [c for c, _ in part], [st for _, st in part],
                               [torch.from_numpy(np.zeros(0, DTYPES[c])).dtype for c, _ in part])
        out[f"group_results/outputs{k}"] = entry(*res)


def window(_C, out):
    for di, dt in enumerate(DTYPES):
        for n in WINDOW_ROWS:
            rng = np.random.default_rng(600 + di)
            glen = rng.integers(1, 700, n // 100 + 2)
            g = np.repeat(np.arange(len(glen), dtype=np.uint64) * np.uint64(3) + np.uint64(5), glen)[:n]
            g = np.concatenate([g, np.full(n - len(g), g[-1] + np.uint64(1), dtype=np.uint64)])  # one long last group
            p = np.repeat(np.arange(n, dtype=np.uint64), rng.integers(1, 4, n))[:n]
            words = dev(np.stack([g, p], 0).view(np.int64))
            v = dev(column(dt, n, 700 + di, odd_rows=(n // 3, n // 2) if n > 16 else ()))
            # (the wrapping integer sum of a float column would convert a NaN: it reads an int32 column there)
            vi = v if np.dtype(dt).kind != "f" else dev(column(np.int32, n, 800 + di))
            vt = [vi.dtype, v.dtype, v.dtype, v.dtype]
            fwd = _C.window_scan(words, 1, False, KINDS, [vi, v, v, v])
            rev = _C.window_scan(words, 1, True, KINDS[:2], [])
            carried = n == WINDOW_ROWS[-1]   # the first group began earlier, the last one runs on
            carry = total = [0] * len(KINDS)
            if carried:
                carry = [0, 0, 3, 77, int(np.float64(2.5).view(np.int64)), int(fwd[5, 9]), int(fwd[6, 9])]
                total = [0, 0, 9, -5, int(np.float64(-1e3).view(np.int64)), int(fwd[5, n - 1]), int(fwd[6, n - 1])]
            asked = [(fn, ch, fr) for fn, ch in FNS for fr in FRAMES]
            res = []
            for k in range(0, len(asked), 16):
                part = asked[k:k + 16]
                res += _C.window_finish(fwd, rev, KINDS, carry, total, carried, carried, 11 if carried else 0,
                                        5000 if carried else 0, [fn for fn, _, _ in part], [fr for _, _, fr in part],
                                        [ch for _, ch, _ in part], [vt[max(ch - 3, 0)] for _, ch, _ in part])
            out[f"window/{name_of(dt)}/n{n}"] = entry(fwd, rev, *res)


def sort_encode(_C, out):
    n = 4097
    keys = [dev(column(dt, n, 900 + c, odd_rows=(50, 60, 70))) for c, dt in enumerate(DTYPES)]
    keys.append(dev(np.random.default_rng(950).integers(0, 2, n).astype(np.bool_)))
    for desc in (False, True):
        out[f"sort_encode/{'descending' if desc else 'ascending'}"] = entry(_C.sort_encode(keys, [desc] * len(keys)))


FAMILIES = {"moments_and_hist": moments_and_hist, "grouped": grouped, "window": window, "sort_encode": sort_encode}


def compute(family: str) -> dict:
    from tensorframes_amd._native import _C
    out: dict = {}
    FAMILIES[family](_C, out)
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_output_bits_are_the_recorded_ones(family, golden):
    got, want = compute(family), golden[family]
    assert sorted(got) == sorted(want), "the cases are not the recorded ones"
    moved = [name for name in sorted(got) if got[name] != want[name]]
    for name in moved:
        print(f"{name}: got {got[name]}, recorded {want[name]}")
    assert not moved, f"{len(moved)} of {len(got)} outputs differ from the recorded bits: {moved[:8]}"


if __name__ == "__main__" and sys.argv[1:2] == ["record"]:
    sys.path.insert(0, os.getcwd())  # the build in the current directory
    target = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    families = []
    for family in sorted(FAMILIES):  # one case per line
        cases = ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in sorted(compute(family).items()))
        families.append(f"{json.dumps(family)}: {{\n{cases}\n}}")
    with open(target, "w") as f:
        f.write("{\n" + ",\n".join(families) + "\n}\n")
    print(f"recorded {target}")
