"""Device row compaction (csrc/kernels/compact.hip, `_C.compact_rows`) and
`DataFrame.filter` on device-resident frames. Everything is compared bitwise
with `col[mask]` computed on the host."""
import numpy as np
import pytest
import torch

import tensorframes_amd as tfs
from tensorframes_amd import tf
from tensorframes_amd._native import _C

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]

DEV = "cuda:0"

# row size in bytes -> (dtype, cell shape)
ROW_KINDS = {
    1: (torch.uint8, ()),
    4: (torch.int32, ()),
    8: (torch.int64, ()),
    12: (torch.float32, (3,)),
    16: (torch.float64, (2,)),
    20: (torch.float32, (5,)),
    2048: (torch.float32, (512,)),
}


def _tile():
    return _C.compact_tile_rows()


def _row_counts():
    t = _tile()
    return [0, 1, 63, 64, 65, t - 1, t, t + 1, 3 * t + 7]


def _masks(n, seed=0):
    """name -> host bool mask [n]"""
    g = torch.Generator().manual_seed(1234 + seed)
    idx = torch.arange(n)
    out = {
        "none": torch.zeros(n, dtype=torch.bool),
        "all": torch.ones(n, dtype=torch.bool),
        "alternating": idx % 2 == 1,
        "last": idx == n - 1,
        "first": idx == 0,
    }
    for pct in (1, 50, 99):
        out[f"random{pct}"] = torch.rand(n, generator=g) < pct / 100.0
    return out


def _column(n, dtype, cell, seed):
    """Host column [n, *cell] whose every row differs (bit patterns, not values, matter)."""
    g = torch.Generator().manual_seed(seed)
    shape = (n,) + tuple(cell)
    if dtype.is_floating_point:
        return torch.randn(shape, generator=g, dtype=dtype)
    hi = 255 if dtype == torch.uint8 else 2 ** 31 - 1
    return torch.randint(0, hi, shape, generator=g, dtype=torch.int64).to(dtype)


def _same_bits(got: torch.Tensor, want: torch.Tensor):
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape)
    assert got.is_contiguous()
    a = got.cpu().contiguous().view(torch.uint8) if got.numel() else got.cpu()
    b = want.contiguous().view(torch.uint8) if want.numel() else want
    assert torch.equal(a, b)


def test_tile_rows_exported():
    t = _tile()
    assert isinstance(t, int) and t >= 64 and t % 64 == 0


@pytest.mark.parametrize("row_bytes", sorted(ROW_KINDS))
def test_compact_row_sizes(row_bytes):
    dtype, cell = ROW_KINDS[row_bytes]
    for n in _row_counts():
        host = _column(n, dtype, cell, seed=n)
        assert (host[0].numel() * host.element_size() if n else row_bytes) == row_bytes
        dev = host.to(DEV)
        for name, hm in _masks(n, seed=row_bytes).items():
            outs, kept, index = _C.compact_rows(hm.to(DEV), [dev], True)
            assert kept == int(hm.sum()), (n, name)
            assert outs[0].is_cuda and index.is_cuda
            _same_bits(outs[0], host[hm])
            assert index.dtype == torch.int64
            assert torch.equal(index.cpu(), torch.nonzero(hm).reshape(-1)), (n, name)
            outs2, kept2, none = _C.compact_rows(hm.to(DEV), [dev])
            assert none is None and kept2 == kept
            _same_bits(outs2[0], host[hm])


def test_sixteen_mixed_columns_and_seventeen_raise():
    n = 3 * _tile() + 7
    kinds = [ROW_KINDS[k] for k in (1, 4, 8, 12, 16, 20, 2048)]
    kinds += [(torch.uint8, (3,)), (torch.uint8, (4,)), (torch.uint8, (16,)), (torch.int32, (4,)),
              (torch.float64, ()), (torch.int64, (3,)), (torch.float32, (1, 2)), (torch.float32, (7, 9)),
              (torch.float32, (300,))]  # 1200-byte rows: 16-byte units, more than 64 of them
    assert len(kinds) == 16
    hosts = [_column(n, dt, cell, seed=i) for i, (dt, cell) in enumerate(kinds)]
    devs = [h.to(DEV) for h in hosts]
    hm = _masks(n)["random50"]
    outs, kept, index = _C.compact_rows(hm.to(DEV), devs, False)
    assert index is None and kept == int(hm.sum()) and len(outs) == 16
    for o, h in zip(outs, hosts):
        _same_bits(o, h[hm])
    with pytest.raises(ValueError, match="16"):
        _C.compact_rows(hm.to(DEV), devs + [devs[0]], False)
    with pytest.raises(ValueError):
        _C.compact_rows(hm.to(DEV), [], False)


def test_wide_rows_take_the_row_loop():
    """Rows of more than 256 access units (16 KiB + 16 of float64) are copied row after row."""
    n = _tile() + 5
    host = _column(n, torch.float64, (2050,), seed=3)
    hm = _masks(n)["random50"]
    outs, kept, _ = _C.compact_rows(hm.to(DEV), [host.to(DEV)], False)
    _same_bits(outs[0], host[hm])
    odd = _column(n, torch.uint8, (1001,), seed=4)   # byte-wise, wide
    outs, _, _ = _C.compact_rows(hm.to(DEV), [odd.to(DEV)], False)
    _same_bits(outs[0], odd[hm])


def test_misaligned_sources_and_masks():
    n = _tile() + 65
    for cell in ((3,), (4,)):
        host = _column(n + 1, torch.float32, cell, seed=5)
        dev = host.to(DEV)[1:]                       # f32[3]: the base is 12 bytes past a 16-byte boundary
        assert (dev.data_ptr() % 16 != 0) == (cell == (3,))
        for name, hm in _masks(n).items():
            outs, kept, _ = _C.compact_rows(hm.to(DEV), [dev], False)
            _same_bits(outs[0], host[1:][hm])
    # 16-byte rows whose base is only 4-byte aligned
    flat = _column(4 * n + 1, torch.float32, (), seed=12)
    dev = flat.to(DEV)[1:].view(n, 4)
    assert dev.data_ptr() % 16 == 4
    for name, hm in _masks(n).items():
        outs, kept, _ = _C.compact_rows(hm.to(DEV), [dev], False)
        _same_bits(outs[0], flat[1:].view(n, 4)[hm])
    # a mask view that does not start on an 8-byte boundary, and a strided one
    host = _column(n, torch.int32, (), seed=6)
    big = torch.zeros(n + 3, dtype=torch.bool)
    big[3:] = _masks(n)["random50"]
    dm = big.to(DEV)[3:]
    assert dm.data_ptr() % 8 != 0
    outs, _, index = _C.compact_rows(dm, [host.to(DEV)], True)
    _same_bits(outs[0], host[big[3:]])
    assert torch.equal(index.cpu(), torch.nonzero(big[3:]).reshape(-1))
    strided = torch.zeros(2 * n, dtype=torch.uint8)
    strided[::2] = big[3:].to(torch.uint8)
    outs, _, _ = _C.compact_rows(strided.to(DEV)[::2], [host.to(DEV)], False)
    _same_bits(outs[0], host[big[3:]])
    # a non-contiguous column
    wide = _column(n, torch.float32, (6,), seed=7)
    outs, _, _ = _C.compact_rows(dm, [wide.to(DEV)[:, ::2]], False)
    _same_bits(outs[0], wide[:, ::2][big[3:]])


def test_bool_and_nonbinary_uint8_masks():
    n = 2 * _tile() + 1
    host = _column(n, torch.float32, (3,), seed=8)
    dev = host.to(DEV)
    g = torch.Generator().manual_seed(9)
    u8 = torch.randint(0, 256, (n,), generator=g, dtype=torch.int64).to(torch.uint8)
    u8[torch.rand(n, generator=g) < 0.5] = 0
    keep = u8 != 0
    assert int((u8 > 1).sum()) > 0                   # values other than 0 / 1 keep the row
    outs, kept, index = _C.compact_rows(u8.to(DEV), [dev], True)
    assert kept == int(keep.sum())
    _same_bits(outs[0], host[keep])
    assert torch.equal(index.cpu(), torch.nonzero(keep).reshape(-1))
    outs, kept, _ = _C.compact_rows(keep.to(DEV), [dev], False)   # the same rows through a bool mask
    _same_bits(outs[0], host[keep])


def test_validation_errors():
    n = 10
    dev = torch.zeros(n, dtype=torch.float32, device=DEV)
    ok = torch.ones(n, dtype=torch.bool, device=DEV)
    with pytest.raises(TypeError, match="bool or uint8"):
        _C.compact_rows(ok.to(torch.float32), [dev], False)
    with pytest.raises(ValueError, match="one entry per row"):
        _C.compact_rows(ok[:5], [dev], False)
    with pytest.raises(ValueError, match="device"):
        _C.compact_rows(ok.cpu(), [dev], False)
    with pytest.raises(ValueError, match="device"):
        _C.compact_rows(ok, [dev.cpu()], False)
    with pytest.raises(ValueError, match="rows"):
        _C.compact_rows(ok, [dev, dev[:4]], False)


def test_past_four_gib():
    """2^21 + 8 rows of 2048 bytes: the last rows start beyond 4 GiB, the
    smallest shape at which a 32-bit byte offset goes wrong."""
    n = 2 ** 21 + 8
    col = torch.empty((n, 2048), dtype=torch.uint8, device=DEV)
    rows = [0, n - 3, n - 2, n - 1]
    g = torch.Generator().manual_seed(11)
    pattern = torch.randint(0, 256, (4, 2048), generator=g, dtype=torch.int64).to(torch.uint8)
    mask = torch.zeros(n, dtype=torch.bool, device=DEV)
    for i, r in enumerate(rows):
        col[r].copy_(pattern[i])
        mask[r] = True
    outs, kept, index = _C.compact_rows(mask, [col], True)
    assert kept == 4
    assert index.cpu().tolist() == rows
    _same_bits(outs[0], pattern)


# ------------------------------------------------------------------ end to end
def _e2e_columns(n):
    x = np.arange(n, dtype=np.float32)
    cols = {"x": x, "k": (np.arange(n, dtype=np.int64) * 7) % 11, "v": np.stack([x, -x, x * 2], 1),
            "s": np.array([f"name-{i}" * (1 + i % 4) for i in range(n)])}
    for j in range(17):                               # more dense columns than one kernel call takes
        cols[f"c{j}"] = (x + j).astype(np.float64)
    return cols


def test_filter_on_device_resident_frame():
    n = 2 * _tile() + 77
    cols = _e2e_columns(n)
    host = tfs.from_columns(cols, num_partitions=3)
    dev = host.cache_on_device(DEV)
    assert all(isinstance(b.columns["s"], tfs.frame.block.StringColumn) and b.columns["s"].is_cuda
               for b in dev.local_blocks().values())
    before = tfs.metrics.snapshot()
    pred = lambda f: (f.k > 2) & (f.v.sum() == f.x * 2) & ((f.k * 3 + 1) > 7)  # noqa: E731
    keep = (cols["k"] > 2) & (cols["v"].sum(1) == cols["x"] * 2) & ((cols["k"] * 3 + 1) > 7)
    got_dev = dev.filter(pred(dev))
    got_host = host.filter(pred(host))
    blocks = got_dev.local_blocks()
    for b in blocks.values():
        for name, c in b.columns.items():
            assert c.is_cuda, name                    # the result stays on the device
    after = tfs.metrics.snapshot()
    assert after.get("filter_rows_kept", 0) - before.get("filter_rows_kept", 0) == int(keep.sum())
    assert after.get("filter_rows_in", 0) - before.get("filter_rows_in", 0) == n
    assert got_dev.count() == got_host.count() == int(keep.sum())
    for name in host.columns:
        a, b = got_dev.to_numpy(name), got_host.to_numpy(name)
        assert a.dtype == b.dtype and a.tolist() == b.tolist(), name
        assert a.tolist() == cols[name][keep].tolist(), name
    with tf.Graph().as_default():
        x = tfs.block(got_dev, "x")
        out = tfs.map_blocks(tf.add(x, 0.5, name="y"), got_dev)
        np.testing.assert_array_equal(out.to_numpy("y"), cols["x"][keep] + 0.5)
    empty = dev.filter(dev.x < 0)
    assert empty.count() == 0
    for b in empty.local_blocks().values():
        assert b.nrows == 0 and tuple(b.columns["v"].shape) == (0, 3) and b.columns["v"].is_cuda
        assert len(b.columns["s"]) == 0
