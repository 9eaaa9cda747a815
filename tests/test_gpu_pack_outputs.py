"""Zero-word packing of pipeline outputs: the device pack kernel
(csrc/kernels/pack_words.hip) against the numpy packer, and run_chunked with
packing on against off, bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from tensorframes_amd import engine, tf  # noqa: E402
from tensorframes_amd._native import _C  # noqa: E402
from tensorframes_amd.config import config, set_config  # noqa: E402

from pack_cases import CONTENTS, ROWS, TILE, WPRS, make_words, np_pack, split_packed, tile_bounds  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 2048                 # rows of 2048 bytes per chunk at the 4 MiB floor
N5 = CHUNK * 4 + 777         # five chunks, the last one ragged
rng = np.random.default_rng(77)
W = (rng.standard_normal((512, 512)) / np.sqrt(512)).astype(np.float32)


@pytest.fixture(autouse=True)
def _small_chunks(monkeypatch):
    monkeypatch.setattr(config, "chunk_bytes", 4 << 20)
    old = config.pack_outputs
    yield
    set_config(pack_outputs=old)


# ------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("content", CONTENTS)
def test_pack_kernel_matches_numpy_packer(content):
    for rows in ROWS:
        for wpr in WPRS:
            words = make_words(content, rows, wpr)
            dev = torch.from_numpy(words.view(np.int32)).cuda()
            packed = _C.pack_words(dev, rows, wpr).cpu().numpy()
            tag = f"{content} {rows}x{wpr}"
            header, mask, values = split_packed(packed, rows, wpr)
            rheader, rmask, _ = split_packed(np_pack(words), rows, wpr)
            np.testing.assert_array_equal(mask, rmask, err_msg=tag)
            tiles = (len(header) - 1) // 2
            np.testing.assert_array_equal(header[2::2], rheader[2::2], err_msg=tag)  # per-tile counts
            assert int(header[0]) == int(header[2::2].sum()) == int((words != 0).sum()), tag
            # the tiles' value runs tile [0, total) in some order ...
            runs = sorted((int(header[1 + 2 * t]), int(header[2 + 2 * t])) for t in range(tiles))
            end = 0
            for off, cnt in runs:
                assert off == end or cnt == 0, tag
                end = max(end, off + cnt)
            assert end == int(header[0]), tag
            # ... and each holds its tile's non-zero words in element order
            flat = words.reshape(-1)
            for t in range(tiles):
                a, b = tile_bounds(rows, wpr, t)
                tile = flat[a:b]
                off, cnt = int(header[1 + 2 * t]), int(header[2 + 2 * t])
                np.testing.assert_array_equal(values[off:off + cnt], tile[tile != 0], err_msg=f"{tag} tile {t}")


def test_pack_kernel_many_tiles_roundtrip():
    """More tiles than CUs, reserved in whatever order the blocks arrive: the
    host expansion restores the buffer."""
    rows, wpr = 700 * TILE + 5, 48
    words = make_words("float_specials", rows, wpr)
    packed = _C.pack_words(torch.from_numpy(words.view(np.int32)).cuda(), rows, wpr).cpu()
    out = torch.full((rows, wpr), 0x55555555, dtype=torch.int32)
    _C.unpack_words(packed, out, rows, wpr, 3)
    np.testing.assert_array_equal(out.numpy().view(np.uint32), words)


# ------------------------------------------------------------------ the pipeline
def _relu_matmul(w):
    g = tf.Graph()
    with g.as_default():
        x = tf.placeholder(tf.float32, [None, 512], name="x")
        tf.nn.relu(tf.matmul(x, tf.constant(w)), name="y")
    return engine.program(g.serialize(), ["y"], ["x"])


def _run(prog, segments, specs, pack):
    """(outputs, this run's share of the program's counters)."""
    set_config(pack_outputs=pack)
    before = prog.stats()
    outs = engine.run_segments_pipelined(prog, segments, specs)
    st = prog.stats()
    return outs, {k: st[k] - before[k] for k in ("chunks", "chunks_packed", "d2h_bytes", "d2h_dense_bytes")}


def _bits(t):
    return t.contiguous().view(torch.uint8).numpy()


def _packed_bytes(out_np, chunk):
    """What the packed D2H copies of a [rows, wpr]-word output move."""
    words = out_np.reshape(out_np.shape[0], -1).view(np.uint32)
    total = 0
    for a in range(0, words.shape[0], chunk):
        part = words[a:a + chunk]
        total += _C.pack_layout(part.shape[0], part.shape[1])["values_off"] + 4 * int((part != 0).sum())
    return total


def test_five_chunks_ragged_packed_equals_dense():
    prog = _relu_matmul(W)
    x = torch.from_numpy(rng.standard_normal((N5, 512)).astype(np.float32))
    spec = [[((N5, 512), torch.float32)]]
    dense, sd = _run(prog, [[x]], spec, False)
    packed, sp = _run(prog, [[x]], spec, True)
    np.testing.assert_array_equal(_bits(packed[0][0]), _bits(dense[0][0]))
    torch.testing.assert_close(dense[0][0][:64], torch.relu(x[:64] @ torch.from_numpy(W)), rtol=1e-4, atol=1e-4)
    assert sd["chunks"] == sp["chunks"] == 5
    assert sd["chunks_packed"] == 0 and sd["d2h_bytes"] == sd["d2h_dense_bytes"] == N5 * 2048
    assert sp["chunks_packed"] == 5 and sp["d2h_dense_bytes"] == N5 * 2048
    assert sp["d2h_bytes"] == _packed_bytes(dense[0][0].numpy(), CHUNK)
    assert sp["d2h_bytes"] < 0.6 * sp["d2h_dense_bytes"]  # about half the words are zero


def test_one_chunk():
    prog = _relu_matmul(W)
    x = torch.from_numpy(rng.standard_normal((1000, 512)).astype(np.float32))
    spec = [[((1000, 512), torch.float32)]]
    dense, _ = _run(prog, [[x]], spec, False)
    packed, sp = _run(prog, [[x]], spec, True)
    np.testing.assert_array_equal(_bits(packed[0][0]), _bits(dense[0][0]))
    assert sp["chunks"] == 1 and sp["chunks_packed"] == 1


def test_two_segments():
    prog = _relu_matmul(W)
    xs = [torch.from_numpy(rng.standard_normal((n, 512)).astype(np.float32)) for n in (CHUNK + 5, 2 * CHUNK + 31)]
    specs = [[((x.shape[0], 512), torch.float32)] for x in xs]
    dense, _ = _run(prog, [[x] for x in xs], specs, False)
    packed, sp = _run(prog, [[x] for x in xs], specs, True)
    for s in range(2):
        np.testing.assert_array_equal(_bits(packed[s][0]), _bits(dense[s][0]))
    assert sp["chunks"] == 5 and sp["chunks_packed"] == 5


def test_all_zero_output():
    prog = _relu_matmul(-np.abs(W))
    x = torch.from_numpy(np.abs(rng.standard_normal((N5, 512))).astype(np.float32))
    spec = [[((N5, 512), torch.float32)]]
    packed, sp = _run(prog, [[x]], spec, True)
    assert not _bits(packed[0][0]).any()
    assert sp["chunks_packed"] == 5
    assert sp["d2h_bytes"] == _packed_bytes(packed[0][0].numpy(), CHUNK) < N5 * 2048 // 16


def test_dense_output_switches_to_plain_copies():
    """Nothing to drop: the first two chunks are packed (the second is already
    enqueued when the first one's size arrives), the rest and later calls
    (but for a one-chunk re-probe) copy dense."""
    g = tf.Graph()
    with g.as_default():
        x = tf.placeholder(tf.float32, [None, 512], name="x")
        tf.matmul(x, tf.constant(W), name="y")
    prog = engine.program(g.serialize(), ["y"], ["x"])
    x = torch.from_numpy(rng.standard_normal((N5, 512)).astype(np.float32))
    spec = [[((N5, 512), torch.float32)]]
    dense, _ = _run(prog, [[x]], spec, False)
    first, s1 = _run(prog, [[x]], spec, True)
    np.testing.assert_array_equal(_bits(first[0][0]), _bits(dense[0][0]))
    assert s1["chunks"] == 5 and s1["chunks_packed"] == 2
    second, s2 = _run(prog, [[x]], spec, True)
    np.testing.assert_array_equal(_bits(second[0][0]), _bits(dense[0][0]))
    assert s2["chunks"] == 5 and s2["chunks_packed"] == 1
    assert s2["d2h_bytes"] == _packed_bytes(dense[0][0][:CHUNK].numpy(), CHUNK) + (N5 - CHUNK) * 2048


def test_int32_fetch():
    g = tf.Graph()
    with g.as_default():
        x = tf.placeholder(tf.int32, [None, 512], name="x")
        tf.maximum(x, tf.constant(np.asarray(0, np.int32)), name="y")
    prog = engine.program(g.serialize(), ["y"], ["x"])
    x = torch.from_numpy(rng.integers(-3, 4, (N5, 512)).astype(np.int32))
    spec = [[((N5, 512), torch.int32)]]
    dense, _ = _run(prog, [[x]], spec, False)
    packed, sp = _run(prog, [[x]], spec, True)
    np.testing.assert_array_equal(packed[0][0].numpy(), np.maximum(x.numpy(), 0))
    np.testing.assert_array_equal(_bits(packed[0][0]), _bits(dense[0][0]))
    assert sp["chunks_packed"] == 5


def test_eligible_and_one_byte_fetch():
    """A fetch of 1-byte rows is not whole words: it stays a plain copy beside
    the packed one."""
    g = tf.Graph()
    with g.as_default():
        x = tf.placeholder(tf.float32, [None, 512], name="x")
        f = tf.placeholder(tf.float32, [None, 1], name="f")
        tf.nn.relu(tf.matmul(x, tf.constant(W)), name="y")
        tf.greater(f, tf.constant(np.asarray(0, np.float32)), name="flag")
    prog = engine.program(g.serialize(), ["y", "flag"], ["x", "f"])
    x = torch.from_numpy(rng.standard_normal((N5, 512)).astype(np.float32))
    f = torch.from_numpy(rng.standard_normal((N5, 1)).astype(np.float32))
    spec = [[((N5, 512), torch.float32), ((N5, 1), torch.bool)]]
    dense, _ = _run(prog, [[x, f]], spec, False)
    packed, sp = _run(prog, [[x, f]], spec, True)
    np.testing.assert_array_equal(_bits(packed[0][0]), _bits(dense[0][0]))
    np.testing.assert_array_equal(packed[0][1].numpy(), f.numpy() > 0)
    assert sp["chunks_packed"] == 5
    assert sp["d2h_bytes"] == _packed_bytes(dense[0][0].numpy(), CHUNK) + N5


def test_deferred_wait_covers_the_expansions():
    """wait=False: the outputs are read only after pipeline_wait, which covers
    the last D2H and every pending expansion."""
    prog = _relu_matmul(W)
    xs = [torch.from_numpy(rng.standard_normal((N5, 512)).astype(np.float32)) for _ in range(2)]
    spec = [[((N5, 512), torch.float32)]]
    dense = [_run(prog, [[x]], spec, False)[0][0][0].clone() for x in xs]
    set_config(pack_outputs=True)
    before = prog.stats()
    try:
        with engine.deferred_pipelines() as handles:
            outs = [engine.run_segments_pipelined(prog, [[x]], spec)[0][0] for x in xs]
            assert len(handles) == 2
            engine.wait_pipelines(handles)
    finally:
        prog.release_pipeline()
    for o, d in zip(outs, dense):
        np.testing.assert_array_equal(_bits(o), _bits(d))
    assert prog.stats()["chunks_packed"] - before["chunks_packed"] == 10


_CHILD = r"""
import json, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
from tensorframes_amd import engine, tf
from tensorframes_amd.config import config
config.chunk_bytes = 4 << 20
n = int(sys.argv[2])
r = np.random.default_rng(3)
g = tf.Graph()
with g.as_default():
    x = tf.placeholder(tf.float32, [None, 512], name="x")
    tf.nn.relu(tf.matmul(x, tf.constant((r.standard_normal((512, 512)) / 22).astype(np.float32))), name="y")
prog = engine.program(g.serialize(), ["y"], ["x"])
out = engine.run_segments_pipelined(prog, [[torch.from_numpy(r.standard_normal((n, 512)).astype(np.float32))]],
                                    [[((n, 512), torch.float32)]])
st = prog.stats()
print("STATS " + json.dumps({k: st[k] for k in ("chunks", "chunks_packed", "d2h_bytes", "d2h_dense_bytes")}
                            | {"pack_outputs": bool(config.pack_outputs), "zeros": float((out[0][0] == 0).float().mean())}))
"""


def test_env_off_reproduces_dense_d2h_bytes():
    """TFA_PACK_OUTPUTS=0 (read by the config and by the native runtime):
    every D2H byte is an output byte, as before packing existed."""
    env = dict(os.environ, TFA_PACK_OUTPUTS="0")
    r = subprocess.run([sys.executable, "-c", _CHILD, REPO, str(N5)], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    st = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("STATS ")][-1][6:])
    assert st["pack_outputs"] is False
    assert st["chunks"] == 5 and st["chunks_packed"] == 0
    assert st["d2h_bytes"] == st["d2h_dense_bytes"] == N5 * 2048
    assert 0.4 < st["zeros"] < 0.6
