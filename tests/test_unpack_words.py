"""Host expansion of zero-word packed buffers (csrc/runtime/unpack.cpp): every
compiled-in variant (scalar, AVX2, AVX-512) against a numpy packer, bit-exact,
plus the worker pool and a stand-alone sanitizer build of the same code."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tensorframes_amd._native import _C

from pack_cases import CONTENTS, ROWS, TILE, WPRS, make_words, np_pack

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = {"scalar": 0, "avx2": 1, "avx512": 2}


@pytest.fixture(params=list(VARIANTS))
def variant(request):
    v = VARIANTS[request.param]
    if not _C.unpack_variant_available(v):
        pytest.skip(f"this CPU has no {request.param}")
    _C.unpack_force_variant(v)
    assert _C.unpack_current_variant() == v
    yield request.param
    _C.unpack_force_variant(-1)


def _out_buffer(n_words, misalign):
    """uint32 [n_words] filled with a marker, 64-byte aligned or 4 bytes past it."""
    raw = np.full(n_words * 4 + 192, 0xAB, np.uint8)
    base = (-raw.ctypes.data) % 64 + (4 if misalign else 0)
    out = raw[base:base + n_words * 4].view(np.uint32)
    assert out.ctypes.data % 64 == (4 if misalign else 0)
    return out


def _expand(words, packed, misalign=False, threads=0):
    rows, wpr = words.shape
    out = _out_buffer(rows * wpr, misalign)
    _C.unpack_words(torch.from_numpy(packed), torch.from_numpy(out.view(np.int32)), rows, wpr, threads)
    return out.reshape(rows, wpr)


@pytest.mark.parametrize("content", CONTENTS)
def test_unpack_matches_numpy_packer(variant, content):
    for rows in ROWS:
        for wpr in WPRS:
            words = make_words(content, rows, wpr)
            got = _expand(words, np_pack(words))
            np.testing.assert_array_equal(got, words, err_msg=f"{variant} {content} {rows}x{wpr}")


def test_unpack_keeps_every_non_zero_bit_pattern(variant):
    words = make_words("float_specials", 3 * TILE + 7, 33)
    f = words.view(np.float32)
    assert np.isnan(f).any() and np.isinf(f).any() and (words == 0x80000000).any() and (words == 1).any()
    got = _expand(words, np_pack(words))
    np.testing.assert_array_equal(got, words)


@pytest.mark.parametrize("wpr", [17, 512])
def test_unpack_misaligned_output(variant, wpr):
    """`out` off the 64-byte grid takes the plain (non-streaming) stores."""
    for rows in ROWS:
        words = make_words("half_zero", rows, wpr)
        np.testing.assert_array_equal(_expand(words, np_pack(words), misalign=True), words)


def test_unpack_shuffled_tile_order(variant):
    """The value runs of the tiles may lie in any order: the header places them."""
    for wpr in (15, 32, 512):
        words = make_words("half_zero", 3 * TILE + 7, wpr)
        packed = np_pack(words, shuffle_seed=5)
        assert not np.array_equal(packed, np_pack(words))
        np.testing.assert_array_equal(_expand(words, packed), words)


@pytest.mark.parametrize("threads", [1, 3, 8])
def test_unpack_pool(variant, threads):
    for rows, wpr in ((1, 33), (TILE + 1, 512), (9 * TILE + 7, 512), (3 * TILE + 7, 17)):
        words = make_words("half_zero", rows, wpr)
        got = _expand(words, np_pack(words, shuffle_seed=2), threads=threads)
        np.testing.assert_array_equal(got, words)


def test_unpack_rejects_header_that_disagrees_with_mask(variant):
    words = make_words("half_zero", TILE + 1, 32)
    packed = np_pack(words)
    header = packed[:8 * 5].view("<u8")
    header[2] -= 1  # tile 0 claims one value fewer than its mask has bits
    with pytest.raises(RuntimeError, match="tile 0"):
        _expand(words, packed)
    with pytest.raises(RuntimeError, match="tile 0"):
        _expand(words, packed, threads=3)


def test_pool_worker_exception_reaches_waiter():
    with pytest.raises(RuntimeError, match="part 2 failed"):
        _C.unpack_pool_raise(3, 8, 2)
    _C.unpack_pool_raise(3, 8, -1)  # nothing throws: returns


def test_default_thread_count(monkeypatch):
    monkeypatch.setenv("TFA_UNPACK_THREADS", "5")
    assert _C.unpack_default_threads() == 5
    monkeypatch.delenv("TFA_UNPACK_THREADS")
    monkeypatch.setenv("OMP_NUM_THREADS", "16")
    assert _C.unpack_default_threads() == 12
    monkeypatch.setenv("OMP_NUM_THREADS", "6")
    assert _C.unpack_default_threads() == 4
    monkeypatch.setenv("OMP_NUM_THREADS", "1")
    assert _C.unpack_default_threads() == 1
    monkeypatch.delenv("OMP_NUM_THREADS")
    assert 1 <= _C.unpack_default_threads() <= min(12, max(1, len(os.sched_getaffinity(0)) - 2))


@pytest.mark.parametrize("sanitizer", ["address,undefined", "thread"])
def test_unpack_native_program_under_sanitizer(tmp_path, sanitizer):
    """tests/native/unpack_main.cpp (its own main, the same cases, a pool run
    and a throwing worker) built with unpack.cpp under a host sanitizer and run
    as a plain program."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "unpack_main"
    # the sanitizer runtime is linked into the program itself: it runs as it
    # is, whatever else the environment loads into a process
    static = ["-static-libasan", "-static-libubsan"] if "address" in sanitizer else ["-static-libtsan"]
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", f"-fsanitize={sanitizer}", *static,
           "-fno-sanitize-recover=all", "-I", os.path.join(REPO, "csrc"),
           os.path.join(REPO, "tests", "native", "unpack_main.cpp"),
           os.path.join(REPO, "csrc", "runtime", "unpack.cpp"), "-o", str(exe), "-lpthread"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "unpack_main: ok" in r.stdout
