"""BGZF without a GPU: bt_diag_bgzf and bt_diag_crc32 run the __host__ __device__ code of the BGZF kernels (bayestyper_amd/csrc/bt_bgzf.hpp over bt_deflate.hpp)
with a team of one thread.  Python's gzip and zlib are the oracle: the stream must decompress to the content, every block must carry the specified header,
a payload that inflates alone to exactly its 65280-byte slice, and that slice's CRC-32 and length; the returned offsets must be the blocks'; the stream
must end with the canonical EOF block.  The CRC routine must equal zlib.crc32 at every length around its segment, row and block sizes."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

import _bgzf as B
import _deflate_inputs as D
from bayestyper_amd import lib

KINDS = ("text", "random", "run")


@functools.lru_cache(maxsize=None)
def content(kind, n):
    rng = np.random.default_rng(1000 + n)
    if kind == "text":
        return D.text(rng, n)   # VCF-like lines: dynamic blocks
    if kind == "random":
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()   # incompressible: the stored fallback
    return b"G" * n   # maximal matches


@pytest.mark.parametrize("n", B.SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_stream(kind, n):
    data = content(kind, n)
    stream, offsets, st = lib.diag_bgzf(data)
    cap, blocks = lib.bgzf_bound(n)
    assert blocks == (n + B.BLOCK - 1) // B.BLOCK == len(offsets) - 1 and len(stream) <= cap
    walked = B.check_stream(stream, data, offsets)
    for b in walked:
        assert b["size"] <= 65536
    for a, b in zip(walked, walked[1:]):
        assert a["offset"] + a["size"] == b["offset"]   # BSIZE + 1 is the distance to the next block
    assert st["pieces"] == blocks and st["bytes_in"] == n and st["bytes_out"] + 26 * blocks + 28 == len(stream)
    if kind == "random" and n >= 4:
        assert st["stored_pieces"] == blocks
    if kind != "random" and n >= B.BLOCK - 1:   # (a short last block may be smaller stored)
        assert st["stored_pieces"] <= (1 if n % B.BLOCK in range(1, 100) else 0)
    again, offsets2, _ = lib.diag_bgzf(data)
    assert again == stream and offsets2 == offsets
    # without the EOF block: the same data blocks, the last offset is the stream's end
    open_stream, open_offsets, _ = lib.diag_bgzf(data, eof=False)
    assert open_stream == stream[:-28] and open_offsets == offsets
    B.check_stream(open_stream, data, open_offsets, eof=False) if n else None


def test_bound():
    assert lib.bgzf_bound(0) == (28, 0) and lib.bgzf_bound(1) == (1 + 36 + 28, 1)
    assert lib.bgzf_bound(B.BLOCK) == (65316 + 28, 1) and lib.bgzf_bound(B.BLOCK + 1) == (65316 + 37 + 28, 2)
    assert lib.bgzf_bound((1 << 33) + 7) == (((1 << 33) + 7) // B.BLOCK * 65316 + ((1 << 33) + 7) % B.BLOCK + 36 + 28, ((1 << 33) + 7) // B.BLOCK + 1)


@pytest.mark.parametrize("n", (0, 5, 2 * B.BLOCK + 1))
def test_capacity_one_short_writes_nothing(n):
    data = np.frombuffer(content("text", n), np.uint8)
    cap, blocks = lib.bgzf_bound(n)
    out, offs, got = np.full(cap + 64, 0xAB, np.uint8), np.full(blocks + 1, 77, np.uint64), C.c_uint64(77)
    ptr = data.ctypes.data if n else None
    assert lib.bt_diag_bgzf(ptr, n, 1, out.ctypes.data, cap - 1, C.byref(got), offs.ctypes.data, None) != 0
    assert "bt_diag_bgzf: buffer too small" in lib.bt_last_error().decode() and got.value == 77 and (out == 0xAB).all() and (offs == 77).all()
    lib.check(lib.bt_diag_bgzf(ptr, n, 1, out.ctypes.data, cap, C.byref(got), offs.ctypes.data, None))   # the exact bound: the guard bytes stay
    assert (out[cap:] == 0xAB).all() and got.value <= cap
    B.check_stream(out[:got.value].tobytes(), data.tobytes(), [int(o) for o in offs])
    if n:
        assert lib.bt_diag_bgzf(None, n, 1, out.ctypes.data, cap, C.byref(got), None, None) != 0 and "null argument" in lib.bt_last_error().decode()


CRC_LENGTHS = list(range(0, 81)) + list(range(1019, 1026)) + [B.BLOCK - 1, B.BLOCK]


@pytest.mark.parametrize("kind", ("random", "zeros", "ff"))
def test_crc32_equals_zlib(kind):
    rng = np.random.default_rng(99)
    full = {"random": rng.integers(0, 256, B.BLOCK, dtype=np.uint8).tobytes(), "zeros": bytes(B.BLOCK), "ff": b"\xff" * B.BLOCK}[kind]
    for n in CRC_LENGTHS:
        for data in (full[:n], full[B.BLOCK - n:]):   # from the buffer's start and (another alignment in memory) up to its end
            assert lib.diag_crc32(data) == zlib.crc32(data), (kind, n)


def test_crc32_of_several_blocks():
    data = content("text", 3 * B.BLOCK + 17)
    assert lib.diag_crc32(data) == zlib.crc32(data)
    crc = C.c_uint32()
    assert lib.bt_diag_crc32(None, 5, C.byref(crc)) != 0 and "null argument" in lib.bt_last_error().decode()
