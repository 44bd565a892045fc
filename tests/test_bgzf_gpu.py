"""bt_bgzf / bt_bgzf_save on the GPU against the same __host__ __device__ code run on the host (bt_diag_bgzf): the device's bytes and block offsets must be
the host's for every size and content of tests/test_bgzf_cpu.py; a content of one block more than a launch batch must read back; a capacity one byte short
is an error that writes nothing; a BGZF file does not depend on the slab size."""
import ctypes as C
import gzip

import numpy as np
import pytest

import _bgzf as B
import _deflate_inputs as D
from bayestyper_amd import lib
from test_bgzf_cpu import KINDS, content

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", B.SIZES)
def test_device_bytes_equal_host_bytes(gpu_ctx, n):
    for kind in KINDS:
        data = content(kind, n)
        want, want_offsets, want_st = lib.diag_bgzf(data)
        got, got_offsets, got_st = lib.bgzf(gpu_ctx, data)
        assert got == want and got_offsets == want_offsets and got_st == want_st, kind
    part, part_offsets, _ = lib.bgzf(gpu_ctx, data, eof=False)
    assert part == want[:-28] and part_offsets == want_offsets


def test_one_block_more_than_a_launch_batch(gpu_ctx):
    rng = np.random.default_rng(3)
    chunk = np.frombuffer(D.text(rng, 1 << 20), np.uint8)
    data = np.concatenate([np.tile(chunk, 1024 * B.BLOCK // chunk.size + 1)[:1024 * B.BLOCK - 7000], rng.integers(0, 256, 7000, dtype=np.uint8), chunk[:100]]).tobytes()
    assert len(data) == 1024 * B.BLOCK + 100
    got, offsets, st = lib.bgzf(gpu_ctx, data)
    assert gzip.decompress(got) == data
    blocks = B.walk(got)
    assert len(blocks) == 1026 and [b["offset"] for b in blocks] == offsets and got[-28:] == B.EOF_BLOCK
    assert blocks[1024]["isize"] == 100 and st["pieces"] == 1025 and len(got) < len(data) // 2


def test_capacity_one_short(gpu_ctx):
    data = np.frombuffer(content("text", 2 * B.BLOCK + 1), np.uint8)
    cap, blocks = lib.bgzf_bound(data.size)
    d_in = gpu_ctx.to_device(data)
    d_out = gpu_ctx.to_device(np.full(cap + 63, 0xAB, np.uint8))   # cap - 1 bytes of buffer, then 64 guard bytes
    n, offs = C.c_uint64(77), np.full(blocks + 1, 77, np.uint64)
    assert lib.bt_bgzf(gpu_ctx.h, d_in.ptr, data.size, 1, d_out.ptr, cap - 1, C.byref(n), offs.ctypes.data, None) != 0
    assert "bt_bgzf: buffer too small" in lib.bt_last_error().decode() and n.value == 77 and (offs == 77).all()
    assert (d_out.download(np.uint8, cap + 63) == 0xAB).all()
    lib.check(lib.bt_bgzf(gpu_ctx.h, d_in.ptr, data.size, 1, d_out.ptr, cap, C.byref(n), offs.ctypes.data, None))   # the exact bound: the guard bytes stay
    back = d_out.download(np.uint8, cap + 63)
    assert (back[cap:] == 0xAB).all()
    B.check_stream(back[:n.value].tobytes(), data.tobytes(), [int(o) for o in offs])
    assert lib.bt_bgzf(gpu_ctx.h, None, data.size, 1, d_out.ptr, cap, C.byref(n), None, None) != 0 and "null argument" in lib.bt_last_error().decode()
    d_in.free(), d_out.free()


def test_bgzf_save_does_not_depend_on_the_slab(gpu_ctx, tmp_path, monkeypatch):
    data = D.interleaved()[:5 * B.BLOCK + 4321]   # with a slab of two blocks: three slabs, the last one short
    want, want_offsets, _ = lib.diag_bgzf(data)
    for slab, threads in ((2 * B.BLOCK - 5, 1), (3 * B.BLOCK, 4), (None, 2)):   # (the first is rounded up to two blocks)
        if slab:
            monkeypatch.setenv("BT_BGZF_SLAB_BYTES", str(slab))
        else:
            monkeypatch.delenv("BT_BGZF_SLAB_BYTES", raising=False)
        path = tmp_path / ("slab_%s.gz" % slab)
        offsets, st = lib.bgzf_save(gpu_ctx, str(path), data, threads)
        assert not (tmp_path / ("slab_%s.gz.tmp" % slab)).exists()
        assert path.read_bytes() == want and offsets == want_offsets
        assert st["bytes_in"] == len(data) and st["pieces"] == 6 and st["bytes_out"] + 6 * 26 + 28 == path.stat().st_size


def test_bgzf_save_empty(gpu_ctx, tmp_path):
    path = tmp_path / "empty.gz"
    offsets, st = lib.bgzf_save(gpu_ctx, str(path), b"")
    assert path.read_bytes() == B.EOF_BLOCK and offsets == [0] and st["pieces"] == 0 and gzip.open(path).read() == b""
    with pytest.raises(lib.BtError, match="cannot create"):
        lib.bgzf_save(gpu_ctx, str(tmp_path / "no_such_directory" / "x.gz"), b"abc")
    offs = np.zeros(1, np.uint64)
    assert lib.bt_bgzf_save(gpu_ctx.h, str(path).encode(), content("text", B.BLOCK + 1), B.BLOCK + 1, 1, offs.ctypes.data, 1, None) != 0
    assert "block offsets" in lib.bt_last_error().decode() and path.read_bytes() == B.EOF_BLOCK
