"""The hand-over between launch batches (1024 units) in the shared pipeline of bt_deflate / bt_gzip_save / bt_bgzf_save (csrc/bt_gz_pipeline.hpp): a raw
deflate stream of one piece more than a batch, and for both file writers a slab that spans two batches followed by a short one.  (bt_bgzf across a batch:
tests/test_bgzf_gpu.py.)  The host replay is not run on these contents: 64 MiB through a team of one thread is too slow for a test."""
import functools
import gzip
import zlib

import numpy as np
import pytest

import _bgzf as B
import _deflate_inputs as D
from bayestyper_amd import lib

pytestmark = pytest.mark.gpu

P = D.P


@functools.lru_cache(maxsize=None)
def chunk():
    return np.frombuffer(D.text(np.random.default_rng(3), 1 << 20), np.uint8)


@functools.lru_cache(maxsize=None)
def content(units, unit):
    """units * unit + 100 bytes, as test_one_block_more_than_a_launch_batch builds its own: a tiled MiB of text, 7000 random bytes up to the boundary of
    the last whole unit, 100 bytes of text behind it"""
    rng = np.random.default_rng(3)
    c = chunk()
    data = np.concatenate([np.tile(c, units * unit // c.size + 1)[:units * unit - 7000], rng.integers(0, 256, 7000, dtype=np.uint8), c[:100]]).tobytes()
    assert len(data) == units * unit + 100
    return data


def test_one_piece_more_than_a_launch_batch(gpu_ctx):
    data = content(1024, P)
    got, st = lib.deflate(gpu_ctx, data)
    assert zlib.decompress(got, -15) == data and st["pieces"] == 1025
    part, _ = lib.deflate(gpu_ctx, data, last=False)
    z = zlib.decompressobj(-15)
    assert len(part) == len(got) and z.decompress(part) == data and not z.eof


def test_gzip_save_slab_of_two_batches(gpu_ctx, tmp_path, monkeypatch):
    data = content(1025, P)   # with a slab of 1025 pieces: two slabs, one of two batches, one of 100 bytes
    monkeypatch.setenv("BT_GZIP_SLAB_BYTES", str(1025 * P))
    st = lib.gzip_save(gpu_ctx, str(tmp_path / "two.gz"), data, 4)
    assert gzip.open(tmp_path / "two.gz").read() == data and st["pieces"] == 1026 and not (tmp_path / "two.gz.tmp").exists()
    monkeypatch.delenv("BT_GZIP_SLAB_BYTES")
    lib.gzip_save(gpu_ctx, str(tmp_path / "default.gz"), data, 4)
    assert (tmp_path / "two.gz").read_bytes() == (tmp_path / "default.gz").read_bytes()


def test_bgzf_save_slab_of_two_batches(gpu_ctx, tmp_path, monkeypatch):
    data = content(1025, B.BLOCK)
    monkeypatch.setenv("BT_BGZF_SLAB_BYTES", str(1025 * B.BLOCK))
    offsets, st = lib.bgzf_save(gpu_ctx, str(tmp_path / "two.gz"), data)
    got = (tmp_path / "two.gz").read_bytes()
    assert gzip.decompress(got) == data and st["pieces"] == 1026 and not (tmp_path / "two.gz.tmp").exists()
    assert offsets == [b["offset"] for b in B.walk(got)]
    monkeypatch.delenv("BT_BGZF_SLAB_BYTES")
    default_offsets, _ = lib.bgzf_save(gpu_ctx, str(tmp_path / "default.gz"), data)
    assert got == (tmp_path / "default.gz").read_bytes() and default_offsets == offsets
