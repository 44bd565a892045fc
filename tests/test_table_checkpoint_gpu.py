"""Packed records and the checkpoint file of the k-mer table, through the C ABI: bt_table_pack / bt_table_unpack / bt_table_save / bt_table_load
(include/btgpu.h).  The table itself is the oracle: what went in through the existing calls (insert, classify, count_intercluster) must come back out
of save -> load as the same set of (key, meta, counts)."""
import os

import numpy as np
import pytest

import _oracle  # noqa: F401  (sys.path set-up)

pytestmark = pytest.mark.gpu

K = 55
HI_BITS = 2 * (K - 32)


def _keys(rng, n):
    """n distinct random keys; the first three are the all-A k-mer, a key with lo == 0 and one with hi == 0 (the cases the ordered publish special-cases)"""
    k = np.empty((n, 2), np.uint64)
    k[:, 0] = rng.integers(1, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    k[:, 1] = rng.integers(1, 1 << HI_BITS, n, dtype=np.uint64)
    special = np.array([[0, 0], [0, 12345], [987654321, 0]], np.uint64)
    k[:min(n, 3)] = special[:min(n, 3)]
    assert len(np.unique(k, axis=0)) == n
    return k


def _records(keys, meta, counts, spad):
    """the packed record of include/btgpu.h: lo, hi (little endian), 4 meta bytes, counts padded with zeros to spad"""
    n = len(keys)
    r = np.zeros((n, 20 + spad), np.uint8)
    r[:, :16] = np.ascontiguousarray(keys, "<u8").view(np.uint8).reshape(n, 16)
    r[:, 16:20] = meta
    r[:, 20:20 + counts.shape[1]] = counts
    return r


def _sorted(export):
    kmers, counts, meta = export
    order = np.lexsort((kmers[:, 0], kmers[:, 1]))
    return kmers[order], counts[order], meta[order]


def _same(a, b):
    a, b = _sorted(a), _sorted(b)
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _unpack_host(table, records):
    buf = table.ctx.to_device(records)
    try:
        table.unpack(buf, len(records))
    finally:
        buf.free()


def _filled(ctx, oracle, lib, rng, S, expected, n):
    """a table whose meta bytes come from the existing calls and whose counts (0 and 255 among them) were set by unpack"""
    keys = _keys(rng, n)
    a = lib.Table(ctx, expected, S, K)
    a.insert(keys[: n // 2], mark_parameter=True)
    a.insert(keys[n // 2:])
    # inter-cluster multiplicities: every k-mer of a random sequence (all of them in the path Bloom), as a diploid / haploid chromosome and as a decoy
    seq = "".join(rng.choice(list("ACGT"), 400)).encode()
    km, va = oracle.kmers_from_sequence(seq, K)
    bloom = lib.Bloom.create(ctx, 1000, 1e-3, K, threaded=True)
    bloom.insert(np.unique(km[va == 1], axis=0))
    a.count_intercluster(bloom, seq, False, 2, 1)
    a.count_intercluster(bloom, seq[:200], True, 0, 0)
    # cluster occurrences: multiplicities up to 200 (above 127: MAX_MULTIPLICITY, and new keys are inserted), some keys in the multigroup Bloom, some twice (MULTICLUSTER)
    bloom.insert(keys[100:140])
    extra = _keys(rng, 60)[3:]
    a.classify(bloom, np.concatenate([keys[50:400], keys[50:120], extra]), rng.integers(1, 201, 350 + 70 + len(extra)).astype(np.uint8))
    bloom.close()
    kmers, _, meta = a.export()
    a.close()
    assert len({tuple(m) for m in meta}) > 20, "the meta bytes should be varied"
    counts = rng.integers(0, 256, (len(kmers), S)).astype(np.uint8)
    counts[::7] = 0
    counts[3::11] = 255
    t = lib.Table(ctx, expected, S, K)
    _unpack_host(t, _records(kmers, meta, counts, (S + 3) & ~3))
    assert _same(t.export(), (kmers, counts, meta))
    return t


@pytest.mark.parametrize("S,slot_bytes", [(3, 32), (10, 48), (30, 64)])
def test_save_load_round_trip(gpu_ctx, oracle, tmp_path, monkeypatch, S, slot_bytes):
    from bayestyper_amd import lib

    rng = np.random.default_rng(100 + S)
    t = _filled(gpu_ctx, oracle, lib, rng, S, 40_000, 5000)   # capacity 2^17: load 0.04
    try:
        assert t.record_bytes() == 20 + ((S + 3) & ~3) and slot_bytes == 4 * ((6 + ((S + 3) & ~3) // 4 + 3) & ~3)
        want, st = t.export(), t.status()
        assert st["capacity"] == 1 << 17 and st["num_keys"] == len(want[0]) > 5000 and not st["overflowed"]
        assert (want[1] == 0).any() and (want[1] == 255).any() and any((want[0] == k).all(1).any() for k in ([0, 0], [0, 12345], [987654321, 0]))
        manifest = "k=55\nsamples=%d\n" % S
        # 64-slot ranges: 2048 of them, some without a READY slot (asserted from the keys' slots); 2048-slot ranges: 64 ranges of about 80 records
        for slots in (64, 2048):
            monkeypatch.setenv("BT_TABLE_CKPT_SLOTS", str(slots))
            occupied = np.unique(t.find(want[0]) // slots)
            assert (1 << 17) // slots >= 5 and (len(occupied) < (1 << 17) // slots) == (slots == 64)
            path = str(tmp_path / f"table_{slots}.ckpt")
            t.save(path, manifest)
            assert not os.path.exists(path + ".tmp")
            assert lib.table_file_info(path) == {"k": K, "num_samples": S, "num_records": st["num_keys"], "manifest": manifest}
            back = lib.Table.load(gpu_ctx, path, manifest)
            try:
                assert _same(back.export(), want)
                fresh = lib.Table(gpu_ctx, st["num_keys"], S, K)   # sized exactly as bt_table_create(expected = records)
                assert back.status() == dict(st, capacity=fresh.status()["capacity"])
                fresh.close()
            finally:
                back.close()
    finally:
        t.close()


@pytest.mark.parametrize("n,expected", [(0, 100), (1, 100), (63, 100), (64, 100), (65, 100), (3000, 2000)],
                         ids=["0-keys", "1-key", "63-keys", "64-keys", "65-keys", "dense-load-0.73"])
def test_pack_counts_and_refuses_a_small_buffer(gpu_ctx, n, expected):
    """the wavefront edges of the pack kernel's reservation; `dense`: capacity 4096 at load 0.73, wavefronts whose lanes are nearly all READY"""
    import ctypes as C

    from bayestyper_amd import lib

    rng = np.random.default_rng(n)
    t = lib.Table(gpu_ctx, expected, 3, K)
    try:
        keys = _keys(rng, n)
        if n:
            t.insert(keys, mark_parameter=True)
        sized = C.c_uint64(99)
        lib.check(lib.bt_table_pack(t.h, None, 0, C.byref(sized)))
        assert sized.value == t.status()["num_keys"] == n
        buf, got = t.pack()
        rb = t.record_bytes()
        rec = buf.download(np.uint8, max(got, 1) * rb)[: got * rb].reshape(got, rb)
        buf.free()
        assert got == n
        want = _records(keys, np.tile(np.array([0x20, 0, 0, 0], np.uint8), (n, 1)), np.zeros((n, 3), np.uint8), 4)
        assert sorted(map(bytes, rec)) == sorted(map(bytes, want))
        if n > 1:   # room for one record too few: an error, and nothing was written (one key: a capacity of zero records is the sizing call)
            small = gpu_ctx.to_device(np.full(n * rb, 0xAB, np.uint8))
            with pytest.raises(lib.BtError, match="too small"):
                lib.check(lib.bt_table_pack(t.h, small.ptr, n - 1, C.byref(sized)))
            assert (small.download(np.uint8, n * rb) == 0xAB).all()
            small.free()
    finally:
        t.close()


def test_unpack_into_other_capacities_and_duplicates(gpu_ctx):
    from bayestyper_amd import lib

    rng = np.random.default_rng(9)
    n, S = 5000, 10
    keys = _keys(rng, n)
    meta = rng.integers(0, 256, (n, 4)).astype(np.uint8)
    counts = rng.integers(0, 256, (n, S)).astype(np.uint8)
    rec = _records(keys, meta, counts, 12)
    src = lib.Table(gpu_ctx, 20_000, S, K)   # capacity 65536
    _unpack_host(src, rec)
    buf, got = src.pack()
    assert got == n
    try:
        for expected in (200_000, 5000):   # capacity 2^19, and 16384: smaller than the source's but sufficient
            dst = lib.Table(gpu_ctx, expected, S, K)
            dst.unpack(buf, got)
            assert dst.status()["capacity"] != src.status()["capacity"] and _same(dst.export(), (keys, counts, meta))
            dst.close()
        # a key that is already there: the call fails, and the record that was there stays as it was
        held = lib.Table(gpu_ctx, 20_000, S, K)
        held.insert(keys[17:18], mark_parameter=True)
        with pytest.raises(lib.BtError, match="1 of 5000 records have a key that the table already held"):
            held.unpack(buf, got)
        slot = held.find(keys[17:18])
        hk, hc, hm = held.export()
        at = int(np.flatnonzero((hk == keys[17]).all(1))[0])
        assert slot[0] >= 0 and list(hm[at]) == [0x20, 0, 0, 0] and not hc[at].any()
        held.close()
        # a table that cannot hold the records raises its overflow flag
        tiny = lib.Table(gpu_ctx, 100, S, K)   # capacity 1024
        tiny.unpack(buf, got)
        st = tiny.status()
        assert st["overflowed"] and st["num_keys"] == 1024
        tiny.close()
    finally:
        buf.free()
        src.close()


def test_load_refuses_and_keeps_nothing(gpu_ctx, tmp_path):
    from bayestyper_amd import lib

    rng = np.random.default_rng(3)
    n, S = 5000, 3
    t = lib.Table(gpu_ctx, 5000, S, K)
    _unpack_host(t, _records(_keys(rng, n), rng.integers(0, 256, (n, 4)).astype(np.uint8), rng.integers(0, 256, (n, S)).astype(np.uint8), 4))
    path = str(tmp_path / "table.ckpt")
    manifest = "k=55\nsamples=3\nsample.0.name=a\nsample.1.name=b\nsample.2.name=c\n"
    t.save(path, manifest)
    t.close()
    gpu_ctx.sync()
    free = gpu_ctx.info()["hbm_free"]
    with pytest.raises(lib.BtError, match=r'manifest line 4 differs: the file has "sample.1.name=b", this run has "sample.1.name=c"'):
        lib.Table.load(gpu_ctx, path, manifest.replace("1.name=b", "1.name=c").replace("2.name=c", "2.name=b"))
    assert gpu_ctx.info()["hbm_free"] == free
    # a damaged record: found by the chunk's CRC after the table was created — which is released again
    data = bytearray(open(path, "rb").read())
    data[len(data) // 2] ^= 0x01
    bad = str(tmp_path / "damaged.ckpt")
    open(bad, "wb").write(bytes(data))
    with pytest.raises(lib.BtError, match="chunk CRC mismatch"):
        lib.Table.load(gpu_ctx, bad, manifest)
    assert gpu_ctx.info()["hbm_free"] == free
    back = lib.Table.load(gpu_ctx, path)   # no expected manifest: any
    assert back.status()["num_keys"] == n
    back.close()
