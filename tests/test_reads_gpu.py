"""GPU tests of the reads scan (bt_reads.hip): the three consumers fed from a reads text compute what the KMC route computes from a database of the same reads."""
import functools

import numpy as np
import pytest

import reads_data as rd
from _oracle import OrcKmc

pytestmark = pytest.mark.gpu


def _sorted_export(kmers, counts, meta):
    o = np.lexsort((kmers[:, 0], kmers[:, 1]))
    return kmers[o], counts[o], meta[o]


def _ascii_sorted(oracle, packed, counts, k):
    """distinct packed k-mers -> (ASCII rows in ascending order, which is the order of a KMC database; their counts)"""
    a = oracle.unpack(packed, k).reshape(-1, k)
    o = np.argsort(np.ascontiguousarray(a).view(f"S{k}").ravel(), kind="stable")
    return np.ascontiguousarray(a[o]), counts[o]


def _write_db(oracle, tmp_path, name, packed, counts, k):
    km, c = _ascii_sorted(oracle, packed, counts, k)
    prefix = str(tmp_path / name)
    oracle.kmc_write(prefix, km.reshape(-1), np.minimum(c, 255).astype(np.uint32), k, k % 4 + 4 if k % 4 else 4, 1)
    return prefix


@functools.lru_cache(maxsize=None)
def _dataset(k):
    """about 3 000 reads of 150 nt from a 50 kb genome (both strands), plus the edge reads -> (text, distinct canonical k-mers, occurrences, a tenth of the
    genome's distinct k-mers)"""
    import _oracle

    orc = _oracle.load_oracle()
    rng = np.random.default_rng(500 + k)
    genome = rd.random_seq(rng, 50_000)
    reads = []
    for s in rng.integers(0, len(genome) - 150, size=3000):
        r = genome[s:s + 150]
        reads.append(rd.revcomp(r) if rng.integers(2) else r)
    reads += rd.edge_reads(rng, k)
    text = rd.reads_text(reads)
    kmers, counts = rd.kmer_multiset(rd.oracle_kmers(orc, text, k)[0])
    gk = rd.kmer_multiset(rd.oracle_kmers(orc, genome, k)[0])[0]
    return text, kmers, counts, np.ascontiguousarray(gk[::10])


@pytest.mark.parametrize("k", [31, 32, 33, 55, 64])
def test_count_equals_the_kmc_route(gpu_ctx, oracle, tmp_path, k):
    """one table filled through bt_kmc_scan_run from a database of the reads' canonical k-mers (counts capped at 255), another through bt_reads_count from the
    reads, same path filter (a tenth of the genome's k-mers at fpr 0.05: false-positive inserts occur), S = 3 with samples 0 and 2, a table that already holds
    parameter k-mers: equal keys, counts and meta; the hit count is the number of occurrences of the k-mers that hit"""
    from bayestyper_amd import lib

    text, kmers, counts, path = _dataset(k)
    rng = np.random.default_rng(k)
    prefix = _write_db(oracle, tmp_path, "reads_db", kmers, counts, k)
    bloom = lib.Bloom.create(gpu_ctx, len(path), 0.05, k, threaded=False)
    bloom.insert(path)
    hit = bloom.contains(kmers).astype(bool)
    path_set = set(map(tuple, path.tolist()))
    in_path = np.array([tuple(x) in path_set for x in kmers.tolist()])
    assert hit[in_path].all() and (hit & ~in_path).sum() > 100   # false positives among the reads' k-mers
    param = np.concatenate([kmers[rng.choice(len(kmers), 300, replace=False)], oracle.pack(np.frombuffer(rd.random_seq(rng, 40 * k), np.uint8), k)])
    tables = []
    for route in ("kmc", "reads"):
        t = lib.Table(gpu_ctx, 200_000, 3, k)
        t.insert(param, mark_parameter=True)
        if route == "kmc":
            db = OrcKmc(oracle, prefix)
            scan = lib.KmcScan(gpu_ctx, db.k, db.p, db.counter_size, db.total, db.lut())
            d = gpu_ctx.to_device(db.payload())
            d_hits = gpu_ctx.buffer(8).zero()
            for s in (0, 2):
                scan.run(bloom, t, s, d.ptr, 0, db.total, d_hits.ptr)
            gpu_ctx.sync()
            assert int(d_hits.download(np.uint64, 1)[0]) == 2 * int(hit.sum())
            d.free(), d_hits.free(), scan.close(), db.close()
        else:
            for s in (0, 2):
                assert lib.reads_count(gpu_ctx, bloom, t, s, text) == int(counts[hit].sum())
        assert not t.status()["overflowed"]
        tables.append(_sorted_export(*t.export()))
        t.close()
    (wk, wc, wm), (gk, gc, gm) = tables
    assert np.array_equal(gk, wk) and np.array_equal(gc, wc) and np.array_equal(gm, wm)
    assert (gc[:, 1] == 0).all() and np.array_equal(gc[:, 0], gc[:, 2]) and gc.max() > 1
    bloom.close()


def _all_hit_counts(gpu_ctx, lib, text, k, host=False, chunk_bytes=0):
    """the table bt_reads_count builds with a path filter that holds every k-mer of the text -> (keys sorted, counts of sample 0); checked against numpy's
    multiset of the oracle's windows"""
    import _oracle

    kmers, counts = rd.kmer_multiset(rd.oracle_kmers(_oracle.load_oracle(), text, k)[0])
    bloom = lib.Bloom.create(gpu_ctx, max(len(kmers), 1), 0.01, k, threaded=False)
    if len(kmers):
        bloom.insert(kmers)
    t = lib.Table(gpu_ctx, 4 * len(kmers) + 1024, 1, k)
    hits = lib.reads_count(gpu_ctx, bloom, t, 0, text, host=host, chunk_bytes=chunk_bytes)
    gk, gc, _ = _sorted_export(*t.export())
    t.close(), bloom.close()
    assert hits == int(counts.sum())
    assert np.array_equal(gk, kmers) and np.array_equal(gc[:, 0], np.minimum(counts, 255).astype(np.uint8))
    return gk, gc


def _fill(rng, n):
    """n bytes of reads of 150 nt (a newline after each; the last one shorter)"""
    out = bytearray(rd.random_reads_text(rng, n // 151 + 1, 150)[:n])
    if n:
        out[-1:] = b"\n"
    return bytes(out)


@pytest.mark.parametrize("k", [31, 64])
def test_tile_and_lane_run_boundaries(gpu_ctx, k):
    """a read that ends on the last byte of a tile, one that starts there and one that straddles it; a text of exactly one tile; a text of k - 1 bytes; no text"""
    from bayestyper_amd import lib

    rng = np.random.default_rng(70 + k)
    T = rd.TILE
    text = _fill(rng, T - 150) + rd.random_seq(rng, 150)                  # [T - 150, T): ends on the last byte of tile 0
    text += b"\n" + _fill(rng, T - 2) + rd.random_seq(rng, 150) + b"\n"   # starts at 2T - 1, the last byte of tile 1
    text += _fill(rng, 3 * T - len(text) - 75) + rd.random_seq(rng, 150) + b"\n"   # straddles the end of tile 2
    text += _fill(rng, 500)
    assert text[T - 1] != 10 and text[T - 151] == 10 and text[2 * T - 2] == 10 and text[2 * T - 1] != 10 and 10 not in text[3 * T - 75:3 * T + 75]
    _all_hit_counts(gpu_ctx, lib, text, k)
    one = _fill(rng, T - 100) + rd.random_seq(rng, 100)
    assert len(one) == T
    _all_hit_counts(gpu_ctx, lib, one, k)
    _all_hit_counts(gpu_ctx, lib, one + b"A", k)
    _all_hit_counts(gpu_ctx, lib, rd.random_seq(rng, k - 1), k)
    _all_hit_counts(gpu_ctx, lib, rd.random_seq(rng, k), k)
    _all_hit_counts(gpu_ctx, lib, b"", k)
    # a read as long as two tiles: every lane's run lies inside it
    _all_hit_counts(gpu_ctx, lib, rd.random_seq(rng, 2 * T + 17) + b"\n", k)


@pytest.mark.parametrize("k", [31, 55])
def test_contention_and_saturation(gpu_ctx, k):
    """400 copies of one 70-mer in a row: every k-mer of the read ends at 255; 64 identical short reads back to back: one wavefront's lanes meet in the same slots"""
    from bayestyper_amd import lib

    rng = np.random.default_rng(90 + k)
    gk, gc = _all_hit_counts(gpu_ctx, lib, rd.random_seq(rng, 70) * 400 + b"\n", k)
    assert len(gk) <= 70 and (gc[:, 0] == 255).all()
    short = rd.random_seq(rng, rd.RUN - 1) + b"\n"   # a read per lane run
    gk, gc = _all_hit_counts(gpu_ctx, lib, short * 64, k)
    assert (gc[:, 0] % 64 == 0).all()
    gk, gc = _all_hit_counts(gpu_ctx, lib, (rd.random_seq(rng, k) + b"\n") * 3000, k)
    assert len(gk) == 1 and gc[0, 0] == 255


def test_make_bloom_equals_the_kmc_route(gpu_ctx, oracle, tmp_path):
    """bt_reads_make_bloom into bt_bloom_create(N, 0.001) sets the bits bt_kmc_scan_make_bloom sets from the database of the same reads, N = its k-mer count"""
    from bayestyper_amd import lib

    k = 55
    text, kmers, counts, _ = _dataset(k)
    db = OrcKmc(oracle, _write_db(oracle, tmp_path, "bloom_db", kmers, counts, k))
    assert db.total == len(kmers)
    want = lib.Bloom.create(gpu_ctx, db.total, 1e-3, k, threaded=False)
    scan = lib.KmcScan(gpu_ctx, db.k, db.p, db.counter_size, db.total, db.lut())
    d = gpu_ctx.to_device(db.payload())
    scan.make_bloom(want, d.ptr, 0, db.total)
    gpu_ctx.sync()
    got = lib.Bloom.create(gpu_ctx, db.total, 1e-3, k, threaded=False)
    lib.reads_make_bloom(gpu_ctx, got, text, k)
    bits = want.bits(0)
    assert bits.any() and np.array_equal(got.bits(0), bits)
    # the host variant over three slabs
    host = lib.Bloom.create(gpu_ctx, db.total, 1e-3, k, threaded=False)
    lib.reads_make_bloom(gpu_ctx, host, text, k, host=True, chunk_bytes=len(text) // 3 + 1)
    assert np.array_equal(host.bits(0), bits)
    with pytest.raises(lib.BtError, match="k mismatch"):
        lib.reads_make_bloom(gpu_ctx, got, text, 31)
    d.free()
    for x in (scan, db, want, got, host):
        x.close()


def _slabs(text, n):
    """the text cut into n slabs at read boundaries"""
    cuts = [0] + [text.index(b"\n", len(text) * i // n) + 1 for i in range(1, n)] + [len(text)]
    return [text[a:b] for a, b in zip(cuts, cuts[1:])]


def test_sketch_equals_the_host_front_end(gpu_ctx):
    """device registers equal the host front end's byte for byte; the text in 1, 2 and 7 slabs gives the same registers; so does the host variant"""
    from bayestyper_amd import lib

    k = 31
    text = _dataset(k)[0]
    want = lib.diag_reads_sketch(text, k)
    assert (want > 0).sum() > 30_000
    for n in (1, 2, 7):
        reg = None
        for slab in _slabs(text, n):
            reg = lib.reads_sketch(gpu_ctx, slab, k, registers=reg)
        assert np.array_equal(reg, want), n
    assert np.array_equal(lib.reads_sketch(gpu_ctx, text, k, host=True, chunk_bytes=len(text) // 3 + 1), want)
    assert np.array_equal(lib.reads_sketch(gpu_ctx, b"", k), np.zeros(lib.SKETCH_REGISTERS, np.uint8))
    assert np.array_equal(lib.reads_sketch(gpu_ctx, text, 64, host=True, chunk_bytes=70_001), lib.diag_reads_sketch(text, 64))


@pytest.mark.parametrize("k", [31, 64])
def test_host_count_over_three_slabs(gpu_ctx, k):
    """bt_reads_count_host returns what the device-buffer call returns, whatever the transfer size: chunks overlap by k - 1 bytes and no window counts twice"""
    from bayestyper_amd import lib

    text = _dataset(k)[0]
    want = _all_hit_counts(gpu_ctx, lib, text, k)
    for chunk in (len(text) // 3 + 1, 64, 4099):
        got = _all_hit_counts(gpu_ctx, lib, text if chunk != 64 else text[:20_000], k, host=True, chunk_bytes=chunk)
        if chunk != 64:
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_error_paths(gpu_ctx):
    from bayestyper_amd import lib

    b31 = lib.Bloom.create(gpu_ctx, 100, 0.01, 31, threaded=False)
    t55, t31 = lib.Table(gpu_ctx, 100, 2, 55), lib.Table(gpu_ctx, 100, 2, 31)
    with pytest.raises(lib.BtError, match="k mismatch"):
        lib.reads_count(gpu_ctx, b31, t55, 0, b"ACGT\n")
    with pytest.raises(lib.BtError, match="sample index out of range"):
        lib.reads_count(gpu_ctx, b31, t31, 2, b"ACGT\n")
    with pytest.raises(lib.BtError, match="sample index out of range"):
        lib.reads_count(gpu_ctx, b31, t31, 2, b"ACGT\n", host=True)
    with pytest.raises(lib.BtError, match="k must lie in 1 .. 64"):
        lib.reads_sketch(gpu_ctx, b"ACGT\n", 65)
    for x in (b31, t55, t31):
        x.close()
