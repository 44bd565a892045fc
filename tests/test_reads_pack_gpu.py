"""GPU tests of the packed reads: bt_reads_pack / bt_reads_unpack against the host code, and the three packed consumers (bt_reads.hip: reads_packed_kernel)
against the three text consumers and against the brute-force windows."""
import functools

import numpy as np
import pytest

import reads_data as rd
import reads_pack_data as rp

pytestmark = pytest.mark.gpu

T = rd.TILE
GPU_LENGTHS = rp.CPU_LENGTHS + (T - 1, T, T + 1, 2 * T + 77)


def _sorted_export(kmers, counts, meta):
    o = np.lexsort((kmers[:, 0], kmers[:, 1]))
    return kmers[o], counts[o], meta[o]


@functools.lru_cache(maxsize=None)
def _dataset(k):
    """test_reads_gpu.py's data set: 3 000 reads of 150 nt from a 50 kb genome (both strands) plus the edge reads -> (text, its distinct canonical k-mers, a
    tenth of the genome's distinct k-mers)"""
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
    kmers = rd.kmer_multiset(rd.oracle_kmers(orc, text, k)[0])[0]
    gk = rd.kmer_multiset(rd.oracle_kmers(orc, genome, k)[0])[0]
    return text, kmers, np.ascontiguousarray(gk[::10])


def test_pack_and_unpack_equal_the_host_code(gpu_ctx):
    """byte for byte, at every length of the CPU test, one tile and its neighbours and two tiles plus 77; the text 16-byte aligned (vector loads and stores) and
    not (byte loads and stores); unpack writes nothing outside its text"""
    from bayestyper_amd import lib

    rng = np.random.default_rng(1800)
    for n in GPU_LENGTHS:
        text = rp.layout_text(rng, n)
        assert len(text) == n
        want = lib.diag_reads_pack(text)
        assert np.array_equal(want, rp.np_pack(text))
        for misalign in (0, 5):
            got = lib.reads_pack(gpu_ctx, text, misalign=misalign)
            assert np.array_equal(got, want), (n, misalign)
            assert lib.reads_unpack(gpu_ctx, want, n, misalign=misalign) == rp.canonical(text), (n, misalign)


@pytest.mark.parametrize("k", [31, 32, 33, 55, 64])
def test_packed_consumers_equal_the_text_consumers(gpu_ctx, oracle, k):
    """count: the exported table (keys, counts, meta) of an S = 3 table that already holds parameter k-mers, samples 0 and 2, a path filter with false positives,
    and the hit counts; Bloom: the filter bytes; sketch: the 65 536 registers.  The packed reads come from the device's bt_reads_pack."""
    from bayestyper_amd import lib

    text, kmers, path = _dataset(k)
    packed = lib.reads_pack(gpu_ctx, text)
    rng = np.random.default_rng(k)
    bloom = lib.Bloom.create(gpu_ctx, len(path), 0.05, k, threaded=False)
    bloom.insert(path)
    hit = bloom.contains(kmers).astype(bool)
    path_set = set(map(tuple, path.tolist()))
    in_path = np.array([tuple(x) in path_set for x in kmers.tolist()])
    assert hit[in_path].all() and (hit & ~in_path).sum() > 100   # false positives among the reads' k-mers
    param = np.concatenate([kmers[rng.choice(len(kmers), 300, replace=False)], oracle.pack(np.frombuffer(rd.random_seq(rng, 40 * k), np.uint8), k)])
    tables, hits = [], []
    for route in ("text", "packed"):
        t = lib.Table(gpu_ctx, 200_000, 3, k)
        t.insert(param, mark_parameter=True)
        for s in (0, 2):
            hits.append(lib.reads_count(gpu_ctx, bloom, t, s, text) if route == "text" else lib.reads_count_packed(gpu_ctx, bloom, t, s, packed, len(text)))
        assert not t.status()["overflowed"]
        tables.append(_sorted_export(*t.export()))
        t.close()
    (wk, wc, wm), (gk, gc, gm) = tables
    assert hits[0] > 0 and hits == [hits[0]] * 4
    assert np.array_equal(gk, wk) and np.array_equal(gc, wc) and np.array_equal(gm, wm)
    assert (gc[:, 1] == 0).all() and np.array_equal(gc[:, 0], gc[:, 2]) and gc.max() > 1
    bloom.close()
    blooms = []
    for route in ("text", "packed"):
        b = lib.Bloom.create(gpu_ctx, len(kmers), 1e-3, k, threaded=False)
        if route == "text":
            lib.reads_make_bloom(gpu_ctx, b, text, k)
        else:
            lib.reads_make_bloom_packed(gpu_ctx, b, packed, len(text), k)
        blooms.append(b.bits(0))
        b.close()
    assert blooms[0].any() and np.array_equal(blooms[0], blooms[1])
    want = lib.reads_sketch(gpu_ctx, text, k)
    assert (want > 0).sum() > 30_000 and np.array_equal(want, lib.diag_reads_sketch(text, k))
    assert np.array_equal(lib.reads_sketch_packed(gpu_ctx, packed, len(text), k), want)


def _packed_counts(gpu_ctx, lib, text, k, want_kmers, want_counts, packed=None, host=False, chunk_bytes=0):
    """the table bt_reads_count_packed builds with a path filter that holds every k-mer of the text -> (keys sorted, counts of sample 0), checked against the
    multiset handed in"""
    bloom = lib.Bloom.create(gpu_ctx, max(len(want_kmers), 1), 0.01, k, threaded=False)
    if len(want_kmers):
        bloom.insert(want_kmers)
    t = lib.Table(gpu_ctx, 4 * len(want_kmers) + 1024, 1, k)
    packed = lib.diag_reads_pack(text) if packed is None else packed
    hits = lib.reads_count_packed(gpu_ctx, bloom, t, 0, packed, len(text), host=host, chunk_bytes=chunk_bytes)
    gk, gc, _ = _sorted_export(*t.export())
    t.close(), bloom.close()
    assert hits == int(want_counts.sum())
    assert np.array_equal(gk, want_kmers) and np.array_equal(gc[:, 0], np.minimum(want_counts, 255).astype(np.uint8))
    return gk, gc


def _oracle_multiset(text, k):
    import _oracle

    return rd.kmer_multiset(rd.oracle_kmers(_oracle.load_oracle(), text, k)[0])


def _fill(rng, n):
    """n bytes of reads of 150 nt (a newline after each; the last one shorter)"""
    out = bytearray(rd.random_reads_text(rng, n // 151 + 1, 150)[:n])
    if n:
        out[-1:] = b"\n"
    return bytes(out)


@pytest.mark.parametrize("k", [1, 31, 64])
def test_tile_boundaries(gpu_ctx, k):
    """against the oracle's windows: a separator exactly at position 15 359 and at 15 360; a read that crosses the tile boundary with its first full window ending
    at 15 360 + k - 2, - 1 and + 0; a text whose last position is a valid base and not a multiple of 128"""
    from bayestyper_amd import lib

    rng = np.random.default_rng(1900 + k)
    tail = rd.random_seq(rng, 200) + b"\n" + rd.random_seq(rng, 77)   # ends in a base
    for sep in (T - 1, T):
        text = rd.random_seq(rng, sep - 300) + b"\n" + rd.random_seq(rng, 299) + b"\n" + tail
        assert text[sep] == 10 and text[sep - 1] != 10 and text[sep + 1] != 10 and len(text) % 128 != 0 and text[-1] != 10
        _packed_counts(gpu_ctx, lib, text, k, *_oracle_multiset(text, k))
    for end in (T + k - 2, T + k - 1, T + k):
        start = end - k + 1   # the read's first base: its first full window ends at `end`
        if start < 1:
            continue
        text = _fill(rng, start) + rd.random_seq(rng, 150) + b"\n" + tail
        assert text[start - 1] == 10 and 10 not in text[start:start + 150] and len(text) % 128 != 0
        want = _oracle_multiset(text, k)
        _packed_counts(gpu_ctx, lib, text, k, *want)
        ends = lib.diag_reads_kmers_packed(lib.diag_reads_pack(text), len(text), k)[2]
        assert end in ends and (k == 1 or end - 1 not in ends)
    # the brute-force restatement agrees with the oracle's windows on a text of a few reads (a whole tile is too slow for it)
    small = rd.reads_text(rd.edge_reads(rng, k), final_newline=False) + b"ACGTACGTAC" * 7
    ascii_kmers, _ = rd.brute_force_kmers(small, k)
    kmers, counts = _oracle_multiset(small, k)
    assert int(counts.sum()) == len(ascii_kmers) and len(kmers) == len(set(ascii_kmers))
    _packed_counts(gpu_ctx, lib, small, k, kmers, counts)
    # nothing, fewer than k positions, exactly k, one tile exactly and one more
    for text in (b"", rd.random_seq(rng, k - 1), rd.random_seq(rng, k), _fill(rng, T - 100) + rd.random_seq(rng, 100), _fill(rng, T - 100) + rd.random_seq(rng, 101)):
        _packed_counts(gpu_ctx, lib, text, k, *_oracle_multiset(text, k))


@pytest.mark.parametrize("k", [31, 55])
def test_saturation(gpu_ctx, k):
    """a k-mer occurring 300 times ends at 255"""
    from bayestyper_amd import lib

    rng = np.random.default_rng(2000 + k)
    text = (rd.random_seq(rng, k) + b"\n") * 300 + rd.random_seq(rng, 200) + b"\n"
    kmers, counts = _oracle_multiset(text, k)
    assert counts.max() == 300
    gk, gc = _packed_counts(gpu_ctx, lib, text, k, kmers, counts)
    assert gc.max() == 255 and (gc[:, 0] == 255).sum() == 1


@pytest.mark.parametrize("k", [31, 64])
def test_packed_host_whatever_the_chunk_size(gpu_ctx, k):
    """_packed_host with chunk_bytes 48 (one block a transfer), 4 080 and the default gives the default's table and registers; so does the Bloom filter"""
    from bayestyper_amd import lib

    text = _dataset(k)[0]
    short = text[:text.index(b"\n", 60_000) + 1]   # one block a transfer is 128 positions a launch: a shorter text keeps the test quick
    for t, chunks in ((text, (0, 4080)), (short, (0, 48, 4080))):
        packed = lib.diag_reads_pack(t)
        kmers, counts = _oracle_multiset(t, k)
        want_reg = lib.diag_reads_sketch(t, k)
        want_bits = None
        for chunk in chunks:
            _packed_counts(gpu_ctx, lib, t, k, kmers, counts, packed=packed, host=True, chunk_bytes=chunk)
            assert np.array_equal(lib.reads_sketch_packed(gpu_ctx, packed, len(t), k, host=True, chunk_bytes=chunk), want_reg), chunk
            b = lib.Bloom.create(gpu_ctx, len(kmers), 1e-3, k, threaded=False)
            lib.reads_make_bloom_packed(gpu_ctx, b, packed, len(t), k, host=True, chunk_bytes=chunk)
            bits = b.bits(0)
            b.close()
            assert want_bits is None or np.array_equal(bits, want_bits), chunk
            want_bits = bits


def test_garbage_in_the_padding_changes_nothing(gpu_ctx):
    from bayestyper_amd import lib

    k = 31
    rng = np.random.default_rng(2100)
    text = _fill(rng, T + 1000) + rd.random_seq(rng, 61)   # ends in a base, 61 positions into its last block
    assert len(text) % 128 != 0
    packed = lib.diag_reads_pack(text)
    kmers, counts = _oracle_multiset(text, k)
    want = lib.reads_sketch_packed(gpu_ctx, packed, len(text), k)
    assert np.array_equal(want, lib.diag_reads_sketch(text, k))
    for p in (rp.garbage_padding(packed, len(text)), rp.garbage_padding(packed, len(text), rng)):
        assert not np.array_equal(p, packed)
        _packed_counts(gpu_ctx, lib, text, k, kmers, counts, packed=p)
        _packed_counts(gpu_ctx, lib, text, k, kmers, counts, packed=p, host=True, chunk_bytes=480)
        assert np.array_equal(lib.reads_sketch_packed(gpu_ctx, p, len(text), k), want)
    # positions beyond `positions` that hold real reads are ignored too
    cut = T + 500
    _packed_counts(gpu_ctx, lib, text[:cut], k, *_oracle_multiset(text[:cut], k), packed=packed)


def test_error_paths(gpu_ctx):
    from bayestyper_amd import lib

    b31 = lib.Bloom.create(gpu_ctx, 100, 0.01, 31, threaded=False)
    t55, t31 = lib.Table(gpu_ctx, 100, 2, 55), lib.Table(gpu_ctx, 100, 2, 31)
    p = lib.diag_reads_pack(b"ACGT\n")
    with pytest.raises(lib.BtError, match="k mismatch"):
        lib.reads_count_packed(gpu_ctx, b31, t55, 0, p, 5)
    with pytest.raises(lib.BtError, match="sample index out of range"):
        lib.reads_count_packed(gpu_ctx, b31, t31, 2, p, 5, host=True)
    with pytest.raises(lib.BtError, match="k must lie in 1 .. 64"):
        lib.reads_sketch_packed(gpu_ctx, p, 5, 65)
    with pytest.raises(lib.BtError, match="k mismatch"):
        lib.reads_make_bloom_packed(gpu_ctx, b31, p, 5, 55)
    for x in (b31, t55, t31):
        x.close()
