"""The device's FASTQ reader (bayestyper_amd/csrc/bt_fastq.hip) against its host run and the independent parser of tests/fastq_data.py, byte for byte: the
kernels at their tile edges, the stream object over BGZF blocks cut anywhere, and its text in the reads consumers."""
import numpy as np
import pytest

import bam_data as bd
import fastq_data as fd
import reads_data as rd

pytestmark = pytest.mark.gpu
K = 55


@pytest.fixture(scope="module")
def edge():
    """the edge file with its last line open, and the independent parser's answer — computed once, never changed"""
    data = fd.edge_file(np.random.default_rng(11), K, None, last_newline=False)
    return data, fd.parse(data)


def test_reads_text_equals_the_host_on_the_edge_file(gpu_ctx, edge):
    from bayestyper_amd import lib

    data, want = edge
    host = lib.diag_fastq_reads_text(data)
    assert host == want
    for misalign in range(4):   # (the binding checks the guard bytes behind text_bytes and behind the capacity)
        assert lib.fastq_reads_text(gpu_ctx, data, misalign=misalign) == host, misalign
    assert lib.fastq_reads_text(gpu_ctx, data, capacity=len(host[0]), misalign=1) == host
    with pytest.raises(lib.BtError, match="capacity"):
        lib.fastq_reads_text(gpu_ctx, data, capacity=len(host[0]) - 1)
    closed = data + b"\r\n"
    for final in (False, True):
        assert lib.fastq_reads_text(gpu_ctx, closed, final=final) == lib.diag_fastq_reads_text(closed, final=final) == fd.parse(closed, final=final)
    assert lib.fastq_reads_text(gpu_ctx, b"") == (b"", 0, {"reads": 0, "bases": 0, "lines": 0})
    assert lib.fastq_reads_text(gpu_ctx, b"\n\r\n", final=False) == (b"", 3, {"reads": 0, "bases": 0, "lines": 2})


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1025])
def test_record_counts_around_the_line_tiles(gpu_ctx, n):
    """4 n lines: the sums per 256 lines and the offsets scan cross their edges; reads of 0..40 bases so that the text's offsets are uneven"""
    from bayestyper_amd import lib

    rng = np.random.default_rng(n)
    data = b"".join(fd.record(rng, i, fd.random_seq(rng, int(b)), (b"\n", b"\r\n")[i % 2], header=b"@%d" % i) for i, b in enumerate(rng.integers(0, 41, size=n)))
    want = fd.parse(data)
    assert want[2]["lines"] == 4 * n
    assert lib.fastq_reads_text(gpu_ctx, data) == want
    assert lib.fastq_reads_text(gpu_ctx, data[:-1]) == fd.parse(data[:-1])   # the last line open
    assert lib.fastq_reads_text(gpu_ctx, data[:-1], final=False) == fd.parse(data[:-1], final=False)


@pytest.mark.parametrize("n", fd.MANY_RECORDS)
def test_more_than_65536_lines_equal_the_parser(gpu_ctx, n):
    """256, 257 and 258 sums per 256 lines: the offsets scan (text_offsets_kernel) carries its total from the first round of 256 sums into the second"""
    from bayestyper_amd import lib

    data = fd.short_records(n)
    want = fd.parse(data)
    assert want[2]["lines"] == 4 * n
    assert lib.fastq_reads_text(gpu_ctx, data) == want
    assert lib.fastq_reads_text(gpu_ctx, data[:-1]) == fd.parse(data[:-1])   # the last line open


def ending_at(rng, end, eol):
    """sound records whose last newline is byte end - 1: the last record's header is padded to fit"""
    tail = eol + b"ACGT" + eol + b"+" + eol + b"IIII" + eol
    lead = b""
    while len(lead) + 300 < end - len(tail):
        lead += fd.record(rng, len(lead), fd.random_seq(rng, 30), eol, kind=2)
    data = lead + b"@" + b"h" * (end - len(lead) - 1 - len(tail)) + tail
    assert len(data) == end
    return data


def test_line_ends_around_the_byte_tiles(gpu_ctx):
    """a '\\n', a '\\r\\n' pair and a blank line of either kind moved byte by byte across the edge between two tiles of the line-finding kernels (the first
    edge and the second), and across the edge between two threads' 16 bytes"""
    from bayestyper_amd import lib

    tile = lib.FASTQ_COUNT_TILE
    rng = np.random.default_rng(1)
    back = b"".join(fd.simple_records(rng, 30, 30))
    for eol, blank in ((b"\n", b"\n"), (b"\r\n", b"\r\n"), (b"\r\n", b"\n"), (b"\n", b"\r\n")):
        for edge_at in (tile, 2 * tile, tile + 16):
            for shift in range(-2, 5):   # the record's last newline on the edge's last bytes and on its first bytes; the blank lines follow it
                data = ending_at(rng, edge_at + shift, eol) + blank + blank + back
                assert lib.fastq_reads_text(gpu_ctx, data) == fd.parse(data), (eol, blank, edge_at, shift)


def test_prefixes(gpu_ctx):
    from bayestyper_amd import lib
    from test_fastq_cpu import three_records

    data = three_records()
    whole = fd.parse(data)[0]
    for cut in list(range(0, len(data) + 1, 7)) + [len(data) - 1, len(data)]:
        got = lib.fastq_reads_text(gpu_ctx, data[:cut], final=False)
        assert got == fd.parse(data[:cut], final=False), cut
        rest = lib.fastq_reads_text(gpu_ctx, data[got[1]:], final=True, first_line=1 + got[2]["lines"])
        assert got[0] + rest[0] == whole and got[1] + rest[1] == len(data), cut


def test_errors_equal_the_host(gpu_ctx):
    from bayestyper_amd import lib
    from test_fastq_cpu import SOUND, VIOLATIONS

    cases = [SOUND + bad + SOUND for bad, _, _ in VIOLATIONS.values()]
    cases += [SOUND + b"@r\nACGT\n+", SOUND + b"@r\nACGT\n", SOUND + b"@r"]   # truncated
    cases += [SOUND + b"@r1\nACGT\nIIII\nx\n" + SOUND + b"r2\nAC\n+\nI\n", SOUND * 300 + b"@r\nAC\n+\nIII\n" + SOUND * 300 + b"@r1\nACGT\nIIII\nx\n", SOUND + b"\r"]   # smallest line wins
    for data in cases:
        for final in (True, False):
            try:
                lib.diag_fastq_reads_text(data, final=final, first_line=77)
                message = None
            except lib.BtError as e:
                message = str(e)
            assert message is not None or not final
            if message is None:
                assert lib.fastq_reads_text(gpu_ctx, data, final=final, first_line=77) == lib.diag_fastq_reads_text(data, final=final, first_line=77)
                continue
            with pytest.raises(lib.BtError) as dev:
                lib.fastq_reads_text(gpu_ctx, data, final=final, first_line=77)
            assert str(dev.value) == message, data[:60]


# ---- the stream object ---------------------------------------------------------------------------------------------------------------------------------------
def straddling_cuts(data):
    """content offsets for the BGZF blocks: inside a header, inside a sequence, between '\\r' and '\\n', inside a blank line ("\\r" | "\\n"), and every 997 bytes"""
    cuts = set(range(997, len(data), 997))
    at = data.find(b"@read2 ")
    cuts.add(at + 3)                                   # inside a header
    cuts.add(data.find(b"\n", at) + 20)                # inside a sequence
    cuts.add(data.find(b"\r\n", at) + 1)               # between '\r' and '\n'
    cuts.add(data.find(b"\r\n\n\r\n") + 4)             # inside a blank line
    cuts.add(data.find(b"\r\n\n\r\n") + 3)             # between two blank lines
    return sorted(c for c in cuts if 0 < c < len(data))


def scan_all(gpu_ctx, stream, edges, blocks_per_slab, max_in_bytes=1 << 20):
    from bayestyper_amd import lib

    scan = lib.FastqScan(gpu_ctx, max_in_bytes)
    try:
        out, stats, calls = [], {"reads": 0, "bases": 0, "lines": 0}, 0
        for i in range(0, len(edges) - 1, blocks_per_slab):
            text, st = scan.text_bytes(stream[edges[i]:edges[min(i + blocks_per_slab, len(edges) - 1)]])
            out.append(text)
            stats = {key: stats[key] + st[key] for key in stats}
            calls += 1
        text, st = scan.finish_bytes()
        return b"".join(out), {key: stats[key] + st[key] for key in stats}, text, calls
    finally:
        scan.close()


def test_stream_object_over_straddling_blocks(gpu_ctx, edge):
    data, want = edge
    cuts = straddling_cuts(data)
    cuts.insert(len(cuts) // 2, cuts[len(cuts) // 2])   # an empty block mid-file
    stream, offsets = bd.bgzf(data, cuts)
    edges = offsets + [len(stream)]
    for per_slab in (1, 3, len(edges)):
        text, stats, last, calls = scan_all(gpu_ctx, stream, edges, per_slab)
        assert text + last == want[0] and stats == want[2], per_slab
        assert last == want[0][-78:], per_slab   # the file's last line has no newline: its read comes from _finish
        assert per_slab > 1 or calls > 20   # the 20 000-base read spans many calls
    closed = data + b"\n"
    stream, offsets = bd.bgzf(closed, straddling_cuts(closed), eof=False)
    text, stats, last, _ = scan_all(gpu_ctx, stream, offsets + [len(stream)], 2)
    assert (text, last) == (want[0], b"") and stats["lines"] == want[2]["lines"]


def test_stream_object_refusals(gpu_ctx, edge):
    from bayestyper_amd import lib

    rng = np.random.default_rng(9)
    long_read = fd.record(rng, 0, fd.random_seq(rng, 8 * 65536 + 10), kind=2)
    stream, offsets = bd.bgzf(fd.record(rng, 1, b"ACGT") + long_read, bd.even_cuts(len(long_read), 60000), level=1)
    with pytest.raises(lib.BtError, match="more than a slab may hold \\(524288, 8 x max_in_bytes\\)"):
        scan_all(gpu_ctx, stream, offsets + [len(stream)], 1, max_in_bytes=65536)
    records = b"".join(fd.simple_records(rng, 40, 60))
    two_of_four = records + b"@r\nACGT\n"
    stream, offsets = bd.bgzf(two_of_four, bd.even_cuts(len(two_of_four), 700))
    with pytest.raises(lib.BtError) as e:
        scan_all(gpu_ctx, stream, offsets + [len(stream)], 2)
    assert str(e.value) == fd.MESSAGES["truncated"] % 2
    missing = records + b"@r\nACGT\nIIII\n" + records
    stream, offsets = bd.bgzf(missing, bd.even_cuts(len(missing), 700))
    with pytest.raises(lib.BtError) as e:   # the file's line number, whichever call meets the line
        scan_all(gpu_ctx, stream, offsets + [len(stream)], 1)
    assert str(e.value) == fd.MESSAGES["plus"] % (160 + 3)
    stream, offsets = bd.bgzf(records, bd.even_cuts(len(records), 700))
    edges = offsets + [len(stream)]
    damaged = bytearray(stream)
    damaged[edges[3] + 30] ^= 4   # a bit of block 3's deflate data
    with pytest.raises(lib.BtError, match=f"BGZF block at offset {edges[3]}: "):
        scan_all(gpu_ctx, bytes(damaged), edges, 2)
    for blocks, words in ((stream[:edges[2] + 9], "ends inside the BGZF block at offset"), (bytes(65537), "handed in, the stream was created for 65536")):
        scan = lib.FastqScan(gpu_ctx, 65536)
        try:
            with pytest.raises(lib.BtError, match=words):
                scan.text(blocks)
        finally:
            scan.close()


def test_consumers_over_the_stream_text_equal_the_reads_text(gpu_ctx):
    """reads_count and reads_sketch over FastqScan's device text equal the same calls over the host text of the same reads: identical table rows, hit count
    and registers"""
    from bayestyper_amd import lib

    k = K
    rng = np.random.default_rng(100 + k)
    reads = rd.edge_reads(rng, k) + [rd.random_seq(rng, int(n)) for n in rng.integers(k, 251, size=300)]
    reads += reads[20:60]   # repeated reads: counts above one
    text = rd.reads_text(reads)
    data = b"".join(fd.record(rng, i, bytes(r), (b"\n", b"\r\n")[i % 2]) for i, r in enumerate(reads))[:-1]   # the last line open
    assert fd.parse(data)[0].split(b"\n") == [x for x in text.split(b"\n") if x] + [b""]
    stream, offsets = bd.bgzf(data, bd.even_cuts(len(data), 4099))
    edges = offsets + [len(stream)]
    kmers = np.unique(lib.diag_reads_kmers(text, k)[0], axis=0)
    path = lib.Bloom.create(gpu_ctx, len(kmers), 0.01, k, threaded=False)
    path.insert(np.ascontiguousarray(kmers[::2]))   # half the k-mers: hits and misses
    want_t, got_t = lib.Table(gpu_ctx, 4 * len(kmers) + 1024, 2, k), lib.Table(gpu_ctx, 4 * len(kmers) + 1024, 2, k)
    want_hits = lib.reads_count(gpu_ctx, path, want_t, 1, text)
    want_reg = lib.reads_sketch(gpu_ctx, text, k)
    scan = lib.FastqScan(gpu_ctx, 1 << 20)
    d_hits, d_reg = gpu_ctx.buffer(8).zero(), gpu_ctx.to_device(np.zeros(lib.SKETCH_REGISTERS, np.uint8))
    try:
        def consume(d_text, n):
            if n:
                lib.check(lib.bt_reads_count(gpu_ctx.h, path.h, got_t.h, 1, d_text, n, d_hits.ptr))
                lib.check(lib.bt_reads_sketch(gpu_ctx.h, d_text, n, k, d_reg.ptr))
                gpu_ctx.sync()

        for i in range(0, len(edges) - 1, 7):
            consume(*scan.text(stream[edges[i]:edges[min(i + 7, len(edges) - 1)]])[:2])
        last = scan.finish()
        assert last[1] > 0
        consume(*last[:2])
        assert int(d_hits.download(np.uint64, 1)[0]) == want_hits > 0
        assert np.array_equal(d_reg.download(np.uint8, lib.SKETCH_REGISTERS), want_reg) and want_reg.any()
        want_rows, got_rows = want_t.export(), got_t.export()
        o1, o2 = (np.lexsort((t[0][:, 0], t[0][:, 1])) for t in (want_rows, got_rows))
        assert len(want_rows[0]) > 1000
        for a, b in zip(want_rows, got_rows):
            assert np.array_equal(a[o1], b[o2])
    finally:
        scan.close()
        for x in (d_hits, d_reg):
            x.free()
        for x in (path, want_t, got_t):
            x.close()
