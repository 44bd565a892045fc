"""GPU tests of the BAM route (bt_inflate.hip, bt_bam.hip): the device's BGZF inflate against the host run of the same code and zlib, the records' text against
the host's, the stream object at every slab size, damaged blocks beside sound ones, and the three reads consumers over the stream's text."""
import zlib

import numpy as np
import pytest

import bam_data as bd
import reads_data as rd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kinds():
    return bd.contents(np.random.default_rng(11), 65536)


def test_inflate_equals_host_equals_zlib(gpu_ctx, kinds):
    """one call of about 300 blocks: every (level, strategy), every size and content kind, full 65280-byte blocks, empty blocks, several deflate blocks in a
    member, a distance code set of one code"""
    from bayestyper_amd import lib

    datas, blocks = [], []
    for level, strategy in bd.STRATEGIES:
        for size in bd.SIZES:
            if level == 0 and size > bd.STORED_MAX:
                continue
            for name, content in kinds.items():
                if size == 65536 and (name == "random" or level == 0):
                    continue
                if size > 32768 and name in ("zeros", "periodic") and level not in (0, 6):
                    continue   # (keeps the call near 300 blocks; the CPU test runs these)
                datas.append(content[:size])
                blocks.append(bd.bgzf_block(datas[-1], level, strategy))
        datas.append(kinds["reads"][:65280])
        blocks.append(bd.bgzf_block(datas[-1], level, strategy))
        blocks.append(bd.EOF_BLOCK)   # an empty block mid-stream
        datas.append(b"")
    many = kinds["reads"][:30000] + kinds["periodic"][:20000] + kinds["random"][:3000]
    datas.append(many)
    blocks.append(bd.frame(bd.raw_deflate(many, 6, flush_at=(1, 29999, 30000, 50001)), many))
    payload, single = bd.single_distance_code(500)
    datas.append(single)
    blocks.append(bd.frame(payload, single))
    run = (b"ab" * 40000)[:65536]
    datas.append(run)
    blocks.append(bd.bgzf_block(run, 9))
    stream, want = b"".join(blocks), b"".join(datas)
    assert 150 <= len(blocks) <= 400
    assert all(zlib.decompress(b[18:-8], -15) == d for b, d in zip(blocks, datas))
    host = lib.diag_bgzf_inflate(stream)
    got = lib.bgzf_inflate(gpu_ctx, stream, guard=256)
    assert host == want
    assert got[:len(want)] == want
    assert got[len(want):] == b"\xa5" * 256, "bytes behind the output were written"


def test_inflate_capacity_below_total_is_refused_before_any_launch(gpu_ctx, kinds):
    from bayestyper_amd import lib

    stream = bd.bgzf(kinds["reads"][:4000], [2000])[0]
    keep = {}
    with pytest.raises(lib.BtError, match="capacity 3999 below the block table's total of 4000"):
        lib.bgzf_inflate(gpu_ctx, stream, capacity=3999, keep=keep)
    assert keep["out"] == b"\xa5" * 4000


def test_damaged_blocks_beside_good_ones(gpu_ctx, kinds):
    """the error path: CRC mismatch, wrong ISIZE, distance before the start — each of which the host code already turned into an error in test_bam_cpu.py — in a
    launch beside 20 good blocks: the host's message, and the good blocks' data intact"""
    from bayestyper_amd import lib

    good = [kinds["reads"][i * 1500:(i + 1) * 1500] for i in range(20)]
    good_blocks = [bd.bgzf_block(g) for g in good]
    body = kinds["reads"][40000:44000]
    payload = bd.raw_deflate(body)
    p, isize = bd.fixed_distance_before_start()
    cases = {"crc": bd.frame(payload, body, crc=zlib.crc32(body) ^ 1), "isize": bd.frame(payload, body, isize=len(body) + 1), "distance": bd.frame(p, bytes(isize))}
    for name, bad in cases.items():
        stream = b"".join(good_blocks[:7]) + bad + b"".join(good_blocks[7:])
        with pytest.raises(lib.BtError) as host:
            lib.diag_bgzf_inflate(stream, file_offset=77)
        keep = {}
        with pytest.raises(lib.BtError) as dev:
            lib.bgzf_inflate(gpu_ctx, stream, file_offset=77, guard=64, keep=keep)
        assert str(dev.value) == str(host.value) and f"BGZF block at offset {77 + sum(map(len, good_blocks[:7]))}: " in str(dev.value), name
        out, bad_isize = keep["out"], lib.bgzf_scan_blocks(bad)[2]
        assert out[:7 * 1500] == b"".join(good[:7]) and out[7 * 1500 + bad_isize:-64] == b"".join(good[7:]), name
        assert out[-64:] == b"\xa5" * 64, name


@pytest.fixture(scope="module")
def edge_bam():
    recs = bd.edge_records(np.random.default_rng(55), 55) + bd.edge_records(np.random.default_rng(31), 31)
    rng = np.random.default_rng(8)
    recs += bd.bam_of_reads([rd.random_seq(rng, int(n)) for n in rng.integers(0, 400, size=700)], flags=[int(f) for f in rng.choice([0, 0x10, 0x100, 0x800, 0x4], size=700)])
    return recs, b"".join(r for r, _, _ in recs)


def test_reads_text_equals_the_host(gpu_ctx, edge_bam):
    """more than two tiles of records, a 20 000-nt read, every cut of the last record, a buffer that starts off a 16-byte boundary"""
    from bayestyper_amd import lib

    recs, bam = edge_bam
    assert len(recs) > 2 * 256
    for skip in (0x900, 0):
        want = lib.diag_bam_reads_text(bam, skip)
        assert want[0] == bd.records_text(recs, skip) and want[1] == len(bam)
        for misalign in (0, 5):
            assert lib.bam_reads_text(gpu_ctx, bam, skip, misalign=misalign) == want
    last = len(recs[-1][0])
    for cut in (1, 3, 4, 5, 35, 36, 37, last - 1):
        part = bam[:len(bam) - last + cut]
        got = lib.bam_reads_text(gpu_ctx, part, 0x900, misalign=3)
        assert got == lib.diag_bam_reads_text(part, 0x900) and got[1] == len(bam) - last
    assert lib.bam_reads_text(gpu_ctx, b"", 0) == (b"", 0, {"kept": 0, "skipped": 0, "bases": 0})
    long = bd.record(rd.random_seq(np.random.default_rng(1), 70000))   # a record that spans many of the walk's segments
    assert lib.bam_reads_text(gpu_ctx, long * 2 + bam[:500], 0) == lib.diag_bam_reads_text(long * 2 + bam[:500], 0)


@pytest.fixture(scope="module")
def many_records():
    return bd.short_records()


@pytest.mark.parametrize("n", bd.MANY_RECORDS)
def test_more_than_65536_records_equal_the_host(gpu_ctx, many_records, n):
    """256, 257 and 258 sums per 256 records: the offsets scan (text_offsets_kernel) carries its total from the first round of 256 sums into the second"""
    from bayestyper_amd import lib

    recs = many_records[:n]
    bam = b"".join(r for r, _, _ in recs)
    for skip in (0x900, 0):
        kept = [s for _, s, f in recs if not f & skip]
        want = lib.diag_bam_reads_text(bam, skip)
        assert want == (bd.records_text(recs, skip), len(bam), {"kept": len(kept), "skipped": n - len(kept), "bases": sum(map(len, kept))})
        assert lib.bam_reads_text(gpu_ctx, bam, skip) == want


def test_bytes_that_look_like_records_do_not_move_a_start(gpu_ctx):
    """the device walks the slab in segments (1 KiB at this size) from guessed record starts and checks the guesses in order.  Here auxiliary arrays hold whole
    chains of well-formed records — some ending with their host record, some running over its end into the next record — so segments guess starts that are
    none: the text is still the host's, which walks from offset 0"""
    from bayestyper_amd import lib

    rng = np.random.default_rng(21)
    fake = b"".join(bd.record(rd.random_seq(rng, 20), name=b"f") for _ in range(70))   # 70 records of 68 bytes
    over = bytearray(fake)
    over[-68:-64] = (64 + 300).to_bytes(4, "little")   # the last one claims 300 bytes behind its host's end
    recs = []
    for i in range(400):
        s = rd.random_seq(rng, int(rng.integers(30, 200)))
        aux = b""
        if i % 40 == 7:
            body = fake if i % 80 == 7 else bytes(over)
            pad = bytes(int(rng.integers(0, 64)))   # the chain starts at any offset inside a segment
            aux = b"XBBC" + (len(pad) + len(body)).to_bytes(4, "little") + pad + body
        recs.append((bd.record(s, name=b"host%d" % i, aux=aux), s, 0))
    bam = b"".join(r for r, _, _ in recs)
    want = lib.diag_bam_reads_text(bam, 0)
    assert want[0] == bd.records_text(recs, 0) and want[1] == len(bam) and want[2]["kept"] == 400
    for misalign in (0, 7):
        assert lib.bam_reads_text(gpu_ctx, bam, 0, misalign=misalign) == want
    cut = bam[:len(bam) - 30]   # the walk ends inside the last record
    assert lib.bam_reads_text(gpu_ctx, cut, 0) == lib.diag_bam_reads_text(cut, 0)


def test_reads_text_errors_equal_the_host(gpu_ctx, edge_bam):
    from bayestyper_amd import lib

    recs, bam = edge_bam
    for tail, offset, words in bd.invalid_records():
        data = bam + tail   # the failing record lies behind two tiles of sound ones
        with pytest.raises(lib.BtError) as host:
            lib.diag_bam_reads_text(data, 0)
        with pytest.raises(lib.BtError) as dev:
            lib.bam_reads_text(gpu_ctx, data, 0)
        assert str(dev.value) == str(host.value) == f"BAM record at offset {len(bam) + offset}: {words}"
    want = bd.records_text(recs, 0)
    with pytest.raises(lib.BtError, match="capacity"):
        lib.bam_reads_text(gpu_ctx, bam, 0, capacity=len(want) - 1)   # (the binding checks the bytes behind the capacity)
    assert lib.bam_reads_text(gpu_ctx, bam, 0, capacity=len(want))[0] == want


def bam_file(recs, block_bytes, level=6):
    """header + records as a BGZF file cut every block_bytes of content, with an empty block mid-file -> (file, its blocks' offsets, header length)"""
    head = bd.header(text=b"@HD\tVN:1.6\n@CO\t" + b"x" * 3000 + b"\n", refs=[("chr%d" % i, 1000 + i) for i in range(40)])
    data = head + b"".join(r for r, _, _ in recs)
    cuts = bd.even_cuts(len(data), block_bytes)
    cuts.insert(len(cuts) // 2, cuts[len(cuts) // 2])
    stream, offsets = bd.bgzf(data, cuts, level)
    return stream, offsets + [len(stream)], len(head)


def scan_text(gpu_ctx, stream, edges, blocks_per_slab, skip_first, skip_flags=0x900):
    from bayestyper_amd import lib

    scan = lib.BamScan(gpu_ctx, 1 << 20, skip_flags)
    try:
        out, stats = [], {"kept": 0, "skipped": 0, "bases": 0}
        for i in range(0, len(edges) - 1, blocks_per_slab):
            text, st = scan.text_bytes(stream[edges[i]:edges[min(i + blocks_per_slab, len(edges) - 1)]], skip_first if i == 0 else 0)
            out.append(text)
            stats = {key: stats[key] + st[key] for key in stats}
        scan.finish()
        return b"".join(out), stats
    finally:
        scan.close()


def test_stream_object_slab_size_sweep(gpu_ctx, edge_bam):
    """one file fed in slabs of 1, 2, 3 and 64 blocks of about 1 KiB of content: records and block_size fields straddle blocks and slabs, the header runs over
    the first slabs, a 20 000-nt record over twenty of them"""
    recs, _ = edge_bam
    stream, edges, head = bam_file(recs, 1021)
    assert head > 3 * 1021
    want = bd.records_text(recs, 0x900)
    kept = [s for _, s, f in recs if not f & 0x900]
    for per_slab in (1, 2, 3, 64):
        text, stats = scan_text(gpu_ctx, stream, edges, per_slab, head)
        assert text == want, per_slab
        assert stats == {"kept": len(kept), "skipped": len(recs) - len(kept), "bases": sum(map(len, kept))}, per_slab
    assert scan_text(gpu_ctx, stream, edges, 5, head, skip_flags=0)[0] == bd.records_text(recs, 0)


def test_stream_object_refusals(gpu_ctx, edge_bam):
    from bayestyper_amd import lib

    recs, _ = edge_bam
    stream, edges, head = bam_file(recs[:40], 1021)
    with pytest.raises(lib.BtError, match="truncated"):   # the file ends inside a record
        scan_text(gpu_ctx, stream, edges[:-3], 4, head)
    scan = lib.BamScan(gpu_ctx, 65536)
    try:
        with pytest.raises(lib.BtError, match="ends inside the BGZF block at offset"):
            scan.text(stream[:edges[2] + 9], head)
    finally:
        scan.close()
    scan = lib.BamScan(gpu_ctx, 65536)
    try:
        with pytest.raises(lib.BtError, match="handed in, the stream was created for 65536"):
            scan.text(bytes(65537))
    finally:
        scan.close()
    huge = bd.header() + (9 * 65536).to_bytes(4, "little") + bytes(100)   # a block_size above 8 x max_in_bytes
    scan = lib.BamScan(gpu_ctx, 65536)
    try:
        with pytest.raises(lib.BtError, match="more than a slab may hold"):
            scan.text(bd.bgzf(huge, [])[0], len(bd.header()))
    finally:
        scan.close()
    # a damaged block inside a file: one of the three cases of test_damaged_blocks_beside_good_ones (CRC mismatch), which the host run refuses first;
    # the stream object names the block by its offset in the file
    damaged = bytearray(stream)
    damaged[edges[4] - 8] ^= 1   # block 3's CRC-32
    with pytest.raises(lib.BtError) as host:
        lib.diag_bgzf_inflate(bytes(damaged[edges[2]:edges[4]]), file_offset=edges[2])
    assert str(host.value) == f"BGZF block at offset {edges[3]}: CRC-32 mismatch"
    with pytest.raises(lib.BtError) as dev:
        scan_text(gpu_ctx, bytes(damaged), edges, 2, head)
    assert str(dev.value) == str(host.value)


@pytest.mark.parametrize("k", [31, 55])
def test_consumers_over_the_stream_text_equal_the_reads_text(gpu_ctx, k):
    """reads_count, reads_make_bloom and reads_sketch over BamScan's device text equal the same calls over reads_data.reads_text of the same reads: identical
    table rows and hit counts, filter bytes, registers"""
    from bayestyper_amd import lib

    rng = np.random.default_rng(100 + k)
    reads = rd.edge_reads(rng, k) + [rd.random_seq(rng, int(n)) for n in rng.integers(k, 251, size=300)]
    reads += reads[20:60]   # repeated reads: counts above one
    text = rd.reads_text(reads)
    recs = bd.bam_of_reads(reads, flags=[(0, 0x10, 0x4)[i % 3] for i in range(len(reads))])
    dup = bd.bam_of_reads(reads[30:50], flags=[0x100, 0x800] * 10)   # secondary and supplementary copies the text does not hold
    recs = recs[:100] + dup + recs[100:]
    stream, edges, head = bam_file(recs, 4099)
    kmers = np.unique(lib.diag_reads_kmers(text, k)[0], axis=0)
    path = lib.Bloom.create(gpu_ctx, len(kmers), 0.01, k, threaded=False)
    path.insert(np.ascontiguousarray(kmers[::2]))   # half the k-mers: hits and misses
    want_t, got_t = lib.Table(gpu_ctx, 4 * len(kmers) + 1024, 2, k), lib.Table(gpu_ctx, 4 * len(kmers) + 1024, 2, k)
    want_b, got_b = (lib.Bloom.create(gpu_ctx, len(kmers), 1e-3, k, threaded=False) for _ in range(2))
    want_hits = lib.reads_count(gpu_ctx, path, want_t, 1, text)
    lib.reads_make_bloom(gpu_ctx, want_b, text, k)
    want_reg = lib.reads_sketch(gpu_ctx, text, k)
    scan = lib.BamScan(gpu_ctx, 1 << 20)
    d_hits, d_reg = gpu_ctx.buffer(8).zero(), gpu_ctx.to_device(np.zeros(lib.SKETCH_REGISTERS, np.uint8))
    try:
        for i in range(0, len(edges) - 1, 7):
            d_text, n, _ = scan.text(stream[edges[i]:edges[min(i + 7, len(edges) - 1)]], head if i == 0 else 0)
            lib.check(lib.bt_reads_count(gpu_ctx.h, path.h, got_t.h, 1, d_text, n, d_hits.ptr))
            lib.check(lib.bt_reads_make_bloom(gpu_ctx.h, got_b.h, d_text, n, k))
            lib.check(lib.bt_reads_sketch(gpu_ctx.h, d_text, n, k, d_reg.ptr))
            gpu_ctx.sync()
        scan.finish()
        assert int(d_hits.download(np.uint64, 1)[0]) == want_hits > 0
        assert np.array_equal(d_reg.download(np.uint8, lib.SKETCH_REGISTERS), want_reg) and want_reg.any()
        assert np.array_equal(got_b.bits(0), want_b.bits(0))
        want_rows, got_rows = want_t.export(), got_t.export()
        o1, o2 = (np.lexsort((t[0][:, 0], t[0][:, 1])) for t in (want_rows, got_rows))
        assert len(want_rows[0]) > 1000
        for a, b in zip(want_rows, got_rows):
            assert np.array_equal(a[o1], b[o2])
    finally:
        scan.close()
        for x in (d_hits, d_reg):
            x.free()
        for x in (path, want_t, got_t, want_b, got_b):
            x.close()
