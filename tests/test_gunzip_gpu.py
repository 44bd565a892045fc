"""The device's gunzip (bayestyper_amd/csrc/bt_gunzip.hip) against Python's zlib and against its own host run, byte for byte and stat for stat, over the
inputs of tests/gunzip_data.py, and the stream object over ordinary gzip FASTQ files cut anywhere against the independent parser of tests/fastq_data.py."""
import gzip
import struct
import zlib

import numpy as np
import pytest

import fastq_data as fd
import gunzip_data as gd
from test_gunzip_cpu import check_invariant, corpus, flip_outcome, flips, resume, start_cases, walked   # noqa: F401  (fixtures and helpers, shared)

pytestmark = pytest.mark.gpu


def both(gpu_ctx):
    """a runner that calls the device and the host run and asserts that they agree in everything, the stats included"""
    from bayestyper_amd import lib

    def run(stream, **kw):
        dev, host = lib.inflate_raw(gpu_ctx, stream, **kw), lib.diag_inflate_raw(stream, **kw)
        assert dev == host, (kw, dev["stats"], host["stats"])
        return dev

    return run


@pytest.mark.parametrize("name", ["fastq_l1", "fastq_l6", "fastq_l9"])
def test_fastq_is_split_at_its_block_starts(gpu_ctx, corpus, name):
    stream, want = corpus[name]
    got = check_invariant(both(gpu_ctx), stream, want)
    st = got[16 * gd.KIB]["stats"]
    assert st["links_verified"] >= len(stream) / (4 * 16 * gd.KIB) and st["links_broken"] == 0, st


def test_many_small_blocks(gpu_ctx, corpus):
    stream, want = corpus["sync_flushed"]
    flushes = len(gd.sync_flushed(gd.fastq(1)[:300_000], 2)[1])
    run = both(gpu_ctx)
    for chunk in (1 * gd.KIB, 2 * gd.KIB, 4 * gd.KIB):
        r = run(stream, chunk_bytes=chunk)
        assert r["data"] == want and r["stream_end"] == 1
        assert r["stats"]["links_verified"] >= min(flushes, len(stream) // chunk) / 4 and r["stats"]["links_broken"] == 0, (chunk, r["stats"])
    check_invariant(run, stream, want)


def test_streams_the_finder_cannot_split(gpu_ctx):
    text = gd.fastq(5, reads=300)
    streams = gd.unsplittable()
    streams["huffman_only"] = gd.raw(text[:15000], 6, zlib.Z_HUFFMAN_ONLY)   # (one block each: these strategies write dynamic blocks)
    streams["rle"] = gd.raw(text[:15000], 6, zlib.Z_RLE)
    for name, stream in streams.items():
        for chunk, r in check_invariant(both(gpu_ctx), stream, gd.inflate(stream)[0]).items():
            assert r["stats"]["candidates"] == 0 and r["stats"]["links_verified"] == 0 and r["stats"]["rounds"] == 1, (name, chunk, r["stats"])


@pytest.mark.parametrize("name", ["huffman_only", "rle", "false_candidates", "repeated_read", "window_edges"])
def test_rounds_cost_no_bytes(gpu_ctx, corpus, name):
    """false candidates on purpose, a team out of room, the windows' edges (the expectations of test_gunzip_cpu.py, on the device)"""
    stream, want = corpus[name]
    got = check_invariant(both(gpu_ctx), stream, want)
    if name == "false_candidates":
        st = got[4 * gd.KIB]["stats"]
        assert st["links_broken"] >= 1 and st["rounds"] >= 3, st
    if name == "repeated_read":
        assert all(r["stats"]["rounds"] > 1 for r in got.values())
    if name == "window_edges":
        assert got[1 * gd.KIB]["stats"]["links_verified"] == 3


def test_every_start_bit(gpu_ctx, walked):
    stream, text, _, _ = walked
    run = both(gpu_ctx)
    for start, produced in start_cases(walked):
        for chunk in (1 * gd.KIB, 16 * gd.KIB):
            r = run(stream, start_bit=start, window=text[max(0, produced - 32768):produced], chunk_bytes=chunk)
            assert r["data"] == text[produced:] and r["stream_end"] == 1 and r["crc32"] == zlib.crc32(text[produced:]), (start, chunk)


@pytest.mark.parametrize("name", ["fastq_l6", "sync_flushed", "window_edges"])
def test_resumption(gpu_ctx, corpus, name):
    """a third of the output as capacity (the binding presets and checks the bytes at and past it), again from end_bit with the last 32 KiB as the window"""
    stream, want = corpus[name]
    assert resume(both(gpu_ctx), stream, want, 4 * gd.KIB) > 3


def test_zero_progress_is_a_result(gpu_ctx, corpus):
    stream, want = corpus["fastq_l6"]
    run = both(gpu_ctx)
    assert run(stream, capacity=100)["data"] == b"" and run(stream[:5000])["end_bit"] == 0 and run(b"")["data"] == b""
    r = run(stream[:100_000], chunk_bytes=4 * gd.KIB)
    assert 0 < len(r["data"]) < len(want) and want.startswith(r["data"]) and r["stream_end"] == 0


def test_damaged_streams_give_the_hosts_message(gpu_ctx, flips):
    """a dozen of the flips the host run has judged: the same message, or the same bytes"""
    from bayestyper_amd import lib

    _, cases = flips
    judged = [(bit, s, flip_outcome(lib.diag_inflate_raw, s)) for bit, s in cases]
    errors = [c for c in judged if c[2][0] == "error"][:8]
    assert len(errors) >= 5
    for bit, stream, host in errors + [c for c in judged if c[2][0] == "ok"][:4]:
        dev = flip_outcome(lambda s, **kw: lib.inflate_raw(gpu_ctx, s, **kw), stream)
        if host[0] == "error":
            assert dev == ("error", host[1].replace("bt_diag_inflate_raw", "bt_inflate_raw")), bit
        else:
            assert dev == host, bit


# ---- the stream object ---------------------------------------------------------------------------------------------------------------------------------------
def scan_file(gpu_ctx, data, slab, max_in=128 * gd.KIB, chunk=4 * gd.KIB):
    """the file in slabs of `slab` bytes -> (text, summed stats, gunzip stats)"""
    from bayestyper_amd import lib

    scan = lib.FastqGzScan(gpu_ctx, max_in, chunk)
    try:
        text, total = b"", {"reads": 0, "bases": 0, "lines": 0}
        pieces = [scan.text_bytes(data[at:at + slab]) for at in range(0, len(data), slab)] + [scan.finish_bytes()]
        for t, st in pieces:
            text += t
            for k in total:
                total[k] += st[k]
        return text, total, scan.stats()
    finally:
        scan.close()


@pytest.fixture(scope="module")
def fastq_file():
    """a FASTQ of the project's shape, and the independent parser's answer — computed once, never changed"""
    data = gd.fastq(1)
    text, consumed, stats = fd.parse(data)
    assert consumed == len(data)
    return data, text, stats


@pytest.mark.parametrize("slab", [64 * gd.KIB, 100_003])
def test_scan_of_slabs(gpu_ctx, fastq_file, slab):
    data, text, stats = fastq_file
    got = scan_file(gpu_ctx, gzip.compress(data, 6), slab)
    assert got[0] == text and got[1] == stats
    assert got[2]["out_bytes"] == len(data) and got[2]["links_verified"] >= 10 and got[2]["links_broken"] == 0, got[2]


def test_scan_byte_by_byte_and_headers(gpu_ctx):
    rng = np.random.default_rng(5)
    data = b"".join(fd.record(rng, i, fd.random_seq(rng, 30 + i), (b"\n", b"\r\n")[i % 2]) for i in range(40)) + b"@last\nACGT\n+\nIIII"   # the last line has no newline
    want = fd.parse(data)
    small = b"".join(fd.simple_records(rng, 6, 30))
    member = gd.gzip_member(small, name=b"reads.fastq", extra=b"AB\x02\x00xy", hcrc=True, comment=b"made by hand")
    got = scan_file(gpu_ctx, member, 1, max_in=64 * gd.KIB)
    assert (got[0], got[1]) == (fd.parse(small)[0], fd.parse(small)[2])
    got = scan_file(gpu_ctx, gd.gzip_member(data, name=b"x"), 777)
    assert (got[0], got[1]) == (want[0], want[2])


def test_scan_of_several_members(gpu_ctx):
    rng = np.random.default_rng(6)
    parts = [b"".join(fd.simple_records(rng, 400, 100)), b"", b"".join(fd.simple_records(rng, 300, 150))]
    whole = b"".join(parts)
    want = fd.parse(whole)
    for members in (parts[:2], parts, [parts[1], parts[0]], [parts[0][:50_000], parts[0][50_000:]]):   # a member may end inside a record
        data = b"".join(members)
        got = scan_file(gpu_ctx, b"".join(gzip.compress(m) for m in members), 10_007)
        assert (got[0], got[1]) == (fd.parse(data)[0], fd.parse(data)[2]), [len(m) for m in members]
    assert want[2]["reads"] == 700


def scan_error(gpu_ctx, data, slab=100_003):
    from bayestyper_amd import lib

    with pytest.raises(lib.BtError) as e:
        scan_file(gpu_ctx, data, slab)
    return str(e.value)


def test_scan_errors_name_the_offset(gpu_ctx):
    records = gd.fastq_records(1, 600)
    data = b"".join(records)
    head = gzip.compress(b"@r\nAC\n+\nII\n")
    sound = gd.gzip_member(data)
    at, trailer = len(head), len(head) + len(sound) - 8
    assert scan_error(gpu_ctx, head + gd.gzip_member(data, crc=zlib.crc32(data) ^ 1)) == \
        "bt_fastq_gz_scan_text: gzip member at offset %d: CRC-32 mismatch (trailer at offset %d)" % (at, trailer)
    assert scan_error(gpu_ctx, head + gd.gzip_member(data, isize=len(data) + 1)) == \
        "bt_fastq_gz_scan_text: gzip member at offset %d: output length differs from ISIZE (trailer at offset %d)" % (at, trailer)
    cut = head + sound[:len(sound) // 2]
    assert scan_error(gpu_ctx, cut) == "bt_fastq_gz_scan_finish: truncated gzip file: it ends at offset %d inside the member at offset %d" % (len(cut), at)
    cut = head + sound[:-3]
    assert scan_error(gpu_ctx, cut) == "bt_fastq_gz_scan_finish: truncated gzip file: it ends at offset %d inside the member at offset %d" % (len(cut), at)
    assert scan_error(gpu_ctx, head + b"\x1f\x8b\x07") == "bt_fastq_gz_scan_text: gzip member at offset %d: gzip compression method is not deflate" % at
    damaged = bytearray(head + sound)
    damaged[at + 10] |= 6   # the first block's type: reserved
    message = scan_error(gpu_ctx, bytes(damaged))
    assert message == "bt_fastq_gz_scan_text: gzip member at offset %d: deflate block at offset %d (bit 0): reserved deflate block type or stored length check" % (at, at + 10)
    # a grammar violation carries ReadsFile's words and the file's line number
    bad = b"".join(records[:300])
    lines = bad.count(b"\n")
    assert scan_error(gpu_ctx, gzip.compress(bad + b"r1\nACGT\n+\nIIII\n" + data[:3000])) == fd.MESSAGES["at"] % (lines + 1)
    # a block that is not whole within max_in_bytes of carried input is refused
    from bayestyper_amd import lib

    scan = lib.FastqGzScan(gpu_ctx, 64 * gd.KIB, 4 * gd.KIB)
    try:
        noise = np.random.default_rng(1).integers(0, 256, size=200_000).astype(np.uint8).tobytes()
        stream = gzip.compress(b"")[:10] + gd.fixed_block([noise], final=True)   # one block of literals, more than 200 KB long
        with pytest.raises(lib.BtError, match="is not whole within max_in_bytes = 65536 of carried input"):
            for off in range(0, len(stream), 60_000):
                scan.text(stream[off:off + 60_000])
    finally:
        scan.close()
