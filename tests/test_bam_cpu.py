"""CPU tests of the BAM route's device code run on the host (no GPU): the BGZF block scan, the inflate of bt_inflate.hpp with a team of one thread
(bt_diag_bgzf_inflate) against zlib, damaged blocks, and the record code of bt_bam.hpp (bt_diag_bam_reads_text) against the texts of bam_data.py."""
import struct
import zlib

import numpy as np
import pytest

import bam_data as bd
from bayestyper_amd import lib

GUARD = 64


def inflate_guarded(stream, blocks=None, out_bytes=None):
    """diag_bgzf_inflate into a buffer with guard bytes behind the capacity, which have to stay as they were"""
    if out_bytes is None:
        out_bytes = lib.bgzf_scan_blocks(stream)[2] if blocks is None else int(sum(int(b["isize"]) for b in blocks))
    out = np.full(out_bytes + GUARD, 0xA5, np.uint8)
    try:
        return lib.diag_bgzf_inflate(stream, blocks=blocks, out=out, capacity=out_bytes, out_bytes=out_bytes)
    finally:
        assert (out[out_bytes:] == 0xA5).all(), "bytes behind the capacity were written"


@pytest.fixture(scope="module")
def kinds():
    return bd.contents(np.random.default_rng(11), 65536)


# ---- the block scan -----------------------------------------------------------------------------------------------------------------------------------------
def test_scan_blocks_table_and_partial_tail(kinds):
    data = kinds["reads"][:5000]
    stream, offsets = bd.bgzf(data, [1000, 1000, 3000])   # an empty block mid-file
    blocks, used, total = lib.bgzf_scan_blocks(stream)
    assert used == len(stream) and total == len(data)
    assert [int(b["in_offset"]) for b in blocks] == offsets
    assert [int(b["isize"]) for b in blocks] == [1000, 0, 2000, 2000, 0]
    assert [int(b["out_offset"]) for b in blocks] == [0, 1000, 1000, 3000, 5000]
    assert int(blocks[0]["in_size"]) == offsets[1]
    for cut in (1, 11, 12, 17, 18, 30, offsets[1] - 1):   # a partial block at the end is not consumed and is no error
        b2, used2, _ = lib.bgzf_scan_blocks(stream[:offsets[3] + cut])
        assert len(b2) == 3 and used2 == offsets[3]
    assert lib.bgzf_scan_blocks(b"")[1:] == (0, 0)


def test_scan_blocks_accepts_other_subfields(kinds):
    data = kinds["periodic"][:300]
    stream = bd.bgzf_block(data, extra=b"XY\x03\x00abc") + bd.EOF_BLOCK
    blocks, used, total = lib.bgzf_scan_blocks(stream)
    assert used == len(stream) and total == 300
    assert inflate_guarded(stream) == data


@pytest.mark.parametrize("at,value,what", [(0, 0x1E, "magic"), (1, 0x8C, "magic"), (2, 7, "CM"), (3, 0, "FLG"), (3, 12, "FLG"), (12, ord("X"), "BC"), (14, 3, "BC"),
                                           (16, 20, "BSIZE")])
def test_scan_blocks_checks_every_header_field(kinds, at, value, what):
    stream = bytearray(bd.bgzf(kinds["reads"][:2000], [1000])[0])
    second = lib.bgzf_scan_blocks(bytes(stream))[0][1]
    off = int(second["in_offset"])
    stream[off + at] = value
    if what == "BSIZE":
        stream[off + 17] = 0
    with pytest.raises(lib.BtError, match=f"block at offset {off}:"):
        lib.bgzf_scan_blocks(bytes(stream))


# ---- inflate against zlib -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level,strategy", bd.STRATEGIES)
def test_inflate_equals_zlib(kinds, level, strategy):
    """every content kind at every size, each as a block of its own, in one stream per (level, strategy)"""
    datas = []
    for size in bd.SIZES:
        if level == 0 and size > bd.STORED_MAX:
            continue
        for name, content in kinds.items():
            if size == 65536 and name == "random" and level:
                continue   # does not compress: the block would not fit BSIZE
            datas.append(content[:size])
    stream = b"".join(bd.bgzf_block(d, level, strategy) for d in datas) + bd.EOF_BLOCK
    blocks, used, total = lib.bgzf_scan_blocks(stream)
    assert used == len(stream) and len(blocks) == len(datas) + 1
    for b, d in zip(blocks, datas):   # the fixture itself: zlib reads what it wrote
        at = int(b["in_offset"])
        assert zlib.decompress(stream[at + 18:at + int(b["in_size"]) - 8], -15) == d
    assert inflate_guarded(stream) == b"".join(datas)


def test_inflate_several_deflate_blocks_in_one_member(kinds):
    data = kinds["reads"][:30000] + kinds["periodic"][:20000] + kinds["random"][:3000]
    for level, strategy in bd.STRATEGIES:
        payload = bd.raw_deflate(data, level, strategy, flush_at=(1, 29999, 30000, 50001))
        assert zlib.decompress(payload, -15) == data
        assert inflate_guarded(bd.frame(payload, data)) == data


def test_inflate_single_distance_code_and_overlapping_copies():
    """a distance code set of ONE code, and matches that overlap their own output (distance 1 < length 3)"""
    payload, data = bd.single_distance_code(500)
    assert zlib.decompress(payload, -15) == data
    assert inflate_guarded(bd.frame(payload, data)) == data
    run = (b"ab" * 40000)[:65536]   # long distance-2 copies of length 258
    assert inflate_guarded(bd.bgzf_block(run, 9)) == run


def test_inflate_capacity_below_total_is_refused(kinds):
    stream = bd.bgzf(kinds["reads"][:4000], [2000])[0]
    out = np.full(4000 + GUARD, 0xA5, np.uint8)
    with pytest.raises(lib.BtError, match="capacity 3999 below the block table's total of 4000"):
        lib.diag_bgzf_inflate(stream, out=out, capacity=3999)
    assert (out == 0xA5).all()


# ---- damaged blocks -------------------------------------------------------------------------------------------------------------------------------------------
def damaged_cases(kinds):
    """name -> (stream of three blocks of which the second is damaged, its offset, the condition's words)"""
    good = kinds["reads"][:3000]
    first, last = bd.bgzf_block(good[:1500]), bd.bgzf_block(good[1500:])
    body = kinds["reads"][5000:9000]
    payload = bd.raw_deflate(body)
    cases = {}
    cases["crc"] = (bd.frame(payload, body, crc=zlib.crc32(body) ^ 1), "CRC-32 mismatch")
    cases["isize+1"] = (bd.frame(payload, body, isize=len(body) + 1), "output length differs from ISIZE")
    cases["isize-1"] = (bd.frame(payload, body, isize=len(body) - 1), "output length differs from ISIZE")
    cases["truncated"] = (bd.frame(payload[:-1], body), "deflate stream runs past the payload's end")
    cases["trailing"] = (bd.frame(payload + b"\0", body), "deflate stream ends before the payload's end")
    p, isize = bd.fixed_distance_before_start()
    cases["distance"] = (bd.frame(p, bytes(isize)), "distance reaches before the block's output")
    cases["oversubscribed"] = (bd.frame(bd.oversubscribed_dynamic(), bytes(10)), "over-subscribed or incomplete code set")
    for i, p in enumerate(bd.fixed_bad_symbols()):
        cases[f"symbol{i}"] = (bd.frame(p, bytes(10)), "invalid length or distance symbol")
    cases["type3"] = (bd.frame(b"\x07", b""), "reserved deflate block type")
    cases["stored-nlen"] = (bd.frame(b"\x01\x03\x00\xfc\xfeabc", b"abc"), "stored length check")
    return {name: (first + block + last, len(first), words) for name, (block, words) in cases.items()}, good


def test_damaged_blocks_are_errors_naming_the_block(kinds):
    cases, good = damaged_cases(kinds)
    assert len(cases) >= 11
    for name, (stream, offset, words) in cases.items():
        blocks, used, total = lib.bgzf_scan_blocks(stream)
        assert used == len(stream) and len(blocks) == 3, name
        out = np.full(total + GUARD, 0xA5, np.uint8)
        with pytest.raises(lib.BtError) as e:
            lib.diag_bgzf_inflate(stream, out=out, capacity=total, out_bytes=total, file_offset=1000)
        assert f"BGZF block at offset {1000 + offset}: " in str(e.value) and words in str(e.value), (name, str(e.value))
        assert (out[total:] == 0xA5).all(), name
        # the sound blocks around it were written all the same
        assert out[:1500].tobytes() == good[:1500] and out[total - 1500:total].tobytes() == good[1500:], name


def test_flipped_payload_bits_end_as_error_or_verified_output(kinds):
    """200 seeded single-bit flips in the payloads of a dynamic, a fixed and a stored block: an error, or (never seen, but legal) the right bytes"""
    rng = np.random.default_rng(5)
    body = kinds["reads"][:6000]
    errors = 0
    for i in range(200):
        level, strategy = [(6, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED), (0, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY)][i % 4]
        block = bytearray(bd.bgzf_block(body, level, strategy))
        bit = int(rng.integers(18 * 8, (len(block) - 8) * 8))
        if i < 8:
            bit = 18 * 8 + i   # the block header's bits, each once
        block[bit >> 3] ^= 1 << (bit & 7)
        try:
            out = inflate_guarded(bytes(block))
        except lib.BtError as e:
            assert "BGZF block at offset 0: " in str(e)
            errors += 1
        else:
            assert out == body and zlib.crc32(out) == struct.unpack("<I", bytes(block[-8:-4]))[0]
    assert errors >= 190


def test_bsize_larger_than_the_buffer(kinds):
    good = bd.bgzf_block(kinds["reads"][:1000])
    good_table = lib.bgzf_scan_blocks(good)[0]
    stream = bytearray(good)
    struct.pack_into("<H", stream, 16, len(stream) + 50 - 1)
    blocks, used, total = lib.bgzf_scan_blocks(bytes(stream))   # to the scan this is a partial block
    assert len(blocks) == 0 and used == 0
    with pytest.raises(lib.BtError, match="BGZF block at offset 0: incomplete"):
        lib.diag_bgzf_inflate(bytes(stream))
    forged = good_table.copy()
    forged["in_size"] = len(stream) + 50
    with pytest.raises(lib.BtError, match="BGZF block at offset 0: block table entry out of range"):
        inflate_guarded(bytes(stream), blocks=forged)
    with pytest.raises(lib.BtError, match="BGZF block at offset 0: bad gzip header"):   # the table says what the buffer holds, BSIZE does not
        inflate_guarded(bytes(stream), blocks=good_table)
    forged = good_table.copy()
    forged["out_offset"] = 1   # would end one byte behind the output
    with pytest.raises(lib.BtError, match="BGZF block at offset 0: block table entry out of range"):
        inflate_guarded(good, blocks=forged, out_bytes=1000)
    assert inflate_guarded(good, blocks=good_table) == kinds["reads"][:1000]


# ---- records -> text --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [31, 55])
def test_reads_text_equals_the_expected_text(k):
    recs = bd.edge_records(np.random.default_rng(k), k)
    bam = b"".join(r for r, _, _ in recs)
    for skip in (0x900, 0, 0x400, 0x10, 0xFFFF):
        text, used, stats = lib.diag_bam_reads_text(bam, skip)
        assert text == bd.records_text(recs, skip), hex(skip)
        kept = [s for _, s, f in recs if not f & skip]
        assert used == len(bam) and stats == {"kept": len(kept), "skipped": len(recs) - len(kept), "bases": sum(map(len, kept))}
    assert bd.records_text(recs, 0x900) != bd.records_text(recs, 0)


def test_more_than_65536_records_equal_the_expected_text():
    """the inputs of the GPU test of the same name: the host run gives the expected text and stats on them, so it is that test's reference"""
    recs = bd.short_records()
    for n in bd.MANY_RECORDS:
        bam = b"".join(r for r, _, _ in recs[:n])
        for skip in (0x900, 0):
            kept = [s for _, s, f in recs[:n] if not f & skip]
            assert skip == 0 or n // 3 < len(kept) < 2 * n // 3
            assert lib.diag_bam_reads_text(bam, skip) == (bd.records_text(recs[:n], skip), len(bam), {"kept": len(kept), "skipped": n - len(kept), "bases": sum(map(len, kept))})


def test_reads_text_every_code_and_empty_line():
    seq = bd.SEQ_CODES.encode()
    text, used, stats = lib.diag_bam_reads_text(bd.record(seq) + bd.record(b"") + bd.record(seq[:15]), 0)
    assert text == b"NACNGNNNTNNNNNNN\n" + b"\n" + b"NACNGNNNTNNNNNN\n"
    assert stats == {"kept": 3, "skipped": 0, "bases": 31}


def test_consumed_at_every_cut_of_a_record():
    rng = np.random.default_rng(2)
    recs = bd.edge_records(rng, 31)[5:12]
    first, cut_rec, _ = b"".join(r for r, _, _ in recs[:3]), recs[3][0], None
    for cut in range(len(cut_rec)):   # inside block_size, inside the fixed fields, the name, the sequence ...
        text, used, stats = lib.diag_bam_reads_text(first + cut_rec[:cut], 0)
        assert used == len(first) and text == bd.records_text(recs[:3], 0), cut
    text, used, _ = lib.diag_bam_reads_text(first + cut_rec, 0)
    assert used == len(first) + len(cut_rec) and text == bd.records_text(recs[:4], 0)
    assert lib.diag_bam_reads_text(b"", 0)[:2] == (b"", 0)


def test_capacity_rule_of_the_text():
    recs = bd.edge_records(np.random.default_rng(3), 31)
    bam = b"".join(r for r, _, _ in recs)
    want = bd.records_text(recs, 0)
    assert lib.diag_bam_reads_text(bam, 0, capacity=len(want))[0] == want   # (the binding checks the guard bytes behind the capacity)
    with pytest.raises(lib.BtError, match="capacity"):
        lib.diag_bam_reads_text(bam, 0, capacity=len(want) - 1)


def test_invalid_block_size_is_an_error_naming_the_record():
    for bam, offset, words in bd.invalid_records():
        with pytest.raises(lib.BtError) as e:
            lib.diag_bam_reads_text(bam, 0)
        assert str(e.value) == f"BAM record at offset {offset}: {words}"


# ---- the BAM file reader (bayestyper_amd/host/BamFile.cpp), no GPU -------------------------------------------------------------------------------------------------
def _host():
    import ctypes as C

    from bayestyper_amd import host

    dll = host.dll
    dll.bth_bam_is_bam.restype = C.c_int
    dll.bth_bam_is_bam.argtypes = [C.c_char_p, C.c_char_p, C.c_uint]
    dll.bth_bam_file_slabs.restype = C.c_longlong
    dll.bth_bam_file_slabs.argtypes = [C.c_char_p, C.c_ulonglong, C.c_char_p, C.c_ulonglong, C.c_void_p, C.c_char_p, C.c_uint]
    dll.bth_bam_skip_flags.restype = C.c_longlong
    dll.bth_bam_skip_flags.argtypes = [C.c_char_p, C.c_uint]
    return dll


def is_bam(path):
    import ctypes as C

    err = C.create_string_buffer(1024)
    rc = _host().bth_bam_is_bam(str(path).encode(), err, 1024)
    if rc < 0:
        raise RuntimeError(err.value.decode())
    return bool(rc)


def bam_slabs(path, slab_bytes=65536):
    """bth_bam_file_slabs -> (the slabs' bytes laid end to end, dict of the reader's numbers); RuntimeError with the reader's message"""
    import ctypes as C

    dll, err, stats = _host(), C.create_string_buffer(1024), np.zeros(7, np.uint64)
    need = dll.bth_bam_file_slabs(str(path).encode(), slab_bytes, None, 0, stats.ctypes.data_as(C.c_void_p), err, 1024)
    if need < 0:
        raise RuntimeError(err.value.decode())
    buf = C.create_string_buffer(max(need, 1))
    assert dll.bth_bam_file_slabs(str(path).encode(), slab_bytes, buf, need, stats.ctypes.data_as(C.c_void_p), err, 1024) == need
    names = ("header_bytes", "references", "skip_first", "first_slab_at", "has_eof", "slabs", "file_bytes")
    return buf.raw[:need], dict(zip(names, (int(x) for x in stats)))


def _text_of_slabs(slabs, skip_first):
    """what the stream object makes of the slabs, by the host runs of its two steps"""
    raw = lib.diag_bgzf_inflate(slabs)
    text, used, _ = lib.diag_bam_reads_text(raw[skip_first:], 0x900)
    assert used == len(raw) - skip_first
    return text


def test_bam_file_header_spanning_three_blocks(tmp_path):
    recs = bd.edge_records(np.random.default_rng(4), 31)
    head = bd.header(text=b"@HD\tVN:1.6\n@CO\t" + b"x" * 3000 + b"\n", refs=[("chr%d" % i, 1000 + i) for i in range(40)])
    data = head + b"".join(r for r, _, _ in recs)
    stream, offsets = bd.bgzf(data, bd.even_cuts(len(data), 1500))
    assert 2 * 1500 < len(head) < 3 * 1500   # the header's text ends in the third block, the reference list lies in it
    path = tmp_path / "three.bam"
    path.write_bytes(stream)
    assert is_bam(path)
    for slab_bytes in (65536, 1 << 20):
        slabs, info = bam_slabs(path, slab_bytes)
        assert info["header_bytes"] == len(head) and info["references"] == 40 and info["has_eof"] == 1 and info["file_bytes"] == len(stream)
        assert info["first_slab_at"] == offsets[2] and info["skip_first"] == len(head) - 2 * 1500   # the blocks that hold header alone are not handed on
        assert slabs == stream[offsets[2]:] and info["slabs"] >= 1
        assert _text_of_slabs(slabs, info["skip_first"]) == bd.records_text(recs, 0x900)


def test_bam_file_zero_references_empty_and_missing_eof(tmp_path):
    recs = bd.edge_records(np.random.default_rng(4), 31)[:8]
    body = b"".join(r for r, _, _ in recs)
    head = bd.header(refs=())
    (tmp_path / "zero.bam").write_bytes(bd.bgzf(head + body, [len(head)])[0])   # the header ends with its block: the slabs start at the next one
    slabs, info = bam_slabs(tmp_path / "zero.bam")
    assert info["references"] == 0 and info["header_bytes"] == len(head) and info["skip_first"] == 0 and info["first_slab_at"] > 0
    assert _text_of_slabs(slabs, 0) == bd.records_text(recs, 0x900)
    (tmp_path / "empty.bam").write_bytes(bd.bgzf(bd.header(), [])[0])   # header only
    slabs, info = bam_slabs(tmp_path / "empty.bam")
    assert info["has_eof"] == 1 and info["references"] == 1 and _text_of_slabs(slabs, info["skip_first"]) == b""
    (tmp_path / "noeof.bam").write_bytes(bd.bgzf(bd.header() + body, [500], eof=False)[0])
    slabs, info = bam_slabs(tmp_path / "noeof.bam")
    assert info["has_eof"] == 0   # the executables print a warning and go on
    assert _text_of_slabs(slabs, info["skip_first"]) == bd.records_text(recs, 0x900)


def test_bam_file_refusals_and_lookalikes(tmp_path):
    (tmp_path / "x.cram").write_bytes(b"CRAM\x03\x00" + bytes(100))
    with pytest.raises(RuntimeError, match="CRAM is not supported"):
        is_bam(tmp_path / "x.cram")
    fastq = b"".join(b"@r%d\nACGTACGTAC\n+\nIIIIIIIIII\n" % i for i in range(50))
    (tmp_path / "reads.fq.gz").write_bytes(bd.bgzf(fastq, [300, 700])[0])   # a FASTQ compressed as BGZF is not a BAM: it goes the old way
    assert not is_bam(tmp_path / "reads.fq.gz")
    from test_reads_cpu import read_slabs

    slabs, bases, reads = read_slabs(tmp_path / "reads.fq.gz", 31, 1 << 20)
    assert (bases, reads) == (500, 50)
    (tmp_path / "plain.fa").write_bytes(b">a\nACGT\n")
    assert not is_bam(tmp_path / "plain.fa")
    (tmp_path / "empty").write_bytes(b"")
    assert not is_bam(tmp_path / "empty")
    with pytest.raises(RuntimeError, match="Unable to open"):
        is_bam(tmp_path / "missing.bam")
    noise = np.random.default_rng(6).integers(33, 127, size=5000, dtype=np.uint8).tobytes()   # a header text that does not compress away
    stream, offsets = bd.bgzf(bd.header(text=b"@CO\t" + noise + b"\n") + bd.record(b"ACGT"), [2000, 4000])
    (tmp_path / "cut.bam").write_bytes(stream[:1000])
    with pytest.raises(RuntimeError, match="BGZF block at offset 0: the file ends inside a BGZF block"):
        bam_slabs(tmp_path / "cut.bam")
    (tmp_path / "cut1.bam").write_bytes(stream[:offsets[1]])   # cut at a block boundary inside the header
    with pytest.raises(RuntimeError, match="the file ends inside the BAM header: truncated"):
        bam_slabs(tmp_path / "cut1.bam")
    full = bd.bgzf(bd.header() + b"".join(bd.record(b"ACGT" * 30) for _ in range(100)), [3000, 6000])[0]
    (tmp_path / "cut2.bam").write_bytes(full[:len(full) - 40])   # the file ends inside a block behind the header
    with pytest.raises(RuntimeError, match="BGZF block at offset \\d+: the file ends inside the block: truncated"):
        bam_slabs(tmp_path / "cut2.bam")


def test_bam_skip_flags_variable(monkeypatch):
    import ctypes as C

    dll, err = _host(), C.create_string_buffer(1024)
    monkeypatch.delenv("BT_BAM_SKIP_FLAGS", raising=False)
    assert dll.bth_bam_skip_flags(err, 1024) == 0x900
    for text, value in (("0", 0), ("0x100", 0x100), ("2304", 0x900), ("65535", 65535)):
        monkeypatch.setenv("BT_BAM_SKIP_FLAGS", text)
        assert dll.bth_bam_skip_flags(err, 1024) == value
    for text in ("65536", "abc", "-1", "", "0x900 "):
        monkeypatch.setenv("BT_BAM_SKIP_FLAGS", text)
        assert dll.bth_bam_skip_flags(err, 1024) == -1 and b"BT_BAM_SKIP_FLAGS must be a number below 65536" in err.value
