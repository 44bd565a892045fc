"""The FASTQ grammar of the device's reader run on the host (bt_diag_fastq_reads_text: the same line code as the kernels, no GPU), against the independent
parser of tests/fastq_data.py and against the host's ReadsFile; the host classes that recognise and deliver a BGZF-compressed FASTQ file."""
import ctypes as C
import gzip

import numpy as np
import pytest

import bam_data as bd
import fastq_data as fd
from bayestyper_amd import lib
from test_reads_cpu import read_slabs

K = 55


def diag(data, final=True, first_line=1, **kw):
    return lib.diag_fastq_reads_text(data, final=final, first_line=first_line, **kw)


def reads_file(tmp_path, data, name="x.fq", slab_bytes=1 << 20):
    """ReadsFile over the bytes written to a file -> (its slabs laid end to end, bases, reads)"""
    path = tmp_path / name
    path.write_bytes(data)
    slabs, bases, reads = read_slabs(path, K, slab_bytes)
    return b"".join(slabs), bases, reads


@pytest.mark.parametrize("eol", [None, b"\n", b"\r\n"], ids=["mixed", "lf", "crlf"])
@pytest.mark.parametrize("last_newline", [True, False], ids=["newline", "open"])
def test_edge_file_equals_the_parser_and_reads_file(tmp_path, eol, last_newline):
    data = fd.edge_file(np.random.default_rng(11), K, eol, last_newline)
    want, consumed, stats = fd.parse(data)
    assert consumed == len(data) and stats["reads"] > 40 and b"\n\n" not in want
    assert max(map(len, want.split(b"\n"))) == 20000 and {0, 1, K - 1, K, K + 1, 150} <= {len(x) for x in want.split(b"\n")}
    text, used, st = diag(data)
    assert text == want and used == len(data) and st == stats
    # ReadsFile tells FASTQ by the file's first byte: it gets the file without the blank lines at its start, which add nothing to the text
    assert data.startswith(fd.LEADING) and diag(data[len(fd.LEADING):])[0] == text
    slabs, bases, reads = reads_file(tmp_path, data[len(fd.LEADING):])   # (slab_bytes above the longest read: no read is cut)
    assert text == slabs and (st["reads"], st["bases"]) == (reads, bases)


@pytest.mark.parametrize("n", fd.MANY_RECORDS)
def test_more_than_65536_lines_equal_the_parser(n):
    """the inputs of the GPU test of the same name: host run and parser agree on them, so either is that test's reference"""
    data = fd.short_records(n)
    want = fd.parse(data)
    assert want[1] == len(data) and want[2]["lines"] == 4 * n and n // 2 < want[2]["reads"] < n
    assert diag(data) == want
    assert diag(data[:-1]) == fd.parse(data[:-1])   # the last line open


def three_records():
    rng = np.random.default_rng(3)
    data = b"\n" + fd.record(rng, 0, b"ACGTNacgtn", b"\r\n") + b"\r\n\n" + fd.record(rng, 1, b"", b"\n") + fd.record(rng, 2, fd.random_seq(rng, 61), b"\n", kind=0) + b"\n"
    assert 150 < len(data) < 260
    return data


def test_every_prefix_of_three_records():
    data = three_records()
    whole, _, whole_stats = fd.parse(data)
    starts = fd.record_starts(data)
    for cut in range(len(data) + 1):
        want, consumed, stats = fd.parse(data[:cut], final=False)
        text, used, st = diag(data[:cut], final=False)
        assert (text, used, st) == (want, consumed, stats), cut
        # the start of the first record that is not whole, or — inside the blank lines in front of it — behind the last whole blank line
        assert starts[0] <= cut or used <= cut
        assert (used in starts and used <= cut) or data[used:cut] in (b"", b"\r"), cut
        assert data[used:cut].count(b"\n") < 4, cut
        # the rest, as the file's end
        rest, used2, st2 = diag(data[used:], final=True, first_line=1 + st["lines"])
        assert text + rest == whole and used + used2 == len(data), cut
        assert {key: st[key] + st2[key] for key in st} == whole_stats, cut


SOUND = b"@s\nACGT\n+\nIIII\n"
VIOLATIONS = {
    "at": (b"r1\nACGT\n+\nIIII\n", 1, ()),
    "plus": (b"@r1\nACGT\nIIII\n@r2\n", 3, ()),
    "plus blank": (b"@r1\nACGT\n\nIIII\n", 3, ()),
    "lengths": (b"@r1\nACGTA\n+\nIIII\n", 4, (5, 4)),
    "lengths crlf": (b"@r1\r\nACG\r\n+\r\nIIII\r\n", 4, (3, 4)),
    "lengths blank bases": (b"@r1\n\n+\nI\n", 4, (0, 1)),
}


@pytest.mark.parametrize("name", ["at", "plus", "plus blank", "lengths", "lengths crlf", "lengths blank bases"])
def test_each_violation_has_reads_files_words(tmp_path, name):
    bad, line, numbers = VIOLATIONS[name]
    data = SOUND + bad + SOUND
    kind = name.split()[0]
    want = fd.MESSAGES[kind] % ((4 + line,) + numbers)
    with pytest.raises(fd.FastqError) as ours:
        fd.parse(data)
    assert str(ours.value) == want
    with pytest.raises(lib.BtError) as e:
        diag(data)
    assert str(e.value) == want
    with pytest.raises(RuntimeError) as host:
        reads_file(tmp_path, data)
    assert str(host.value).split(": ", 1)[0].startswith("read file ") and str(host.value).split("x.fq: ", 1)[1] == want
    with pytest.raises(lib.BtError) as e:   # first_line shows up in the number
        diag(data, first_line=1001)
    assert str(e.value) == fd.MESSAGES[kind] % ((1004 + line,) + numbers)
    with pytest.raises(lib.BtError) as e:   # judged by its complete lines while it is not whole
        diag(data, final=False)
    assert str(e.value) == want


@pytest.mark.parametrize("lines", [1, 2, 3])
def test_truncated_record_at_the_end(tmp_path, lines):
    for tail in (b"\n", b""):   # the last line with and without its newline
        data = SOUND + b"\n".join([b"@r", b"ACGT", b"+", b"IIII"][:lines]) + tail
        want = fd.MESSAGES["truncated"] % lines
        with pytest.raises(lib.BtError) as e:
            diag(data)
        assert str(e.value) == want
        with pytest.raises(RuntimeError) as host:
            reads_file(tmp_path, data)
        assert str(host.value).split("x.fq: ", 1)[1] == want
        text, used, st = diag(data, final=False)   # not the file's end: the record is not whole, and no error
        assert (text, used, st["lines"]) == (b"ACGT\n", len(SOUND), 4)


def test_the_smallest_line_wins_and_blank_lines_count():
    data = SOUND + b"@r1\nACGT\nIIII\nx\n" + SOUND + b"r2\nAC\n+\nI\n"   # '+' missing at line 7, then more
    with pytest.raises(lib.BtError) as e:
        diag(data)
    assert str(e.value) == fd.MESSAGES["plus"] % 7
    data = SOUND + b"@r\nAC\n+\nIII\n" + b"@r1\nACGT\nIIII\nx\n"   # lengths at line 8, '+' at line 11
    with pytest.raises(lib.BtError) as e:
        diag(data)
    assert str(e.value) == fd.MESSAGES["lengths"] % (8, 2, 3)
    data = b"\n\r\n" + SOUND + b"\n" + b"r1\nACGT\n+\nIIII\n"   # the file's line number: the three skipped blank lines count
    with pytest.raises(lib.BtError) as e:
        diag(data)
    assert str(e.value) == fd.MESSAGES["at"] % 8 == str(pytest.raises(fd.FastqError, fd.parse, data).value)
    with pytest.raises(lib.BtError) as e:   # an open last line that is a lone '\r' where a record starts is no blank line between records
        diag(SOUND + b"\r")
    assert str(e.value) == fd.MESSAGES["at"] % 5 == str(pytest.raises(fd.FastqError, fd.parse, SOUND + b"\r").value)


def test_capacity_rule_and_null_arguments():
    data = fd.edge_file(np.random.default_rng(5), K)
    want = fd.parse(data)[0]
    assert len(want) < len(data)
    assert diag(data, capacity=len(want))[0] == want   # (the binding checks the bytes behind the capacity and behind the text)
    with pytest.raises(lib.BtError, match="capacity"):
        diag(data, capacity=len(want) - 1)
    assert diag(b"", capacity=0) == (b"", 0, {"reads": 0, "bases": 0, "lines": 0})
    for null in ("text", "text_bytes", "consumed"):
        with pytest.raises(lib.BtError, match="bt_diag_fastq_reads_text: null argument"):
            diag(data, null=null)
    out, n, used = np.zeros(8, np.uint8), C.c_uint64(), C.c_uint64()
    assert lib.bt_diag_fastq_reads_text(None, 5, 1, 1, out.ctypes.data_as(C.c_void_p), 8, C.byref(n), C.byref(used), None) != 0
    assert "null argument" in lib.bt_last_error().decode()


# ---- the host classes (bayestyper_amd/host/BgzfFile.cpp), no GPU ---------------------------------------------------------------------------------------------
def _host():
    from bayestyper_amd import host

    dll = host.dll
    dll.bth_fastq_is_bgzf.restype = C.c_int
    dll.bth_fastq_is_bgzf.argtypes = [C.c_char_p, C.c_char_p, C.c_uint]
    dll.bth_bgzf_fastq_file_slabs.restype = C.c_longlong
    dll.bth_bgzf_fastq_file_slabs.argtypes = [C.c_char_p, C.c_ulonglong, C.c_char_p, C.c_ulonglong, C.c_void_p, C.c_char_p, C.c_uint]
    return dll


def is_bgzf_fastq(path):
    err = C.create_string_buffer(1024)
    rc = _host().bth_fastq_is_bgzf(str(path).encode(), err, 1024)
    if rc < 0:
        raise RuntimeError(err.value.decode())
    return bool(rc)


def fastq_slabs(path, slab_bytes=65536):
    """bth_bgzf_fastq_file_slabs -> (the slabs' bytes laid end to end, dict of the reader's numbers); RuntimeError with the reader's message"""
    dll, err, stats = _host(), C.create_string_buffer(1024), np.zeros(4, np.uint64)
    need = dll.bth_bgzf_fastq_file_slabs(str(path).encode(), slab_bytes, None, 0, stats.ctypes.data_as(C.c_void_p), err, 1024)
    if need < 0:
        raise RuntimeError(err.value.decode())
    buf = C.create_string_buffer(max(need, 1))
    assert dll.bth_bgzf_fastq_file_slabs(str(path).encode(), slab_bytes, buf, need, stats.ctypes.data_as(C.c_void_p), err, 1024) == need
    return buf.raw[:need], dict(zip(("first_slab_at", "has_eof", "slabs", "file_bytes"), (int(x) for x in stats)))


def test_is_bgzf_fastq_and_its_lookalikes(tmp_path):
    from test_bam_cpu import is_bam

    fastq = b"".join(fd.simple_records(np.random.default_rng(2), 50))
    verdicts = {
        "bgzf.fq.gz": (bd.bgzf(fastq, [300, 700])[0], True),
        "empty_first.fq.gz": (bd.bgzf(fastq, [0, 0, 300])[0], True),   # the first blocks are empty
        "x.bam": (bd.bgzf(bd.header() + bd.record(b"ACGT"), [])[0], False),
        "bgzf.fa.gz": (bd.bgzf(b">a\nACGT\n", [])[0], False),
        "plain.fq.gz": (gzip.compress(fastq), False),
        "plain.fq": (fastq, False),
        "empty": (b"", False),
        "only_eof.gz": (bd.EOF_BLOCK, False),
        "subfield.fq.gz": (bd.bgzf(fastq, [])[0].replace(b"BC", b"BX", 1), False),
    }
    for name, (content, want) in verdicts.items():
        (tmp_path / name).write_bytes(content)
        assert is_bgzf_fastq(tmp_path / name) == want, name
        assert is_bam(tmp_path / name) == (name == "x.bam"), name   # isBam's verdicts are what they were
    with pytest.raises(RuntimeError, match="Unable to open"):
        is_bgzf_fastq(tmp_path / "missing.fq.gz")


def test_bgzf_fastq_file_slabs_are_the_file(tmp_path):
    rng = np.random.default_rng(8)
    fastq = b"".join(fd.simple_records(rng, 6000, 100))   # about 1.3 MB of text in blocks of 9 KiB of content
    stream = bd.bgzf(fastq, bd.even_cuts(len(fastq), 9001), level=1)[0]
    assert len(stream) > 3 * 65536
    (tmp_path / "a.fq.gz").write_bytes(stream)
    for slab_bytes, at_least in ((65536, 4), (1 << 20, 1)):
        slabs, info = fastq_slabs(tmp_path / "a.fq.gz", slab_bytes)
        assert slabs == stream and info == {"first_slab_at": 0, "has_eof": 1, "slabs": info["slabs"], "file_bytes": len(stream)} and info["slabs"] >= at_least
    text = diag(lib.diag_bgzf_inflate(slabs))[0]
    assert text == fd.parse(fastq)[0]
    (tmp_path / "noeof.fq.gz").write_bytes(bd.bgzf(fastq[:5000], [700], eof=False)[0])
    slabs, info = fastq_slabs(tmp_path / "noeof.fq.gz")
    assert info["has_eof"] == 0 and lib.diag_bgzf_inflate(slabs) == fastq[:5000]   # the executables print a warning and go on
    (tmp_path / "cut.fq.gz").write_bytes(stream[:len(stream) - 40])
    with pytest.raises(RuntimeError, match="BGZF block at offset \\d+: the file ends inside the block: truncated"):
        fastq_slabs(tmp_path / "cut.fq.gz")
    head = bd.bgzf(fastq[:5000], [700], eof=False)[0]
    (tmp_path / "mixed.fq.gz").write_bytes(head + gzip.compress(fastq[5000:9000]))   # starts as BGZF, goes on as a plain gzip member
    with pytest.raises(RuntimeError, match=f"BGZF block at offset {len(head)}: not a BGZF block header.*BT_FASTQ_BGZF_ON_HOST=1"):
        fastq_slabs(tmp_path / "mixed.fq.gz")
