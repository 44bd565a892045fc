"""The host layer's view of an ordinary gzip FASTQ (bayestyper_amd/host/GzipFile.cpp): which files isGzipFastq takes, and GzipFastqFile's slabs.  No GPU."""
import ctypes as C
import gzip

import numpy as np
import pytest

import bam_data as bd
import fastq_data as fd
import gunzip_data as gd


def _host():
    from bayestyper_amd import host

    dll = host.dll
    dll.bth_fastq_is_gzip.restype = C.c_int
    dll.bth_fastq_is_gzip.argtypes = [C.c_char_p, C.c_char_p, C.c_uint]
    dll.bth_gzip_fastq_file_slabs.restype = C.c_longlong
    dll.bth_gzip_fastq_file_slabs.argtypes = [C.c_char_p, C.c_ulonglong, C.c_char_p, C.c_ulonglong, C.c_void_p, C.c_char_p, C.c_uint]
    return dll


def is_gzip_fastq(path):
    err = C.create_string_buffer(1024)
    rc = _host().bth_fastq_is_gzip(str(path).encode(), err, 1024)
    if rc < 0:
        raise RuntimeError(err.value.decode())
    return bool(rc)


def test_is_gzip_fastq_and_its_lookalikes(tmp_path):
    from test_fastq_cpu import is_bgzf_fastq

    fastq = b"".join(fd.simple_records(np.random.default_rng(2), 50))
    verdicts = {
        "plain.fq.gz": (gzip.compress(fastq), True),
        "named.fq.gz": (gd.gzip_member(fastq, name=b"reads.fastq", extra=b"AB\x02\x00xy", hcrc=True, comment=b"c"), True),
        "level0.fq.gz": (gzip.compress(fastq, 0), True),
        "two_members.fq.gz": (gzip.compress(fastq[:100]) + gzip.compress(fastq[100:]), True),
        "bgzf.fq.gz": (bd.bgzf(fastq, [300, 700])[0], False),        # isBgzfFastq's
        "plain.fa.gz": (gzip.compress(b">a\nACGT\n"), False),        # stays with zlib
        "empty_member.gz": (gzip.compress(b""), False),
        "plain.fq": (fastq, False),
        "empty": (b"", False),
        "x.bam": (bd.bgzf(bd.header() + bd.record(b"ACGT"), [])[0], False),
        "method.gz": (b"\x1f\x8b\x07" + gzip.compress(fastq)[3:], False),
        "short.gz": (gzip.compress(fastq)[:12], False),
    }
    for name, (content, want) in verdicts.items():
        (tmp_path / name).write_bytes(content)
        assert is_gzip_fastq(tmp_path / name) == want, name
        assert is_bgzf_fastq(tmp_path / name) == (name == "bgzf.fq.gz"), name   # isBgzfFastq's verdicts are what they were
    with pytest.raises(RuntimeError, match="Unable to open"):
        is_gzip_fastq(tmp_path / "missing.fq.gz")


@pytest.mark.parametrize("slab", [1, 4096, 100_003, 1 << 20])
def test_gzip_fastq_file_slabs_are_the_file(tmp_path, slab):
    content = gzip.compress(gd.fastq(3, reads=200 if slab > 1 else 5))
    path = tmp_path / "reads.fq.gz"
    path.write_bytes(content)
    dll, err, stats = _host(), C.create_string_buffer(1024), np.zeros(3, np.uint64)
    need = dll.bth_gzip_fastq_file_slabs(str(path).encode(), slab, None, 0, stats.ctypes.data_as(C.c_void_p), err, 1024)
    assert need == len(content), err.value
    buf = C.create_string_buffer(need)
    assert dll.bth_gzip_fastq_file_slabs(str(path).encode(), slab, buf, need, stats.ctypes.data_as(C.c_void_p), err, 1024) == need
    assert buf.raw[:need] == content
    assert [int(x) for x in stats] == [-(-len(content) // slab), len(content), min(slab, len(content))]
