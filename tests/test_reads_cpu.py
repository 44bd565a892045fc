"""CPU tests of the reads scan (bt_reads.hip): the kernels' window code run on the host (bt_diag_reads_kmers, bt_diag_reads_sketch) against a brute-force
restatement and the oracle, and the sketch's estimator.  No GPU."""
import numpy as np
import pytest

import reads_data as rd

KS = [1, 31, 32, 33, 55, 63, 64]


def _check_text(lib, oracle, text, k):
    kmers, hashes, ends = lib.diag_reads_kmers(text, k)
    # brute force: per window the alphabet check, the reverse complement, the minimum
    want, want_ends = rd.brute_force_kmers(text, k)
    assert len(kmers) == len(want)
    assert np.array_equal(ends, np.array(want_ends, np.uint64))
    if want:
        flat = np.frombuffer(b"".join(want), np.uint8)
        assert np.array_equal(kmers, oracle.pack(flat, k))
        assert np.array_equal(hashes, oracle.ntp64(flat, k))   # the rolled hash is nthash64(canonical, k) bit for bit
    # the oracle's own sliding window over the text
    ok, oe = rd.oracle_kmers(oracle, text, k)
    assert np.array_equal(kmers, ok) and np.array_equal(ends, oe)
    return len(want)


@pytest.mark.parametrize("k", KS)
def test_host_front_end_equals_brute_force(oracle, k):
    """reads of length k-1, k, k+1 and 150, N at the first, the last and every k-th base, lower case, a reverse-palindromic k-mer, an empty line, with and
    without the final newline"""
    from bayestyper_amd import lib

    rng = np.random.default_rng(1000 + k)
    reads = rd.edge_reads(rng, k)
    n = _check_text(lib, oracle, rd.reads_text(reads), k)
    assert n > 0
    assert _check_text(lib, oracle, rd.reads_text(reads[:4], final_newline=False), k) == 1 + 2 + (151 - k)
    # every read alone: nothing is carried from one text to the next
    assert sum(len(lib.diag_reads_kmers(r, k)[0]) for r in reads) == n
    # a text shorter than k, and an empty one
    assert len(lib.diag_reads_kmers(rd.random_seq(rng, k - 1), k)[0]) == 0
    assert len(lib.diag_reads_kmers(b"", k)[0]) == 0


@pytest.mark.parametrize("k", [31, 64])
def test_host_front_end_across_its_tiles(oracle, k):
    """the host team walks tiles of 4096 positions: reads that end on, start at and straddle a tile's last byte"""
    from bayestyper_amd import lib

    rng = np.random.default_rng(2000 + k)
    pad = rd.random_seq(rng, 4096 - 150 - 1)
    text = pad + b"\n" + rd.random_seq(rng, 150) + rd.random_seq(rng, 150) + b"\n" + rd.random_seq(rng, 4096 - 151 - 75) + b"\n" + rd.random_seq(rng, 150) + b"\n"
    _check_text(lib, oracle, text, k)


def test_no_kmer_spans_two_reads(oracle):
    from bayestyper_amd import lib

    a, b = b"ACGTACGTAC", b"GGGTTTCCCA"
    assert len(lib.diag_reads_kmers(a + b, 5)[0]) == 16
    apart = lib.diag_reads_kmers(a + b"\n" + b, 5)[0]
    assert len(apart) == 12
    for sep in (b"\n", b"\r\n", b"N", b"n", b" ", b"\x00", b"\xff"):
        assert np.array_equal(lib.diag_reads_kmers(a + sep + b, 5)[0], apart)


def test_diag_reads_kmers_reports_a_small_buffer():
    import ctypes as C

    from bayestyper_amd import lib

    text = np.frombuffer(b"ACGTACGTACGT", np.uint8)
    out = np.zeros((2, 2), np.uint64)
    n = C.c_uint64()
    rc = lib.bt_diag_reads_kmers(text.ctypes.data_as(C.c_void_p), text.size, 4, out.ctypes.data_as(C.c_void_p), None, None, 2, C.byref(n))
    assert rc != 0 and n.value == 9 and b"buffer too small" in lib.bt_last_error()
    with pytest.raises(lib.BtError, match="k must lie in 1 .. 64"):
        lib.diag_reads_kmers(b"ACGT", 65)
    with pytest.raises(lib.BtError, match="k must lie in 1 .. 64"):
        lib.diag_reads_kmers(b"ACGT", 0)


def test_host_sketch_equals_its_restatement(oracle):
    """bt_diag_reads_sketch: register = top 16 bits of the finalised hash, rank = 1 + leading zeros of the other 48 bits, maximum per register; merging two texts'
    registers equals the sketch of both"""
    from bayestyper_amd import lib

    rng = np.random.default_rng(31)
    k = 31
    reads = [rd.random_seq(rng, 150) for _ in range(400)]
    text = rd.reads_text(reads)
    want = rd.sketch_registers(lib.diag_reads_kmers(text, k)[1])
    got = lib.diag_reads_sketch(text, k)
    assert np.array_equal(got, want) and got.max() <= 49 and (got > 0).sum() > 20_000
    half = lib.diag_reads_sketch(rd.reads_text(reads[:137]), k)
    assert np.array_equal(lib.diag_reads_sketch(rd.reads_text(reads[137:]), k, registers=half), want)


SKETCH_BOUND = 0.025   # six standard errors of a 2^16-register sketch: 6 * 1.04 / 256 = 2.44 %


@pytest.mark.parametrize("n", [2_000, 50_000, 400_000])
def test_sketch_estimate(n):
    """registers built by the host front end from n distinct random k-mers: linear counting (2 000 and 50 000 lie below 2.5 x 2^16 = 163 840) and the raw
    estimator (400 000)"""
    from bayestyper_amd import lib

    rng = np.random.default_rng(n)
    k = 31
    text = rd.random_reads_text(rng, n, k)
    distinct = len(rd.kmer_multiset(lib.diag_reads_kmers(text, k)[0])[0])
    assert distinct >= n - 2
    est = lib.reads_sketch_estimate(lib.diag_reads_sketch(text, k))
    print(f"distinct {distinct}, estimate {est:.1f}, error {abs(est - distinct) / distinct:.4%}")
    assert abs(est - distinct) <= SKETCH_BOUND * distinct


def test_sketch_estimate_edges():
    from bayestyper_amd import lib

    assert lib.reads_sketch_estimate(np.zeros(lib.SKETCH_REGISTERS, np.uint8)) == 0.0
    one = np.zeros(lib.SKETCH_REGISTERS, np.uint8)
    one[7] = 3
    assert abs(lib.reads_sketch_estimate(one) - 1.0) < 1e-4   # linear counting: m ln(m / (m - 1))
    with pytest.raises(lib.BtError, match="above 49"):
        lib.reads_sketch_estimate(np.full(lib.SKETCH_REGISTERS, 50, np.uint8))


# ---- the reads reader (bayestyper_amd/host/ReadsFile.cpp) ----
def _reader():
    import ctypes as C

    from bayestyper_amd import host

    dll = host.dll
    dll.bth_reads_file_slabs.restype = C.c_longlong
    dll.bth_reads_file_slabs.argtypes = [C.c_char_p, C.c_uint, C.c_ulonglong, C.c_char_p, C.c_ulonglong, C.c_void_p, C.c_char_p, C.c_uint]
    dll.bth_reads_list.restype = C.c_longlong
    dll.bth_reads_list.argtypes = [C.c_char_p, C.c_char_p, C.c_ulonglong, C.c_char_p, C.c_uint]
    return dll


def read_slabs(path, k, slab_bytes):
    """bth_reads_file_slabs -> (list of slabs, bases, reads); RuntimeError with the reader's message"""
    import ctypes as C

    dll = _reader()
    err = C.create_string_buffer(1024)
    stats = np.zeros(2, np.uint64)
    need = dll.bth_reads_file_slabs(str(path).encode(), k, slab_bytes, None, 0, stats.ctypes.data_as(C.c_void_p), err, 1024)
    if need < 0:
        raise RuntimeError(err.value.decode())
    buf = C.create_string_buffer(max(need, 1))
    assert dll.bth_reads_file_slabs(str(path).encode(), k, slab_bytes, buf, need, stats.ctypes.data_as(C.c_void_p), err, 1024) == need
    raw = buf.raw[:need]
    return (raw[:-1].split(b"\0") if need else []), int(stats[0]), int(stats[1])


def _fastq(reads, rng, eol=b"\n"):
    out = []
    for i, r in enumerate(reads):
        q = bytearray(rng.integers(33, 74, size=len(r)).astype(np.uint8).tobytes())
        if q:
            q[0] = ord("@") if i % 2 == 0 else ord("+")   # quality lines that look like headers
        out.append(b"@read%d some text" % i + eol + r + eol + b"+" + (b"read%d" % i if i % 3 == 0 else b"") + eol + bytes(q) + eol)
    return b"".join(out)


def _fasta(reads, width=None, eol=b"\n"):
    out = []
    for i, r in enumerate(reads):
        lines = [r[a:a + width] for a in range(0, len(r), width)] if width else [r]
        out.append(b">read%d" % i + eol + b"".join(line + eol for line in lines))
    return b"".join(out)


def test_reads_file_formats_give_identical_slabs(tmp_path):
    """the same reads as FASTA, FASTA wrapped at 60 columns, FASTQ with quality lines starting with '@' and '+', with CRLF, without the final newline and gzipped:
    identical slabs, each made of whole reads and no larger than asked for"""
    import gzip

    rng = np.random.default_rng(77)
    k = 31
    reads = [rd.random_seq(rng, int(n)) for n in rng.integers(1, 400, size=500)] + [r for r in rd.edge_reads(rng, k) if r]
    files = {
        "plain.fa": _fasta(reads), "wrapped.fa": _fasta(reads, 60), "reads.fq": _fastq(reads, rng), "crlf.fa": _fasta(reads, 60, b"\r\n"), "crlf.fq": _fastq(reads, rng, b"\r\n"),
        "no_newline.fa": _fasta(reads, 60)[:-1], "no_newline.fq": _fastq(reads, rng)[:-1], "blank_lines.fq": _fastq(reads[:250], rng) + b"\n\n" + _fastq(reads[250:], rng).replace(b"@read", b"@x") + b"\n",
    }
    for name, data in list(files.items()):
        files[name + ".gz"] = gzip.compress(data)
    want = None
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
        slabs, bases, n = read_slabs(tmp_path / name, k, 4096)
        assert b"".join(slabs) == rd.reads_text(reads), name
        assert bases == sum(map(len, reads)) and n == len(reads), name
        assert all(0 < len(s) <= 4096 and s.endswith(b"\n") for s in slabs) and len(slabs) > 10, name
        want = want or slabs
        assert slabs == want, name
    # one slab when it is large enough; an empty file has no slab
    assert read_slabs(tmp_path / "reads.fq.gz", k, 1 << 20)[0] == [rd.reads_text(reads)]
    (tmp_path / "empty.fa").write_bytes(b"")
    assert read_slabs(tmp_path / "empty.fa", k, 4096) == ([], 0, 0)


@pytest.mark.parametrize("k", [31, 64])
def test_reads_file_cuts_long_reads_with_an_overlap(tmp_path, k):
    """a slab smaller than a read: the pieces overlap by k - 1 bases, so the multiset of k-mers equals the uncut text's"""
    from bayestyper_amd import lib

    rng = np.random.default_rng(78 + k)
    reads = [rd.random_seq(rng, 3000), rd.random_seq(rng, 100), rd.random_seq(rng, 799), rd.random_seq(rng, 800), rd.random_seq(rng, 12_345), rd.random_seq(rng, 10)]
    (tmp_path / "long.fa").write_bytes(_fasta(reads, 70))
    slabs, bases, _ = read_slabs(tmp_path / "long.fa", k, 800)
    assert bases == sum(map(len, reads)) and all(len(s) <= 800 for s in slabs) and len(slabs) > 20
    got = np.concatenate([lib.diag_reads_kmers(s, k)[0] for s in slabs])
    want = lib.diag_reads_kmers(rd.reads_text(reads), k)[0]
    gk, gc = rd.kmer_multiset(got)
    wk, wc = rd.kmer_multiset(want)
    assert len(got) == len(want) and np.array_equal(gk, wk) and np.array_equal(gc, wc)
    # the smallest slab the reader accepts (2k + 2) still loses nothing
    tiny = np.concatenate([lib.diag_reads_kmers(s, k)[0] for s in read_slabs(tmp_path / "long.fa", k, 1)[0]])
    assert len(tiny) == len(want)


def test_reads_file_errors(tmp_path):
    import gzip

    rng = np.random.default_rng(79)
    reads = [rd.random_seq(rng, 150) for _ in range(2000)]
    gz = gzip.compress(_fastq(reads, rng))
    (tmp_path / "truncated.fq.gz").write_bytes(gz[:len(gz) // 2])
    with pytest.raises(RuntimeError, match="truncated.fq.gz: damaged or truncated compressed data"):
        read_slabs(tmp_path / "truncated.fq.gz", 31, 1 << 16)
    lines = _fastq(reads[:10], rng).split(b"\n")
    for drop in range(4, 8):   # a FASTQ with a missing line (each of a record's four in turn), and one that ends inside a record
        (tmp_path / "missing.fq").write_bytes(b"\n".join(lines[:drop] + lines[drop + 1:]))
        with pytest.raises(RuntimeError, match=r"missing.fq: .*a missing line\?"):
            read_slabs(tmp_path / "missing.fq", 31, 1 << 16)
    (tmp_path / "short.fq").write_bytes(b"\n".join(lines[:38]) + b"\n")
    with pytest.raises(RuntimeError, match="short.fq: truncated FASTQ record at the end of the file"):
        read_slabs(tmp_path / "short.fq", 31, 1 << 16)
    (tmp_path / "other.txt").write_bytes(b"ACGT\n")
    with pytest.raises(RuntimeError, match="neither FASTA nor FASTQ"):
        read_slabs(tmp_path / "other.txt", 31, 1 << 16)
    with pytest.raises(RuntimeError, match="Unable to open read file"):
        read_slabs(tmp_path / "nothing_here.fq", 31, 1 << 16)


def test_reads_list(tmp_path):
    import ctypes as C

    dll = _reader()
    (tmp_path / "sub").mkdir()
    (tmp_path / "sub" / "s1.reads").write_bytes(b"a_1.fq.gz\n\n../b.fa \r\n/abs/c.fq\n")
    buf, err = C.create_string_buffer(4096), C.create_string_buffer(1024)
    n = dll.bth_reads_list(str(tmp_path / "sub" / "s1").encode(), buf, 4096, err, 1024)
    d = str(tmp_path / "sub") + "/"
    assert buf.raw[:n].decode().split("\n")[:-1] == [d + "a_1.fq.gz", d + "../b.fa", "/abs/c.fq"]
    assert dll.bth_reads_list(str(tmp_path / "sub" / "s2").encode(), buf, 4096, err, 1024) == -1 and b"Unable to open reads list" in err.value
    (tmp_path / "sub" / "s3.reads").write_bytes(b"\n\n")
    assert dll.bth_reads_list(str(tmp_path / "sub" / "s3").encode(), buf, 4096, err, 1024) == -1 and b"names no read file" in err.value
