"""CPU tests of the packed reads (bt_reads_pack.hpp, run on the host through bt_diag_reads_pack / _unpack / bt_diag_reads_kmers_packed) and of the reads pack
file (bt_reads_pack_file.hpp).  No GPU."""
import os

import numpy as np
import pytest

import reads_data as rd
import reads_pack_data as rp


def _texts():
    rng = np.random.default_rng(1400)
    out = []
    for n in rp.CPU_LENGTHS:
        for _ in range(4):
            out.append(rp.layout_text(rng, n))
    out.append(bytes(range(256)) + b"A")   # every byte value in one text of 257
    return out


def test_packed_bytes():
    from bayestyper_amd import lib

    for n, want in ((0, 0), (1, 48), (127, 48), (128, 48), (129, 96), (256, 96), (257, 144), ((1 << 40) + 1, 48 * ((1 << 33) + 1))):
        assert lib.reads_packed_bytes(n) == want


def test_pack_equals_the_layout_and_unpack_the_canonical_text():
    from bayestyper_amd import lib

    texts = _texts()
    assert sorted({len(t) for t in texts}) == sorted(rp.CPU_LENGTHS)
    assert len(set(b"".join(texts))) == 256 and any(b"\r\n" in t for t in texts) and any(b"NNNN" in t for t in texts) and any(b"aCg" in t for t in texts)
    for t in texts:
        got = lib.diag_reads_pack(t)
        assert got.size == lib.reads_packed_bytes(len(t)) == 48 * -(-len(t) // 128)
        assert np.array_equal(got, rp.np_pack(t)), len(t)
        assert lib.diag_reads_unpack(got, len(t)) == rp.canonical(t), len(t)
        # unpack never trusts more than it is asked for: a shorter prefix of the same packed reads
        if len(t) > 20:
            assert lib.diag_reads_unpack(got, len(t) - 17) == rp.canonical(t)[:-17]


@pytest.mark.parametrize("k", [1, 31, 32, 33, 55, 63, 64])
def test_packed_front_end_equals_the_text_front_end(k):
    """k-mers, hashes and end positions of the packed front end equal the text front end's, on the edge reads plus enough reads to cross the host team's tile
    (4096 positions); the same with every padding bit of the last block set; and against the brute-force restatement for the k-mers"""
    from bayestyper_amd import lib

    rng = np.random.default_rng(1500 + k)
    reads = rd.edge_reads(rng, k) + [rd.random_seq(rng, 150) for _ in range(40)] + [rd.random_seq(rng, 4096 + k), b"ACGTN" * 30]
    for final_newline in (True, False):
        text = rd.reads_text(reads, final_newline)
        assert len(text) > 2 * 4096 and (final_newline or len(text) % 128 != 0)
        want = lib.diag_reads_kmers(text, k)
        assert len(want[0]) > 1000
        packed = lib.diag_reads_pack(text)
        for p in (packed, rp.garbage_padding(packed, len(text)), rp.garbage_padding(packed, len(text), rng)):
            got = lib.diag_reads_kmers_packed(p, len(text), k)
            for g, w in zip(got, want):
                assert np.array_equal(g, w)
    # a prefix of the positions: the bits beyond it are real reads and must be ignored
    cut = len(text) - 333
    want = lib.diag_reads_kmers(text[:cut], k)
    got = lib.diag_reads_kmers_packed(packed, cut, k)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    small = rd.reads_text(rd.edge_reads(rng, k))
    ascii_kmers, ends = rd.brute_force_kmers(small, k)
    got = lib.diag_reads_kmers_packed(lib.diag_reads_pack(small), len(small), k)
    assert got[2].tolist() == ends and len(got[0]) == len(ascii_kmers)
    for n in (0, 1, k - 1, k):
        t = rd.random_seq(rng, n)
        assert len(lib.diag_reads_kmers_packed(lib.diag_reads_pack(t), n, k)[0]) == (1 if n == k else 0)


def _sections(rng, count):
    out = []
    for i in range(count):
        text = rp.layout_text(rng, int(rng.integers(1, 3000)) if i != 2 else 128 * 5)
        out.append((text, int(rng.integers(0, len(text) + 1)), int(rng.integers(0, 40))))
    return out


def _write(lib, path, sections, k=55, manifest="reads\tsample.reads\t17\t1a2b3c4d\nk\t55\n"):
    w = lib.ReadsPackWriter(path, k, manifest)
    try:
        for text, bases, reads in sections:
            w.add(lib.diag_reads_pack(text), len(text), bases, reads)
        w.finish()
    finally:
        w.close()


@pytest.mark.parametrize("count", [0, 1, 5])
def test_file_round_trip(tmp_path, count):
    from bayestyper_amd import lib

    rng = np.random.default_rng(1600 + count)
    sections = _sections(rng, count)
    path = str(tmp_path / "sample.reads.pack")
    manifest = "reads\tsample.reads\t17\t1a2b3c4d\nk\t31\n"
    _write(lib, path, sections, k=31, manifest=manifest)
    want = {"version": 1, "k": 31, "block_positions": 128, "manifest_bytes": len(manifest), "sections": count, "positions": sum(len(t) for t, _, _ in sections),
            "bases": sum(b for _, b, _ in sections), "reads": sum(r for _, _, r in sections), "max_section_positions": max([len(t) for t, _, _ in sections], default=0)}
    assert lib.reads_pack_file_info(path) == want
    r = lib.ReadsPackReader(path)
    assert r.info() == want and r.manifest() == manifest
    got = list(r.sections())
    assert r.next() is None
    r.close()
    assert len(got) == count
    for (packed, positions, bases, reads), (text, b, n) in zip(got, sections):
        assert (positions, bases, reads) == (len(text), b, n)
        assert np.array_equal(packed, rp.np_pack(text)) and lib.diag_reads_unpack(packed, positions) == rp.canonical(text)
    # the size is the sum of its parts: header, sections, trailer
    assert os.path.getsize(path) == 9 + 16 + len(manifest) + 4 + sum(4 + 24 + lib.reads_packed_bytes(len(t)) + 4 for t, _, _ in sections) + 40


def test_writer_leaves_nothing_under_the_final_name_until_finish(tmp_path):
    from bayestyper_amd import lib

    path = str(tmp_path / "sample.reads.pack")
    w = lib.ReadsPackWriter(path, 55, "m")
    w.add(lib.diag_reads_pack(b"ACGT\n"), 5, 4, 1)
    assert not os.path.exists(path)
    assert os.listdir(tmp_path) == ["sample.reads.pack.tmp.%d" % os.getpid()]   # the temporary name carries the process id
    w.close()   # destroyed before finish: the temporary file goes too
    assert os.listdir(tmp_path) == []
    w = lib.ReadsPackWriter(path, 55, "m")
    w.add(lib.diag_reads_pack(b"ACGT\n"), 5, 4, 1)
    w.finish()
    w.close()
    assert os.listdir(tmp_path) == ["sample.reads.pack"]
    with pytest.raises(lib.BtError, match="k must lie in 1 .. 64"):
        lib.ReadsPackWriter(path, 65, "m")
    with pytest.raises(lib.BtError, match="cannot create"):
        lib.ReadsPackWriter(str(tmp_path / "no_such_dir" / "x.pack"), 55, "m")


def test_damaged_files_are_refused_with_the_defect_named(tmp_path):
    from bayestyper_amd import lib

    rng = np.random.default_rng(1700)
    sections = _sections(rng, 3)
    manifest = "reads\tsample.reads\t17\t1a2b3c4d\n"
    good = str(tmp_path / "good.pack")
    _write(lib, good, sections, manifest=manifest)
    data = open(good, "rb").read()
    header = 9 + 16 + len(manifest) + 4
    sizes = [4 + 24 + lib.reads_packed_bytes(len(t)) + 4 for t, _, _ in sections]
    offsets = [header, header + sizes[0], header + sizes[0] + sizes[1]]

    def refused(name, content, match, reader_only=False):
        p = str(tmp_path / name)
        open(p, "wb").write(content)
        if not reader_only:
            with pytest.raises(lib.BtError, match=match):
                lib.reads_pack_file_info(p)
        with pytest.raises(lib.BtError, match=match):
            r = lib.ReadsPackReader(p)
            try:
                list(r.sections())
            finally:
                r.close()

    # cut inside a section (in its payload, and in its head)
    refused("cut_payload", data[:offsets[1] + 40], "truncated in section 1 at offset %d" % offsets[1])
    refused("cut_head", data[:offsets[2] + 10], "truncated in section 2 at offset %d" % offsets[2])
    # every section whole, no trailer; a trailer cut short
    refused("no_trailer", data[:-40], "missing trailer")
    refused("cut_trailer", data[:-7], "truncated trailer")
    # a flipped header byte (k), a flipped manifest byte
    flipped = bytearray(data)
    flipped[9 + 4] ^= 0x04
    refused("header_k", bytes(flipped), "header CRC mismatch")
    flipped = bytearray(data)
    flipped[9 + 16 + 3] ^= 0x01
    refused("header_manifest", bytes(flipped), "header CRC mismatch")
    # another magic
    refused("magic", b"BTAMDKTBL1" + data[10:], "bad magic")
    # a flipped payload bit: open() succeeds (no payload is read there), reading names the section and its offset
    flipped = bytearray(data)
    flipped[offsets[1] + 28 + 5] ^= 0x10
    p = str(tmp_path / "payload")
    open(p, "wb").write(bytes(flipped))
    assert lib.reads_pack_file_info(p)["sections"] == 3
    r = lib.ReadsPackReader(p)
    assert r.next()[1] == len(sections[0][0])
    with pytest.raises(lib.BtError, match="section 1 at offset %d: CRC mismatch" % offsets[1]):
        r.next()
    r.close()
    # a flipped count in a section head is caught by the same CRC, a flipped total by the trailer's
    flipped = bytearray(data)
    flipped[offsets[0] + 4 + 8] ^= 0x01   # bases of section 0
    refused("head_bases", bytes(flipped), "totals mismatch|section 0 at offset %d: CRC mismatch" % offsets[0])
    flipped = bytearray(data)
    flipped[-30] ^= 0x01
    refused("trailer", bytes(flipped), "trailer CRC mismatch")
    refused("extra", data + b"\0", "data after the trailer")
    with pytest.raises(lib.BtError, match="cannot open"):
        lib.reads_pack_file_info(str(tmp_path / "absent"))
