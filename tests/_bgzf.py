"""Shared by the tests of the BGZF route (bt_bgzf / bt_diag_bgzf / bt_bgzf_save, the tabix index): a BGZF block walker, a .tbi parser and a region query,
all written from the specifications (SAM specification sections 4.1 and 5.3, "The Tabix index file format") over Python's zlib and gzip — no code of the
project's is used to read what the project wrote."""
import gzip
import struct
import zlib

BLOCK = 65280   # input bytes per block (include/btgpu.h)
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
SIZES = (0, 1, 3, 4, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK, 2 * BLOCK + 1, 3 * BLOCK + 17)


def walk(stream):
    """the blocks of a BGZF stream: a list of dictionaries offset, size, payload, crc, isize; every header field is checked on the way"""
    blocks, at = [], 0
    while at < len(stream):
        assert len(stream) - at >= 26, "a truncated block at %d" % at
        magic, cm, flg, mtime, xfl, os_, xlen = struct.unpack_from("<HBBIBBH", stream, at)
        assert (magic, cm, flg, mtime, xfl, os_, xlen) == (0x8b1f, 8, 4, 0, 0, 0xff, 6), "header of the block at %d" % at
        si1, si2, slen, bsize = struct.unpack_from("<BBHH", stream, at + 12)
        assert (si1, si2, slen) == (66, 67, 2), "extra field of the block at %d" % at
        size = bsize + 1
        assert 26 <= size <= 65536 and at + size <= len(stream), "BSIZE of the block at %d" % at
        crc, isize = struct.unpack_from("<II", stream, at + size - 8)
        blocks.append(dict(offset=at, size=size, payload=stream[at + 18:at + size - 8], crc=crc, isize=isize))
        at += size
    return blocks


def check_stream(stream, content, offsets=None, eof=True):
    """everything tests/test_bgzf_cpu.py asks of a stream that holds `content`; returns the walker's blocks"""
    assert gzip.decompress(stream) == content
    blocks = walk(stream)
    data = blocks[:-1] if eof else blocks
    assert len(data) == (len(content) + BLOCK - 1) // BLOCK
    for i, b in enumerate(data):
        want = content[i * BLOCK:(i + 1) * BLOCK]
        z = zlib.decompressobj(-15)
        assert z.decompress(b["payload"]) == want and z.eof and z.unused_data == b""   # a complete raw deflate stream, nothing behind it
        assert b["crc"] == zlib.crc32(want) and b["isize"] == len(want) and len(want) > 0
    if eof:
        assert stream[-28:] == EOF_BLOCK and blocks[-1]["size"] == 28 and blocks[-1]["isize"] == 0
    if offsets is not None:
        assert list(offsets) == [b["offset"] for b in data] + [blocks[-1]["offset"] if eof else len(stream)]
    return blocks


class Reader:
    """reads a BGZF file by virtual offsets (block offset << 16 | offset inside the block's data)"""

    def __init__(self, stream):
        self.stream = stream
        self.blocks = walk(stream)
        self.index = {b["offset"]: i for i, b in enumerate(self.blocks)}
        self.cache = {}

    def data(self, i):
        if i not in self.cache:
            self.cache[i] = zlib.decompress(self.blocks[i]["payload"], -15)
        return self.cache[i]

    def read(self, vbeg, vend):
        """the bytes from virtual offset vbeg up to vend"""
        assert vbeg <= vend
        i, within = self.index[vbeg >> 16], vbeg & 0xFFFF
        j, upto = self.index[vend >> 16], vend & 0xFFFF
        assert within <= len(self.data(i)) and upto <= len(self.data(j))
        out = []
        while i < j:
            out.append(self.data(i)[within:])
            i, within = i + 1, 0
        out.append(self.data(j)[within:upto])
        return b"".join(out)


def parse_tbi(raw):
    """the uncompressed bytes of a .tbi -> dictionary: header fields, names, per contig bins {bin: [(beg, end), ..]} and the linear index, n_no_coor"""
    assert raw[:4] == b"TBI\x01"
    n_ref, fmt, col_seq, col_beg, col_end, meta, skip, l_nm = struct.unpack_from("<8i", raw, 4)
    at = 36
    names = raw[at:at + l_nm].split(b"\0")
    assert names[-1] == b"" and len(names) == n_ref + 1
    at += l_nm
    refs = []
    for _ in range(n_ref):
        (n_bin,) = struct.unpack_from("<i", raw, at)
        at += 4
        bins = {}
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", raw, at)
            at += 8
            assert b not in bins
            bins[b] = [struct.unpack_from("<QQ", raw, at + 16 * c) for c in range(n_chunk)]
            at += 16 * n_chunk
        (n_intv,) = struct.unpack_from("<i", raw, at)
        at += 4
        linear = list(struct.unpack_from("<%dQ" % n_intv, raw, at))
        at += 8 * n_intv
        refs.append(dict(bins=bins, linear=linear))
    n_no_coor = None
    if at < len(raw):
        (n_no_coor,) = struct.unpack_from("<Q", raw, at)
        at += 8
    assert at == len(raw)
    return dict(format=fmt, col_seq=col_seq, col_beg=col_beg, col_end=col_end, meta=meta, skip=skip, names=[n.decode() for n in names[:-1]], refs=refs, n_no_coor=n_no_coor)


def reg2bin(beg, end):
    """SAM specification 5.3: the bin of [beg, end), 0-based half-open"""
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def reg2bins(beg, end):
    """SAM specification 5.3: the bins that may hold records overlapping [beg, end)"""
    end -= 1
    bins = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        bins.extend(range(first + (beg >> shift), first + (end >> shift) + 1))
    return bins


def line_interval(line):
    """(contig, beg, end) of a VCF data line: [POS - 1, POS - 1 + len(REF))"""
    f = line.split(b"\t", 4)
    return f[0].decode(), int(f[1]) - 1, int(f[1]) - 1 + len(f[3])


def query(tbi, reader, contig, beg, end):
    """the data lines of `contig` that overlap [beg, end), found the way a tabix reader finds them: candidate bins, chunks that end before the linear
    index's offset of the region's first window dropped, lines read from each chunk's start to its end"""
    if contig not in tbi["names"] or beg >= end:
        return []
    ref = tbi["refs"][tbi["names"].index(contig)]
    linear = ref["linear"]
    min_off = 0 if not linear else linear[min(beg >> 14, len(linear) - 1)]
    chunks = sorted(c for b in reg2bins(beg, end) for c in ref["bins"].get(b, ()) if c[1] > min_off)
    out = []
    for cbeg, cend in chunks:
        text = reader.read(cbeg, cend)
        assert text.endswith(b"\n")   # a chunk holds whole lines
        for line in text.split(b"\n")[:-1]:
            assert not line.startswith(b"#")
            name, lbeg, lend = line_interval(line)
            if name == contig and lbeg < end and lend > beg:
                out.append(line)
    return out


def brute_force(text, contig, beg, end):
    out = []
    for line in text.split(b"\n"):
        if line and not line.startswith(b"#"):
            name, lbeg, lend = line_interval(line)
            if name == contig and lbeg < end and lend > beg and beg < end:
                out.append(line)
    return out
