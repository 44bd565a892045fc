"""Inputs of the BAM tests (test_bam_cpu.py, test_bam_gpu.py), written from the SAM specification (sections 4.1 BGZF, 4.2 BAM) with struct and zlib
alone: no project code is used here, so what the tests compare against is independent of what they test."""
import struct
import zlib

import numpy as np

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
# (level, strategy) of the deflate streams the readers have to take: stored, fast / default / best, fixed codes only, distance-1 runs, literals only
STRATEGIES = [(0, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED), (6, zlib.Z_RLE),
              (6, zlib.Z_HUFFMAN_ONLY)]
SIZES = [0, 1, 3, 258, 32768, 32769, 65280, 65536]
STORED_MAX = 65280   # a stored block of more content would not fit BSIZE


def raw_deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=()):
    """a raw deflate stream; flush_at: content offsets at which a Z_FULL_FLUSH ends the deflate block (several deflate blocks in one stream)"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    out, last = b"", 0
    for cut in flush_at:
        out += c.compress(data[last:cut]) + c.flush(zlib.Z_FULL_FLUSH)
        last = cut
    return out + c.compress(data[last:]) + c.flush()


def frame(payload, data, isize=None, crc=None, extra=b""):
    """one BGZF block (SAM 4.1) around a raw deflate payload of `data`; extra: further subfields in front of BC"""
    xlen = len(extra) + 6
    bsize = 12 + xlen + len(payload) + 8 - 1
    assert bsize < 65536, "the block does not fit BSIZE"
    head = struct.pack("<4BI2BH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, xlen) + extra + struct.pack("<2BHH", ord("B"), ord("C"), 2, bsize)
    return head + payload + struct.pack("<II", zlib.crc32(data) if crc is None else crc, len(data) if isize is None else isize)


def bgzf_block(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=(), **kw):
    return frame(raw_deflate(data, level, strategy, flush_at), data, **kw)


def bgzf(data, cuts, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, eof=True):
    """data cut into blocks at the content offsets `cuts` (ascending), the EOF block behind them -> (stream, list of the blocks' offsets in it)"""
    edges = [0] + list(cuts) + [len(data)]
    out, offsets = b"", []
    for a, b in zip(edges[:-1], edges[1:]):
        offsets.append(len(out))
        out += bgzf_block(data[a:b], level, strategy)
    if eof:
        offsets.append(len(out))
        out += EOF_BLOCK
    return out, offsets


def even_cuts(n, size):
    return list(range(size, n, size))


# ---- contents -------------------------------------------------------------------------------------------------------------------------------------------
def contents(rng, n):
    """n bytes of each kind: random, a 7-letter periodic text, zeros, reads text"""
    reads = b"".join(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=150)].tobytes() + b"\n" for _ in range(n // 151 + 1))
    return {"random": rng.integers(0, 256, size=n, dtype=np.uint8).tobytes(), "periodic": (b"GATTACA" * (n // 7 + 1))[:n], "zeros": bytes(n), "reads": reads[:n]}


# ---- hand-assembled deflate streams -----------------------------------------------------------------------------------------------------------------------
class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, value, count):   # least significant bit first (RFC 1951 3.1.1: everything but Huffman codes)
        self.acc |= value << self.n
        self.n += count
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, value, count):   # a Huffman code: most significant bit first
        for i in reversed(range(count)):
            self.bits((value >> i) & 1, 1)

    def done(self):
        if self.n:
            self.out.append(self.acc & 0xFF)
        return bytes(self.out)


def fixed_literal(w, byte):
    if byte < 144:
        w.code(0x30 + byte, 8)
    else:
        w.code(0x190 + byte - 144, 9)


def fixed_distance_before_start():
    """a fixed-Huffman block: literals 'a' 'b', then a match of length 3 at distance 3 — one byte before the output's start -> (payload, what ISIZE says)"""
    w = BitWriter()
    w.bits(1, 1)
    w.bits(1, 2)
    fixed_literal(w, ord("a"))
    fixed_literal(w, ord("b"))
    w.code(1, 7)        # length symbol 257: length 3
    w.code(2, 5)        # distance symbol 2: distance 3
    w.code(0, 7)        # end of block
    return w.done(), 5


def fixed_bad_symbols():
    """fixed-Huffman blocks that use length symbol 286 and distance symbol 30 -> [payload, payload]"""
    out = []
    w = BitWriter()
    w.bits(1, 1)
    w.bits(1, 2)
    w.code(0xC0 + 286 - 280, 8)   # symbols 280..287: 8 bits from 11000000
    w.code(0, 5)
    w.code(0, 7)
    out.append(w.done())
    w = BitWriter()
    w.bits(1, 1)
    w.bits(1, 2)
    fixed_literal(w, ord("a"))
    w.code(1, 7)
    w.code(30, 5)
    w.code(0, 7)
    out.append(w.done())
    return out


def oversubscribed_dynamic():
    """a dynamic header whose code-length code has three codes of one bit -> payload"""
    w = BitWriter()
    w.bits(1, 1)
    w.bits(2, 2)
    w.bits(0, 5)   # HLIT 257
    w.bits(0, 5)   # HDIST 1
    w.bits(0, 4)   # HCLEN 4: lengths of symbols 16, 17, 18, 0
    for length in (1, 1, 1, 0):
        w.bits(length, 3)
    w.bits(0, 32)
    return w.done()


def single_distance_code(n):
    """a dynamic block with literal 'x', length symbol 257 and ONE distance code (symbol 0, one bit): 'x' then n matches of length 3 at distance 1
    -> (payload, data).  Code lengths: literal 'x' 2 bits, end of block 2, symbol 257 1 bit; sent one by one through a code-length code with
    symbols 0, 1, 2 of 1, 2, 2 bits."""
    w = BitWriter()
    w.bits(1, 1)
    w.bits(2, 2)
    w.bits(258 - 257, 5)
    w.bits(0, 5)
    w.bits(18 - 4, 4)   # lengths for 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1]
    cl = {0: 1, 1: 2, 2: 2}
    for s in order:
        w.bits(cl.get(s, 0), 3)
    clcode = {0: (0, 1), 1: (2, 2), 2: (3, 2)}   # canonical: 0 -> 0, 1 -> 10, 2 -> 11
    lens = [0] * 258
    lens[ord("x")], lens[256], lens[257] = 2, 2, 1
    for length in lens + [1]:   # + the single distance code
        w.code(*clcode[length])
    # canonical literal-length codes: 257 -> 0 (1 bit), 'x' -> 10, 256 -> 11
    w.code(2, 2)
    for _ in range(n):
        w.code(0, 1)
        w.code(0, 1)    # the one distance code
    w.code(3, 2)
    return w.done(), b"x" * (1 + 3 * n)


# ---- BAM records (SAM 4.2) --------------------------------------------------------------------------------------------------------------------------------
SEQ_CODES = "=ACMGRSVTWYHKDBN"


def pack_seq(seq):
    codes = [SEQ_CODES.index(c) for c in seq.decode()] + [0]
    return bytes(codes[i] << 4 | codes[i + 1] for i in range(0, len(seq), 2))


def record(seq, flag=0, name=b"r", cigar=(), aux=b"", ref_id=-1, pos=-1):
    """one alignment record; seq: bytes over SEQ_CODES; cigar: list of (length, op)"""
    name = name + b"\0"
    body = struct.pack("<iiBBHHHiiii", ref_id, pos, len(name), 0, 4680, len(cigar), flag, len(seq), -1, -1, 0)
    body += name + b"".join(struct.pack("<I", n << 4 | op) for n, op in cigar) + pack_seq(seq) + b"\xff" * len(seq) + aux
    return struct.pack("<I", len(body)) + body


def expected_line(seq):
    return bytes(c if c in b"ACGT" else ord("N") for c in seq) + b"\n"


def header(text=b"@HD\tVN:1.6\n", refs=(("chr1", 1000),)):
    """the BAM header: magic, text, reference list"""
    out = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for name, length in refs:
        n = name.encode() + b"\0"
        out += struct.pack("<i", len(n)) + n + struct.pack("<i", length)
    return out


def edge_records(rng, k):
    """[(record bytes, seq, flag)]: odd and even l_seq, l_seq 0, k - 1, k, k + 1, 150 and 20 000, every 4-bit code, the flags that matter, long names,
    CIGARs and auxiliary fields"""
    def seq(n):
        return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n)].tobytes()

    recs = []
    for i, n in enumerate([0, 1, 2, k - 1, k, k + 1, 149, 150, 20000]):
        s = seq(n)
        recs.append((record(s, name=b"len%d" % n), s, 0))
    s = SEQ_CODES.encode() + seq(40) + SEQ_CODES.encode()[::-1]
    recs.append((record(s, name=b"codes"), s, 0))
    for flag in (0, 0x10, 0x100, 0x800, 0x900, 0x400, 0x4, 0x1 | 0x40, 0x1 | 0x80 | 0x10):
        s = seq(150)
        recs.append((record(s, flag=flag, name=b"flag%x" % flag, cigar=[(150, 0)], ref_id=0, pos=100), s, flag))
    s = seq(151)
    recs.append((record(s, name=b"n" * 254, cigar=[(1, 0)] * 300, aux=b"NMC\x01" + b"RGZgroup\0" + b"XBBc" + struct.pack("<I", 500) + bytes(500)), s, 0))
    return recs


def records_text(recs, skip_flags):
    return b"".join(expected_line(s) for _, s, f in recs if not f & skip_flags)


def bam_of_reads(reads, flags=None):
    """[(record, seq, flag)] of plain reads (bytes over ACGTN...; lower case is written upper, as a BAM cannot hold case)"""
    out = []
    for i, r in enumerate(reads):
        f = flags[i] if flags else 0
        s = r.upper()
        out.append((record(s, flag=f, name=b"read%d" % i), s, f))
    return out


MANY_RECORDS = [65536, 65537, 66000]   # 256, 257 and 258 workgroups of 256 records: the offsets scan's second round of 256 sums


def short_records(n=MANY_RECORDS[-1]):
    """[(record, seq, flag)] of n reads of 0 to 8 bases with flags drawn from 0, 0x10, 0x100 and 0x800 (about half are skipped under 0x900): many records in
    few bytes (about 45 per record); the tests take prefixes of one list"""
    rng = np.random.default_rng(n)
    reads = [np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=int(b))].tobytes() for b in rng.integers(0, 9, size=n)]
    return bam_of_reads(reads, flags=[int(f) for f in rng.choice([0, 0x10, 0x100, 0x800], size=n)])


def invalid_records():
    """(bytes, offset of the failing record, words) — the failing record stands behind a sound one"""
    good = record(b"ACGT" * 10)
    bad = bytearray(record(b"ACGTACGTAC", cigar=[(10, 0)]))
    out = []
    short = bytearray(bad)
    struct.pack_into("<I", short, 0, struct.unpack_from("<I", bad, 0)[0] - 1)   # one byte less than its own fields
    out.append((good + bytes(short) + good, len(good), "block_size smaller than the record's own fields"))
    tiny = bytearray(bad)
    struct.pack_into("<I", tiny, 0, 31)
    out.append((good + bytes(tiny), len(good), "block_size smaller than the record's own fields"))
    out.append((good + bytes(tiny[:4]), len(good), "block_size smaller than the record's own fields"))   # judged as soon as block_size is there
    neg = bytearray(bad)
    struct.pack_into("<i", neg, 20, -1)
    out.append((good + bytes(neg) + good, len(good), "negative l_seq"))
    out.append((good + bytes(neg[:36]), len(good), "negative l_seq"))   # a record that is not whole is judged by what is there of it
    big = bytearray(bad)
    struct.pack_into("<i", big, 20, 2000)   # l_seq beyond the record
    out.append((good + bytes(big) + good, len(good), "block_size smaller than the record's own fields"))
    return out
