"""Raw deflate streams and gzip files for the tests of the parallel gunzip (bayestyper_amd/csrc/bt_gunzip.hpp), from Python's zlib and from a few lines of
RFC 1951 written here: no project code.  The yardstick for every stream is zlib's own inflate (`inflate`); `walk_blocks` lists a small stream's block
boundaries bit by bit."""
import struct
import zlib

import numpy as np

import fastq_data as fd

KIB = 1024
CHUNKS = (1 * KIB, 4 * KIB, 16 * KIB, 1024 * KIB)


def inflate(raw, window=b""):
    """zlib's answer for a raw deflate stream (that starts at a byte boundary) -> (bytes, stream ended, compressed bytes used)"""
    d = zlib.decompressobj(-15, zdict=window) if window else zlib.decompressobj(-15)
    out = d.decompress(raw)
    return out, d.eof, len(raw) - len(d.unused_data)


def fastq_records(seed, reads=3000, bases=150):
    """the project's own shape: reads of 150 nt, about 330 bytes a record"""
    rng = np.random.default_rng(seed)
    return [fd.record(rng, i, fd.random_seq(rng, bases)) for i in range(reads)]


def fastq(seed, reads=3000, bases=150):
    return b"".join(fastq_records(seed, reads, bases))


def raw(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(data) + c.flush()


def sync_flushed(data, seed, lo=2000, hi=5000, level=6, final=True):
    """pigz-like: a Z_SYNC_FLUSH every lo..hi bytes (an empty stored block; back-references cross it) -> (stream, content offsets of the flush points)"""
    rng = np.random.default_rng(seed)
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8)
    out, at, cuts = b"", 0, []
    while at < len(data):
        step = int(rng.integers(lo, hi + 1))
        out += c.compress(data[at:at + step])
        at += step
        if at < len(data):
            out += c.flush(zlib.Z_SYNC_FLUSH)
            cuts.append(at)
    return out + (c.flush() if final else c.flush(zlib.Z_SYNC_FLUSH)), cuts


def stored(payload, final=True):
    """payload as stored blocks of at most 65535 bytes (what level 0 writes)"""
    out, pieces = b"", [payload[i:i + 65535] for i in range(0, len(payload), 65535)] or [b""]
    for i, p in enumerate(pieces):
        out += bytes([1 if final and i + 1 == len(pieces) else 0]) + struct.pack("<HH", len(p), len(p) ^ 0xFFFF) + p
    return out


# ---- RFC 1951 by hand ----------------------------------------------------------------------------------------------------------------------------------------
class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, value, count):   # least significant bit first
        self.acc |= value << self.n
        self.n += count
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, value, count):   # a Huffman code: most significant bit first
        self.bits(int(format(value, "0%db" % count)[::-1], 2), count)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def bytes(self):
        assert self.n == 0
        return bytes(self.out)


def _fixed_litlen(w, s):
    if s < 144:
        w.code(0x30 + s, 8)
    elif s < 256:
        w.code(0x190 + s - 144, 9)
    elif s < 280:
        w.code(s - 256, 7)
    else:
        w.code(0xC0 + s - 280, 8)


_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def fixed_block(items, final=False, pad_bits=0):
    """one fixed-Huffman block: items are bytes (literals) or (length, distance) pairs; then, when not final, an empty stored block that realigns the stream
    (pad_bits: an empty fixed block of 10 bits is put in front that many times, so that the block starts at another bit)"""
    w = BitWriter()
    for _ in range(pad_bits):
        w.bits(0b010, 3)
        _fixed_litlen(w, 256)
    w.bits((1 if final else 0) | 2, 3)
    for it in items:
        if isinstance(it, tuple):
            length, dist = it
            lc = max(i for i, b in enumerate(_LEN_BASE) if b <= length) if length != 258 else 28
            _fixed_litlen(w, 257 + lc)
            w.bits(length - _LEN_BASE[lc], _LEN_EXTRA[lc])
            dc = max(i for i, b in enumerate(_DIST_BASE) if b <= dist)
            w.code(dc, 5)
            w.bits(dist - _DIST_BASE[dc], _DIST_EXTRA[dc])
        else:
            for byte in it:
                _fixed_litlen(w, byte)
    _fixed_litlen(w, 256)
    if not final:
        w.bits(0, 3)
    w.align()
    if not final:
        w.bits(0x0000, 16)
        w.bits(0xFFFF, 16)
    return w.bytes()


def walk_blocks(stream, start_bit=0):
    """a bit-by-bit inflate of a SMALL stream -> (the bit offset of every block's start and of the stream's end, the output's length at each of them)"""
    pos = start_bit

    def bits(n):
        nonlocal pos
        v = 0
        for i in range(n):
            v |= ((stream[(pos + i) >> 3] >> ((pos + i) & 7)) & 1) << i
        pos += n
        return v

    def table(lengths):
        codes, code = {}, 0
        for l in range(1, 16):
            for s, sl in enumerate(lengths):
                if sl == l:
                    codes[(l, code)] = s
                    code += 1
            code <<= 1
        return codes

    def symbol(codes):
        code = 0
        for l in range(1, 16):
            code = (code << 1) | bits(1)
            if (l, code) in codes:
                return codes[(l, code)]
        raise ValueError("no code")

    starts, lengths_at, out_len = [], [], 0
    while True:
        starts.append(pos)
        lengths_at.append(out_len)
        last, kind = bits(1), bits(2)
        if kind == 0:
            pos = (pos + 7) & ~7
            n = bits(16)
            assert bits(16) == n ^ 0xFFFF
            pos += 8 * n
            out_len += n
        else:
            if kind == 1:
                lit, dist = table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), table([5] * 30)
            else:
                nlit, ndist, nclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
                cl = [0] * 19
                for i in range(nclen):
                    cl[(16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)[i]] = bits(3)
                clt, lens = table(cl), []
                while len(lens) < nlit + ndist:
                    s = symbol(clt)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + bits(2))
                    elif s == 17:
                        lens += [0] * (3 + bits(3))
                    else:
                        lens += [0] * (11 + bits(7))
                lit, dist = table(lens[:nlit]), table(lens[nlit:])
            while True:
                s = symbol(lit)
                if s < 256:
                    out_len += 1
                elif s == 256:
                    break
                else:
                    out_len += _LEN_BASE[s - 257] + bits(_LEN_EXTRA[s - 257])
                    d = symbol(dist)
                    bits(_DIST_EXTRA[d])
        if last:
            break
    return starts + [pos], lengths_at + [out_len]


# ---- the inputs ------------------------------------------------------------------------------------------------------------------------------------------------
def window_edges(seed):
    """A stream for the windows: 40 000 random bytes; a compressed text; a fixed block with a 258-byte match at distance 32768, a short match at distance 32768
    and an overlapping copy (distance 1, length 258) of its last byte; two more compressed texts, each followed by a fixed block that copies from the
    output of the fixed block two parts before.  Every part starts with a dynamic header at a byte boundary (a candidate) and its matches reach before it."""
    rng = np.random.default_rng(seed)
    noise = rng.integers(0, 256, size=40000).astype(np.uint8).tobytes()
    text = [b"".join(fd.simple_records(np.random.default_rng(seed + 1 + i), 60, 40)) for i in range(3)]

    def part(t):
        c = zlib.compressobj(6, zlib.DEFLATED, -15, 8)
        return c.compress(t) + c.flush(zlib.Z_SYNC_FLUSH)

    stream = raw_nonfinal(noise)
    stream += part(text[0]) + fixed_block([(258, 32768), b"x", (3, 32768), (258, 1), b"y"])
    stream += part(text[1]) + fixed_block([(258, len(text[1]) + 300), (100, 32768), (258, 1)], pad_bits=3)
    stream += part(text[2]) + fixed_block([(258, len(text[2]) + 400), (258, 1), b"z"], final=True)
    return stream


def raw_nonfinal(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8)
    return c.compress(data) + c.flush(zlib.Z_SYNC_FLUSH)


def unsplittable():
    text = fastq(5, reads=300)
    return {
        "level0": raw(text, 0),
        "fixed": raw(text, 6, zlib.Z_FIXED),
        "huffman_only": raw(text, 6, zlib.Z_HUFFMAN_ONLY),
        "rle": raw(text, 6, zlib.Z_RLE),
        "empty": raw(b""),
        "one_final_block": raw(text[:20000]),
    }


def false_candidates():
    """a level-6 stream as the payload of a level-0 stream: full of true dynamic headers that are no block starts of the outer stream"""
    return stored(raw(fastq(6, reads=1500)))


def repeated_read():
    """1 MB of one read: a ratio far above any budget"""
    rng = np.random.default_rng(8)
    rec = fd.record(rng, 1, fd.random_seq(rng, 150))
    return raw(rec * (1_000_000 // len(rec)))


def gzip_member(data, level=6, name=None, extra=None, hcrc=False, comment=None, crc=None, isize=None, payload=None):
    flg = (2 if hcrc else 0) | (4 if extra is not None else 0) | (8 if name is not None else 0) | (16 if comment is not None else 0)
    head = struct.pack("<4BI2B", 0x1F, 0x8B, 8, flg, 0, 0, 3)
    if extra is not None:
        head += struct.pack("<H", len(extra)) + extra
    if name is not None:
        head += name + b"\0"
    if comment is not None:
        head += comment + b"\0"
    if hcrc:
        head += struct.pack("<H", zlib.crc32(head) & 0xFFFF)
    body = raw(data, level) if payload is None else payload
    return head + body + struct.pack("<II", zlib.crc32(data) if crc is None else crc, (len(data) & 0xFFFFFFFF) if isize is None else isize)


def bit_flips(stream, count, seed):
    """`count` copies of the stream with one bit flipped each, the bits spread over the stream"""
    rng = np.random.default_rng(seed)
    out = []
    for bit in sorted(rng.choice(len(stream) * 8, size=count, replace=False)):
        b = bytearray(stream)
        b[bit >> 3] ^= 1 << (bit & 7)
        out.append((int(bit), bytes(b)))
    return out


def flip_base():
    """the stream the flips are made in: sync-flushed FASTQ, small enough for 200 runs"""
    return sync_flushed(fastq(9, reads=120), 9, 2000, 5000)[0]


def corpus():
    """name -> raw deflate stream: the list of the issue, for tools/gunzip_host_check.cpp and the tests"""
    text = fastq(1)
    c = {"fastq_l%d" % level: raw(text, level) for level in (1, 6, 9)}
    c["sync_flushed"] = sync_flushed(text[:300_000], 2)[0]
    c.update(unsplittable())
    c["false_candidates"] = false_candidates()
    c["repeated_read"] = repeated_read()
    c["window_edges"] = window_edges(3)
    return c


def write_corpus(directory):
    """the corpus and 200 single-bit flips as files <name>.deflate (sound) and flip_<bit>.deflate, for tools/gunzip_host_check.cpp"""
    import os

    os.makedirs(directory, exist_ok=True)
    for name, stream in corpus().items():
        with open(os.path.join(directory, name + ".deflate"), "wb") as f:
            f.write(stream)
    for bit, stream in bit_flips(flip_base(), 200, 4):
        with open(os.path.join(directory, "flip_%07d.deflate" % bit), "wb") as f:
            f.write(stream)


if __name__ == "__main__":
    import sys

    write_corpus(sys.argv[1])
