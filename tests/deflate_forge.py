"""Valid deflate streams that zlib never writes, for the tests of the device inflate (bayestyper_amd/csrc/bt_inflate.hpp, bt_gunzip.hpp): an encoder that takes
its code lengths from the caller (codes of up to 15 / 15 / 7 bits, HLIT 286, HDIST 30, any run-length coding of the header, any bit phase), a scanner that
inflates a stream bit by bit and says what it held, and the rules for a dynamic block header (`header_ok`), all written from RFC 1951 with zlib, struct,
random and numpy alone: no project code.  The yardstick for every stream handed out is zlib's own inflate (`checked`)."""
import functools
import random
import struct
import zlib

import numpy as np

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CLEN_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 30
GRID_LENGTHS = (3, 23, 24, 25, 63, 64, 65, 127, 128, 129, 257, 258)
HEADER_MESSAGES = ("invalid block type", "too many length or distance symbols", "invalid code lengths set", "invalid bit length repeat",
                   "invalid code -- missing end-of-block", "invalid literal/lengths set", "invalid distances set")


def grid_distances(length):
    return sorted({1, 2, 3, 7, 23, 24, 25, 63, 64, 65, length - 1, length, length + 1, 32768} - {0})


# ---- the encoder ---------------------------------------------------------------------------------------------------------------------------------------------
class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, value, count):   # least significant bit first; a Huffman code is handed in already reversed
        self.acc |= value << self.n
        self.n += count
        if self.n >= 8:
            k = self.n >> 3
            self.out += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def done(self):
        self.align()
        return bytes(self.out)


def canonical(lengths):
    """code lengths by symbol -> (bit-reversed code, length) by symbol, None where the length is 0 (RFC 1951 3.2.2)"""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lengths:
        if l == 0:
            out.append(None)
        else:
            out.append((int(format(nxt[l], "0%db" % l)[::-1], 2), l))
            nxt[l] += 1
    return out


def complete_lengths(rng, n, maxbits):
    """a complete multiset of n code lengths whose longest is maxbits (or n - 1, when n codes cannot reach it): the chain 1, 2, .., m, m with random leaves
    split until there are n.  One code: a single one-bit code (incomplete, and accepted for what it is)."""
    if n <= 1:
        return [1] * n
    while n > 1 << maxbits:   # (more codes than that length holds)
        maxbits += 1
    m = min(maxbits, n - 1)
    leaves = list(range(1, m + 1)) + [m]
    while len(leaves) < n:
        i = rng.choice([j for j, l in enumerate(leaves) if l < maxbits])
        leaves[i] += 1
        leaves.append(leaves[i])
    return sorted(leaves)


def assign(lengths, symbols, freq, mode, rng):
    """hand the lengths to the symbols: "deep" the longest codes to the most frequent symbols, "shallow" the reverse, "random" any
    ("matches", in dynamic_block: "shallow" with the length and distance symbols in use last of all)"""
    order = sorted(symbols, key=lambda s: (-freq.get(s, 0), s))
    ls = sorted(lengths, reverse=(mode == "deep"))
    if mode == "random":
        rng.shuffle(ls)
    return dict(zip(order, ls))


def token_symbols(tokens, alt258=False):
    """tokens (a byte, or (length, distance)) -> (literal,) and (length symbol, extra, bits, distance symbol, extra, bits); alt258: length 258 as symbol 284
    with extra bits 31, which RFC 1951 leaves valid beside symbol 285"""
    out = []
    for t in tokens:
        if not isinstance(t, tuple):
            out.append((t,))
            continue
        length, dist = t
        assert 3 <= length <= 258 and 1 <= dist <= 32768
        lc = 28 if length == 258 else max(i for i in range(28) if LEN_BASE[i] <= length)
        if length == 258 and alt258:
            lc = 27
        dc = max(i for i in range(30) if DIST_BASE[i] <= dist)
        out.append((257 + lc, length - LEN_BASE[lc], LEN_EXTRA[lc], dc, dist - DIST_BASE[dc], DIST_EXTRA[dc]))
    return out


def emit(w, syms, lit, dist):
    for s in syms:
        w.bits(*lit[s[0]])
        if len(s) > 1:
            w.bits(s[1], s[2])
            w.bits(*dist[s[3]])
            w.bits(s[4], s[5])
    w.bits(*lit[256])


def rle_lengths(seq, rng, style, force=None):
    """the code lengths as symbols of the code-length code -> [(symbol, extra value, extra bits)].  style: "plain" (no repeat codes), "greedy" (the longest
    run every time) or "random" (16, 17, 18 or plain by chance, with a random run length); force: {position: (symbol, run)} taken as given.  Runs cross
    from the literal/length lengths into the distance lengths wherever the values allow it: seq is one list."""
    force = force or {}
    out, i, n = [], 0, len(seq)
    while i < n:
        stop = min([f for f in force if f > i] + [n])
        if i in force:
            sym, rep = force[i]
        else:
            v, run = seq[i], 1
            while i + run < stop and seq[i + run] == v:
                run += 1
            choices = [(v, 1)]
            if i > 0 and seq[i - 1] == v and run >= 3:
                choices.append((16, min(run, 6) if style == "greedy" else rng.randint(3, min(run, 6))))
            if v == 0 and run >= 3:
                choices.append((17, min(run, 10) if style == "greedy" else rng.randint(3, min(run, 10))))
            if v == 0 and run >= 11:
                choices.append((18, min(run, 138) if style == "greedy" else rng.randint(11, min(run, 138))))
            sym, rep = choices[0] if style == "plain" else choices[-1] if style == "greedy" else rng.choice(choices)
        if sym == 16:
            assert i > 0 and all(x == seq[i - 1] for x in seq[i:i + rep]) and 3 <= rep <= 6
            out.append((16, rep - 3, 2))
        elif sym == 17:
            assert not any(seq[i:i + rep]) and 3 <= rep <= 10
            out.append((17, rep - 3, 3))
        elif sym == 18:
            assert not any(seq[i:i + rep]) and 11 <= rep <= 138
            out.append((18, rep - 11, 7))
        else:
            out.append((sym, 0, 0))
        assert i + rep <= n
        i += rep
    return out


def dynamic_block(w, tokens, final, rng, lit_bits=15, dist_bits=15, clen_bits=7, full=False, mode="deep", rle="random", cross16=False, alt258=False,
                  clen_full=False):
    """one dynamic block (RFC 1951 3.2.7) at the writer's bit position.  The code lengths are chosen, not computed from frequencies: complete sets that reach
    lit_bits / dist_bits / clen_bits where there are symbols enough.  full: every one of the 286 and 30 symbols gets a code (HLIT 286, HDIST 30); clen_full:
    every one of the 19; cross16: a repeat code 16 is made to run from the last literal/length lengths into the first distance lengths (full only)."""
    syms = token_symbols(tokens, alt258)
    lfreq, dfreq = {256: 1}, {}
    for s in syms:
        lfreq[s[0]] = lfreq.get(s[0], 0) + 1
        if len(s) > 1:
            dfreq[s[3]] = dfreq.get(s[3], 0) + 1
    lsyms, dsyms = (range(286), range(30)) if full else (sorted(lfreq), sorted(dfreq))
    if mode == "matches":   # the symbols of the matches get the longest codes, behind the symbols that are not used at all
        lfreq, dfreq, mode = {s: -1 if s > 256 else f for s, f in lfreq.items()}, {s: -1 for s in dfreq}, "shallow"
    lit_len, dist_len = [0] * 286, [0] * 30
    for s, l in assign(complete_lengths(rng, len(lsyms), lit_bits), lsyms, lfreq, mode, rng).items():
        lit_len[s] = l
    for s, l in assign(complete_lengths(rng, len(dsyms), dist_bits), dsyms, dfreq, mode, rng).items():
        dist_len[s] = l
    hlit, hdist = max(max(lsyms) + 1, 257), max(list(dsyms) + [0]) + 1
    force = None
    if cross16:
        assert full
        both = [l for l in range(1, 16) if lit_len.count(l) >= 2 and dist_len.count(l) >= 2]
        l = max(both)
        for lens, places in ((lit_len, (284, 285)), (dist_len, (0, 1))):
            for p in places:
                q = next(j for j in range(len(lens)) if lens[j] == l and j not in places) if lens[p] != l else p
                lens[p], lens[q] = lens[q], lens[p]
        force = {hlit - 1: (16, 3)}
    seq = lit_len[:hlit] + dist_len[:hdist]
    items = rle_lengths(seq, rng, rle, force)
    cfreq = {}
    for s, _, _ in items:
        cfreq[s] = cfreq.get(s, 0) + 1
    csyms = list(range(19)) if clen_full else sorted(cfreq)
    for extra in (0, 18):   # the code-length code has to be complete: at least two codes
        if len(csyms) < 2 and extra not in csyms:
            csyms.append(extra)
    clen_len = [0] * 19
    for s, l in assign(complete_lengths(rng, len(csyms), clen_bits), csyms, cfreq, mode, rng).items():
        clen_len[s] = l
    hclen = max(4, max(i + 1 for i in range(19) if clen_len[CLEN_ORDER[i]]))
    w.bits((1 if final else 0) | 4, 3)
    w.bits(hlit - 257, 5)
    w.bits(hdist - 1, 5)
    w.bits(hclen - 4, 4)
    for i in range(hclen):
        w.bits(clen_len[CLEN_ORDER[i]], 3)
    ccode = canonical(clen_len)
    for s, v, nb in items:
        w.bits(*ccode[s])
        w.bits(v, nb)
    emit(w, syms, canonical(lit_len), canonical(dist_len))


def fixed_block(w, tokens, final):
    w.bits((1 if final else 0) | 2, 3)
    emit(w, token_symbols(tokens), canonical(FIXED_LIT), canonical(FIXED_DIST))


def stored_block(w, data, final):
    assert len(data) <= 65535
    w.bits(1 if final else 0, 3)
    w.align()
    w.bits(len(data), 16)
    w.bits(len(data) ^ 0xFFFF, 16)
    assert w.n == 0
    w.out += data


def build(blocks, seed):
    """[("stored", bytes) | ("fixed", tokens) | ("dynamic", tokens, options)] -> a raw deflate stream; the last block is the final one"""
    rng, w = random.Random(seed), BitWriter()
    for i, b in enumerate(blocks):
        final = i + 1 == len(blocks)
        if b[0] == "stored":
            stored_block(w, b[1], final)
        elif b[0] == "fixed":
            fixed_block(w, b[1], final)
        else:
            dynamic_block(w, b[1], final, rng, **(b[2] if len(b) > 2 else {}))
    return w.done()


def expand(blocks):
    """what the blocks decode to"""
    out = bytearray()
    for b in blocks:
        if b[0] == "stored":
            out += b[1]
            continue
        for t in b[1]:
            if isinstance(t, tuple):
                for _ in range(t[0]):
                    out.append(out[-t[1]])
            else:
                out.append(t)
    return bytes(out)


def checked(stream, data):
    """every stream handed out has been inflated by zlib: it returns the data, reaches the stream's end and leaves nothing over"""
    d = zlib.decompressobj(-15)
    got = d.decompress(stream)
    assert got == data and d.eof and not d.unused_data, "the forge wrote a stream zlib does not take"
    return stream


def forged(blocks, seed):
    """blocks -> (stream, data), checked"""
    data = expand(blocks)
    return checked(build(blocks, seed), data), data


def match_tokens(data, rng, take=0.6, far=0.0):
    """a small hash matcher: at a position whose three bytes were seen before, the match is taken with probability `take` and cut to a random length, which
    spreads (length, distance) pairs far wider than a compressor's choices; far: the probability of trying distance 32768 first"""
    toks, table, i, n = [], {}, 0, len(data)
    while i < n:
        key, cand = data[i:i + 3], None
        if len(key) == 3:
            if far and i >= 32768 and data[i - 32768:i - 32765] == key and rng.random() < far:
                cand = i - 32768
            else:
                c = table.get(key)
                if c is not None and i - c <= 32768 and rng.random() < take:
                    cand = c
        if cand is None:
            toks.append(data[i])
            table[key] = i
            i += 1
            continue
        length, most = 3, min(258, n - i)
        while length < most and data[cand + length] == data[i + length]:
            length += 1
        length = rng.randint(3, length)
        toks.append((length, i - cand))
        for j in range(i, i + length):
            table[data[j:j + 3]] = j
        i += length
    return toks


def split(tokens, pieces):
    edges = [len(tokens) * i // pieces for i in range(pieces + 1)]
    return [tokens[a:b] for a, b in zip(edges[:-1], edges[1:])]


# ---- the scanner ---------------------------------------------------------------------------------------------------------------------------------------------
class PastEnd(Exception):
    pass


class BitReader:
    def __init__(self, stream, pos=0):
        self.s, self.pos, self.end = stream, pos, 8 * len(stream)

    def peek(self, n):   # the next n bits, zeros behind the end
        p = self.pos
        return (int.from_bytes(self.s[p >> 3:(p >> 3) + 4], "little") >> (p & 7)) & ((1 << n) - 1)

    def bits(self, n):
        if self.pos + n > self.end:
            raise PastEnd
        v = self.peek(n)
        self.pos += n
        return v


def decode_table(lengths):
    """lengths by symbol -> (list over the next `longest` bits of symbol << 4 | length, 0 where there is no code; longest)"""
    longest = max(lengths + [0])
    if not longest:
        return [0], 0
    table = np.zeros(1 << longest, np.int32)
    for s, c in enumerate(canonical(lengths)):
        if c:
            table[c[0]::1 << c[1]] = s << 4 | c[1]
    return table.tolist(), longest


def scan(stream, start_bit=0):
    """a bit-by-bit inflate -> (data, blocks, end bit).  Per block a dict: type, start (bit), out (output length at its start); for a dynamic block hlit, hdist,
    hclen, body (the bit behind the header), the longest code of the three sets (lit_max, dist_max, clen_max), the number of codes of the two sets, lit_used / dist_used / clen_used (decoded
    symbols by code length), runs (the (repeat symbol, run length) pairs of the header), cross (repeat symbols whose run went from the literal/length lengths
    into the distance lengths), alt258 (length symbol 284 with extra bits 31); for every compressed block pairs, the (length, distance) list"""
    r, out, blocks = BitReader(stream, start_bit), bytearray(), []

    def symbol(table, longest, used=None):
        e = table[r.peek(longest)]
        if not e:
            raise ValueError("no code")
        if r.pos + (e & 15) > r.end:
            raise PastEnd
        r.pos += e & 15
        if used is not None:
            used[e & 15] = used.get(e & 15, 0) + 1
        return e >> 4

    while True:
        blk = {"start": r.pos, "out": len(out)}
        blocks.append(blk)
        last, kind = r.bits(1), r.bits(2)
        blk["type"] = kind
        if kind == 3:
            raise ValueError("block type 3")
        if kind == 0:
            r.pos = (r.pos + 7) & ~7
            n = r.bits(16)
            if r.bits(16) != n ^ 0xFFFF:
                raise ValueError("stored length check")
            if r.pos + 8 * n > r.end:
                raise PastEnd
            out += stream[r.pos >> 3:(r.pos >> 3) + n]
            r.pos += 8 * n
            blk["stored"] = n
        else:
            if kind == 1:
                lit_len, dist_len = list(FIXED_LIT), list(FIXED_DIST)
            else:
                hlit, hdist, hclen = r.bits(5) + 257, r.bits(5) + 1, r.bits(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[CLEN_ORDER[i]] = r.bits(3)
                ctab, cmax = decode_table(cl)
                lens, runs, cross, cused = [], set(), set(), {}
                while len(lens) < hlit + hdist:
                    s = symbol(ctab, cmax, cused)
                    if s < 16:
                        lens.append(s)
                        continue
                    rep = 3 + r.bits(2) if s == 16 else 3 + r.bits(3) if s == 17 else 11 + r.bits(7)
                    runs.add((s, rep))
                    if len(lens) < hlit < len(lens) + rep:
                        cross.add(s)
                    lens += [lens[-1] if s == 16 else 0] * rep
                assert len(lens) == hlit + hdist
                lit_len, dist_len = lens[:hlit], lens[hlit:]
                blk.update(body=r.pos, hlit=hlit, hdist=hdist, hclen=hclen, clen_max=cmax, clen_used=cused, runs=runs, cross=cross, lit_max=max(lit_len), dist_max=max(dist_len),
                           lit_codes=sum(1 for l in lit_len if l), dist_codes=sum(1 for l in dist_len if l))
            ltab, lmax = decode_table(lit_len)
            dtab, dmax = decode_table(dist_len)
            lused, dused, pairs, alt = {}, {}, [], 0
            while True:
                s = symbol(ltab, lmax, lused)
                if s < 256:
                    out.append(s)
                elif s == 256:
                    break
                else:
                    extra = r.bits(LEN_EXTRA[s - 257])
                    length = LEN_BASE[s - 257] + extra
                    alt += s == 284 and extra == 31
                    d = symbol(dtab, dmax, dused)
                    dist = DIST_BASE[d] + r.bits(DIST_EXTRA[d])
                    if dist > len(out):
                        raise ValueError("distance too far back")
                    pairs.append((length, dist))
                    for _ in range(length):
                        out.append(out[-dist])
            blk.update(lit_used=lused, dist_used=dused, pairs=pairs, alt258=alt)
        if last:
            return bytes(out), blocks, r.pos


# ---- the rules for a dynamic block's header --------------------------------------------------------------------------------------------------------------------
def kraft(lengths, unit):
    return sum(unit >> l for l in lengths if l)


def header_ok(stream, at, any_final=False):
    """Does a sound non-final dynamic block header that lies wholly inside the stream start at bit `at`? -> (yes or no, refused because it ran past the end).
    RFC 1951 3.2.7 and zlib's rule for incomplete sets: HLIT at most 286 and HDIST at most 30; the code-length code complete; no repeat of a length before
    the first, none past the last; symbol 256 coded; the literal/length set and the distance set not over-subscribed, and complete unless the set is a single
    one-bit code or, for distances, empty.  any_final: BFINAL is not looked at."""
    r = BitReader(stream, at)
    try:
        final, kind = r.bits(1), r.bits(2)
        if kind != 2 or (final and not any_final):
            return False, False
        hlit, hdist, hclen = r.bits(5) + 257, r.bits(5) + 1, r.bits(4) + 4
        if hlit > 286 or hdist > 30:
            return False, False
        cl = [0] * 19
        for i in range(hclen):
            cl[CLEN_ORDER[i]] = r.bits(3)
        if kraft(cl, 128) != 128:
            return False, False
        codes = {(c[1], c[0]): s for s, c in enumerate(canonical(cl)) if c}
        lens = []
        while len(lens) < hlit + hdist:
            code, n = 0, 0
            while (n, code) not in codes:   # a complete code: some prefix of any seven bits is a code
                code |= r.bits(1) << n
                n += 1
            s = codes[(n, code)]
            if s < 16:
                lens.append(s)
                continue
            rep = 3 + r.bits(2) if s == 16 else 3 + r.bits(3) if s == 17 else 11 + r.bits(7)
            if s == 16 and not lens:
                return False, False
            if rep > hlit + hdist - len(lens):
                return False, False
            lens += [lens[-1] if s == 16 else 0] * rep
    except PastEnd:
        return False, True
    lit, dist = lens[:hlit], lens[hlit:]
    if not lit[256]:
        return False, False
    for lengths, may_be_empty in ((lit, False), (dist, True)):
        k, coded = kraft(lengths, 32768), [l for l in lengths if l]
        if k > 32768:
            return False, False
        if k < 32768 and not (coded == [1] or (may_be_empty and not coded)):
            return False, False
    return True, False


def header_ok_all(stream):
    """header_ok at every bit offset of the stream -> uint8 array.  The first three rules (BFINAL, BTYPE, HLIT, HDIST) are applied to all offsets at once."""
    n = 8 * len(stream)
    bits = np.unpackbits(np.frombuffer(stream + bytes(2), np.uint8), bitorder="little").astype(np.uint32)
    field = lambda first, count: sum(bits[first + i:first + i + n] << i for i in range(count))
    maybe = (field(0, 3) == 4) & (field(3, 5) <= 29) & (field(8, 5) <= 29)
    flags = np.zeros(n, np.uint8)
    for at in np.flatnonzero(maybe):
        flags[at] = header_ok(stream, int(at))[0]
    return flags


# ---- what zlib says to a stream --------------------------------------------------------------------------------------------------------------------------------
def zlib_outcome(stream):
    """-> (class, bytes): "end" (the stream's end reached, nothing left over), "trailing" (reached, input left over), "short" (the input ends first), or
    zlib's message"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(stream)
    except zlib.error as e:
        return str(e).split(": ", 1)[-1], None
    return ("short" if not d.eof else "trailing" if d.unused_data else "end"), out


def flips(stream, first=0, count=None):
    """(bit, the stream with that bit flipped) for every bit from `first` on"""
    for bit in range(first, 8 * len(stream) if count is None else min(first + count, 8 * len(stream))):
        b = bytearray(stream)
        b[bit >> 3] ^= 1 << (bit & 7)
        yield bit, bytes(b)


# ---- the corpus ------------------------------------------------------------------------------------------------------------------------------------------------
def content(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
    if kind == "periodic":
        return (b"GATTACA" * (n // 7 + 1))[:n]
    if kind == "zeros":
        return bytes(n)
    lines = [np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=150)].tobytes() for _ in range(n // 151 + 1)]
    if kind == "reads":
        return b"\n".join(lines)[:n]
    quals = [np.frombuffer(b"#,5:AFGI", np.uint8)[rng.integers(0, 8, size=150)].tobytes() for _ in lines]
    return b"".join(b"@run7.%d length=150\n%s\n+\n%s\n" % (i, s, q) for i, (s, q) in enumerate(zip(lines, quals)))[:n]   # "records"


KINDS = ("random", "reads", "periodic", "zeros", "records")
DEEP = dict(lit_bits=15, dist_bits=15, clen_bits=7, full=True, clen_full=True, mode="deep")
SHALLOW = dict(DEEP, mode="shallow")


def grid_cell(length, dist, seed):
    """the tokens of one cell: distinct literals (stored one by one, by the team's first lane), the match under test, a 3-byte match at distance 2 that reads the
    tail of what the match wrote, a literal"""
    rng = np.random.default_rng(seed)
    run = min(dist, 300) + int(rng.integers(2, 9))
    return list(rng.integers(0, 256, size=run, dtype=np.uint8).tobytes()) + [(length, dist), (3, 2), 0x5A]


def grid_members(kind):
    """every cell of the match grid as a block of its own: in fixed blocks (kind "fixed") or in dynamic blocks with codes of 15 bits, where the symbols of the
    matches, used once, get the longest codes (kind "dynamic").  A cell at distance 32768 stands behind a stored block that gives it the output to reach."""
    out = []
    for length in GRID_LENGTHS:
        for dist in grid_distances(length):
            seed = 1000 * length + dist % 1000
            cell = grid_cell(length, dist, seed)
            lead = dist - (len(cell) - 3) if dist > 300 else 0
            blocks = [("stored", content("random", lead, seed))] if lead else []
            blocks.append(("fixed", cell) if kind == "fixed" else ("dynamic", cell, dict(SHALLOW, mode="matches", rle="random")))
            out.append(("grid_%s_%d_%d" % (kind, length, dist),) + forged(blocks, seed) + ({"grid"},))
    return out


def small_members():
    """the members of under 250 bytes of payload, each with something of its own: what the single-bit flips are made in"""
    text = b"GATTACA,CATTAG;TAGGAT.ACTGA!" * 3
    toks = match_tokens(text, random.Random(5), 0.8)
    long = match_tokens(content("records", 420, 3), random.Random(6), 0.7)
    out = [
        ("small_deep", [("dynamic", toks[:24], dict(DEEP, rle="random"))]),                                               # HLIT 286, HDIST 30, 15 / 15 / 7 bits
        ("small_fixed", [("fixed", long[:210])]),
        ("small_mixed", [("stored", b"ACGT"), ("dynamic", toks[:30], dict(mode="shallow", rle="greedy")), ("stored", b""), ("fixed", toks[30:]),
                         ("dynamic", toks + toks[:25], dict(mode="random", rle="random"))]),
        ("small_one_distance", [("dynamic", [120] + [(3, 1)] * 20 + [(n, 1) for n in range(4, 240, 13)] + [(258, 1), 121], dict(rle="plain", clen_bits=3))]),   # distance 1 alone
        ("small_empty_block", [("dynamic", [], dict(rle="greedy")), ("fixed", list(b"after an empty block")), ("dynamic", long[:64], dict(mode="deep"))]),
        ("small_literals_only", [("dynamic", list(b"no distance code: literals only, 0123456789 " * 3), dict(mode="random", rle="random"))]),
        ("small_runs", [("dynamic", [0, 11, 150, 11, 0, 150] * 12, dict(rle="greedy", mode="shallow", clen_full=True)),   # a 17 run of 10, an 18 run of 138
                        ("dynamic", long[:110], dict(mode="shallow", rle="plain"))]),
        ("small_alt258", [("dynamic", list(b"ab") + [(258, 2), (258, 1), 99] + toks + toks[:40], dict(alt258=True, mode="deep"))]),
    ]
    out = [(name,) + forged(blocks, 40 + i) + ({"small"},) for i, (name, blocks) in enumerate(out)]
    assert all(len(m[1]) < 250 for m in out), [(m[0], len(m[1])) for m in out]
    return out


LAYOUT = {1: "d", 4: "dfed", 16: "ddfdddseddfddsed"}   # d dynamic, f fixed, s stored, e an empty stored block


def mixed_blocks(data, rng, pieces, options):
    """the data's tokens in exactly `pieces` deflate blocks, by LAYOUT"""
    layout = LAYOUT[pieces]
    parts, blocks, at = split(match_tokens(data, rng, 0.6), len(layout) - layout.count("e")), [], 0
    for i, kind in enumerate(layout):
        if kind == "e":
            blocks.append(("stored", b""))
            continue
        p = parts.pop(0)
        n = sum(t[0] if isinstance(t, tuple) else 1 for t in p)
        if kind == "s":   # the tokens' bytes as they are
            blocks.append(("stored", data[at:at + n]))
        elif kind == "f":
            blocks.append(("fixed", p))
        else:
            blocks.append(("dynamic", p, dict(options[i % len(options)], rle=("random", "greedy", "plain")[i % 3])))
        at += n
    return blocks


def header_streams(final=False):
    """four small streams that begin with a forged dynamic block whose header is long: non-final and followed by a fixed block, or (final) that block alone"""
    toks = match_tokens(content("records", 300, 9), random.Random(9), 0.7)
    out = []
    for i, options in enumerate((dict(DEEP, rle="random"), dict(SHALLOW, cross16=True, rle="greedy"), dict(mode="deep", rle="random"), dict(DEEP, rle="plain", clen_bits=4))):
        out.append(forged([("dynamic", toks, options)] + ([] if final else [("fixed", list(b"the block behind"))]), 90 + i)[0])
    return out


def kind_members():
    """five kinds of content under deep and shallow codes of 15, 15 and 7 bits with HLIT 286 and HDIST 30, in one, four and sixteen deflate blocks"""
    out = []
    for k, kind in enumerate(KINDS):
        for pieces, size in ((1, 6000), (4, 14000), (16, 36000)):
            for name, options in (("deep", [DEEP]), ("shallow", [SHALLOW]), ("mix", [DEEP, dict(SHALLOW, cross16=True), dict(mode="random"), dict(DEEP, full=False)])):
                if (pieces == 16) != (name == "mix"):
                    continue
                size_here = size // 2 if kind == "random" and name == "deep" else size
                seed = 100 * k + pieces + len(name)
                data = content(kind, size_here, seed)
                out.append(("%s_%s_%d" % (kind, name, pieces),) + forged(mixed_blocks(data, random.Random(seed), pieces, options), seed) + (set(),))
    return out


def long_blocks(data, rng, pieces, far=0.0):
    """the data's tokens in `pieces` dynamic blocks under deep and shallow codes in turn"""
    options = [DEEP, SHALLOW, dict(SHALLOW, cross16=True), dict(mode="deep"), dict(DEEP, clen_bits=5)]
    parts = split(match_tokens(data, rng, 0.6, far=far), pieces)
    return [("dynamic", p, dict(options[j % len(options)], rle=("random", "greedy")[j % 2])) for j, p in enumerate(parts)]


def bgzf_file(data, cuts, seed, eof=True):
    """data cut at the content offsets `cuts` into forged BGZF members of four deflate blocks each, the EOF block behind them -> (file, the members' offsets)"""
    edges, out, offsets = [0] + list(cuts) + [len(data)], b"", []
    for i, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        payload, piece = forged(mixed_blocks(data[a:b], random.Random(seed + i), 4, [DEEP, SHALLOW, dict(mode="random")]), seed + i)
        offsets.append(len(out))
        out += bgzf_member(payload, piece)
    if eof:
        offsets.append(len(out))
        out += bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    return out, offsets


def raw_streams():
    """name -> (stream, data): long streams of twenty-four and more non-final dynamic blocks under deep and shallow codes, whose second 32 KiB repeats the
    first with changes, so that matches at distance 32768 cross the blocks (and, in the parallel gunzip, the teams)"""
    out = {}
    for i, kind in enumerate(("records", "reads", "random")):
        rng, n = random.Random(70 + i), (44000, 50000, 40000)[i]
        first = bytearray(content(kind, 32768, 70 + i))
        again = bytearray(first[:n - 32768])
        for _ in range(len(again) // 40):
            again[rng.randrange(len(again))] = rng.randrange(256)
        data = bytes(first + again)
        blocks = long_blocks(data, rng, 28, far=0.7)
        if i == 1:
            blocks[9:9] = [("stored", b"")]
            blocks[17] = ("fixed", blocks[17][1])
        out["raw_" + kind] = forged(blocks, 70 + i)
    return out


@functools.lru_cache(maxsize=None)
def corpus():
    """{"members": [(name, raw deflate payload, data, tags)], "raw": {name: (stream, data)}} — built once per process and never changed.  Tags: "grid" a cell
    of the match grid, "small" a member the flips are made in."""
    members = small_members() + kind_members() + grid_members("fixed") + grid_members("dynamic")
    return {"members": members, "raw": raw_streams()}


def bgzf_member(payload, data, crc=None):
    """one BGZF block (SAM specification 4.1) around a raw deflate payload of `data`"""
    assert 18 + len(payload) + 8 <= 65536 and len(data) <= 65536, "the member does not fit a BGZF block"
    head = struct.pack("<4BI2BH2BHH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, 6, ord("B"), ord("C"), 2, 18 + len(payload) + 8 - 1)
    return head + payload + struct.pack("<II", zlib.crc32(data) if crc is None else crc, len(data))


def small_flips():
    """[(name, payload, data, [(bit, flipped payload)])]: every single-bit flip of the small members' payloads"""
    return [(name, payload, data, list(flips(payload))) for name, payload, data, tags in corpus()["members"] if "small" in tags]


def write_corpus(directory):
    """The sound corpus and its flips as files, for tools/bam_host_check.cpp (<name>.bgzf: a member; flips_<name>.bgzf: every single-bit flip of a small
    member's payload, framed with the sound data's CRC-32 and ISIZE, one BGZF block after the other) and tools/gunzip_host_check.cpp (<name>.deflate: the raw
    streams and the members' payloads; flip_<name>_<bit>.deflate)."""
    import os

    os.makedirs(directory, exist_ok=True)

    def write(name, content):
        with open(os.path.join(directory, name), "wb") as f:
            f.write(content)

    c = corpus()
    for name, payload, data, _ in c["members"]:
        write(name + ".bgzf", bgzf_member(payload, data))
        write(name + ".deflate", payload)
    for name, (stream, _) in c["raw"].items():
        write(name + ".deflate", stream)
    for name, _, data, flipped in small_flips():
        write("flips_%s.bgzf" % name, b"".join(bgzf_member(p, data) for _, p in flipped))
        for bit, p in flipped:
            write("flip_%s_%05d.deflate" % (name, bit), p)


if __name__ == "__main__":
    import sys

    write_corpus(sys.argv[1])
