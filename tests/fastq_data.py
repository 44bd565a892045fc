"""FASTQ text for the tests of the device's FASTQ reader (bayestyper_amd/csrc/bt_fastq.hpp, bt_fastq.hip), and the independent side: a FASTQ parser written
from the grammar alone, no project code.

The grammar (that of the host's ReadsFile): lines end at '\\n' and one trailing '\\r' is stripped from every line.  A record is four lines: a header that
starts with '@', the bases, a line that starts with '+', and as many quality values as bases.  A blank line (empty, or a lone '\\r') is skipped only where a
record's first line is expected; anywhere else it is that line of the record.  The file's last line needs no newline.  The text is, per record with at least
one base and in record order, the bases verbatim and '\\n'."""
import numpy as np

MESSAGES = {
    "at": "line %d: a FASTQ record must start with '@' (a missing line?)",
    "plus": "line %d: the third line of a FASTQ record must start with '+' (a missing line?)",
    "lengths": "FASTQ record ending at line %d: %d bases but %d quality values (a missing line?)",
    "truncated": "truncated FASTQ record at the end of the file (%d of 4 lines)",
}


class FastqError(Exception):
    pass


def parse(data, final=True, first_line=1):
    """-> (text, consumed, {"reads", "bases", "lines"}) of the whole records of `data`, which starts at a record boundary; FastqError with the message.
    final: the data is the file's end (its last line needs no newline; an unfinished record is an error); otherwise a line counts when its newline is
    there, and the record that is not whole is only judged by such lines."""
    lines, at = [], 0   # (start, end, has_newline) per line
    while at < len(data):
        nl = data.find(b"\n", at)
        if nl < 0:
            if final:
                lines.append((at, len(data), False))
            break
        lines.append((at, nl, True))
        at = nl + 1
    text, consumed, stats = [], 0, {"reads": 0, "bases": 0, "lines": 0}
    record = []   # the stripped lines of the record under way
    for number, (start, end, has_newline) in enumerate(lines):
        line = data[start:end]
        if line.endswith(b"\r"):
            line = line[:-1]
        if not record:
            if not line and has_newline:   # a blank line between records
                consumed, stats["lines"] = end + 1, number + 1
                continue
            if not line.startswith(b"@"):
                raise FastqError(MESSAGES["at"] % (first_line + number))
        elif len(record) == 2 and not line.startswith(b"+"):
            raise FastqError(MESSAGES["plus"] % (first_line + number))
        elif len(record) == 3 and len(line) != len(record[1]):
            raise FastqError(MESSAGES["lengths"] % (first_line + number, len(record[1]), len(line)))
        record.append(line)
        if len(record) == 4:
            if record[1]:
                text.append(record[1] + b"\n")
                stats["reads"] += 1
                stats["bases"] += len(record[1])
            record = []
            consumed, stats["lines"] = min(end + 1, len(data)), number + 1
    if final and record:
        raise FastqError(MESSAGES["truncated"] % len(record))
    return b"".join(text), consumed, stats


def record_starts(data):
    """offsets at which a record of a sound file starts (behind the blank lines in front of it), and len(data)"""
    starts, at = [], 0
    while at < len(data):
        while at < len(data) and data[at:at + 1] in (b"\n", b"\r"):   # blank lines: "\n" or "\r\n"
            at += 1 if data[at:at + 1] == b"\n" else 2
        if at >= len(data):
            break
        starts.append(at)
        for _ in range(4):
            nl = data.find(b"\n", at)
            at = len(data) if nl < 0 else nl + 1
    return starts + [len(data)]


def random_seq(rng, n, alphabet=b"ACGT"):
    return np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), size=n)].tobytes()


def qualities(rng, n, kind):
    """kind 0: starts with '@'; 1: starts with '+'; 2: plain"""
    q = bytearray(rng.integers(33, 74, size=n).astype(np.uint8).tobytes())
    if q and kind < 2:
        q[0] = ord("@+"[kind])
    return bytes(q)


def record(rng, i, seq, eol=b"\n", header=None, kind=None):
    header = b"@read%d some text" % i if header is None else header
    return header + eol + seq + eol + b"+" + (b"read%d" % i if i % 3 == 0 else b"") + eol + qualities(rng, len(seq), i % 3 if kind is None else kind) + eol


LEADING = b"\n\r\n\n"   # the blank lines at the start of edge_file (ReadsFile tells a file's format by its first byte, so it takes the file without them)


def edge_file(rng, k=55, eol=None, last_newline=True):
    """Reads of 0, 1, k - 1, k, k + 1, 150 and 20 000 bases, lower case and N, line ends CRLF, LF or mixed (eol None), blank lines and lone-'\\r' lines between
    records and at the start and the end, quality lines that start with '@' and '+', that are exactly '@', and that are empty (the 0-base read), a header of
    300 bytes, the last line with or without its newline -> the file's bytes"""
    eols = (lambda i: (b"\n", b"\r\n")[i % 2]) if eol is None else (lambda i: eol)
    seqs = [random_seq(rng, n) for n in (0, 1, k - 1, k, k + 1, 150, 20000)]
    seqs += [random_seq(rng, 150, b"acgtnACGTN"), b"N" * 60, random_seq(rng, 2 * k).lower(), b"", random_seq(rng, 151)]
    seqs += [random_seq(rng, int(n)) for n in rng.integers(1, 300, size=30)]
    out = [LEADING]
    for i, s in enumerate(seqs):
        e = eols(i)
        header = b"@" + b"h" * 299 if i == 5 else None
        out.append(record(rng, i, s, e, header))
        if i % 4 == 1:
            out.append(b"\n")
        if i % 4 == 2:
            out.append(b"\r\n\n\r\n")
    out.append(b"@one" + eols(0) + b"A" + eols(1) + b"+" + eols(0) + b"@" + eols(1))   # a quality line that is exactly '@'
    out.append(b"\n\r\n")   # blank lines at the end
    data = b"".join(out)
    if not last_newline:
        last = record(rng, 999, random_seq(rng, 77), eols(1), kind=1)
        data += last[:-len(eols(1))]
    return data


def simple_records(rng, n, bases=20, eol=b"\n"):
    return [record(rng, i, random_seq(rng, bases), eol, header=b"@r%d" % i, kind=2) for i in range(n)]


MANY_RECORDS = [16384, 16385, 16500]   # 65 536, 65 540 and 66 000 lines: 256, 257 and 258 workgroups of 256 lines, the offsets scan's second round of 256 sums


def short_records(n):
    """n records of 0 to 8 bases, '\\n' and '\\r\\n' alternating: many lines in few bytes (about 30 per record) -> the file's bytes"""
    rng = np.random.default_rng(n)
    return b"".join(record(rng, i, random_seq(rng, int(b)), (b"\n", b"\r\n")[i % 2], header=b"@%d" % i) for i, b in enumerate(rng.integers(0, 9, size=n)))
