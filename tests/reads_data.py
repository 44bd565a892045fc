"""Shared inputs and restatements of the reads-scan tests (test_reads_cpu.py, test_reads_gpu.py): reads texts with the edge reads the window code can get
wrong, a brute-force list of a text's canonical k-mers, and the sketch's register rule in numpy."""
import numpy as np

_COMP = bytes.maketrans(b"ACGT", b"TGCA")
TILE = 256 * 60   # start positions of one workgroup tile of the reads kernels (bt_reads.hip: LANES x RUN)
RUN = 60          # consecutive positions one lane walks


def revcomp(s):
    return s.translate(_COMP)[::-1]


def random_seq(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n)].tobytes()


def random_reads_text(rng, n, length):
    """n random reads of one length, a newline after each"""
    a = np.full((n, length + 1), ord("\n"), np.uint8)
    a[:, :length] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=(n, length))]
    return a.tobytes()


def edge_reads(rng, k):
    """reads of length k-1, k, k+1 and 150; N at the first base, at the last base and at every k-th base; lower and mixed case; a k-mer equal to its own reverse
    complement (even k only: none exists for odd k); an empty line"""
    reads = [random_seq(rng, k - 1), random_seq(rng, k), random_seq(rng, k + 1), random_seq(rng, 150)]
    r = random_seq(rng, 150)
    reads += [b"N" + r[1:], r[:-1] + b"N"]
    e = bytearray(random_seq(rng, 150))
    e[k - 1::k] = b"N" * len(e[k - 1::k])
    reads.append(bytes(e))
    e = bytearray(random_seq(rng, 3 * k + 7))   # N at every (k+1)-th base: a window fits between two of them
    e[k::k + 1] = b"N" * len(e[k::k + 1])
    reads.append(bytes(e))
    reads.append(random_seq(rng, 150).lower())
    m = bytearray(random_seq(rng, 150))
    m[::3] = bytes(m[::3]).lower()
    reads.append(bytes(m))
    if k % 2 == 0:
        h = random_seq(rng, k // 2)
        reads.append(random_seq(rng, 20) + h + revcomp(h) + random_seq(rng, 20))
    reads.append(b"")
    return reads


def reads_text(reads, final_newline=True):
    return b"\n".join(reads) + (b"\n" if final_newline else b"")


def brute_force_kmers(text, k):
    """per window: alphabet check, reverse complement, minimum -> (list of canonical ASCII k-mers, list of the index of each window's last byte), in text order"""
    out, ends = [], []
    for i in range(len(text) - k + 1):
        w = text[i:i + k]
        if all(c in b"ACGTacgt" for c in w):
            u = w.upper()
            out.append(min(u, revcomp(u)))
            ends.append(i + k - 1)
    return out, ends


def oracle_kmers(orc, text, k):
    """the oracle's sliding window over the whole text -> (packed canonical k-mers (n, 2) of the valid windows in text order, index of each one's last byte)"""
    if len(text) < k:
        return np.zeros((0, 2), np.uint64), np.zeros(0, np.uint64)
    km, valid = orc.kmers_from_sequence(bytes(text), k)
    idx = np.flatnonzero(valid)
    return km[idx], idx.astype(np.uint64)


def kmer_multiset(packed):
    """packed (n, 2) -> (distinct k-mers sorted by (hi, lo), occurrences of each)"""
    if len(packed) == 0:
        return np.zeros((0, 2), np.uint64), np.zeros(0, np.int64)
    u, c = np.unique(packed[:, ::-1], axis=0, return_counts=True)
    return np.ascontiguousarray(u[:, ::-1]), c


def splitmix64_finalise(h):
    z = np.asarray(h, np.uint64).copy()
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def sketch_registers(hashes):
    """the sketch of bt_reads_sketch from the k-mers' ntHash words: register = top 16 bits of the finalised hash, rank = 1 + leading zeros of the other 48 bits"""
    x = splitmix64_finalise(hashes)
    reg = (x >> np.uint64(48)).astype(np.int64)
    rest = (x & np.uint64((1 << 48) - 1)).astype(np.float64)   # below 2^53: exact
    bit_length = np.frexp(rest)[1]                             # 0 for 0
    rank = (49 - bit_length).astype(np.uint8)
    out = np.zeros(1 << 16, np.uint8)
    np.maximum.at(out, reg, rank)
    return out
