"""Shared by the tests of the deflate compressor (bt_deflate / bt_diag_deflate / bt_gzip_save): the edge-case inputs, and a VCF text of several pieces
produced by the project's own writer from fabricated sampler results."""
import functools
import os
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

P = 65536   # include/btgpu.h: the piece size


def text(rng, n):
    """VCF-like lines, n bytes"""
    out, size, pos = [], 0, 1000
    while size < n:
        pos += int(rng.integers(1, 5000))
        line = "chr%d\t%d\t.\t%s\t%s\t%.2f\tPASS\tAC=%d;AF=%.3f;AN=%d\tGT:GQ:GPP\t%d/%d:%d:%.4f,%.4f\n" % (
            rng.integers(1, 23), pos, "ACGT"[rng.integers(4)], "ACGT"[rng.integers(4)], rng.uniform(0, 99), rng.integers(7), rng.random(), 2 * rng.integers(1, 4), rng.integers(2),
            rng.integers(2), rng.integers(99), rng.random(), rng.random())
        out.append(line)
        size += len(line)
    return "".join(out).encode()[:n]


def de_bruijn(k, n):
    """the de Bruijn sequence B(k, n) (Lyndon words in order), one period: k ** n symbols, every n-gram of the cyclic sequence once"""
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    return seq


def block_at_distance(rng, dist, random_filler=True):
    """a 300-byte block of random bytes (no 4-gram of it repeats inside it, so the only candidate for the second copy is the first) twice, `dist` bytes apart, inside one piece of random filler — or of zeros: random filler passes through every entry of a
    head table of a few thousand words, so a one-candidate matcher has forgotten the first block by then; zeros all fall into one entry, and the
    candidate at `dist` is still there to be taken or dropped"""
    b = bytearray(rng.integers(0, 256, 40000, dtype=np.uint8).tobytes() if random_filler else bytes(40000))
    blk = rng.integers(0, 256, 300, dtype=np.uint8).tobytes()
    b[100:400] = blk
    b[100 + dist:400 + dist] = blk
    return bytes(b)


@functools.lru_cache(maxsize=None)
def inputs():
    """name -> bytes: the cases of tests/test_deflate_cpu.py, computed once"""
    rng = np.random.default_rng(2024)
    rnd = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()   # noqa: E731
    d = {"empty": b"", "one byte": b"x", "two bytes": b"xy", "three bytes": b"xyz"}
    for n in (P - 1, P, P + 1, 2 * P + 17):
        d["text %d" % n] = text(rng, n)
    d["70000 equal bytes"] = b"A" * 70000
    # a match of every length 3 .. 258: a fresh random block of L bytes, 64 random bytes (the positions of one matching round do not see each other, so the
    # copy must lie a round or more behind its source), the L bytes again, a random byte that ends the match
    every = bytearray()
    for L in range(3, 259):
        blk = rnd(L)
        every += blk + rnd(64) + blk + rnd(1)
    d["every match length"] = bytes(every)
    d["all byte values"] = bytes(range(256)) * 2 + bytes(range(255, -1, -1)) * 2
    d["random"] = rnd(3 * P + 1000)
    d["distance 32769"] = block_at_distance(rng, 32769)
    d["distance 32768"] = block_at_distance(rng, 32768)
    d["distance 32769, zeros between"] = block_at_distance(rng, 32769, False)
    d["distance 32768, zeros between"] = block_at_distance(rng, 32768, False)
    d["de bruijn"] = bytes(97 + s for s in de_bruijn(16, 3))
    d["text random text"] = text(rng, P) + rnd(P) + text(rng, P - 5)
    return d


@functools.lru_cache(maxsize=None)
def interleaved():
    """about 40 pieces, stored and compressed ones interleaved (several workgroups, the compaction)"""
    rng = np.random.default_rng(7)
    parts = []
    for i in range(40):
        parts.append(rng.integers(0, 256, P, dtype=np.uint8).tobytes() if i % 3 == 1 else text(rng, P))
    return b"".join(parts) + text(rng, 12345)


@functools.lru_cache(maxsize=None)
def vcf_fixture():
    """a VCF text of at least 4 pieces from bthost::GenotypeWriter over fabricated sampler results (tests/test_genotype_writer_cpu.py's way, more variants
    and samples)"""
    import test_cluster_stage_cpu as T
    from test_genotype_writer_cpu import fabricate_results

    from bayestyper_amd.host import genotypes
    from bayestyper_amd.host.cluster_stage import ClusterStage, GenotypeWriter

    k, S = 15, 8
    rng = np.random.default_rng(4242)
    genome = T.random_genome(rng, [60000, 30000], ())
    vcf = T.make_vcf(rng, genome, k, 250, True, extra_contig=False, sv_blocks=4)
    st = ClusterStage(k)
    for g in genome:
        st.add_sequence(*g)
    st.set_variants(vcf_text=vcf)
    assert st.next_unit(10 ** 9)
    units, *_ = T.parse_dump("UNIT 1\n" + st.unit_text())
    w = GenotypeWriter(st, ["sample_%d" % s for s in range(S)])
    mf = genotypes.min_fraction_observed_kmers([15.0] * S)
    for gi, g in enumerate(units[0]):
        for vi, v in enumerate(g["vertices"]):
            ploidy = np.array([2] * (S - 2) + [1 if gi % 3 == 0 else 2, 0 if gi % 5 == 0 else 2], np.uint8)
            num_alleles = [1 + len(alts) + dep for (_, _, dep, alts) in v["vars"]]
            H = int(rng.integers(2, 7))
            hap_allele, h1, h2, freq, stats = fabricate_results(rng, S, H, num_alleles, ploidy)
            w.add_cluster(gi, vi, S, H, hap_allele, h1, h2, freq, stats, ploidy, mf)
    got = w.text("ref.fa", "##graph=x\n", "##genotype=y\n").encode()
    w.close(), st.close()
    assert len(got) > 3 * P, len(got)
    return got


def order0_bytes(data):
    """the order-0 entropy size of data: sum over byte values of count * log2(n / count), in bytes"""
    c = np.bincount(np.frombuffer(data, np.uint8), minlength=256).astype(np.float64)
    c = c[c > 0]
    return float((c * np.log2(len(data) / c)).sum() / 8)


def zlib_pieces(data, level):
    """the size of zlib's raw deflate at `level` over independent pieces of P bytes, each closed with a sync flush (the last with the final block)"""
    total = 0
    for at in range(0, max(len(data), 1), P):
        z = zlib.compressobj(level, zlib.DEFLATED, -15)
        total += len(z.compress(data[at:at + P])) + len(z.flush(zlib.Z_FINISH if at + P >= len(data) else zlib.Z_SYNC_FLUSH))
    return total
