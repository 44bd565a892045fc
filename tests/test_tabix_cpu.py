"""The tabix index builder (bayestyper_amd/host/TabixIndex.cpp) without a GPU: a synthetic VCF text over two used contigs and an empty one between them,
written as BGZF by bt_diag_bgzf, its line table indexed, and the index read by tests/_bgzf.py — a parser and a region query written from the
specification.  Structure: every record's start lies inside a chunk of its own bin, a bin's chunks are sorted and disjoint, every chunk boundary is a line
start.  Queries: for each region, the lines found through the index are exactly those a scan of the whole text finds."""
import functools

import numpy as np

import _bgzf as B
from bayestyper_amd import lib
from bayestyper_amd.host import tabix

CONTIGS = ["chrA", "chrEmpty", "chrB"]
HEADER = b"##fileformat=VCFv4.2\n##contig=<ID=chrA>\n##contig=<ID=chrEmpty>\n##contig=<ID=chrB>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"


def _line(contig, pos, ref_len, rng, filler=0):
    ref = "".join("ACGT"[i] for i in rng.integers(0, 4, ref_len))
    return ("%s\t%d\t.\t%s\t%s\t99\tPASS\tAC=1;X=%s\n" % (contig, pos, ref, "ACGT"[rng.integers(4)], "x" * filler)).encode()


@functools.lru_cache(maxsize=None)
def fixture():
    """(text, rows of the line table, BGZF stream, block offsets, parsed index)"""
    rng = np.random.default_rng(31)
    records = {int(p): int(rng.integers(1, 4)) if rng.random() < 0.2 else 1 for p in rng.integers(1, 400_000, 3500)}
    records.update({16_380: 10, 16_384: 2,        # across a 16 kb window boundary, which is a boundary of the smallest bins too
                    32_768: 1, 32_769: 1, 49_150: 5,
                    121_072: 20_000,             # a 20 kb REF across 131072, a boundary of the second-smallest bins
                    262_140: 9, 393_216: 1})
    a = sorted(records.items())
    b = sorted({int(p): 1 for p in rng.integers(1, 120_000, 1200)}.items()) + [(300_000_000, 3), ((1 << 29) - 3, 2)]   # the last one ends at 2^29 - 2
    text, rows = bytearray(HEADER), []
    exact_end_done = False
    for ci, recs in ((0, a), (2, b)):
        for pos, ref_len in recs:
            line = _line(CONTIGS[ci], pos, ref_len, rng)
            if not exact_end_done and len(text) + len(line) > B.BLOCK - 200:   # this record ends exactly where the first block ends
                line = _line(CONTIGS[ci], pos, ref_len, rng, B.BLOCK - len(text) - len(line))
                assert len(text) + len(line) == B.BLOCK
                exact_end_done = True
            rows.append((ci, pos, ref_len, len(text), len(line)))
            text += line
    text = bytes(text)
    assert exact_end_done and len(text) > 2 * B.BLOCK
    stream, offsets, _ = lib.diag_bgzf(text)
    raw, warning = tabix.tabix_index(CONTIGS, offsets, rows)
    assert warning is None
    return text, rows, stream, offsets, B.parse_tbi(raw)


def _voff(offsets, u):
    return offsets[u // B.BLOCK] << 16 | u % B.BLOCK


def test_header():
    tbi = fixture()[4]
    assert tbi["names"] == CONTIGS and (tbi["format"], tbi["col_seq"], tbi["col_beg"], tbi["col_end"], tbi["meta"], tbi["skip"]) == (2, 1, 2, 0, ord("#"), 0)
    assert tbi["n_no_coor"] == 0
    assert tbi["refs"][1] == dict(bins={}, linear=[])   # the empty contig
    assert all(37450 not in r["bins"] for r in tbi["refs"])   # no pseudo-bin


def test_reg2bin_matches_the_specification():
    rng = np.random.default_rng(5)
    cases = [(0, 1), (16383, 16385), (16384, 16385), (131071, 131073), (0, 1 << 29), ((1 << 29) - 1, 1 << 29), (121071, 141071)]
    for _ in range(300):
        beg = int(rng.integers(0, (1 << 29) - 1))
        cases.append((beg, min(1 << 29, beg + int(rng.integers(1, 1 << int(rng.integers(1, 29)))))))
    for beg, end in cases:
        assert tabix.reg2bin(beg, end) == B.reg2bin(beg, end) and B.reg2bin(beg, end) in B.reg2bins(beg, end)
    assert B.reg2bin(16383, 16385) == 585 and B.reg2bin(16384, 16385) == 4682 and B.reg2bin(121071, 141071) == 73


def test_structure():
    text, rows, stream, offsets, tbi = fixture()
    starts = {_voff(offsets, r[3]) for r in rows} | {_voff(offsets, len(text))}
    assert _voff(offsets, B.BLOCK) == offsets[1] << 16 and offsets[1] << 16 in starts   # the record that ends at the block's end: the next block's start
    for ci, ref in enumerate(tbi["refs"]):
        for chunks in ref["bins"].values():
            assert chunks and all(beg < end for beg, end in chunks)
            assert all(x[1] <= y[0] for x, y in zip(chunks, chunks[1:]))   # sorted and disjoint
            assert all(beg in starts and end in starts for beg, end in chunks)
        mine = [r for r in rows if r[0] == ci]
        assert (len(ref["linear"]) == 0) == (len(mine) == 0)
        for _, pos, ref_len, off, _ in mine:
            beg, end, v = pos - 1, pos - 1 + ref_len, _voff(offsets, off)
            assert any(c[0] <= v < c[1] for c in ref["bins"][B.reg2bin(beg, end)])
            for w in range(beg >> 14, ((end - 1) >> 14) + 1):
                assert ref["linear"][w] <= v
        # the linear index: the smallest start of an overlapping record, the previous window's value where there is none
        for w in range(min(len(ref["linear"]), 64)):
            over = [_voff(offsets, r[3]) for r in mine if (r[1] - 1) >> 14 <= w <= (r[1] - 2 + r[2]) >> 14]
            assert ref["linear"][w] == (min(over) if over else (ref["linear"][w - 1] if w else 0))
    reader = B.Reader(stream)   # lines read back from their virtual offsets
    for r in rows[:40] + rows[-40:]:
        assert reader.read(_voff(offsets, r[3]), _voff(offsets, r[3] + r[4])) == text[r[3]:r[3] + r[4]]


def _regions():
    rng = np.random.default_rng(77)
    regions = [("chrA", 0, 1 << 29), ("chrB", 0, 1 << 29), ("chrEmpty", 0, 1 << 29), ("chrNone", 0, 1000),   # whole contigs, the empty one, an unknown one
               ("chrA", 16383, 16384), ("chrA", 16384, 16385), ("chrA", 16385, 16386), ("chrA", 16379, 16380), ("chrA", 16388, 16389), ("chrA", 16389, 16390),
               ("chrA", 131071, 131072), ("chrA", 131072, 131073), ("chrA", 141070, 141071), ("chrA", 141071, 141072), ("chrA", 121070, 121071), ("chrA", 121071, 121072),
               ("chrA", 130000, 132000), ("chrA", 32767, 32768), ("chrA", 32768, 32769), ("chrA", 49152, 49153), ("chrA", 49154, 49155), ("chrA", 262143, 262145),
               ("chrA", 400_000, 500_000), ("chrA", 5, 5), ("chrA", 1 << 28, 1 << 29),   # empty regions
               ("chrB", 299_999_999, 300_000_000), ("chrB", 300_000_001, 300_000_002), ("chrB", 300_000_002, 300_000_003), ("chrB", 200_000, 299_999_999),
               ("chrB", (1 << 29) - 4, 1 << 29), ("chrB", (1 << 29) - 2, 1 << 29), ("chrB", 120_000, 1 << 29)]
    for _ in range(30):
        c = "chrA" if rng.random() < 0.6 else "chrB"
        beg = int(rng.integers(0, 400_000 if c == "chrA" else 120_000))
        regions.append((c, beg, beg + int(rng.integers(1, 1 << int(rng.integers(1, 18))))))
    return regions


def test_queries():
    text, rows, stream, offsets, tbi = fixture()
    reader = B.Reader(stream)
    regions, hits = _regions(), 0
    assert len(regions) >= 50
    for contig, beg, end in regions:
        got, want = B.query(tbi, reader, contig, beg, end), B.brute_force(text, contig, beg, end)
        assert got == want, (contig, beg, end, len(got), len(want))
        hits += len(want)
    assert hits > 2000 and len(B.brute_force(text, "chrA", 131071, 131072)) >= 1 and B.brute_force(text, "chrA", 1 << 28, 1 << 29) == []


def test_coordinate_out_of_range_gives_no_index():
    _, _, _, offsets, _ = fixture()
    for pos, ref_len in ((1 << 29, 1), ((1 << 29) - 1, 2), (1 << 31, 1)):
        raw, warning = tabix.tabix_index(["chrA"], offsets, [(0, 100, 1, len(HEADER), 30), (0, pos, ref_len, len(HEADER) + 30, 30)])
        assert raw is None and "2^29" in warning and "\n" not in warning
    raw, warning = tabix.tabix_index(["chrA"], offsets, [(0, (1 << 29) - 1, 1, len(HEADER), 30)])   # the last coordinate inside the scheme
    assert warning is None and B.parse_tbi(raw)["refs"][0]["bins"] == {4681 + 32767: [(_voff(offsets, len(HEADER)), _voff(offsets, len(HEADER) + 30))]}
    raw, warning = tabix.tabix_index(["chrA"], offsets, [(0, 200, 1, len(HEADER), 30), (0, 100, 1, len(HEADER) + 30, 30)])
    assert raw is None and "not sorted" in warning


def test_no_lines():
    stream, offsets, _ = lib.diag_bgzf(HEADER)
    raw, warning = tabix.tabix_index([], offsets, [])
    tbi = B.parse_tbi(raw)
    assert warning is None and tbi["names"] == [] and tbi["refs"] == [] and tbi["n_no_coor"] == 0


def test_writer_line_table_indexes_the_writers_text():
    """GenotypeWriter::vcfText's optional line table (the project's own writer over fabricated sampler results, two contigs): the text is the same with and
    without it, every row names its line, and the index built from it answers region queries over the BGZF-compressed text as a scan does"""
    import test_cluster_stage_cpu as T
    from test_genotype_writer_cpu import fabricate_results

    from bayestyper_amd.host import genotypes
    from bayestyper_amd.host.cluster_stage import ClusterStage, GenotypeWriter

    k, S = 15, 2
    rng = np.random.default_rng(4243)
    genome = T.random_genome(rng, [60000, 30000], ())
    st = ClusterStage(k)
    for g in genome:
        st.add_sequence(*g)
    st.set_variants(vcf_text=T.make_vcf(rng, genome, k, 250, True, extra_contig=False, sv_blocks=4))
    assert st.next_unit(10 ** 9)
    units, *_ = T.parse_dump("UNIT 1\n" + st.unit_text())
    w = GenotypeWriter(st, ["sample_%d" % s for s in range(S)])
    mf = genotypes.min_fraction_observed_kmers([15.0] * S)
    for gi, g in enumerate(units[0]):
        for vi, v in enumerate(g["vertices"]):
            H = int(rng.integers(2, 5))
            ploidy = np.array([2] * S, np.uint8)
            hap_allele, h1, h2, freq, stats = fabricate_results(rng, S, H, [1 + len(alts) + dep for (_, _, dep, alts) in v["vars"]], ploidy)
            w.add_cluster(gi, vi, S, H, hap_allele, h1, h2, freq, stats, ploidy, mf)
    text = w.text("ref.fa", "##graph=x\n", "##genotype=y\n").encode()
    contigs, rows = w.line_table("ref.fa", "##graph=x\n", "##genotype=y\n")
    assert w.text("ref.fa", "##graph=x\n", "##genotype=y\n").encode() == text   # (collecting the table does not change the text)
    w.close(), st.close()
    lines = [ln for ln in text.split(b"\n") if ln and not ln.startswith(b"#")]
    assert len(rows) == len(lines) > 100 and len(contigs) == 2 and len(text) > B.BLOCK
    at = text.index(lines[0])
    for (ci, pos, ref_len, off, length), ln in zip(rows, lines):
        assert off == at and text[off:off + length] == ln + b"\n" and B.line_interval(ln) == (contigs[ci], pos - 1, pos - 1 + ref_len)
        at += length
    assert at == len(text)
    stream, offsets, _ = lib.diag_bgzf(text)
    raw, warning = tabix.tabix_index(contigs, offsets, rows)
    assert warning is None
    tbi, reader = B.parse_tbi(raw), B.Reader(stream)
    for contig in contigs:
        for beg, end in [(0, 1 << 29), (0, 16384), (16383, 16385), (20000, 20100), (29999, 30001), (59000, 70000)] + [(int(b), int(b) + 700) for b in rng.integers(0, 60000, 10)]:
            assert B.query(tbi, reader, contig, beg, end) == B.brute_force(text, contig, beg, end)
