"""`bayesTyper genotype -z` with BT_VCF_BGZF=1 (the VCF written as BGZF on the device, bt_bgzf_save, and its tabix index beside it) against the same run
without the switch: the decompressed VCF must be identical, every member must be a BGZF block and the file must end with the EOF block, region queries
through the index must return what a scan of the text returns, and the stage table must name the route exactly when the switch is set and applies.
Without -z the switch does nothing.  With several ranks, rank 0 writes both files."""
import gzip
import os
import zlib

import numpy as np
import pytest

import _bgzf as B
import _oracle  # noqa: F401  (sys.path set-up of the helpers below)
import c1_dataset
from test_candidates_device_cli_gpu import _cluster, _genotype

pytestmark = pytest.mark.gpu

LABEL = "BGZF on the device (bt_bgzf_save)"
GIBBS = dict(chains=3, burn=12, samples=30)


@pytest.fixture(scope="module")
def c1(tmp_path_factory, oracle):
    d = tmp_path_factory.mktemp("c1")
    ds = c1_dataset.make(str(d / "data"), oracle, 70_000, 350, 3, num_error_kmers=150_000, genders=["F", "M", "F"])
    prefix = str(d / "bt")
    _cluster(ds["dir"], prefix, 7)
    base = str(d / "base")   # the parent's route: -z, no switch
    out, err = _genotype(base, prefix, ds["dir"], 7, GIBBS, ("-z",), {})
    assert LABEL not in err and "write VCF (sort + output)" in err
    assert not os.path.exists(base + ".vcf.gz.tbi")
    return ds["dir"], prefix, _lines(_one_member(base + ".vcf.gz"))


def _lines(text):
    return [x for x in text.split(b"\n") if not x.startswith(b"##BayesTyperOptions=")]   # (the options line names the output prefix)


def _one_member(path):
    """the content of a gz file that is ONE gzip member without an extra field, as the routes without the switch write it"""
    raw = open(path, "rb").read()
    z = zlib.decompressobj(31)
    text = z.decompress(raw)
    assert raw[3] == 0 and z.eof and z.unused_data == b"" and len(text) > 1000
    return text


def _check_bgzf_outputs(prefix, base_lines):
    assert not os.path.exists(prefix + ".vcf") and not os.path.exists(prefix + ".vcf.gz.tmp") and not os.path.exists(prefix + ".vcf.gz.tbi.tmp")
    raw = open(prefix + ".vcf.gz", "rb").read()
    text = gzip.decompress(raw)
    assert _lines(text) == base_lines   # the decompressed VCF is the plain -z run's
    B.check_stream(raw, text)           # every member is a BGZF block; the EOF block ends the file
    index_raw = open(prefix + ".vcf.gz.tbi", "rb").read()
    B.check_stream(index_raw, gzip.decompress(index_raw))   # the index is BGZF itself
    tbi = B.parse_tbi(gzip.decompress(index_raw))
    lines = [ln for ln in text.split(b"\n") if ln and not ln.startswith(b"#")]
    contigs = []
    for ln in lines:
        name = ln.split(b"\t", 1)[0].decode()
        if name not in contigs:
            contigs.append(name)
    assert tbi["names"] == contigs and len(lines) > 100 and tbi["n_no_coor"] == 0 and (tbi["format"], tbi["col_seq"], tbi["col_beg"], tbi["col_end"]) == (2, 1, 2, 0)
    assert sum(len(r["bins"]) for r in tbi["refs"]) >= len(contigs)
    reader = B.Reader(raw)
    rng = np.random.default_rng(11)
    regions = [(c, 0, 1 << 29) for c in contigs] + [("no_such_contig", 0, 1000), (contigs[0], 5, 5)]
    spans = [B.line_interval(ln) for ln in lines]
    while len(regions) < 20:
        name, beg, end = spans[int(rng.integers(len(spans)))]
        w = int(rng.integers(1, 5000))
        regions.append((name, max(0, beg - int(rng.integers(0, w))), end + int(rng.integers(0, w))))
    found = 0
    for contig, beg, end in regions:
        got, want = B.query(tbi, reader, contig, beg, end), B.brute_force(text, contig, beg, end)
        assert got == want, (contig, beg, end)
        found += len(want)
    assert found >= len(lines)


def test_genotype_z_bgzf(c1, tmp_path):
    ds_dir, unit_prefix, text = c1
    on = str(tmp_path / "on")
    out, err = _genotype(on, unit_prefix, ds_dir, 7, GIBBS, ("-z",), {"BT_VCF_BGZF": "1"})
    assert "write VCF (sort + output), " + LABEL in err, err[-3000:]
    _check_bgzf_outputs(on, text)
    # a switch value other than 1 is the parent's route: one member, no index, no label
    off = str(tmp_path / "off")
    out, err = _genotype(off, unit_prefix, ds_dir, 7, GIBBS, ("-z",), {"BT_VCF_BGZF": "0"})
    assert LABEL not in err and not os.path.exists(off + ".vcf.gz.tbi") and _lines(_one_member(off + ".vcf.gz")) == text


def test_switch_without_z_does_nothing(c1, tmp_path):
    ds_dir, unit_prefix, text = c1
    plain = str(tmp_path / "plain")
    out, err = _genotype(plain, unit_prefix, ds_dir, 7, GIBBS, (), {"BT_VCF_BGZF": "1"})
    assert LABEL not in err and not os.path.exists(plain + ".vcf.gz") and not os.path.exists(plain + ".vcf.gz.tbi") and not os.path.exists(plain + ".vcf.tbi")
    assert _lines(open(plain + ".vcf", "rb").read()) == text


def test_three_ranks_rank0_writes_both_files(c1, tmp_path):
    ds_dir, unit_prefix, text = c1
    many = str(tmp_path / "many")
    out, err = _genotype(many, unit_prefix, ds_dir, 7, GIBBS, ("-z",), {"BT_VCF_BGZF": "1", "BT_GPUS": "3", "BT_COMM_TRANSPORT": "files", "BT_DEVICE": "0"})
    assert "Rank 0 of " in out and "write VCF (sort + output), " + LABEL in err, err[-3000:]
    _check_bgzf_outputs(many, text)
