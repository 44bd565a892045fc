"""`bayesTyper cluster` with BT_FIND_PATHS_SAMPLES: the data set of test_find_paths_wave_cli_gpu (2 000 isolated SNVs and a stretch of 120) with a third
sample, run with the switch unset, = 2, = 3 and = 8 (more than there are samples).  Every file the stage writes is equal as that test compares them, and
the stage table of a switched run names the samples per launch, so a silently ignored switch cannot pass."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import _oracle  # noqa: F401  (sys.path set-up of the helpers below)
from _oracle import OrcBloom
from test_cli_gpu import EXE, K
from test_find_paths_wave_cli_gpu import _content, _files

pytestmark = pytest.mark.gpu

NT = "ACGT"
LABEL = "samples per launch"


def _dataset(oracle, d, rng):
    """test_find_paths_wave_cli_gpu._dataset with three samples"""
    from test_pipeline_gpu import sample_haplotype

    num_isolated, spacing, stretch, step = 2000, 3 * K, 120, 20
    length = (num_isolated + 4) * spacing + stretch * step + 4 * K
    seq = "".join(rng.choice(list(NT), length))
    positions, p = [], 2 * K
    for i in range(num_isolated):
        if i == 700:   # the stretch sits between two isolated SNVs, more than k away from both
            positions += [p + 2 * K + j * step for j in range(stretch)]
            p += stretch * step + 4 * K
        positions.append(p)
        p += spacing
    records = [(q, seq[q], [NT[(NT.find(seq[q]) + 1 + int(rng.integers(3))) % 4]]) for q in positions]
    os.makedirs(d)
    with open(os.path.join(d, "genome.fa"), "w") as fh:
        fh.write(">chr1\n" + "\n".join(seq[i:i + 60] for i in range(0, len(seq), 60)) + "\n")
    with open(os.path.join(d, "candidates.vcf"), "w") as fh:
        fh.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
        for q, ref, alts in records:
            fh.write(f"chr1\t{q + 1}\t.\t{ref}\t{alts[0]}\t.\t.\t.\n")
    with open(os.path.join(d, "samples.tsv"), "w") as sf:
        for s, gender in enumerate(["F", "M", "F"]):
            text = "N".join(sample_haplotype(rng, seq, records) for _ in range(2))
            km, va = oracle.kmers_from_sequence(text.encode(), K)
            present = np.unique(km[va == 1], axis=0)
            cnt = (rng.poisson(14, len(present)) + 1).astype(np.uint32)
            asc = oracle.unpack(present, K).reshape(-1, K)
            order = np.lexsort(asc.T[::-1])   # KMC order = ascending ASCII order
            prefix = os.path.join(d, f"sample{s + 1}")
            oracle.kmc_write(prefix, np.ascontiguousarray(asc[order]).reshape(-1), cnt[order], K, 7, 1)
            bloom = OrcBloom(oracle, len(present), 1e-3, K)
            bloom.insert(np.ascontiguousarray(asc).reshape(-1))
            bloom.save(prefix)
            bloom.close()
            sf.write(f"sample{s + 1}\t{gender}\t{prefix}\n")
    return len(records)


def _cluster(d, run_dir, per_call):
    """the same command line in a directory of its own; the stretch (120 SNVs, three vertices each) on a wavefront of its own in every run"""
    e = dict(os.environ, BT_STAGE_TIMES="1", BT_FIND_PATHS_WAVE_MIN="200")
    e.pop("BT_FIND_PATHS_SAMPLES", None)
    if per_call is not None:
        e["BT_FIND_PATHS_SAMPLES"] = str(per_call)
    os.makedirs(run_dir)
    r = subprocess.run([EXE, "cluster", "-v", os.path.join(d, "candidates.vcf"), "-s", os.path.join(d, "samples.tsv"), "-g", os.path.join(d, "genome.fa"), "-o", "bt", "-r", "13"],
                       capture_output=True, text=True, env=e, cwd=run_dir, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stderr


def test_cluster_with_several_samples_per_launch(oracle, tmp_path):
    d = str(tmp_path / "data")
    assert _dataset(oracle, d, np.random.default_rng(97)) == 2120
    base_prefix = str(tmp_path / "unset" / "bt")
    err = _cluster(d, os.path.dirname(base_prefix), None)
    assert LABEL not in err, err[-3000:]
    a = _files(base_prefix)
    assert "_unit_1/variant_clusters.bin" in a and any(key.startswith("_cluster_data") for key in a)
    assert b'time:"' in gzip.decompress(a["_unit_1/variant_clusters.bin"])   # (the one field the comparison blanks is there)
    for per_call, launches in ((2, "samples per launch 2 + 1 (2 launch(es)"), (3, "samples per launch 3 (1 launch(es)"), (8, "samples per launch 3 (1 launch(es)")):
        prefix = str(tmp_path / f"n{per_call}" / "bt")
        err = _cluster(d, os.path.dirname(prefix), per_call)
        line = [ln for ln in err.split("\n") if LABEL in ln]
        assert len(line) == 1 and launches in line[0] and f"BT_FIND_PATHS_SAMPLES={per_call})" in line[0], err[-3000:]
        b = _files(prefix)
        assert sorted(a) == sorted(b)
        for key in a:
            assert len(a[key]) > 0 and _content(a[key]) == _content(b[key]), (per_call, key)
