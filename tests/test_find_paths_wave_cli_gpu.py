"""`bayesTyper cluster` on candidates with one wide cluster — a stretch of 120 SNVs 20 nt apart among 2 000 isolated SNVs, two samples —, once with every
cluster on a lane (BT_FIND_PATHS_WAVE_MIN=0) and once with the stretch on a wavefront of its own: every file the stage writes must be byte-identical, and
the second run's stage table must name the wave route, so a silently ignored switch cannot pass.

The unit file records the options header of the run, and that header carries the run's start time (Options.cpp: time:"..."): two runs a few seconds apart
cannot agree on it.  The files are therefore compared as their contents — gunzipped where they are gzip members, deflate being deterministic — with the
value of that one field blanked; everything else, byte for byte."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import _oracle  # noqa: F401  (sys.path set-up of the helpers below)
from _oracle import OrcBloom
from test_cli_gpu import EXE, K

pytestmark = pytest.mark.gpu

NT = "ACGT"
WAVE_LABEL = "vertices on a wavefront each"


def _dataset(oracle, d, rng):
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
        for s, gender in enumerate(["F", "M"]):
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


def _cluster(d, run_dir, wave_min):
    """the same command line in a directory of its own (the unit file records the options, output prefix included)"""
    e = dict(os.environ, BT_STAGE_TIMES="1", BT_FIND_PATHS_WAVE_MIN=str(wave_min))
    os.makedirs(run_dir)
    r = subprocess.run([EXE, "cluster", "-v", os.path.join(d, "candidates.vcf"), "-s", os.path.join(d, "samples.tsv"), "-g", os.path.join(d, "genome.fa"), "-o", "bt", "-r", "13"],
                       capture_output=True, text=True, env=e, cwd=run_dir, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stderr


def _files(prefix):
    out = {}
    for base in (prefix + "_unit_1", prefix + "_cluster_data"):
        for dp, _, fns in os.walk(base):
            for fn in fns:
                path = os.path.join(dp, fn)
                out[os.path.relpath(path, os.path.dirname(prefix))[len(os.path.basename(prefix)):]] = open(path, "rb").read()
    return out


def _content(raw):
    data = gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw
    return re.sub(rb'time:"[^"]*"', b'time:""', data)


def test_cluster_with_a_wide_cluster_on_a_wavefront(oracle, tmp_path):
    d = str(tmp_path / "data")
    n = _dataset(oracle, d, np.random.default_rng(97))
    assert n == 2120
    lane_prefix, wave_prefix = str(tmp_path / "lane" / "bt"), str(tmp_path / "wave" / "bt")
    err_lane = _cluster(d, os.path.dirname(lane_prefix), 0)
    err_wave = _cluster(d, os.path.dirname(wave_prefix), 200)   # 120 SNVs: three vertices each
    assert WAVE_LABEL not in err_lane, err_lane[-3000:]
    line = [ln for ln in err_wave.split("\n") if WAVE_LABEL in ln]
    assert len(line) == 1 and " 1 cluster(s) of >= 200 vertices" in line[0], err_wave[-3000:]
    a, b = _files(lane_prefix), _files(wave_prefix)
    assert "_unit_1/variant_clusters.bin" in a and any(key.startswith("_cluster_data") for key in a)
    assert sorted(a) == sorted(b)
    for key in a:
        assert len(a[key]) > 0 and _content(a[key]) == _content(b[key]), key
    assert b'time:"' in gzip.decompress(a["_unit_1/variant_clusters.bin"])   # (the one field the comparison blanks is there)
