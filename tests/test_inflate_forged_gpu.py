"""The device inflate (bgzf_inflate_kernel, the parallel gunzip's kernels: wavefront teams, lane-parallel table fill, team copies between barriers, tables in
LDS) over the forged streams of tests/deflate_forge.py, against zlib and against the same code's host run (test_inflate_forged_cpu.py): the whole sound
corpus in one launch, the raw streams through the finder and the marker decoder, damaged streams one call each, and the three stream objects over forged
files."""
import gzip
import random
import time
import zlib

import numpy as np
import pytest

import bam_data as bd
import deflate_forge as df
import fastq_data as fd
import gunzip_data as gd
from test_bam_gpu import scan_text
from test_fastq_gpu import scan_all
from test_gunzip_gpu import scan_file
from test_inflate_forged_cpu import KIB, RAW_CAPACITY, concatenated, flip_cases, forge, outcome   # noqa: F401  (fixtures and helpers, shared)

pytestmark = pytest.mark.gpu
GUARD = 256


def test_corpus_in_one_launch(gpu_ctx, forge):
    """every member of the sound corpus, the match grid included, as one BGZF stream: a wavefront per member"""
    from bayestyper_amd import lib

    stream, want = concatenated(forge)
    assert len(forge["members"]) > 300
    got = lib.bgzf_inflate(gpu_ctx, stream, guard=GUARD)
    if got[:-GUARD] != want:   # name the first member that differs
        at = 0
        for name, _, data, _ in forge["members"]:
            assert got[at:at + len(data)] == data, name
            at += len(data)
    assert got[:-GUARD] == want and got[-GUARD:] == b"\xa5" * GUARD
    assert lib.diag_bgzf_inflate(stream) == want


@pytest.mark.parametrize("name", ["raw_records", "raw_reads", "raw_random"])
def test_raw_route(gpu_ctx, forge, name):
    """twenty and more forged non-final dynamic blocks, matches at distance 32768 across blocks and teams: zlib's bytes, the scanner's end bit, and the host
    run's stats; the finder finds forged headers and teams are linked through them"""
    from bayestyper_amd import lib

    stream, want = forge["raw"][name]
    end = df.scan(stream)[2]
    for chunk in (1 * KIB, 4 * KIB):
        dev = lib.inflate_raw(gpu_ctx, stream, chunk_bytes=chunk, capacity=len(want) + 100)
        host = lib.diag_inflate_raw(stream, chunk_bytes=chunk, capacity=len(want) + 100)
        assert dev["data"] == want and dev["end_bit"] == end and dev["stream_end"] == 1 and dev["crc32"] == zlib.crc32(want), chunk
        assert dev == host, (chunk, dev["stats"], host["stats"])
        assert dev["stats"]["candidates"] >= 1 and dev["stats"]["links_verified"] >= 1, (chunk, dev["stats"])


DAMAGED = ("small_mixed", "small_one_distance", "small_empty_block")   # stored, fixed and dynamic blocks; a single distance code; an empty block
PER_CLASS = 12


def damaged_selection(flip_cases):
    """for each (stream, zlib's outcome class) the first PER_CLASS flips in bit order and the last one, and every flip the BGZF frame accepts, up to 60 ->
    ([(name, data, bit, flipped payload, class)], the classes seen over all eight streams)"""
    chosen, every, accepted = [], set(), 0
    for name, payload, data, cases in flip_cases:
        by_class = {}
        for bit, flipped, cls, out in cases:
            cls = "accepted" if cls == "end" and out == data else cls
            every.add(cls)
            by_class.setdefault(cls, []).append((name, data, bit, flipped, cls))
        if name in DAMAGED:
            for cls, flips in sorted(by_class.items()):
                if cls == "accepted":
                    chosen += flips[:60 - accepted]
                    accepted += len(flips[:60 - accepted])
                else:
                    chosen += flips[:PER_CLASS] + flips[PER_CLASS:][-1:]
    return chosen, every


def test_damaged_streams_one_call_each(gpu_ctx, flip_cases):
    """every way a stream can be damaged, on the device: as a BGZF block (the sound data's CRC-32 and ISIZE around the flipped payload) and as a raw stream,
    the device gives the host's message or the host's bytes, and writes nothing behind its output"""
    from bayestyper_amd import lib

    chosen, every = damaged_selection(flip_cases)
    assert {c[4] for c in chosen} == every and len(every) >= 14, every - {c[4] for c in chosen}   # every class zlib shows over all the flips runs here
    started, messages = time.perf_counter(), set()
    for name, data, bit, flipped, cls in chosen:
        block, keep = df.bgzf_member(flipped, data), {}
        host = outcome(lib.diag_bgzf_inflate, block)
        dev = outcome(lib.bgzf_inflate, gpu_ctx, block, guard=GUARD, keep=keep)
        assert keep["out"][-GUARD:] == b"\xa5" * GUARD, (name, bit)
        if host[0] == "error":
            assert dev == ("error", host[1].replace("bt_diag_bgzf_inflate", "bt_bgzf_inflate")), (name, bit, cls, dev)
            messages.add(host[1].split(": ")[-1])
        else:
            assert cls == "accepted" and dev == ("ok", data + b"\xa5" * GUARD), (name, bit, cls)
        host = outcome(lib.diag_inflate_raw, flipped, chunk_bytes=1 * KIB, capacity=RAW_CAPACITY)
        dev = outcome(lib.inflate_raw, gpu_ctx, flipped, chunk_bytes=1 * KIB, capacity=RAW_CAPACITY)   # (the binding checks the bytes behind the capacity)
        if host[0] == "error":
            assert dev == ("error", host[1].replace("bt_diag_inflate_raw", "bt_inflate_raw")), (name, bit, cls, dev)
            messages.add(host[1].split(": ")[-1])
        else:
            assert dev == host, (name, bit, cls)
    print("damaged streams: %d flips, two calls each, %.2f s; messages: %s" % (len(chosen), time.perf_counter() - started, sorted(messages)))
    assert len(messages) >= 9, messages   # the statuses of bt_inflate.hpp a payload can reach


# ---- the product path ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reads():
    rng = np.random.default_rng(77)
    return [np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=150)].tobytes() for _ in range(300)]


def test_forged_bgzf_fastq(gpu_ctx, reads):
    rng = np.random.default_rng(78)
    data = b"".join(b"@read%d\n%s\n+\n%s\n" % (i, r, np.frombuffer(b"#,5:AFGI", np.uint8)[rng.integers(0, 8, size=150)].tobytes()) for i, r in enumerate(reads))
    cuts = bd.even_cuts(len(data), 12001)
    forged, offsets = df.bgzf_file(data, cuts, 300)
    plain, plain_offsets = bd.bgzf(data, cuts)
    for per_slab in (1, 4):
        got = scan_all(gpu_ctx, forged, offsets + [len(forged)], per_slab)
        want = scan_all(gpu_ctx, plain, plain_offsets + [len(plain)], per_slab)
        assert got == want and got[1]["reads"] == 300, per_slab
    assert got[0] + got[2] == fd.parse(data)[0]


def test_forged_bam(gpu_ctx, reads):
    recs = bd.bam_of_reads(reads)
    head = bd.header()
    data = head + b"".join(r for r, _, _ in recs)
    cuts = bd.even_cuts(len(data), 9001)
    forged, offsets = df.bgzf_file(data, cuts, 400)
    plain, plain_offsets = bd.bgzf(data, cuts)
    for per_slab in (1, 5):
        got = scan_text(gpu_ctx, forged, offsets + [len(forged)], per_slab, len(head))
        assert got == scan_text(gpu_ctx, plain, plain_offsets + [len(plain)], per_slab, len(head)), per_slab
        assert got[0] == bd.records_text(recs, 0) and got[1]["kept"] == 300


def test_forged_gzip_fastq(gpu_ctx, reads):
    data = b"".join(b"@read%d\n%s\n+\n%s\n" % (i, r, b"I" * 150) for i, r in enumerate(reads))
    stream, _ = df.forged(df.long_blocks(data, random.Random(500), 40), 500)
    forged, plain = gd.gzip_member(data, payload=stream), gzip.compress(data, 6)
    for slab in (16 * KIB, 50_021):
        got = scan_file(gpu_ctx, forged, slab, max_in=256 * KIB)
        want = scan_file(gpu_ctx, plain, slab, max_in=256 * KIB)
        assert got[:2] == want[:2] and got[1]["reads"] == 300 and got[2]["out_bytes"] == len(data), slab
        assert got[2]["candidates"] >= 1 and got[2]["links_verified"] >= 1, got[2]
