"""The parallel gunzip's code run by one host thread (bt_diag_inflate_raw: bayestyper_amd/csrc/bt_gunzip.hpp with a team of one) against Python's zlib, byte
for byte, over the inputs of tests/gunzip_data.py: what the finder splits, what it cannot, false candidates, teams out of room, the windows' edges, every
start bit, resumed calls, and single-bit damage.  The same list runs on the device in test_gunzip_gpu.py."""
import zlib

import numpy as np
import pytest

import gunzip_data as gd


@pytest.fixture(scope="module")
def corpus():
    """name -> (stream, zlib's bytes): computed once, never changed"""
    return {name: (s, gd.inflate(s)[0]) for name, s in gd.corpus().items()}


def check_invariant(run, stream, want):
    """the bytes, end_bit, stream_end and crc32 over the four chunk sizes -> the results by chunk size"""
    got = {chunk: run(stream, chunk_bytes=chunk) for chunk in gd.CHUNKS}
    for chunk, r in got.items():
        assert r["data"] == want and r["stream_end"] == 1 and r["crc32"] == zlib.crc32(want), chunk
        assert (r["end_bit"] + 7) // 8 == gd.inflate(stream)[2], chunk
        assert r["end_bit"] == got[gd.CHUNKS[0]]["end_bit"]
        assert r["stats"]["out_bytes"] == len(want)
    return got


@pytest.mark.parametrize("name", ["fastq_l1", "fastq_l6", "fastq_l9"])
def test_fastq_is_split_at_its_block_starts(corpus, name):
    """the project's own shape: every candidate is a true block start, and a decode in one team would miss the count of links"""
    from bayestyper_amd import lib

    stream, want = corpus[name]
    got = check_invariant(lib.diag_inflate_raw, stream, want)
    st = got[16 * gd.KIB]["stats"]
    assert st["links_verified"] >= len(stream) / (4 * 16 * gd.KIB) and st["links_broken"] == 0, st
    assert got[1024 * gd.KIB]["stats"]["candidates"] == 0   # one chunk: nothing to find


def test_many_small_blocks(corpus):
    """a sync flush every 2 - 5 KB: empty stored blocks, back-references across them"""
    from bayestyper_amd import lib

    stream, want = corpus["sync_flushed"]
    flushes = len(gd.sync_flushed(gd.fastq(1)[:300_000], 2)[1])
    assert flushes > 60
    for chunk in (1 * gd.KIB, 2 * gd.KIB, 4 * gd.KIB):
        r = lib.diag_inflate_raw(stream, chunk_bytes=chunk)
        assert r["data"] == want and r["stream_end"] == 1
        assert r["stats"]["links_verified"] >= min(flushes, len(stream) // chunk) / 4 and r["stats"]["links_broken"] == 0, (chunk, r["stats"])
    check_invariant(lib.diag_inflate_raw, stream, want)


def test_streams_the_finder_cannot_split():
    """stored and fixed blocks are no candidates; Z_HUFFMAN_ONLY and Z_RLE write dynamic blocks, so their streams are kept to one (final) block here"""
    from bayestyper_amd import lib

    text = gd.fastq(5, reads=300)
    streams = gd.unsplittable()
    streams["huffman_only"] = gd.raw(text[:15000], 6, zlib.Z_HUFFMAN_ONLY)
    streams["rle"] = gd.raw(text[:15000], 6, zlib.Z_RLE)
    for name, stream in streams.items():
        want = gd.inflate(stream)[0]
        for chunk, r in check_invariant(lib.diag_inflate_raw, stream, want).items():
            assert r["stats"]["candidates"] == 0 and r["stats"]["links_verified"] == 0 and r["stats"]["rounds"] == 1, (name, chunk, r["stats"])


def test_longer_huffman_only_and_rle_streams(corpus):
    from bayestyper_amd import lib

    for name in ("huffman_only", "rle"):
        check_invariant(lib.diag_inflate_raw, *corpus[name])


def test_false_candidates_cost_rounds_not_bytes(corpus):
    from bayestyper_amd import lib

    stream, want = corpus["false_candidates"]
    got = check_invariant(lib.diag_inflate_raw, stream, want)
    st = got[4 * gd.KIB]["stats"]
    assert st["links_broken"] >= 1 and st["rounds"] >= 3 and st["candidates"] >= 3, st


def test_a_team_out_of_room(corpus):
    from bayestyper_amd import lib

    stream, want = corpus["repeated_read"]
    assert len(want) > 100 * lib.GUNZIP_EXPAND * len(stream) / 16   # a ratio far above the budget
    got = check_invariant(lib.diag_inflate_raw, stream, want)
    assert all(r["stats"]["rounds"] > 1 for r in got.values())


def test_window_edges(corpus):
    """matches at distance 32768 into the part before, a copy of what was itself copied through markers two parts before, an overlapping copy of a marker"""
    from bayestyper_amd import lib

    stream, want = corpus["window_edges"]
    got = check_invariant(lib.diag_inflate_raw, stream, want)
    assert got[1 * gd.KIB]["stats"]["links_verified"] == 3, got[1 * gd.KIB]["stats"]


@pytest.fixture(scope="module")
def walked():
    """a small sync-flushed stream, zlib's bytes, and its block boundaries from the walker of gunzip_data"""
    text = gd.fastq(21, reads=260)
    stream, _ = gd.sync_flushed(text, 21, 1500, 3000)
    starts, lengths = gd.walk_blocks(stream)
    assert lengths[-1] == len(text) and (starts[-1] + 7) // 8 == len(stream)
    return stream, text, starts, lengths


def start_cases(walked):
    """a block start for every start_bit & 7, none of them the stream's first block"""
    stream, text, starts, lengths = walked
    by_bit = {}
    for s, n in list(zip(starts, lengths))[1:-1]:
        by_bit.setdefault(s & 7, (s, n))
    assert sorted(by_bit) == list(range(8))
    return [by_bit[b] for b in range(8)]


def test_every_start_bit(walked):
    from bayestyper_amd import lib

    stream, text, _, _ = walked
    for start, produced in start_cases(walked):
        for chunk in (1 * gd.KIB, 16 * gd.KIB):
            r = lib.diag_inflate_raw(stream, start_bit=start, window=text[max(0, produced - 32768):produced], chunk_bytes=chunk)
            assert r["data"] == text[produced:] and r["stream_end"] == 1 and r["crc32"] == zlib.crc32(text[produced:]), (start, chunk)
    # without the bytes before it, a start whose block reaches back is the error of the distance
    start, produced = start_cases(walked)[3]
    with pytest.raises(lib.BtError, match="bt_diag_inflate_raw: deflate block at offset .*: distance reaches before the stream's start"):
        lib.diag_inflate_raw(stream, start_bit=start, window=text[produced - 10:produced])


def resume(run, stream, want, chunk):
    """calls with a third of the output as capacity, each from the end_bit of the one before with the last 32 KiB as the window"""
    out, at, calls = b"", 0, 0
    while True:
        r = run(stream, start_bit=at, window=out[-32768:], chunk_bytes=chunk, capacity=len(want) // 3)
        out += r["data"]
        calls += 1
        if r["stream_end"]:
            break
        assert r["data"] and r["end_bit"] > at and calls < 100
        at = r["end_bit"]
    assert out == want and calls > 3
    return calls


@pytest.mark.parametrize("name", ["fastq_l6", "sync_flushed", "window_edges"])
def test_resumption(corpus, name):
    from bayestyper_amd import lib

    stream, want = corpus[name]
    assert resume(lib.diag_inflate_raw, stream, want, 4 * gd.KIB) == resume(lib.diag_inflate_raw, stream, want, 1024 * gd.KIB)


def test_zero_progress_is_a_result(corpus):
    from bayestyper_amd import lib

    stream, want = corpus["fastq_l6"]
    r = lib.diag_inflate_raw(stream, capacity=100)      # the first block does not fit
    assert (r["data"], r["end_bit"], r["stream_end"]) == (b"", 0, 0)
    r = lib.diag_inflate_raw(stream[:5000])             # the first block is not whole
    assert (r["data"], r["end_bit"], r["stream_end"]) == (b"", 0, 0)
    r = lib.diag_inflate_raw(stream[:100_000], chunk_bytes=4 * gd.KIB)   # whole blocks, then one that is not
    assert 0 < len(r["data"]) < len(want) and want.startswith(r["data"]) and r["stream_end"] == 0 and r["crc32"] == zlib.crc32(r["data"])
    assert lib.diag_inflate_raw(b"")["data"] == b""


def flip_outcome(run, stream):
    from bayestyper_amd import lib

    try:
        r = run(stream, chunk_bytes=1 * gd.KIB, capacity=200_000)
        return ("ok", r["data"], r["end_bit"], r["stream_end"], r["crc32"])
    except lib.BtError as e:
        return ("error", str(e))


def zlib_outcome(stream):
    try:
        out, eof, _ = gd.inflate(stream)
        return out, eof
    except zlib.error:
        return None, False


@pytest.fixture(scope="module")
def flips():
    base = gd.flip_base()
    return gd.inflate(base)[0], gd.bit_flips(base, 200, 4)


def test_single_bit_flips(flips):
    """a flipped bit gives an error, a stop short of the stream's end, zlib's own bytes, or bytes whose CRC-32 is not the sound stream's"""
    from bayestyper_amd import lib

    sound, cases = flips
    errors = 0
    for bit, stream in cases:
        got = flip_outcome(lib.diag_inflate_raw, stream)
        want, eof = zlib_outcome(stream)
        if got[0] == "error":
            assert want is None and got[1].startswith("bt_diag_inflate_raw: deflate block at offset "), (bit, got)
            errors += 1
        elif eof:
            assert got[1] == want and got[3] == 1 and got[4] == zlib.crc32(want), bit
            assert want == sound or zlib.crc32(want) != zlib.crc32(sound), bit
        else:
            assert got[3] == 0, bit
    assert errors >= 5


def test_arguments():
    from bayestyper_amd import lib

    with pytest.raises(lib.BtError, match="chunk_bytes must be at least 1024"):
        lib.diag_inflate_raw(b"\x03\x00", chunk_bytes=512)
    with pytest.raises(lib.BtError, match="start_bit lies behind the input"):
        lib.diag_inflate_raw(b"\x03\x00", start_bit=17)
    with pytest.raises(lib.BtError, match="at most 32768"):
        lib.diag_inflate_raw(b"\x03\x00", window=bytes(32769))
    assert lib.diag_inflate_raw(b"\x03\x00")["stream_end"] == 1
    assert lib.GUNZIP_DEFAULT_CHUNK >= 1024 and lib.GUNZIP_EXPAND >= 4
