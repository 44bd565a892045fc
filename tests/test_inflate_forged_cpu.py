"""The device inflate's code run by one host thread (bt_diag_bgzf_inflate, bt_diag_inflate_raw, bt_diag_gunzip_plausible: bayestyper_amd/csrc/bt_inflate.hpp
and bt_gunzip.hpp with a team of one) over the forged streams of tests/deflate_forge.py: valid deflate that zlib never writes (codes of 15, 15 and 7 bits,
HLIT 286, HDIST 30, every run-length coding of the header, a grid of match lengths against distances), every single-bit flip of eight small members, and the
header finder against an independent statement of its rules.  zlib's inflate is the yardstick.  The same corpus runs on the device in
test_inflate_forged_gpu.py."""
import zlib

import numpy as np
import pytest

import deflate_forge as df
import gunzip_data as gd

KIB = 1024
RAW_CAPACITY = 1 << 19   # a flipped stream of under 250 bytes decodes to at most 258 bytes per two bits: less than this


@pytest.fixture(scope="module")
def forge():
    """the corpus — built once, never changed"""
    return df.corpus()


@pytest.fixture(scope="module")
def scanned(forge):
    """name -> the scanner's blocks, of every member and raw stream"""
    out = {}
    for name, payload, data, _ in forge["members"]:
        got, blocks, end = df.scan(payload)
        assert got == data and (end + 7) // 8 == len(payload), name
        out[name] = blocks
    for name, (stream, data) in forge["raw"].items():
        got, blocks, end = df.scan(stream)
        assert got == data and (end + 7) // 8 == len(stream), name
        out[name] = blocks
    return out


def test_census(forge, scanned):
    """the corpus holds what it was built for, by the scanner's word (no project code): the forge must not silently stop reaching any of it"""
    blocks = [b for bs in scanned.values() for b in bs]
    dynamic = [b for b in blocks if b["type"] == 2]
    used = lambda key, l: sum(b[key].get(l, 0) for b in blocks if key in b)
    assert all(used("lit_used", l) >= 100 for l in range(11, 16)), [used("lit_used", l) for l in range(11, 16)]
    assert all(used("dist_used", l) >= 1 for l in range(9, 16)), [used("dist_used", l) for l in range(9, 16)]
    assert used("clen_used", 7) >= 1 and max(b["clen_max"] for b in dynamic) == 7
    assert any(b["hlit"] == 286 and b["hdist"] == 30 for b in dynamic) and any(b["hlit"] == 257 and b["hdist"] == 1 for b in dynamic)
    assert any(16 in b["cross"] for b in dynamic)
    assert any((18, 138) in b["runs"] for b in dynamic) and any((17, 10) in b["runs"] for b in dynamic)
    assert any(b["lit_codes"] == 1 and b["lit_max"] == 1 and not b["lit_used"].keys() - {1} and sum(b["lit_used"].values()) == 1 for b in dynamic)   # the end-of-block code alone
    assert any(b["dist_codes"] == 1 and b["pairs"] for b in dynamic)
    assert any(b["dist_codes"] == 0 and sum(b["lit_used"].values()) > 1 for b in dynamic)
    assert any(b["alt258"] for b in dynamic)   # zlib takes length 258 as symbol 284 with extra bits 31: df.checked has inflated that member
    for count in (1, 4, 16):
        members = [scanned[name] for name, _, _, tags in forge["members"] if not tags and len(scanned[name]) == count]
        assert len(members) >= 5, count
        if count > 1:
            assert all({b["type"] for b in bs} == {0, 1, 2} and any(b.get("stored") == 0 for b in bs) for bs in members), count
    assert {b["start"] & 7 for b in dynamic} == set(range(8))
    cells = {(length, dist) for length in df.GRID_LENGTHS for dist in df.grid_distances(length)}
    assert len(cells) > 140
    for kind in ("fixed", "dynamic"):
        found = set()
        for name, _, _, tags in forge["members"]:
            if "grid" in tags and name.startswith("grid_" + kind):
                b = scanned[name][-1]
                assert b["type"] == (1 if kind == "fixed" else 2) and len(b["pairs"]) == 2 and b["pairs"][1] == (3, 2) and b["pairs"][0][1] <= b["out"] + sum(b["lit_used"].values()), name
                if kind == "dynamic":   # the match under test is written with codes of 15 bits
                    assert b["lit_max"] == 15 and b["dist_max"] == 15 and b["lit_used"].get(15, 0) >= 1 and b["dist_used"].get(15, 0) >= 1, name
                found.add(b["pairs"][0])
        assert found == cells, kind
    raw = [scanned[name] for name in forge["raw"]]
    assert all(sum(b["type"] == 2 for b in bs[:-1]) >= 20 and any(p[1] == 32768 for b in bs for p in b.get("pairs", ())) for bs in raw)
    assert all(30_000 <= len(s) <= 60_000 for s, _ in forge["raw"].values())
    assert all(len(data) <= 40 * KIB + 1000 for _, _, data, _ in forge["members"])


def concatenated(forge):
    """the sound corpus as one BGZF stream -> (stream, its data)"""
    return b"".join(df.bgzf_member(p, d) for _, p, d, _ in forge["members"]), b"".join(d for _, _, d, _ in forge["members"])


def test_corpus_as_bgzf(forge):
    from bayestyper_amd import lib

    stream, want = concatenated(forge)
    assert lib.diag_bgzf_inflate(stream) == want
    for name, payload, data, _ in forge["members"]:   # and one by one, so that a failure names its member
        assert lib.diag_bgzf_inflate(df.bgzf_member(payload, data)) == data, name


def check_raw(run, stream, want, end_bit):
    """bytes, end_bit, stream_end and CRC-32 at chunk sizes of 1 KiB, 4 KiB and the default -> the results by chunk size"""
    got = {chunk: run(stream, chunk_bytes=chunk, capacity=len(want) + 100) for chunk in (1 * KIB, 4 * KIB, 0)}
    for chunk, r in got.items():
        assert r["data"] == want and r["stream_end"] == 1 and r["crc32"] == zlib.crc32(want) and r["end_bit"] == end_bit, chunk
        assert r["stats"]["out_bytes"] == len(want)
    return got


def test_corpus_raw(forge, scanned):
    """the raw streams through the parallel gunzip: the finder has to find forged headers, and markers have to pass through matches written with deep codes"""
    from bayestyper_amd import lib

    for name, (stream, want) in forge["raw"].items():
        end = df.scan(stream)[2]
        got = check_raw(lib.diag_inflate_raw, stream, want, end)
        for chunk in (1 * KIB, 4 * KIB):
            assert got[chunk]["stats"]["candidates"] >= 1 and got[chunk]["stats"]["links_verified"] >= 1, (name, chunk, got[chunk]["stats"])
        # every non-final forged dynamic header is one the finder takes
        flags = lib.diag_gunzip_plausible(stream)
        assert all(flags[b["start"]] for b in scanned[name][:-1] if b["type"] == 2), name
    for name, payload, data, tags in forge["members"]:
        if "grid" not in tags:
            r = lib.diag_inflate_raw(payload, chunk_bytes=1 * KIB, capacity=len(data) + 100)
            assert r["data"] == data and r["stream_end"] == 1 and r["crc32"] == zlib.crc32(data) and (r["end_bit"] + 7) // 8 == len(payload), name


# ---- single-bit flips ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def flip_cases():
    """[(name, payload, data, [(bit, flipped payload, zlib's class, zlib's bytes)])] for the eight small members: every single-bit flip, judged by zlib once"""
    return [(name, payload, data, [(bit, p) + df.zlib_outcome(p) for bit, p in flipped]) for name, payload, data, flipped in df.small_flips()]


def outcome(run, *args, **kw):
    from bayestyper_amd import lib

    try:
        return "ok", run(*args, **kw)
    except lib.BtError as e:
        return "error", str(e)


def test_flips_as_bgzf(flip_cases):
    """a flipped payload, framed with the sound data's CRC-32 and ISIZE, is taken exactly when zlib consumes the whole payload, reaches the stream's end and
    returns the sound data.  No class of flips is excepted."""
    from bayestyper_amd import lib

    streams = accepted = padding = 0
    for name, payload, data, cases in flip_cases:
        padding += 8 * len(payload) - df.scan(payload)[2]   # the bits behind the final block belong to no code: their flips are accepted, at the least
        for bit, flipped, cls, out in cases:
            got = outcome(lib.diag_bgzf_inflate, df.bgzf_member(flipped, data))
            want = cls == "end" and out == data
            assert (got[0] == "ok") == want and (not want or got[1] == data), (name, bit, cls, got)
            if got[0] == "error":
                assert "BGZF block at offset 0: " in got[1], (name, bit, got)
            streams += 1
            accepted += want
    print("flips as BGZF: %d streams, %d accepted, 0 disagreements" % (streams, accepted))
    assert streams > 13000 and accepted >= padding >= 8


def raw_agrees(got, cls, out):
    """bt_(diag_)inflate_raw's outcome against zlib's for one stream: an error exactly when zlib raises; zlib's bytes and the stream's end where zlib reaches
    it (the call has no frame, so input behind the stream's end is nobody's business); a stop short of the end where zlib runs out of input"""
    if cls in ("end", "trailing"):
        return got[0] == "ok" and got[1]["stream_end"] == 1 and got[1]["data"] == out and got[1]["crc32"] == zlib.crc32(out)
    if cls == "short":
        return got[0] == "ok" and got[1]["stream_end"] == 0
    return got[0] == "error"


def test_flips_raw(flip_cases):
    """the same flips through the parallel gunzip's host run.  DESIGN.md 4.13 lists no deviation that bears on this, and none is excepted."""
    from bayestyper_amd import lib

    classes = {}
    for name, payload, data, cases in flip_cases:
        for bit, flipped, cls, out in cases:
            got = outcome(lib.diag_inflate_raw, flipped, chunk_bytes=1 * KIB, capacity=RAW_CAPACITY)
            assert raw_agrees(got, cls, out), (name, bit, cls, got if got[0] == "error" else (got[1]["stream_end"], len(got[1]["data"])))
            if got[0] == "error":
                assert got[1].startswith("bt_diag_inflate_raw: deflate block at offset "), (name, bit, got)
            classes[cls] = classes.get(cls, 0) + 1
    print("flips raw: %s" % sorted(classes.items()))
    assert sum(classes.values()) > 13000 and len(classes) >= 8


# ---- the header finder -------------------------------------------------------------------------------------------------------------------------------------------
def test_finder_at_every_bit_offset(forge):
    """plausible_header against header_ok over every bit offset of the forged raw streams, a zlib sync-flushed stream and random bytes"""
    from bayestyper_amd import lib

    inputs = dict((name, s) for name, (s, _) in forge["raw"].items())
    inputs["sync_flushed"] = gd.sync_flushed(gd.fastq(31, reads=150), 31, 1500, 3000, final=False)[0]
    inputs["random"] = np.random.default_rng(17).integers(0, 256, size=2500, dtype=np.uint8).tobytes()
    for name, stream in inputs.items():
        want, got = df.header_ok_all(stream), lib.diag_gunzip_plausible(stream)
        assert got.shape == want.shape and not (got != want).any(), (name, np.flatnonzero(got != want)[:10])
        assert name == "random" or want.sum() >= 5, name


def test_finder_on_flipped_and_truncated_headers():
    """offset 0 of four small forged non-final blocks: every single-bit flip inside the first 2 200 bits, every truncation of the first 280 bytes"""
    from bayestyper_amd import lib

    seen = {True: 0, False: 0, "past": 0}
    for stream in df.header_streams():
        assert df.header_ok(stream, 0) == (True, False) and lib.diag_gunzip_plausible(stream, 0, 1)[0] == 1
        cases = [("flip", bit, s) for bit, s in df.flips(stream, 0, 2200)] + [("cut", n, stream[:n]) for n in range(1, min(280, len(stream)) + 1)]
        for what, at, s in cases:
            ok, past = df.header_ok(s, 0)
            assert bool(lib.diag_gunzip_plausible(s, 0, 1)[0]) == ok, (what, at)
            seen[ok] += 1
            seen["past"] += past
    assert seen[True] > 500 and seen[False] > 2000 and seen["past"] > 200, seen


def test_rules_against_zlib():
    """header_ok itself against zlib, once: single-final-block forged streams, so that every error zlib raises belongs to that block; every flip of a header
    bit but BFINAL (not looked at) and the high bit of BTYPE (which makes a stored block, no dynamic header at all).  zlib raises one of its header messages
    exactly when the rules refuse.  The one class left out is a header that runs past the input, which zlib cannot refuse: the rules report it, and zlib
    then says nothing and waits for input."""
    checked = past_end = refused = 0
    for stream in df.header_streams(final=True):
        _, blocks, _ = df.scan(stream)
        assert len(blocks) == 1 and df.header_ok(stream, 0, any_final=True) == (True, False)
        for bit, s in df.flips(stream, 1, blocks[0]["body"] - 1):
            if bit == 2:
                continue
            (ok, past), cls = df.header_ok(s, 0, any_final=True), df.zlib_outcome(s)[0]
            if past:
                assert cls == "short", (bit, cls)
                past_end += 1
                continue
            assert (cls in df.HEADER_MESSAGES) == (not ok), (bit, cls, ok)
            checked += 1
            refused += not ok
    print("rules against zlib: %d flips, %d refused by both, %d headers ran past the input" % (checked, refused, past_end))
    assert checked > 3000 and refused > 500


def test_plausible_arguments():
    from bayestyper_amd import lib

    stream = df.header_streams()[0]
    assert lib.diag_gunzip_plausible(b"").size == 0 and lib.diag_gunzip_plausible(stream, 8 * len(stream), 0).size == 0
    assert list(lib.diag_gunzip_plausible(stream, 0, 3)) == [1, 0, 0]
    with pytest.raises(lib.BtError, match="bt_diag_gunzip_plausible: the bit offsets lie behind the input"):
        lib.diag_gunzip_plausible(stream, 8 * len(stream) - 2, 3)
    with pytest.raises(lib.BtError, match="bt_diag_gunzip_plausible: the bit offsets lie behind the input"):
        lib.diag_gunzip_plausible(stream, 8 * len(stream) + 1, 0)
