"""The bytes of the two device compressors, pinned: tests/golden/gz_byte_pin.json holds SHA-256 digests of bt_diag_deflate's and bt_diag_bgzf's streams (and
the BGZF block offsets) recorded by tests/golden/make_gz_byte_pin.py from the library as it was BEFORE the gzip and BGZF pipelines were folded into
csrc/bt_gz_pipeline.hpp.  The input's digest is asserted first, so that a change of the input generators is told apart from a change of the compressor."""
import json
import os
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)

import make_gz_byte_pin as mk  # noqa: E402

from bayestyper_amd import lib  # noqa: E402

with open(os.path.join(GOLDEN, "gz_byte_pin.json")) as f:
    PIN = json.load(f)


def test_every_case_is_pinned():
    assert set(PIN["deflate"]) == set(mk.deflate_cases()) and len(PIN["deflate"]) == 19
    assert set(PIN["bgzf"]) == set(mk.bgzf_cases()) and len(PIN["bgzf"]) == 30


@pytest.mark.parametrize("name", sorted(PIN["deflate"]))
def test_deflate_bytes(name):
    data, want = mk.deflate_cases()[name], PIN["deflate"][name]
    assert mk.sha(data) == want["input"], "the input generator changed, not the compressor"
    assert mk.sha(lib.diag_deflate(data, True)[0]) == want["last"]
    assert mk.sha(lib.diag_deflate(data, False)[0]) == want["open"]


@pytest.mark.parametrize("name", sorted(PIN["bgzf"]))
def test_bgzf_bytes_and_offsets(name):
    data, want = mk.bgzf_cases()[name], PIN["bgzf"][name]
    assert mk.sha(data) == want["input"], "the input generator changed, not the compressor"
    stream, offsets, _ = lib.diag_bgzf(data, True)
    assert mk.sha(stream) == want["eof"] and offsets == want["offsets"]
    stream, offsets, _ = lib.diag_bgzf(data, False)
    assert mk.sha(stream) == want["open"] and offsets == want["open_offsets"]
