"""Frozen digests of the host runs of the two device compressors, bt_diag_deflate and bt_diag_bgzf, over the inputs of tests/test_deflate_cpu.py and
tests/test_bgzf_cpu.py: per case the SHA-256 of the input, the SHA-256 of the stream with the closing flag (last / eof) set and unset, and for BGZF the
block offsets.  tests/test_gz_byte_pin_cpu.py recomputes them.

THE COMMITTED FILE WAS WRITTEN ON THE PARENT of the change that folded the gzip and BGZF pipelines into csrc/bt_gz_pipeline.hpp, from a libbtgpu.so built
before that code was touched: it pins the bytes across that refactor.  Run it again only for a change that is meant to alter the compressor's bytes.

usage: python tests/golden/make_gz_byte_pin.py     (rewrites tests/golden/gz_byte_pin.json)"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def sha(data):
    return hashlib.sha256(data).hexdigest()


def deflate_cases():
    """name -> bytes: every entry of _deflate_inputs.inputs(), and interleaved()"""
    import _deflate_inputs as D

    cases = dict(D.inputs())
    cases["interleaved"] = D.interleaved()
    return cases


def bgzf_cases():
    """"kind n" -> bytes: test_bgzf_cpu.KINDS x _bgzf.SIZES"""
    import _bgzf as B
    from test_bgzf_cpu import KINDS, content

    return {"%s %d" % (kind, n): content(kind, n) for kind in KINDS for n in B.SIZES}


def deflate_entry(lib, data):
    return dict(input=sha(data), last=sha(lib.diag_deflate(data, True)[0]), open=sha(lib.diag_deflate(data, False)[0]))


def bgzf_entry(lib, data):
    stream, offsets, _ = lib.diag_bgzf(data, True)
    open_stream, open_offsets, _ = lib.diag_bgzf(data, False)
    return dict(input=sha(data), eof=sha(stream), open=sha(open_stream), offsets=offsets, open_offsets=open_offsets)


if __name__ == "__main__":
    from bayestyper_amd import lib

    out = dict(deflate={name: deflate_entry(lib, data) for name, data in deflate_cases().items()},
               bgzf={name: bgzf_entry(lib, data) for name, data in bgzf_cases().items()})
    dst = os.path.join(HERE, "gz_byte_pin.json")
    with open(dst, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", dst, os.path.getsize(dst), "bytes,", len(out["deflate"]), "+", len(out["bgzf"]), "cases")
