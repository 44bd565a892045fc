"""Throughput of the gzip FASTQ route (one long gzip member inflated on the device) on one GPU -> the text of profiles/fastq_gzip_scan.txt (stdout).

    BT_GUNZIP_STAGE_TIMES=1 python tools/gunzip_scan.py [--reads 1700000] [--workdir DIR] [--no-cli]

Input: the synthetic FASTQ of tools/fastq_scan.py (--reads reads of 150 nt, random bases, qualities from eight values) as ONE gzip member, zlib level 6.
GPU times are event times around one call, a warm-up and three runs, sorted; the figure is the median.  In the same run: the same data as BGZF through
bt_bgzf_inflate, and host zlib on one thread.  Per stage: the wall seconds the library sums (bt_diag_gunzip_stage_seconds) over one further call; with
BT_GUNZIP_STAGE_TIMES set the windows and resolve stages are told apart.  The end-to-end rows are wall times of `bayesTyperTools makeBloom -r --num-kmers`
over the input as one file and as sixteen, with -p 1 and -p 16, with BT_FASTQ_GZIP_ON_DEVICE=1 and without it (zlib on the host: the route of the commit
before)."""
import argparse
import ctypes as C
import os
import struct
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bayestyper_amd import lib   # noqa: E402
from fastq_scan import L, bgzf, gpu_times, make_fastq   # noqa: E402


def gzip_member(data):
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8)
    return bytes.fromhex("1f8b08000000000000ff") + c.compress(data) + c.flush() + struct.pack("<II", zlib.crc32(data), len(data) & 0xFFFFFFFF)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_700_000)
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--no-cli", action="store_true")
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    t0 = time.perf_counter()
    fq, _ = make_fastq(args.reads, rng)
    data = fq.tobytes()
    member = gzip_member(data)
    n_bases = args.reads * L
    print(f"input: {args.reads} reads of {L} nt = {n_bases} bases; FASTQ {len(data)} bytes, {len(member)} bytes as one gzip member (zlib level 6); built in "
          f"{time.perf_counter() - t0:.1f} s; expansion budget {lib.GUNZIP_EXPAND} symbols per compressed byte, default chunk_bytes {lib.GUNZIP_DEFAULT_CHUNK}", flush=True)
    ctx = lib.Ctx(0)
    print("device:", ctx.info())

    # (1) host zlib on one thread
    ts = []
    for _ in range(3):
        t = time.perf_counter()
        out = zlib.decompress(member, 31)
        ts.append(time.perf_counter() - t)
    assert out == data
    del out
    ts.sort()
    print(f"host zlib, one thread: {[round(x, 2) for x in ts]} s  median {len(data) / ts[1] / 1e9:.3f} GB/s of data", flush=True)

    # (2) bt_inflate_raw over the member's deflate stream (resident) in calls of 64 MiB of input, each resumed from end_bit with the window, over chunk_bytes
    raw = np.frombuffer(member, np.uint8)[10:-8]
    piece = 64 << 20
    cap = min(len(data), 1 << 30)
    d_raw, d_out, d_win = ctx.to_device(raw), ctx.buffer(cap + 64), ctx.buffer(32768)
    n, end, fin, crc, st = C.c_uint64(), C.c_uint64(), C.c_int(), C.c_uint32(), lib.GunzipStats()

    def whole(chunk, check_bytes=False):
        """the whole stream: calls of at most `piece` input bytes, each from the last end_bit, the window copied from the output's end"""
        at_bit, total, known, sums = 0, 0, 0, {}
        while True:
            first = at_bit >> 3
            size = min(piece, raw.size - first)
            lib.check(lib.bt_inflate_raw(ctx.h, d_raw.ptr + first, size, at_bit & 7, d_win.ptr if known else None, known, chunk, d_out.ptr, cap, C.byref(n), C.byref(end), C.byref(fin),
                                         C.byref(crc), C.byref(st)))
            for k, v in lib.parse_gunzip_stats(st).items():
                sums[k] = sums.get(k, 0) + v
            if check_bytes and n.value:
                assert d_out.download(np.uint8, n.value).tobytes() == data[total:total + n.value], "bytes differ"
            if n.value:
                known = min(32768, n.value)
                lib.check(lib.bt_memcpy_d2d(ctx.h, d_win.ptr, d_out.ptr + n.value - known, known))
            total += n.value
            at_bit = first * 8 + end.value
            if fin.value:
                break
            assert n.value, "no progress"
        assert total == len(data)
        return sums

    whole(lib.GUNZIP_DEFAULT_CHUNK, check_bytes=True)
    for chunk in (8 << 10, 16 << 10, 32 << 10, 64 << 10, 128 << 10, 256 << 10, 512 << 10, 1 << 20):
        ms = gpu_times(ctx, lambda: whole(chunk))
        lib.gunzip_stage_seconds(reset=True)
        sums = whole(chunk)
        stage = lib.gunzip_stage_seconds(reset=True)
        share = sum(stage.values()) or 1.0
        print(f"bt_inflate_raw, chunk_bytes {chunk >> 10:5d} KiB (input resident): {[round(x, 1) for x in ms]} ms  median {len(data) / ms[1] / 1e6:.2f} GB/s of data; "
              f"rounds {sums['rounds']} candidates {sums['candidates']} links verified {sums['links_verified']} broken {sums['links_broken']} blocks {sums['blocks']}; "
              + "stage shares " + " ".join(f"{k} {100 * v / share:.0f}%" for k, v in stage.items()), flush=True)

    # (3) the same data as BGZF through bt_bgzf_inflate
    stream = np.frombuffer(bgzf(data), np.uint8)
    blocks, used, total = lib.bgzf_scan_blocks(stream)
    assert used == stream.size and total == len(data)
    d_in, d_tab = ctx.to_device(stream), ctx.to_device(blocks)
    ms = gpu_times(ctx, lambda: lib.check(lib.bt_bgzf_inflate(ctx.h, d_in.ptr, stream.size, d_tab.ptr, blocks.size, d_out.ptr, cap, total, 0)))
    print(f"bt_bgzf_inflate, the same data as {blocks.size} BGZF blocks (input resident): {[round(x, 1) for x in ms]} ms  median {len(data) / ms[1] / 1e6:.2f} GB/s of data", flush=True)
    for x in (d_raw, d_in, d_tab, d_out, d_win):
        x.free()
    ctx.close()
    if args.no_cli:
        return

    # (4) end to end: makeBloom -r --num-kmers on one file and on sixteen, -p 1 and -p 16, the switch on and off
    tools = os.path.join(ROOT, "bayestyper_amd", "bayesTyperTools")
    with tempfile.TemporaryDirectory(dir=args.workdir) as d:
        for files in (1, 16):
            per = -(-args.reads // files)
            names = []
            for i in range(files):
                names.append(f"s{files}_{i}.fq.gz")
                open(os.path.join(d, names[-1]), "wb").write(member if files == 1 else gzip_member(fq[i * per:(i + 1) * per].tobytes()))
            open(os.path.join(d, f"f{files}.reads"), "w").write("".join(x + "\n" for x in names))
        filters = {}
        for files in (1, 16):
            for threads in (1, 16):
                for route, env in (("switch on (device)", {"BT_FASTQ_GZIP_ON_DEVICE": "1"}), ("switch off (host zlib)", {})):
                    ts = []
                    for _ in range(3):
                        t = time.perf_counter()
                        r = subprocess.run([tools, "makeBloom", "-r", os.path.join(d, f"f{files}"), "-p", str(threads), "--num-kmers", str(args.reads * (L - 54))], capture_output=True,
                                           text=True, env=dict(os.environ, **env))
                        ts.append(time.perf_counter() - t)
                        assert r.returncode == 0 and f"of {args.reads} reads in {files} file(s)" in r.stdout, r.stdout[-2000:] + r.stderr
                    ts.sort()
                    filters[(files, threads, route)] = [open(os.path.join(d, f"f{files}" + e), "rb").read() for e in (".bloomMeta", ".bloomData")]
                    print(f"makeBloom -r --num-kmers, {files:2d} file(s), -p {threads:2d}, {route:22s}: {[round(x, 2) for x in ts]} s wall (process start, context, filter create and save "
                          f"included)  median {ts[1]:.2f} s = {n_bases / ts[1] / 1e9:.3f} Gbases/s", flush=True)
        print("filter bytes equal over all inputs and routes:", all(v == filters[(1, 1, "switch off (host zlib)")] for v in filters.values()))


if __name__ == "__main__":
    main()
