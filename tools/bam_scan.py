"""Throughput of the BAM route's device stages on one GPU -> the text of profiles/bam_scan.txt (stdout).

    python tools/bam_scan.py [--reads 1700000] [--workdir DIR] [--no-cli]

Input: a synthetic BAM of --reads unmapped reads of 150 nt (random bases, qualities from eight values), BGZF blocks of 65280 bytes, zlib level 6 — the
shape of profiles/reads_scan.txt.  GPU times are event times around one call, a warm-up and three runs, sorted; the figure is the median.  Host zlib runs
over the same blocks in the same process.  The end-to-end rows are wall times of `bayesTyperTools makeBloom -r` over the BAM and over its .fastq.gz twin."""
import argparse
import concurrent.futures
import ctypes as C
import gzip
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
from bayestyper_amd import lib   # noqa: E402

L = 150
BLOCK = 65280


def bgzf_block(data):
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8)
    payload = c.compress(data) + c.flush()
    head = struct.pack("<4BI2BH2BHH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, 6, 66, 67, 2, 18 + len(payload) + 8 - 1)
    return head + payload + struct.pack("<II", zlib.crc32(data), len(data))


def make_bam(n, rng):
    """-> (BGZF stream, header bytes, bases (n, L) ASCII, qualities (n, L))"""
    bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=(n, L))]
    qual = np.array([2, 11, 25, 37, 37, 37, 37, 40], np.uint8)[rng.integers(0, 8, size=(n, L))]
    name = b"r\0"
    fixed = struct.pack("<IiiBBHHHiiii", 32 + len(name) + L // 2 + L, -1, -1, len(name), 0, 4680, 0, 4, L, -1, -1, 0) + name
    rec = np.empty((n, len(fixed) + L // 2 + L), np.uint8)
    rec[:, :len(fixed)] = np.frombuffer(fixed, np.uint8)
    code = np.zeros(256, np.uint8)
    code[[65, 67, 71, 84]] = [1, 2, 4, 8]
    nib = code[bases]
    rec[:, len(fixed):len(fixed) + L // 2] = nib[:, 0::2] << 4 | nib[:, 1::2]
    rec[:, len(fixed) + L // 2:] = qual
    header = b"BAM\1" + struct.pack("<i", 0) + struct.pack("<i", 0)
    data = header + rec.tobytes()
    with concurrent.futures.ThreadPoolExecutor(16) as pool:
        blocks = list(pool.map(bgzf_block, (data[i:i + BLOCK] for i in range(0, len(data), BLOCK))))
    eof = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    return b"".join(blocks) + eof, len(header), bases, qual, len(data)


def gpu_times(ctx, call, runs=3):
    timer = lib.Timer(ctx)
    call()   # warm-up
    ctx.sync()
    out = []
    for _ in range(runs):
        timer.start()
        call()
        timer.stop()
        out.append(timer.elapsed_ms())
    timer.close()
    return sorted(out)


def wall_times(call, runs=3):
    call()
    out = []
    for _ in range(runs):
        t = time.perf_counter()
        call()
        out.append((time.perf_counter() - t) * 1e3)
    return sorted(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_700_000)
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--no-cli", action="store_true")
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    t0 = time.perf_counter()
    stream, head, bases, qual, raw_bytes = make_bam(args.reads, rng)
    n_bases = args.reads * L
    print(f"input: {args.reads} reads of {L} nt = {n_bases} bases; BAM {raw_bytes} bytes inflated, {len(stream)} bytes BGZF (zlib level 6, blocks of {BLOCK}); "
          f"built in {time.perf_counter() - t0:.1f} s")
    ctx = lib.Ctx(0)
    print("device:", ctx.info())
    a = np.frombuffer(stream, np.uint8)
    blocks, used, total = lib.bgzf_scan_blocks(a)
    assert used == a.size and total == raw_bytes
    print(f"blocks: {len(blocks)}; bt_bgzf_scan_blocks (host, one thread): {wall_times(lambda: lib.bgzf_scan_blocks(a))[1]:.2f} ms")

    # (1) bt_bgzf_inflate alone, blocks resident
    d_in, d_tab, d_raw = ctx.to_device(a), ctx.to_device(blocks), ctx.buffer(total)
    ms = gpu_times(ctx, lambda: lib.check(lib.bt_bgzf_inflate(ctx.h, d_in.ptr, a.size, d_tab.ptr, blocks.size, d_raw.ptr, total, total, 0)))
    raw = d_raw.download(np.uint8, total)
    print(f"bt_bgzf_inflate (device, blocks resident): {ms} ms  median {total / ms[1] / 1e6:.2f} GB/s of inflated data ({len(stream) / ms[1] / 1e6:.2f} GB/s of BGZF)")
    payloads = [stream[int(b['in_offset']) + 18:int(b['in_offset']) + int(b['in_size']) - 8] for b in blocks]

    def host_inflate(threads):
        if threads == 1:
            return [zlib.decompress(p, -15) for p in payloads]
        with concurrent.futures.ThreadPoolExecutor(threads) as pool:
            return list(pool.map(lambda p: zlib.decompress(p, -15), payloads))

    assert b"".join(host_inflate(16)) == raw.tobytes(), "device inflate differs from zlib"
    for threads in (1, 16):
        ms_h = wall_times(lambda: host_inflate(threads))
        print(f"host zlib inflate of the same blocks, {threads:2d} thread(s): {[round(x, 1) for x in ms_h]} ms  median {total / ms_h[1] / 1e6:.2f} GB/s of inflated data")

    # (2) bt_bam_reads_text alone, records resident
    d_text = ctx.buffer(total)
    n, used, st = C.c_uint64(), C.c_uint64(), lib.BamStats()
    ms = gpu_times(ctx, lambda: lib.check(lib.bt_bam_reads_text(ctx.h, d_raw.ptr + head, total - head, 0x900, d_text.ptr, total, C.byref(n), C.byref(used), C.byref(st))))
    text = d_text.download(np.uint8, n.value)
    want = np.full((args.reads, L + 1), 10, np.uint8)
    want[:, :L] = bases
    assert used.value == total - head and st.kept == args.reads and np.array_equal(text, want.reshape(-1)), "text differs"
    print(f"bt_bam_reads_text (device, records resident; guess + stitch + fill + measure + offsets + emit, two host round trips): {ms} ms  median {n_bases / ms[1] / 1e6:.2f} Gbases/s "
          f"({(total - head) / ms[1] / 1e6:.2f} GB/s of records)")

    # (3) the stream object: host blocks -> device text, slabs of 16 MiB of BGZF
    slab = 16 << 20
    cuts = [0]
    for b in blocks:
        if int(b["in_offset"]) + int(b["in_size"]) - cuts[-1] > slab:
            cuts.append(int(b["in_offset"]))
    cuts.append(a.size)

    def stream_all(consume):
        scan = lib.BamScan(ctx, slab)
        got = 0
        for i, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
            d, m, s = scan.text(a[lo:hi], head if i == 0 else 0)
            got += s["bases"]
            consume(d, m)
        scan.finish()
        scan.close()
        ctx.sync()
        assert got == n_bases

    ms = wall_times(lambda: stream_all(lambda d, m: None))
    print(f"bt_bam_scan_text, {len(cuts) - 1} slabs of <= 16 MiB (memcpy to pinned + H2D + inflate + text, one after the other): {[round(x, 1) for x in ms]} ms wall  "
          f"median {n_bases / ms[1] / 1e6:.2f} Gbases/s")
    reg = ctx.to_device(np.zeros(lib.SKETCH_REGISTERS, np.uint8))
    ms = wall_times(lambda: stream_all(lambda d, m: lib.check(lib.bt_reads_sketch(ctx.h, d, m, 55, reg.ptr))))
    print(f"bt_bam_scan_text + bt_reads_sketch (k = 55) per slab: {[round(x, 1) for x in ms]} ms wall  median {n_bases / ms[1] / 1e6:.2f} Gbases/s")
    tw = np.frombuffer(want.tobytes(), np.uint8)
    ms = wall_times(lambda: lib.reads_sketch(ctx, tw, 55, host=True))
    print(f"for comparison, the same reads as resident HOST TEXT through bt_reads_sketch_host (memcpy to pinned + H2D + scan, overlapped): {[round(x, 1) for x in ms]} ms wall  "
          f"median {n_bases / ms[1] / 1e6:.2f} Gbases/s")
    for x in (d_in, d_tab, d_raw, d_text, reg):
        x.free()
    ctx.close()
    if args.no_cli:
        return

    # (4) end to end through bayesTyperTools makeBloom -r: the BAM against its .fastq.gz twin (16 files, as in profiles/reads_scan.txt)
    tools = os.path.join(ROOT, "bayestyper_amd", "bayesTyperTools")
    with tempfile.TemporaryDirectory(dir=args.workdir) as d:
        open(os.path.join(d, "s.bam"), "wb").write(stream)
        open(os.path.join(d, "bam.reads"), "w").write("s.bam\n")
        fq = np.empty((args.reads, 3 + L + 3 + L + 1), np.uint8)
        fq[:, :3] = np.frombuffer(b"@r\n", np.uint8)
        fq[:, 3:3 + L] = bases
        fq[:, 3 + L:6 + L] = np.frombuffer(b"\n+\n", np.uint8)
        fq[:, 6 + L:6 + 2 * L] = qual + 33
        fq[:, -1] = 10
        per = -(-args.reads // 16)
        parts = [fq[i * per:(i + 1) * per].tobytes() for i in range(16)]
        with concurrent.futures.ThreadPoolExecutor(16) as pool:
            gz = list(pool.map(lambda p: gzip.compress(p, compresslevel=6), parts))
        for i, g in enumerate(gz):
            open(os.path.join(d, f"s_{i}.fq.gz"), "wb").write(g)
        open(os.path.join(d, "gz.reads"), "w").write("".join(f"s_{i}.fq.gz\n" for i in range(16)))
        print(f"files: s.bam {len(stream)} bytes; 16 x .fastq.gz (gzip -6) {sum(map(len, gz))} bytes")
        for tag, threads in (("bam", 16), ("gz", 16), ("bam", 1), ("gz", 1)):
            for mode, extra in (("one pass (--num-kmers)", ["--num-kmers", str(args.reads * (L - 54))]), ("sketch pass + filter pass", [])):
                ts = []
                for _ in range(3):
                    t = time.perf_counter()
                    r = subprocess.run([tools, "makeBloom", "-r", os.path.join(d, tag), "-p", str(threads)] + extra, capture_output=True, text=True)
                    ts.append(time.perf_counter() - t)
                    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
                ts.sort()
                print(f"makeBloom -r {tag:3s} -p {threads:2d} {mode:26s}: {[round(x, 2) for x in ts]} s wall (process start, context, filter create and save included)  "
                      f"median {n_bases / ts[1] / 1e9:.3f} Gbases/s")
        same = all(open(os.path.join(d, "bam" + e), "rb").read() == open(os.path.join(d, "gz" + e), "rb").read() for e in (".bloomMeta", ".bloomData"))
        print("filter bytes of the BAM and of its twin equal:", same)


if __name__ == "__main__":
    main()
