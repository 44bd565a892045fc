"""Throughput of the BGZF FASTQ route's device stages on one GPU -> the text of profiles/fastq_bgzf_scan.txt (stdout).

    python tools/fastq_scan.py [--reads 1700000] [--workdir DIR] [--no-cli] [--parent-tools PATH]

Input: a synthetic FASTQ of --reads reads of 150 nt (random bases, qualities from eight values: the reads of profiles/reads_scan.txt and bam_scan.txt)
compressed as BGZF, blocks of 65280 bytes, zlib level 6.  GPU times are event times around one call, a warm-up and three runs, sorted; the figure is the
median.  The end-to-end rows are wall times of `bayesTyperTools makeBloom -r --num-kmers` over the input as one, two and sixteen files, with -p 1 and -p 16,
on the device route and with BT_FASTQ_BGZF_ON_HOST=1 (zlib on the host, the path of the commit before); --parent-tools names a bayesTyperTools built from
that commit, timed on the one-file input to confirm that the switch gives its path."""
import argparse
import concurrent.futures
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
from bayestyper_amd import lib   # noqa: E402

L = 150
BLOCK = 65280
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf_block(data):
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8)
    payload = c.compress(data) + c.flush()
    head = struct.pack("<4BI2BH2BHH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, 6, 66, 67, 2, 18 + len(payload) + 8 - 1)
    return head + payload + struct.pack("<II", zlib.crc32(data), len(data))


def bgzf(data):
    with concurrent.futures.ThreadPoolExecutor(16) as pool:
        return b"".join(pool.map(bgzf_block, (data[i:i + BLOCK] for i in range(0, len(data), BLOCK)))) + EOF


def make_fastq(n, rng):
    """-> (FASTQ rows (n, record bytes) uint8, bases (n, L) ASCII)"""
    bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=(n, L))]
    qual = np.array([2, 11, 25, 37, 37, 37, 37, 40], np.uint8)[rng.integers(0, 8, size=(n, L))]
    fq = np.empty((n, 3 + L + 3 + L + 1), np.uint8)
    fq[:, :3] = np.frombuffer(b"@r\n", np.uint8)
    fq[:, 3:3 + L] = bases
    fq[:, 3 + L:6 + L] = np.frombuffer(b"\n+\n", np.uint8)
    fq[:, 6 + L:6 + 2 * L] = qual + 33
    fq[:, -1] = 10
    return fq, bases


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
    ap.add_argument("--parent-tools", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    t0 = time.perf_counter()
    fq, bases = make_fastq(args.reads, rng)
    data = fq.tobytes()
    stream = bgzf(data)
    n_bases = args.reads * L
    print(f"input: {args.reads} reads of {L} nt = {n_bases} bases; FASTQ {len(data)} bytes, {len(stream)} bytes BGZF (zlib level 6, blocks of {BLOCK}); "
          f"built in {time.perf_counter() - t0:.1f} s", flush=True)
    ctx = lib.Ctx(0)
    print("device:", ctx.info())
    a = np.frombuffer(stream, np.uint8)
    blocks, used, total = lib.bgzf_scan_blocks(a)
    assert used == a.size and total == len(data)

    # (1) bt_fastq_reads_text alone, text resident
    d_raw, d_text = ctx.to_device(np.frombuffer(data, np.uint8)), ctx.buffer(total)
    n, used, st = C.c_uint64(), C.c_uint64(), lib.FastqStats()
    ms = gpu_times(ctx, lambda: lib.check(lib.bt_fastq_reads_text(ctx.h, d_raw.ptr, total, 1, 1, d_text.ptr, total, C.byref(n), C.byref(used), C.byref(st))))
    text = d_text.download(np.uint8, n.value)
    want = np.full((args.reads, L + 1), 10, np.uint8)
    want[:, :L] = bases
    assert used.value == total and st.reads == args.reads and st.lines == 4 * args.reads and np.array_equal(text, want.reshape(-1)), "text differs"
    print(f"bt_fastq_reads_text (device, text resident; tiles + scan + lines + measure + offsets + emit, two host round trips): {ms} ms  median {n_bases / ms[1] / 1e6:.2f} Gbases/s "
          f"({total / ms[1] / 1e6:.2f} GB/s of FASTQ)   [bt_bam_reads_text: 44 Gbases/s, bt_reads_count: 58 Gbases/s (profiles/bam_scan.txt, reads_scan.txt)]", flush=True)

    # (2) the stream object: host blocks -> device text, slabs of 16 MiB of BGZF
    slab = 16 << 20
    cuts = [0]
    for b in blocks:
        if int(b["in_offset"]) + int(b["in_size"]) - cuts[-1] > slab:
            cuts.append(int(b["in_offset"]))
    cuts.append(a.size)

    def stream_all(consume):
        scan = lib.FastqScan(ctx, slab)
        got = 0
        for lo, hi in zip(cuts, cuts[1:]):
            d, m, s = scan.text(a[lo:hi])
            got += s["bases"]
            consume(d, m)
        d, m, s = scan.finish()
        got += s["bases"]
        scan.close()
        ctx.sync()
        assert got == n_bases

    ms = wall_times(lambda: stream_all(lambda d, m: None))
    print(f"bt_fastq_scan_text, {len(cuts) - 1} slabs of <= 16 MiB (memcpy to pinned + H2D + inflate + text, one after the other): {[round(x, 1) for x in ms]} ms wall  "
          f"median {n_bases / ms[1] / 1e6:.2f} Gbases/s", flush=True)
    for x in (d_raw, d_text):
        x.free()
    ctx.close()
    if args.no_cli:
        return

    # (3) end to end through bayesTyperTools makeBloom -r --num-kmers: one, two and sixteen files; -p 1 and -p 16; device route and host route
    tools = os.path.join(ROOT, "bayestyper_amd", "bayesTyperTools")
    with tempfile.TemporaryDirectory(dir=args.workdir) as d:
        for files in (1, 2, 16):
            per = -(-args.reads // files)
            names = []
            for i in range(files):
                names.append(f"s{files}_{i}.fq.gz")
                open(os.path.join(d, names[-1]), "wb").write(stream if files == 1 else bgzf(fq[i * per:(i + 1) * per].tobytes()))
            open(os.path.join(d, f"f{files}.reads"), "w").write("".join(x + "\n" for x in names))

        def timed(exe, files, threads, env):
            ts = []
            for _ in range(3):
                t = time.perf_counter()
                r = subprocess.run([exe, "makeBloom", "-r", os.path.join(d, f"f{files}"), "-p", str(threads), "--num-kmers", str(args.reads * (L - 54))], capture_output=True, text=True,
                                   env=dict(os.environ, **env))
                ts.append(time.perf_counter() - t)
                assert r.returncode == 0 and f"of {args.reads} reads in {files} file(s)" in r.stdout, r.stdout[-2000:] + r.stderr
            return sorted(ts)

        filters = {}
        for files in (1, 2, 16):
            for threads in (1, 16):
                for route, env in (("device", {}), ("host (BT_FASTQ_BGZF_ON_HOST=1)", {"BT_FASTQ_BGZF_ON_HOST": "1"})):
                    ts = timed(tools, files, threads, env)
                    filters[(files, route)] = [open(os.path.join(d, f"f{files}" + e), "rb").read() for e in (".bloomMeta", ".bloomData")]
                    print(f"makeBloom -r --num-kmers, {files:2d} file(s), -p {threads:2d}, {route:32s}: {[round(x, 2) for x in ts]} s wall (process start, context, filter create and save "
                          f"included)  median {ts[1]:.2f} s = {n_bases / ts[1] / 1e9:.3f} Gbases/s", flush=True)
        print("filter bytes equal over all inputs and routes:", all(v == filters[(1, "device")] for v in filters.values()))
        if args.parent_tools:
            for threads in (1, 16):
                ts = timed(args.parent_tools, 1, threads, {})
                print(f"the commit before (its own bayesTyperTools), 1 file, -p {threads:2d}: {[round(x, 2) for x in ts]} s wall  median {ts[1]:.2f} s", flush=True)
        else:
            print("the commit before on the one-file input: NOT measured (no --parent-tools given)")


if __name__ == "__main__":
    main()
