"""The reads pack on one GPU -> the text of profiles/reads_pack.txt (stdout).

    python tools/reads_pack_scan.py [--files 16] [--reads-per-file 400000] [--threads 16] [--workdir DIR] [--no-cli]

Input: the synthetic FASTQ of tools/fastq_scan.py (reads of 150 nt, random bases) in --files files, once plain and once as `gzip -1` members.
(1) Resident data: the three consumers over the packed reads against the same three over the reads text — the same reads, event times around one call, a
    warm-up and three runs, sorted; the figure is the median.  Also bt_reads_pack and bt_reads_unpack themselves.
(2) End to end: wall times of the two-pass `bayesTyperTools makeBloom -r` (sketch pass, then filter pass), three rounds, the routes alternating within a round:
    without the variable and without a pack; BT_READS_PACK=1 on a first run, which writes the pack in the sketch pass and reads it in the filter pass; a second
    run, which reads it in both.  Process start, context, filter create and save are included in every figure.
`genotype`'s reads row is printed by `bayesTyper genotype` itself under BT_STAGE_TIMES ("parse sample k-mers (reads route) ... (from the reads pack)"); this
tool builds no candidate set and does not time it."""
import argparse
import concurrent.futures
import os
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
from fastq_scan import L, gpu_times, make_fastq   # noqa: E402

K = 55


def gzip1(data):
    c = zlib.compressobj(1, zlib.DEFLATED, 31)
    return c.compress(data) + c.flush()


def resident(ctx, bases):
    """bases (n, L) ASCII -> the rows of part (1)"""
    n = len(bases)
    text = np.full((n, L + 1), 10, np.uint8)
    text[:, :L] = bases
    text = text.reshape(-1)
    packed = lib.diag_reads_pack(text)
    d_text, d_packed = ctx.to_device(text), ctx.to_device(packed)
    d_out, d_back = ctx.buffer(packed.size), ctx.buffer(text.size)
    rate = lambda ms: n * L / ms / 1e6   # noqa: E731  (Gbases/s)
    ms = gpu_times(ctx, lambda: lib.check(lib.bt_reads_pack(ctx.h, d_text.ptr, text.size, d_out.ptr)))
    assert np.array_equal(d_out.download(np.uint8, packed.size), packed)
    print(f"bt_reads_pack   ({text.size} bytes -> {packed.size}): {[round(x, 2) for x in ms]} ms  median {rate(ms[1]):.1f} Gbases/s = {(text.size + packed.size) / ms[1] / 1e6:.0f} GB/s moved")
    ms = gpu_times(ctx, lambda: lib.check(lib.bt_reads_unpack(ctx.h, d_packed.ptr, text.size, d_back.ptr)))
    assert np.array_equal(d_back.download(np.uint8, text.size), text)
    print(f"bt_reads_unpack ({packed.size} bytes -> {text.size}): {[round(x, 2) for x in ms]} ms  median {rate(ms[1]):.1f} Gbases/s")
    distinct = n * (L - K + 1)
    d_reg = ctx.buffer(lib.SKETCH_REGISTERS)
    results = {}
    for route in ("text", "packed"):
        size = text.size
        call_sketch = (lambda: lib.check(lib.bt_reads_sketch(ctx.h, d_text.ptr, size, K, d_reg.ptr))) if route == "text" else (
            lambda: lib.check(lib.bt_reads_sketch_packed(ctx.h, d_packed.ptr, size, K, d_reg.ptr)))
        d_reg.zero()
        ms = gpu_times(ctx, call_sketch)
        results[("sketch", route)] = d_reg.download(np.uint8, lib.SKETCH_REGISTERS)
        print(f"sketch, {route:6s} input resident: {[round(x, 2) for x in ms]} ms  median {rate(ms[1]):.1f} Gbases/s")
        bloom = lib.Bloom.create(ctx, distinct, 1e-3, K, threaded=False)
        call_bloom = (lambda: lib.check(lib.bt_reads_make_bloom(ctx.h, bloom.h, d_text.ptr, size, K))) if route == "text" else (
            lambda: lib.check(lib.bt_reads_make_bloom_packed(ctx.h, bloom.h, d_packed.ptr, size, K)))
        ms = gpu_times(ctx, call_bloom)
        results[("bloom", route)] = bloom.bits(0)
        print(f"bloom,  {route:6s} input resident: {[round(x, 2) for x in ms]} ms  median {rate(ms[1]):.1f} Gbases/s")
        # count: a path filter of a hundredth of the reads' k-mers, an S = 1 table
        path = lib.Bloom.create(ctx, max(distinct // 100, 1), 1e-3, K, threaded=False)
        lib.check(lib.bt_reads_make_bloom(ctx.h, path.h, d_text.ptr, size // 100, K))
        table = lib.Table(ctx, distinct // 50 + 1024, 1, K)
        d_hits = ctx.buffer(8).zero()
        call_count = (lambda: lib.check(lib.bt_reads_count(ctx.h, path.h, table.h, 0, d_text.ptr, size, d_hits.ptr))) if route == "text" else (
            lambda: lib.check(lib.bt_reads_count_packed(ctx.h, path.h, table.h, 0, d_packed.ptr, size, d_hits.ptr)))
        ms = gpu_times(ctx, call_count)
        results[("count", route)] = (int(d_hits.download(np.uint64, 1)[0]), table.status())
        print(f"count,  {route:6s} input resident: {[round(x, 2) for x in ms]} ms  median {rate(ms[1]):.1f} Gbases/s  (hits {results[('count', route)][0]})")
        for x in (bloom, path, table):
            x.close()
        d_hits.free()
    print("registers equal:", np.array_equal(results[("sketch", "text")], results[("sketch", "packed")]), " filter bytes equal:",
          np.array_equal(results[("bloom", "text")], results[("bloom", "packed")]), " hits and table status equal:", results[("count", "text")] == results[("count", "packed")])
    for x in (d_text, d_packed, d_out, d_back, d_reg):
        x.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--reads-per-file", type=int, default=400_000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--no-cli", action="store_true")
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    t0 = time.perf_counter()
    fq, bases = make_fastq(args.reads_per_file, rng)   # one file's reads; the other files hold the same records with the bases rolled, so every file differs
    reads = args.files * args.reads_per_file
    print(f"input: {args.files} files of {args.reads_per_file} reads of {L} nt = {reads * L} bases, k {K}; built in {time.perf_counter() - t0:.1f} s", flush=True)
    ctx = lib.Ctx(0)
    print("device:", ctx.info())
    resident(ctx, bases)
    ctx.close()
    if args.no_cli:
        return
    tools = os.path.join(ROOT, "bayestyper_amd", "bayesTyperTools")
    with tempfile.TemporaryDirectory(dir=args.workdir) as d:
        def one(i):
            rows = fq.copy()
            rows[:, 3:3 + L] = np.roll(bases, 7 * i + 1, axis=1) if i else bases
            data = rows.tobytes()
            open(os.path.join(d, f"p{i}.fq"), "wb").write(data)
            open(os.path.join(d, f"z{i}.fq.gz"), "wb").write(gzip1(data))
            return len(data)

        t0 = time.perf_counter()
        with concurrent.futures.ThreadPoolExecutor(min(16, args.files)) as pool:
            sizes = list(pool.map(one, range(args.files)))
        for tag, ext in (("plain", "p{}.fq"), ("gzip", "z{}.fq.gz")):
            for route in ("files", "pack"):
                open(os.path.join(d, f"{tag}_{route}.reads"), "w").write("".join(ext.format(i) + "\n" for i in range(args.files)))
        print(f"files written in {time.perf_counter() - t0:.1f} s: {sum(sizes)} bytes of FASTQ, {sum(os.path.getsize(os.path.join(d, f'z{i}.fq.gz')) for i in range(args.files))} as gzip -1", flush=True)
        env0 = {k: v for k, v in os.environ.items() if k != "BT_READS_PACK"}

        def run(prefix, env):
            t = time.perf_counter()
            r = subprocess.run([tools, "makeBloom", "-r", os.path.join(d, prefix), "-p", str(args.threads)], capture_output=True, text=True, env=dict(env0, **env))
            dt = time.perf_counter() - t
            assert r.returncode == 0 and f"of {reads} reads in {args.files} file(s)" in r.stdout, r.stdout[-2000:] + r.stderr
            return dt, [open(os.path.join(d, prefix + e), "rb").read() for e in (".bloomMeta", ".bloomData")]

        for tag in ("plain", "gzip"):
            times = {"no pack, no variable": [], "BT_READS_PACK=1, first run (writes)": [], "pack present, second run (reads)": []}
            filters = []
            for _ in range(3):
                pack = os.path.join(d, f"{tag}_pack.reads.pack")
                if os.path.exists(pack):
                    os.remove(pack)
                dt, f = run(f"{tag}_files", {})
                times["no pack, no variable"].append(dt)
                filters.append(f)
                dt, f = run(f"{tag}_pack", {"BT_READS_PACK": "1"})
                times["BT_READS_PACK=1, first run (writes)"].append(dt)
                filters.append(f)
                dt, f = run(f"{tag}_pack", {})
                times["pack present, second run (reads)"].append(dt)
                filters.append(f)
            for name, ts in times.items():
                ts.sort()
                print(f"makeBloom -r (two passes), {tag:5s} files, -p {args.threads}, {name:36s}: {[round(x, 2) for x in ts]} s wall  median {ts[1]:.2f} s = "
                      f"{reads * L / ts[1] / 1e9:.3f} Gbases/s", flush=True)
            print(f"  pack: {os.path.getsize(os.path.join(d, f'{tag}_pack.reads.pack'))} bytes; filter bytes equal over all nine runs: {all(f == filters[0] for f in filters)}", flush=True)


if __name__ == "__main__":
    main()
