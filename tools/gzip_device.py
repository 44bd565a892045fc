#!/usr/bin/env python3
"""The gz outputs measured (the table under profiles/gzip_device.txt), on a GPU machine from the repository root:

  tools/gzip_device.py <tag> [--genome 256000000 --variants 800000 --samples 3 --error-kmers 560000000 --sv 10] [--runs 3] [--parent DIR] [--out DIR]

One data set (tools/make_c2_dataset.cpp), makeBloom, `bayesTyper cluster` without and with BT_GZIP_ON_DEVICE=1, then `bayesTyper genotype -z` with
BT_STAGE_TIMES=1 <runs> times without the switch (the parent's route: one gzwrite) and <runs> times with it: the "write VCF" row, the wall clock, the file sizes,
and the decompressed VCFs compared.  With --parent (a directory holding the parent build's bayesTyper and libraries) `genotype` without -z runs <runs> times on
the parent's executable and on this build with the switch unset, and every stage's median is set against the parent's median and spread.
Then, on the VCF text and on the parameter k-mer FASTA of that run, in this process: zlib's gzwrite in one call (what GenotypeWriter::finalise does), writeGzFile
at 16 and 32 threads (bth_write_gz), bt_gzip_save split into copies in / kernels / copies out / CRC-32 + writes, and the sizes against zlib levels 1 and 6.
With --bgzf the script measures the BGZF route instead (profiles/bgzf_device.txt): the same data set, `cluster` once, `genotype -z` <runs>
times with BT_GZIP_ON_DEVICE=1 (the parent's device route) and <runs> times with BT_VCF_BGZF=1 — the "write VCF" row, the file sizes, the decompressed VCFs
compared, the .tbi parsed and queried (tests/_bgzf.py) — then the VCF text through bt_gzip_save and bt_bgzf_save in this process, <runs> calls each after a
first one: whole call, copies in, kernels (bt_gzip_save's have no CRC, bt_bgzf_save's compute it), copies out, host part.  With --parent, `genotype` without
and with -z on the parent's executable and on this build, switch unset, into the same output prefix: the files compared byte for byte.
Every child process runs under a time limit; the first failure ends the script."""
import argparse
import ctypes as C
import gzip
import hashlib
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = []


def say(*a):
    line = " ".join(str(x) for x in a)
    OUT.append(line)
    print(line, flush=True)


def run(cmd, limit, env=None, cwd=None, quiet=True):
    """a child under `timeout`; output polled so that the caller's log never falls silent; a failure ends the script"""
    t0 = time.time()
    with tempfile.TemporaryFile() as fo, tempfile.TemporaryFile() as fe:
        p = subprocess.Popen(["timeout", "-k", "10", str(limit)] + cmd, stdout=fo, stderr=fe, env=env, cwd=cwd)
        while p.poll() is None:
            time.sleep(1)
            if int(time.time() - t0) % 60 == 59:
                print("#   ... %s running for %d s" % (os.path.basename(cmd[0]), time.time() - t0), flush=True)
        fo.seek(0), fe.seek(0)
        out, err = fo.read().decode(errors="replace"), fe.read().decode(errors="replace")
    if p.returncode != 0:
        say("FAILED rc", p.returncode, " ".join(cmd[:3]), "\n", out[-1500:], err[-1500:])
        finish(1)
    return out, err, time.time() - t0


def rows(err):
    """the stage table of a run's stderr -> {name: seconds}"""
    return {m.group(1).strip(): float(m.group(2)) for m in re.finditer(r"^(.+?)\s+([0-9.]+) s$", err, re.M)}


def timed(f):
    t0 = time.time()
    r = f()
    return time.time() - t0, r


def finish(rc):
    os.makedirs(ARGS.out, exist_ok=True)
    with open(os.path.join(ARGS.out, ARGS.tag + ("_bgzf_device.txt" if ARGS.bgzf else "_gzip_device.txt")), "w") as f:
        f.write("\n".join(OUT) + "\n")
    sys.exit(rc)


def vcf_body_md5(path):
    h = hashlib.md5()
    with gzip.open(path) as f:
        for line in f:
            if not line.startswith(b"##BayesTyperOptions="):
                h.update(line)
    return h.hexdigest()


def content_table(name, data, threads, ctx, lib, dll, tmp):
    """the same content through every writer, in this process"""
    z = C.CDLL("libz.so.1")
    z.gzopen.restype, z.gzopen.argtypes = C.c_void_p, [C.c_char_p, C.c_char_p]
    z.gzwrite.restype, z.gzwrite.argtypes = C.c_int, [C.c_void_p, C.c_char_p, C.c_uint]
    z.gzclose.restype, z.gzclose.argtypes = C.c_int, [C.c_void_p]
    say("## %s: %d bytes" % (name, len(data)))
    sizes = {}
    if len(data) < (1 << 31):
        path = os.path.join(tmp, "gzwrite.gz")

        def one_gzwrite():
            f = z.gzopen(path.encode(), b"wb")
            assert z.gzwrite(f, data, len(data)) == len(data) and z.gzclose(f) == 0

        for rep in range(ARGS.runs):
            say("gzwrite, one call, one thread (the parent's -z)          %8.3f s" % timed(one_gzwrite)[0])
        sizes["gzwrite (zlib level 6, one stream)"] = os.path.getsize(path)
    for t in (16, 32):
        path = os.path.join(tmp, "writegz_%d.gz" % t)
        for rep in range(ARGS.runs):
            say("writeGzFile, %2d threads (bth_write_gz)                   %8.3f s" % (t, timed(lambda: dll.bth_write_gz(path.encode(), data, len(data), t))[0]))
        sizes["writeGzFile (zlib level 6, 4 MB pieces)"] = os.path.getsize(path)
    path = os.path.join(tmp, "device.gz")
    for rep in range(ARGS.runs + 1):   # the first call also pays the first launch of the kernels
        sec, st = timed(lambda: lib.gzip_save(ctx, path, data, threads))
        say("bt_gzip_save, -p %2d%s  %8.3f s   copies in %.3f  kernels %.3f  copies out %.3f  (device times, overlapping)  staging + CRC-32 + writes %.3f (host)" % (
            threads, " (first call)" if rep == 0 else "             ", sec, st["seconds_h2d"], st["seconds_kernels"], st["seconds_d2h"], st["seconds_host"]))
    sizes["bt_gzip_save (64 KiB pieces)"] = os.path.getsize(path)
    say("   pieces %d, stored %d, literals %d, matches %d, matched bytes %d" % (st["pieces"], st["stored_pieces"], st["literals"], st["matches"], st["matched_bytes"]))
    with gzip.open(path) as f:
        h, n = hashlib.md5(), 0
        for chunk in iter(lambda: f.read(1 << 24), b""):
            h.update(chunk)
            n += len(chunk)
    say("   reads back with gzip: %s" % ("the content" if n == len(data) and h.digest() == hashlib.md5(data).digest() else "DIFFERENT"))
    for level in (1, 6):
        sec, out = timed(lambda: zlib.compress(data, level))
        sizes["zlib level %d, one stream (python, %.1f s)" % (level, sec)] = len(out)
    for k, v in sizes.items():
        say("   size %-48s %12d  %.4f of the content" % (k, v, v / max(len(data), 1)))


def bgzf_tables(d, exe, geno, base_env, T):
    """--bgzf: genotype -z through bt_gzip_save and through bt_bgzf_save, then the VCF text through both in this process"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _bgzf

    routes = (("gzip", dict(base_env, BT_GZIP_ON_DEVICE="1"), "gzip on the device"), ("bgzf", dict(base_env, BT_VCF_BGZF="1"), "BGZF on the device"))
    say("## bayesTyper genotype -z: the write VCF row, the wall clock since main()")
    md5s, write_rows = set(), {"gzip": [], "bgzf": []}
    for rep in range(ARGS.runs):
        for route, env, label in routes:
            prefix = os.path.join(d, "run_" + route)
            for f in (prefix + ".vcf.gz", prefix + ".vcf.gz.tbi"):
                if os.path.exists(f):
                    os.remove(f)
            _, err, wall = run([exe] + geno + ["-o", prefix, "-z"], 900, env=env)
            r = rows(err)
            key = [k for k in r if k.startswith("write VCF")]
            assert len(key) == 1 and label in key[0], key
            write_rows[route].append(r[key[0]])
            md5s.add(vcf_body_md5(prefix + ".vcf.gz"))
            tbi = prefix + ".vcf.gz.tbi"
            say("run %d %-5s %-62s %8.3f s   wall since main() %8.3f s   .vcf.gz %d bytes%s" % (
                rep + 1, route, key[0], r[key[0]], r["wall since main()"], os.path.getsize(prefix + ".vcf.gz"), "   .tbi %d bytes" % os.path.getsize(tbi) if os.path.exists(tbi) else ""))
    say("decompressed VCFs of all %d runs (without the options line): %s" % (2 * ARGS.runs, "identical" if len(md5s) == 1 else "DIFFER"))
    for route in ("gzip", "bgzf"):
        w = write_rows[route]
        say("write VCF, %s route: median %.3f s (%.3f .. %.3f)" % (route, statistics.median(w), min(w), max(w)))
    # the BGZF file and its index read back by the specification's rules
    raw = open(os.path.join(d, "run_bgzf.vcf.gz"), "rb").read()
    text = gzip.decompress(raw)
    t0 = time.time()
    blocks = _bgzf.walk(raw)
    assert raw[-28:] == _bgzf.EOF_BLOCK and sum(b["isize"] for b in blocks) == len(text) and all(b["isize"] == _bgzf.BLOCK for b in blocks[:-2])
    tbi = _bgzf.parse_tbi(gzip.decompress(open(os.path.join(d, "run_bgzf.vcf.gz.tbi"), "rb").read()))
    reader, lines = _bgzf.Reader(raw), [ln for ln in text.split(b"\n") if ln and not ln.startswith(b"#")]
    step, bad = max(1, len(lines) // 40), 0
    for ln in lines[::step]:   # a window around every sampled record: the index's answer against the neighbouring lines' own intervals
        name, beg, end = _bgzf.line_interval(ln)
        got = _bgzf.query(tbi, reader, name, max(0, beg - 3000), end + 3000)
        bad += ln not in got or any(not (n == name and b < end + 3000 and e > max(0, beg - 3000)) for n, b, e in map(_bgzf.line_interval, got))
    say("BGZF file: %d blocks + EOF block, every block but the last of 65280 input bytes; .tbi: %d contigs, %d bins, %d chunks; %d region queries around sampled records: %s (%.1f s)" % (
        len(blocks) - 1, len(tbi["names"]), sum(len(r["bins"]) for r in tbi["refs"]), sum(len(c) for r in tbi["refs"] for c in r["bins"].values()), len(lines[::step]),
        "every record found, nothing outside its region" if not bad else "%d WRONG" % bad, time.time() - t0))
    if ARGS.parent:
        say("## the switches unset: the parent build's files against this build's, the same output prefix: the bytes, the time:\"...\" field of the options line blanked")
        blank = lambda t: re.sub(rb'(##BayesTyperOptions=[^\n]*?time:")[^"]*', rb"\1", t)   # noqa: E731  (cluster's options line and genotype's: the fields that hold when a run started)
        for extra, name in (([], "run_plain.vcf"), (["-z"], "run_plain.vcf.gz")):
            got = {}
            for who, binary in (("parent", os.path.join(ARGS.parent, "bayesTyper")), ("this", exe)):
                path = os.path.join(d, name)
                if os.path.exists(path):
                    os.remove(path)
                run([binary] + geno + ["-o", os.path.join(d, "run_plain")] + extra, 900, env=base_env)
                raw = open(path, "rb").read()
                if extra:
                    z = zlib.decompressobj(31)
                    text_z = z.decompress(raw)
                    assert z.eof and z.unused_data == b"" and raw[3] == 0   # one gzip member, no extra field
                    got[who] = (len(raw), blank(text_z))
                else:
                    got[who] = (len(raw), blank(raw))
            say("%-18s parent %d bytes, this build %d bytes%s: %s" % (name, got["parent"][0], got["this"][0], ", each one gzip member; decompressed" if extra else "",
                                                                    "identical" if got["parent"][1] == got["this"][1] else "DIFFER"))
    from bayestyper_amd import lib

    ctx = lib.Ctx(0)
    say("## the VCF text, %d bytes, through both writers in this process (device times are event pairs summed over the slabs; they overlap)" % len(text))
    sizes = {}
    for name, call in (("bt_gzip_save", lambda p: lib.gzip_save(ctx, p, text, T)), ("bt_bgzf_save", lambda p: lib.bgzf_save(ctx, p, text, T)[1])):
        path, whole, kern = os.path.join(d, name + ".gz"), [], []
        for rep in range(ARGS.runs + 1):   # the first call also pays the first launch of the kernels
            sec, st = timed(lambda: call(path))
            if rep:
                whole.append(sec), kern.append(st["seconds_kernels"])
            say("%s%s  %8.3f s   copies in %.3f  kernels %.3f  copies out %.3f   host (staging%s + writes) %.3f" % (
                name, " (first call)" if rep == 0 else "             ", sec, st["seconds_h2d"], st["seconds_kernels"], st["seconds_d2h"], " + CRC-32" if name == "bt_gzip_save" else "", st["seconds_host"]))
        say("%s: whole call median %.3f s (%.3f .. %.3f), kernels median %.3f s (%.3f .. %.3f) — %s" % (
            name, statistics.median(whole), min(whole), max(whole), statistics.median(kern), min(kern), max(kern),
            "deflate_piece_kernel + deflate_compact_kernel, no CRC on the device" if name == "bt_gzip_save" else "bgzf_block_kernel (deflate_piece + CRC-32) + bgzf_frame_kernel"))
        sizes[name] = os.path.getsize(path)
        assert gzip.open(path).read() == text
    say("sizes: bt_gzip_save %d bytes (%.4f of the text), bt_bgzf_save %d bytes (%.4f), + %d bytes = %.1f per block of 65280" % (
        sizes["bt_gzip_save"], sizes["bt_gzip_save"] / len(text), sizes["bt_bgzf_save"], sizes["bt_bgzf_save"] / len(text), sizes["bt_bgzf_save"] - sizes["bt_gzip_save"],
        (sizes["bt_bgzf_save"] - sizes["bt_gzip_save"]) / max(1, (len(text) + 65279) // 65280)))
    ctx.close()


def main():
    global ARGS
    ap = argparse.ArgumentParser()
    ap.add_argument("tag")
    ap.add_argument("--genome", type=int, default=256000000)
    ap.add_argument("--variants", type=int, default=800000)
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--error-kmers", type=int, default=560000000)
    ap.add_argument("--sv", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--bgzf", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "gzip_device"))
    ARGS = ap.parse_args()
    from bayestyper_amd import hostinfo

    T = hostinfo.baseline_threads(hostinfo.host_facts())
    exe, tools_exe = os.path.join(ROOT, "bayestyper_amd", "bayesTyper"), os.path.join(ROOT, "bayestyper_amd", "bayesTyperTools")
    d = tempfile.mkdtemp(prefix="gz_" + ARGS.tag + "_", dir="/tmp")
    try:
        say("# " + ("BGZF" if ARGS.bgzf else "gzip") + " on the device: genome %d nt, %d candidate variants (%d per mille long deletions), %d sample(s), k=55, -p %d; %s" % (
            ARGS.genome, ARGS.variants, ARGS.sv, ARGS.samples, T, time.strftime("%Y-%m-%d %H:%M:%S UTC", time.gmtime())))
        t0 = time.time()
        run(["g++", "-O2", "-std=c++17", "-fopenmp", os.path.join(ROOT, "tools", "make_c2_dataset.cpp"), "-o", os.path.join(d, "make_c2_dataset")], 300)
        run([os.path.join(d, "make_c2_dataset"), d, str(ARGS.genome), str(ARGS.variants), str(ARGS.samples), str(ARGS.error_kmers), str(ARGS.sv)], 900)
        for s in range(1, ARGS.samples + 1):
            run([tools_exe, "makeBloom", "-k", "sample%d" % s, "-p", str(T)], 300, cwd=d)
        base_env = dict(os.environ, BT_STAGE_TIMES="1")
        base_env.pop("BT_GZIP_ON_DEVICE", None)
        base_env.pop("BT_VCF_BGZF", None)
        on_env = dict(base_env, BT_GZIP_ON_DEVICE="1")
        common = ["-s", os.path.join(d, "samples.tsv"), "-g", os.path.join(d, "genome.fa"), "-p", str(T), "-r", "42"]
        say("# data set and makeBloom took %.0f s" % (time.time() - t0))
        if ARGS.bgzf:
            run([exe, "cluster", "-v", os.path.join(d, "candidates.vcf"), "-o", os.path.join(d, "bt")] + common, 600, env=base_env)
            bgzf_tables(d, exe, ["genotype", "-v", os.path.join(d, "bt_unit_1", "variant_clusters.bin"), "-c", os.path.join(d, "bt_cluster_data")] + common, base_env, T)
            finish(0)
        # ---- cluster
        say("## bayesTyper cluster: the rows of the gz outputs")
        for label, env, prefix in (("switch unset", base_env, "bt"), ("BT_GZIP_ON_DEVICE=1", on_env, "btdev")):
            _, err, wall = run([exe, "cluster", "-v", os.path.join(d, "candidates.vcf"), "-o", os.path.join(d, prefix)] + common, 600, env=env)
            r = rows(err)
            for k, v in r.items():
                if "parameter k-mers: write" in k or "gzip on the device" in k or "inter-cluster regions, parameter" in k or k == "wall since main()":
                    say("%-22s %-70s %8.3f s" % (label, k, v))
        same = True
        for name in ("parameter_kmers.fa.gz", "intercluster_regions.txt.gz"):
            a, b = os.path.join(d, "bt_cluster_data", name), os.path.join(d, "btdev_cluster_data", name)
            eq = gzip.open(a).read() == gzip.open(b).read()
            same &= eq
            say("%-28s host route %10d bytes, device route %10d bytes, contents %s" % (name, os.path.getsize(a), os.path.getsize(b), "identical" if eq else "DIFFER"))
        # ---- genotype -z
        geno = ["genotype", "-v", os.path.join(d, "bt_unit_1", "variant_clusters.bin"), "-c", os.path.join(d, "bt_cluster_data")] + common
        say("## bayesTyper genotype -z: the write VCF row, the wall clock since main()")
        md5s, write_rows = set(), {"host": [], "device": []}
        for rep in range(ARGS.runs):
            for route, env in (("host", base_env), ("device", on_env)):
                prefix = os.path.join(d, "run_" + route)
                for f in (prefix + ".vcf.gz",):
                    if os.path.exists(f):
                        os.remove(f)
                _, err, wall = run([exe] + geno + ["-o", prefix, "-z"], 900, env=env)
                r = rows(err)
                key = [k for k in r if k.startswith("write VCF")]
                assert len(key) == 1 and (("gzip on the device" in key[0]) == (route == "device")), key
                write_rows[route].append(r[key[0]])
                md5s.add(vcf_body_md5(prefix + ".vcf.gz"))
                say("run %d %-7s %-62s %8.3f s   wall since main() %8.3f s   .vcf.gz %d bytes" % (rep + 1, route, key[0], r[key[0]], r["wall since main()"], os.path.getsize(prefix + ".vcf.gz")))
        say("decompressed VCFs of all %d runs (without the options line): %s" % (2 * ARGS.runs, "identical" if len(md5s) == 1 else "DIFFER"))
        say("write VCF medians: host route %.3f s, device route %.3f s" % (statistics.median(write_rows["host"]), statistics.median(write_rows["device"])))
        # ---- the switch unset against the parent build
        if ARGS.parent:
            say("## bayesTyper genotype (no -z): the parent build against this build with the switch unset, %d runs each: median (min .. max) per stage" % ARGS.runs)
            tables = {"parent": [], "this": []}
            plain = {}
            for rep in range(ARGS.runs):
                for who, binary in (("parent", os.path.join(ARGS.parent, "bayesTyper")), ("this", exe)):
                    prefix = os.path.join(d, "plain_" + who)
                    _, err, wall = run([binary] + geno + ["-o", prefix], 900, env=base_env)
                    tables[who].append(rows(err))
                    plain.setdefault(who, set()).add(hashlib.md5(b"".join(ln for ln in open(prefix + ".vcf", "rb") if not ln.startswith(b"##BayesTyperOptions="))).hexdigest())
            worse = []
            for k in tables["parent"][0]:
                if not all(k in t for t in tables["parent"] + tables["this"]) or k.startswith("kmc stream"):   # (that row's name holds its own timings)
                    continue
                p, m = [t[k] for t in tables["parent"]], [t[k] for t in tables["this"]]
                say("%-56s parent %8.3f (%8.3f .. %8.3f)   this %8.3f (%8.3f .. %8.3f)" % (k[:56], statistics.median(p), min(p), max(p), statistics.median(m), min(m), max(m)))
                if statistics.median(m) > statistics.median(p) + (max(p) - min(p)):
                    worse.append("%s (+%.3f s over the median, spread %.3f s)" % (k, statistics.median(m) - statistics.median(p), max(p) - min(p)))
            say("stages whose median exceeds the parent's by more than the parent's spread:", ", ".join(worse) if worse else "none")
            say("plain .vcf of the parent and of this build (without the options line):", "identical" if plain["parent"] == plain["this"] and len(plain["this"]) == 1 else "DIFFER")
        # ---- the same contents through every writer, in this process
        from bayestyper_amd import lib
        from bayestyper_amd.host import cluster_stage

        dll = cluster_stage.dll
        dll.bth_write_gz.argtypes = [C.c_char_p, C.c_char_p, C.c_ulonglong, C.c_uint]
        ctx = lib.Ctx(0)
        content_table("the VCF text", gzip.open(os.path.join(d, "run_host.vcf.gz")).read(), T, ctx, lib, dll, d)
        content_table("the parameter k-mer FASTA", gzip.open(os.path.join(d, "bt_cluster_data", "parameter_kmers.fa.gz")).read(), T, ctx, lib, dll, d)
        ctx.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    finish(0)


if __name__ == "__main__":
    main()
