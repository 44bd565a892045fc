#!/usr/bin/env python3
"""Measurements of the multigroup pass's workgroup route (mg_order_wide_kernel, BT_MG_WIDE_MIN) for profiles/multigroup_wide.txt.  On the GPU box, from the
repository root, after build():

    python tools/multigroup_wide.py [--out FILE] [--parent-dir DIR] [--sizes 1000,10000,100000,1000000] [--skip-exe]

1. Kernel crossover: 50 000 groups of about 130 k-mers plus one group of n distinct k-mers (first, in a fresh set: the most stages); bt_kmer_set_orders with
   wide_min = 0 (every group on a lane) and wide_min = n (the one group on a workgroup), median of three calls after one warm-up, the two routes alternating in
   one process.  The time is the host's clock around the call, which ends in a device synchronise and includes the upload of the k-mers — the same bytes for both
   routes.  Every size runs in a process of its own under `timeout`; the first size that fails or runs out of time ends the part.
2. Executable: the C3-shaped `bayesTyper cluster` of tools/e2e_c2.sh (256 Mnt, 800 000 variants, 3 samples, 10 per mille SVs), three runs each of the parent
   commit's build (--parent-dir: a directory holding that commit's bayesTyper, libbthost.so, libbtgpu.so, libbtcomm.so; left out when not given), this build
   with BT_MG_WIDE_MIN unset and this build with it at the crossover of part 1, the builds alternating.  Rows "count path / multigroup k-mers" and
   "wall since main()", the largest group of the unit, and a SHA-256 of the content of every file each run wrote (gzip streams decompressed, the one
   time:"..." field of variant_clusters.bin blanked, as the executable's tests compare these files).
A step that fails — an exit status other than 0, a time limit — ends the run with a non-zero status: nothing is started after it, the executable part
included.  Progress lines go to the terminal only, not into the report."""
import argparse
import ctypes as C
import gzip
import hashlib
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K = 55
SMALL_GROUPS, SMALL_SIZE = 50_000, 130


def one_size(n):
    """child process: both routes at one size -> one JSON line"""
    import numpy as np

    from bayestyper_amd import lib

    rng = np.random.default_rng(n)
    sizes = [n] + [int(x) for x in rng.integers(SMALL_SIZE - 30, SMALL_SIZE + 31, SMALL_GROUPS)]
    total = sum(sizes)
    flat = np.empty((total, 2), np.uint64)   # random 110-bit words: distinct for all practical purposes (2^-60 per pair)
    flat[:, 0] = rng.integers(0, 2 ** 64, total, dtype=np.uint64)
    flat[:, 1] = rng.integers(0, 2 ** (2 * K - 64), total, dtype=np.uint64)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    ctx = lib.Ctx(0)
    rank = {0: np.zeros(total, np.uint32), n: np.zeros(total, np.uint32)}
    stats = lib.MultigroupStats()
    times = {0: [], n: []}
    for rep in range(4):   # rep 0 is the warm-up
        for wide_min in (0, n):
            t0 = time.perf_counter()
            lib.check(lib.bt_kmer_set_orders(ctx.h, flat.ctypes.data, off.ctypes.data, len(sizes), K, 1, wide_min, rank[wide_min].ctypes.data, None, C.byref(stats)))
            dt = time.perf_counter() - t0
            if rep:
                times[wide_min].append(dt)
            if wide_min:
                wide_stats = stats.as_dict()
    same = bool(np.array_equal(rank[0], rank[n]))
    ctx.close()
    print(json.dumps({"n": n, "lane_ms": [1e3 * t for t in times[0]], "wide_ms": [1e3 * t for t in times[n]], "same_ranks": same, "stats": wide_stats}), flush=True)
    return 0 if same else 3


def run(cmd, limit, log, env=None, cwd=None, out_path=None, err_path=None):
    """one step under its own time limit, with a line every minute while it runs; returns the exit status (124: the limit)"""
    so = open(out_path, "w") if out_path else subprocess.DEVNULL
    se = open(err_path, "w") if err_path else subprocess.STDOUT
    p = subprocess.Popen(["timeout", "-k", "10", str(limit)] + cmd, stdout=so, stderr=se, env=env, cwd=cwd)
    t0 = time.time()
    while True:
        try:
            rc = p.wait(timeout=60)
            break
        except subprocess.TimeoutExpired:
            print(f"#   ... {os.path.basename(cmd[0])} running for {int(time.time() - t0)} s", flush=True)   # (terminal only)
    for f in (so, se):
        if hasattr(f, "close"):
            f.close()
    return rc


def crossover(sizes, limit, log):
    log("## kernel crossover: bt_kmer_set_orders, 50 000 groups of ~130 k-mers + one group of n (first, fresh set), wide_min 0 (lane) vs n (workgroup)")
    log("# n, lane ms (median of 3), workgroup ms (median of 3), lane / workgroup, lane - workgroup ms, stages of the group, work area bytes")
    results = []
    for n in sizes:
        out = os.path.join("/tmp", f"mgw_one_{n}.json")
        rc = run([sys.executable, os.path.abspath(__file__), "--one", str(n)], limit, log, out_path=out)
        if rc != 0:
            log(f"# n = {n}: exit status {rc}" + (" (time limit of %d s)" % limit if rc in (124, 137) else "") + ": the run ends here; the sizes above are the ones that finished")
            return results, None, False
        r = json.loads(open(out).read().strip().splitlines()[-1])
        lane, wide = statistics.median(r["lane_ms"]), statistics.median(r["wide_ms"])
        results.append((n, lane, wide))
        log(f"{n:>8} {lane:10.2f} {wide:10.2f} {lane / wide:8.2f}x {lane - wide:10.2f}  {r['stats']['max_stages']:>3} {r['stats']['wide_scratch_bytes']:>12}"
            f"   (lane {', '.join('%.2f' % x for x in r['lane_ms'])}; workgroup {', '.join('%.2f' % x for x in r['wide_ms'])}; same ranks: {r['same_ranks']})")
    wins = [(n, lane, wide) for n, lane, wide in results if wide < lane]
    if wins:
        n, lane, wide = wins[0]
        log(f"# smallest n at which the workgroup route wins: {n} ({lane:.2f} ms -> {wide:.2f} ms, {lane / wide:.2f}x)")
    else:
        log("# the workgroup route wins at none of the sizes that finished")
    return results, (wins[0][0] if wins else None), True


def stage_rows(err_text):
    rows = {}
    for line in err_text.splitlines():
        m = re.match(r"^(.*\S)\s+([0-9.]+) s$", line)
        if m:
            rows[m.group(1).strip()] = float(m.group(2))
    return rows


def content(raw):
    """what a file holds, apart from when it was written: a gzip stream decompressed, the time:"..." field of variant_clusters.bin blanked"""
    data = gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw
    return re.sub(rb'time:"[^"]*"', b'time:""', data)


def tree_hash(prefix):
    """SHA-256 of the content of every file a `cluster -o prefix` run wrote, keyed by its path below the output directory"""
    out = {}
    base = os.path.dirname(prefix)
    for dp, _, fns in os.walk(base):
        for fn in sorted(fns):
            path = os.path.join(dp, fn)
            with open(path, "rb") as f:
                out[os.path.relpath(path, base)] = hashlib.sha256(content(f.read())).hexdigest()
    return out


def executable(parent_dir, wide_min, shape, log):
    from bayestyper_amd import hostinfo

    L, NV, NS, NE, SV = shape
    threads = hostinfo.baseline_threads(hostinfo.host_facts())
    d = "/tmp/mgw_c3"
    shutil.rmtree(d, ignore_errors=True)
    os.makedirs(d)
    log(f"## executable: bayesTyper cluster, genome {L} nt, {NV} candidate variants, {NS} sample(s), {NE} error k-mers per sample, {SV} per mille SVs, k=55, -p {threads}")
    gen = os.path.join(d, "make_c2_dataset")
    if run(["g++", "-O2", "-std=c++17", "-fopenmp", os.path.join(ROOT, "tools", "make_c2_dataset.cpp"), "-o", gen], 300, log) != 0:
        log("# building the data set generator failed")
        return 1
    t0 = time.time()
    if run([gen, d, str(L), str(NV), str(NS), str(NE), str(SV)], 900, log) != 0:
        log("# the data set generator failed or ran out of time")
        return 1
    log(f"# data set generated in {time.time() - t0:.0f} s")
    here = os.path.join(ROOT, "bayestyper_amd")
    for s in range(1, NS + 1):
        if run([os.path.join(here, "bayesTyperTools"), "makeBloom", "-k", f"sample{s}", "-p", str(threads)], 300, log, cwd=d) != 0:
            log("# makeBloom failed")
            return 1
    builds = []
    if parent_dir:
        builds.append(("parent", os.path.join(os.path.abspath(parent_dir), "bayesTyper"), None))
    else:
        log("# no --parent-dir: the parent commit's build is left out")
    builds.append(("this, switch unset", os.path.join(here, "bayesTyper"), None))
    if wide_min:
        builds.append((f"this, BT_MG_WIDE_MIN={wide_min}", os.path.join(here, "bayesTyper"), str(wide_min)))
    rows = {b[0]: [] for b in builds}
    hashes = {}
    route = {}
    for rep in range(3):
        for name, exe, switch in builds:
            env = dict(os.environ, BT_STAGE_TIMES="1")
            env.pop("BT_MG_WIDE_MIN", None)
            if switch:
                env["BT_MG_WIDE_MIN"] = switch
            run_dir = os.path.join(d, "run")
            shutil.rmtree(run_dir, ignore_errors=True)
            os.makedirs(run_dir)
            prefix = os.path.join(run_dir, "bt")
            err_path = os.path.join(d, "cluster.err")
            rc = run([exe, "cluster", "-v", f"{d}/candidates.vcf", "-s", f"{d}/samples.tsv", "-g", f"{d}/genome.fa", "-o", prefix, "-p", str(threads), "-r", "42"], 300, log,
                     env=env, out_path=os.path.join(d, "cluster.out"), err_path=err_path)
            err_text = open(err_path).read()
            if rc != 0:
                log(f"# {name}, run {rep + 1}: exit status {rc}\n" + err_text[-2000:])
                return 1
            r = stage_rows(err_text)
            rows[name].append(r)
            for key in r:
                if key.startswith("multigroup pass (device)"):
                    route[name] = key
            hashes.setdefault(name, []).append(tree_hash(prefix))
            log(f"# {name}, run {rep + 1}: count path / multigroup k-mers {r.get('count path / multigroup k-mers', float('nan')):.3f} s, wall since main() "
                f"{r.get('wall since main()', float('nan')):.3f} s")
    log("# stage medians over the three runs [min .. max], seconds")
    stages = [k for k in rows[builds[0][0]][0] if not k.startswith("multigroup pass (device)")]
    med = {name: {k: statistics.median(r[k] for r in rows[name] if k in r) for k in stages if all(k in r for r in rows[name])} for name, _, _ in builds}
    for k in stages:
        line = f"{k[:58]:<58}"
        for name, _, _ in builds:
            v = [r[k] for r in rows[name] if k in r]
            line += f" | {name}: {statistics.median(v):.3f} [{min(v):.3f} .. {max(v):.3f}]" if v else f" | {name}: -"
        log(line)
    for name in route:
        log(f"# route ({name}): {route[name]}")
    ok = True
    if parent_dir:
        name = "this, switch unset"
        for k in stages:
            v = [r[k] for r in rows["parent"] if k in r]
            if not v or k not in med[name]:
                continue
            spread = max(v) - min(v)
            if med[name][k] > med["parent"][k] + spread:
                ok = False
                log(f"# CONDITION MISSED at '{k}': switch unset {med[name][k]:.3f} s > parent {med['parent'][k]:.3f} s + its spread {spread:.3f} s")
        log("# condition (switch unset: no stage's median above the parent's by more than the parent's spread over its three runs): " + ("met" if ok else "MISSED"))
    first = hashes[builds[0][0]][0]
    same = all(h == first for hs in hashes.values() for h in hs)
    log(f"# files written by the stage ({len(first)}): " + ("content identical across all builds and runs (gzip decompressed, time field blanked)" if same else "DIFFER"))
    if not same:
        for name, hs in hashes.items():
            for i, h in enumerate(hs):
                for path in sorted(set(h) | set(first)):
                    if h.get(path) != first.get(path):
                        log(f"#   {name}, run {i + 1}: {path} differs from {builds[0][0]}, run 1")
    shutil.rmtree(d, ignore_errors=True)
    return 0 if ok and same else 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", type=int, help="(child) both routes at one size")
    ap.add_argument("--out", default="multigroup_wide.txt", help="where the report goes (default: multigroup_wide.txt in the current directory)")
    ap.add_argument("--sizes", default="1000,10000,100000,1000000")
    ap.add_argument("--size-limit", type=int, default=240, help="seconds per size")
    ap.add_argument("--parent-dir")
    ap.add_argument("--wide-min", type=int, default=0, help="switch value of the third executable leg (default: the measured crossover)")
    ap.add_argument("--shape", default="256000000,800000,3,560000000,10", help="genome length, variants, samples, error k-mers per sample, SVs per mille")
    ap.add_argument("--skip-exe", action="store_true")
    a = ap.parse_args()
    if a.one is not None:
        return one_size(a.one)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    dst = open(a.out, "w")

    def log(line):
        print(line, flush=True)
        dst.write(line + "\n")
        dst.flush()

    log("# " + " ".join(["python", "tools/multigroup_wide.py"] + sys.argv[1:]) + time.strftime("   (%Y-%m-%d %H:%M UTC)", time.gmtime()))
    results, cross, finished = crossover([int(x) for x in a.sizes.split(",")], a.size_limit, log)
    if not finished:   # a size failed or ran out of time: nothing more is started
        log("# a step of the kernel crossover failed: the executable part is not run")
        return 1
    if a.skip_exe:
        return 0
    wide_min = a.wide_min or cross or results[0][0]
    if not (a.wide_min or cross):
        log(f"# no crossover measured: the third leg runs with BT_MG_WIDE_MIN={wide_min}, the smallest size tried")
    return executable(a.parent_dir, wide_min, [int(x) for x in a.shape.split(",")], log)


if __name__ == "__main__":
    sys.exit(main())
