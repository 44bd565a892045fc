#!/usr/bin/env python3
"""Per-wavefront timeline of the default-mode sampling launch (bt_gibbs_timeline_*) on the bench's two batches.

    python tools/wave_timeline.py [--runs 3] [--out profiles/wave_timeline] [--batches S3,S10]

For each batch — `S3`: bench.py's 600 000-group mixture at three samples; `S10`: its `samples10` record's batch (4 x 100 000 groups at ten samples) —
a child process of its own, under `timeout`, builds the batch with the builders bench.py uses, creates two samplers on it and runs the whole default
schedule `--runs` times on each in turn: one with the timeline off (the product's kernels), one with it on (the stamped siblings).  After every pair of
runs the two samplers' posterior summaries must be equal, after the last their whole result strings.  The parent collects the children's records into
<out>.json (summaries, per-class table, per-XCC busy share, the ten longest and the ten last wavefronts per stamped run) and <out>.txt.

The stamped runs are measured against the unstamped runs of the same build; that is a measurement, not a gate: if they differ by more than the
unstamped spread, read the profile's SHARES, not its length."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KERNELS = ("gibbs_kernel", "gibbs_hot_kernel", "gibbs_simple_kernel", "gibbs_single_kernel")


def build_batch(name):
    """-> (flat, lut_g, lut_n, description): what bench.py times (S3) / what its samples10 record times (S10)"""
    import numpy as np

    import bench
    from bayestyper_amd import synth
    from bayestyper_amd.host import count_model

    if name == "S3":
        args = bench.parser().parse_args([])
        S = args.samples
        flat, _, _, _ = bench.rank_batch(args.groups, S, 0, 1, args.scaling, bench.mix_templates(args))
        what = "bench.py's batch: %d groups of the mixture, S = %d" % (flat["num_groups"], S)
    elif name == "S10":
        S = 10
        f10 = synth.make_mixture(100_000, S, seed=1010)
        flat = synth.concat([f10] * 4)
        flat["group_index"] = np.arange(flat["num_groups"], dtype=np.uint32)
        what = "bench.py's samples10 batch: %d groups (4 copies of %d generated groups, each with group indices of its own), S = 10" % (flat["num_groups"], f10["num_groups"])
    else:
        raise SystemExit("unknown batch " + name)
    lut_g, lut_n = count_model.build_luts(S, mean=15.0, var=30.0, noise_rate=0.05)
    return flat, lut_g, lut_n, what


def seconds(ticks, khz):
    return ticks / (khz * 1e3)


def describe(rec, launch, khz):
    """one stamped launch -> dict of summaries (times in seconds)"""
    import numpy as np

    from bayestyper_amd import lib

    def summary(cls=None):
        s = lib.timeline_summary(rec, launch=launch, launch_class=cls)
        span = s["last_end"] - s["first_start"]
        return s, {"records": s["records"], "unfinished": s["unfinished"], "makespan_s": seconds(span, khz), "busy_s": seconds(s["busy_ticks"], khz),
                   "mean_live": s["busy_ticks"] / span if span else 0.0, "peak_live": s["peak_live"],
                   "busy_over_peak_s": seconds(s["busy_ticks"], khz) / s["peak_live"] if s["peak_live"] else 0.0,
                   "median_end_s": seconds(s["median_end"] - s["first_start"], khz) if s["records"] else 0.0,
                   "idle_after_median_s": seconds(s["idle_after_median_ticks"], khz),
                   "idle_after_median_share": s["idle_after_median_ticks"] / (s["peak_live"] * span) if span and s["peak_live"] else 0.0}

    r = rec[rec["launch"] == launch]
    raw, out = summary()
    t0 = raw["first_start"]
    out["classes"] = []
    for c in sorted(set(r["launch_class"].tolist())):
        rc = r[r["launch_class"] == c]
        craw, cs = summary(c)
        cs.update({"class": int(c), "kernel": KERNELS[int(rc["kernel"][0])], "wavefronts": int(len(rc)), "tiles": int(len(np.unique(rc["tile"]))),
                   "lds_bytes_max": int(rc["lds_bytes"].max()), "start_s": seconds(craw["first_start"] - t0, khz), "end_s": seconds(craw["last_end"] - t0, khz)})
        out["classes"].append(cs)
    length = (r["end_tick"] - r["start_tick"]).astype(np.int64)

    def rows(idx):
        return [{"tile": int(r["tile"][i]), "wave": int(r["wave"][i]), "class": int(r["launch_class"][i]), "kernel": KERNELS[int(r["kernel"][i])],
                 "start_s": seconds(int(r["start_tick"][i]) - t0, khz), "end_s": seconds(int(r["end_tick"][i]) - t0, khz), "seconds": seconds(int(length[i]), khz),
                 "groups": int(r["groups"][i]), "lds_bytes": int(r["lds_bytes"][i]), "xcc": int(r["xcc_id"][i] & 0xF)} for i in idx]

    out["longest"] = rows(np.argsort(-length, kind="stable")[:10])
    out["last"] = rows(np.argsort(-r["end_tick"].astype(np.int64), kind="stable")[:10])
    xcc = (r["xcc_id"] & 0xF).astype(np.int64)   # XCC_ID register, bits 3:0: the XCC the wavefront ran on
    total = max(int(length.sum()), 1)
    out["xcc_busy_share"] = {str(x): float(length[xcc == x].sum()) / total for x in sorted(set(xcc.tolist()))}
    out["xcc_wavefronts"] = {str(x): int((xcc == x).sum()) for x in sorted(set(xcc.tolist()))}
    # live wavefronts at tenths of the makespan
    span = raw["last_end"] - t0
    out["live_at_tenths"] = [int(((r["start_tick"] <= t0 + span * k // 10) & (r["end_tick"] > t0 + span * k // 10)).sum()) for k in range(10)]
    return out


def child(name, runs):
    import numpy as np

    from bayestyper_amd import lib

    t_build = time.perf_counter()
    flat, lut_g, lut_n, what = build_batch(name)
    t_build = time.perf_counter() - t_build
    ctx = lib.Ctx(0)
    plain = lib.Gibbs(ctx, flat, lut_g, lut_n, seed=42)
    stamped = lib.Gibbs(ctx, flat, lut_g, lut_n, seed=42)
    bytes_off = stamped.device_bytes()
    stamped.timeline_enable(runs)
    timer = lib.Timer(ctx)
    ms = {"unstamped": [], "stamped": []}
    equal = []
    for _ in range(runs):
        for label, g in (("unstamped", plain), ("stamped", stamped)):
            ctx.sync()
            timer.start()
            g.run()
            timer.stop()
            ms[label].append(timer.elapsed_ms())
        equal.append(bool(np.array_equal(plain.posterior_summary(), stamped.posterior_summary())))
    words_equal = bool(np.array_equal(plain.result_words_host(), stamped.result_words_host()))
    rec, khz, dropped = stamped.timeline()
    out = {"batch": name, "workload": what, "groups": int(flat["num_groups"]), "clusters": int(flat["num_clusters"]), "S": int(flat["S"]), "runs": runs,
           "build_seconds": t_build, "tick_khz": khz, "dropped": dropped, "records_bytes": stamped.device_bytes() - bytes_off,
           "ms_per_schedule": ms, "summaries_equal_after_each_run": equal, "result_words_equal": words_equal,
           "launches": [describe(rec, l, khz) for l in range(runs)]}
    plain.close(), stamped.close(), ctx.close()
    print("WAVE_TIMELINE " + json.dumps(out), flush=True)
    return 0 if all(equal) and words_equal and dropped == 0 else 1


def text(results):
    L = []
    for b in results:
        u, s = b["ms_per_schedule"]["unstamped"], b["ms_per_schedule"]["stamped"]
        L.append("== %s: %s" % (b["batch"], b["workload"]))
        L.append("   stamped and unstamped results equal: after every run %s, whole result strings %s; launches dropped %d; records %d bytes; tick %d kHz"
                 % (all(b["summaries_equal_after_each_run"]), b["result_words_equal"], b["dropped"], b["records_bytes"], b["tick_khz"]))
        L.append("   ms per schedule, unstamped: %s (spread %.1f)" % (", ".join("%.1f" % x for x in u), max(u) - min(u)))
        L.append("   ms per schedule, stamped:   %s (spread %.1f); median stamped - median unstamped = %+.1f ms"
                 % (", ".join("%.1f" % x for x in s), max(s) - min(s), sorted(s)[len(s) // 2] - sorted(u)[len(u) // 2]))
        for l, d in enumerate(b["launches"]):
            L.append("   -- stamped run %d: %d wavefronts (%d without an end stamp), makespan %.4f s, busy %.2f wavefront-s, mean live %.1f, peak live %d" %
                     (l, d["records"], d["unfinished"], d["makespan_s"], d["busy_s"], d["mean_live"], d["peak_live"]))
            L.append("      busy / peak live = %.4f s of work at the measured peak; median end at %.4f s; idle after the median end %.2f wavefront-s = %.1f %% of peak x makespan"
                     % (d["busy_over_peak_s"], d["median_end_s"], d["idle_after_median_s"], 100 * d["idle_after_median_share"]))
            L.append("      live wavefronts at 0, 10, .. 90 %% of the makespan: %s" % " ".join(str(x) for x in d["live_at_tenths"]))
            L.append("      class kernel                 tiles  waves  lds max  start s    end s   busy wf-s  mean live  peak  idle share")
            for c in d["classes"]:
                L.append("      %5d %-22s %6d %6d %8d %8.4f %8.4f %11.2f %10.1f %5d %10.3f" % (c["class"], c["kernel"], c["tiles"], c["wavefronts"], c["lds_bytes_max"], c["start_s"],
                                                                                               c["end_s"], c["busy_s"], c["mean_live"], c["peak_live"], c["idle_after_median_share"]))
            L.append("      busy share per XCC: %s" % "  ".join("%s: %.3f" % kv for kv in d["xcc_busy_share"].items()))
            for title, key in (("the ten longest wavefronts", "longest"), ("the ten last wavefronts to end", "last")):
                L.append("      %s (tile.wave class kernel: start .. end s, groups, LDS, XCC)" % title)
                for r in d[key]:
                    L.append("        %7d.%d %2d %-20s %8.4f .. %8.4f  %3d groups %7d B  xcc %d" % (r["tile"], r["wave"], r["class"], r["kernel"], r["start_s"], r["end_s"], r["groups"],
                                                                                                     r["lds_bytes"], r["xcc"]))
        L.append("")
    return "\n".join(L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wave_timeline"))
    ap.add_argument("--batches", default="S3,S10")
    ap.add_argument("--timeout", type=int, default=420, help="seconds a batch's child process may take")
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.runs)
    results = []
    for name in a.batches.split(","):
        r = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", name, "--runs", str(a.runs)], capture_output=True, text=True)
        lines = [x for x in r.stdout.splitlines() if x.startswith("WAVE_TIMELINE ")]
        if lines:
            results.append(json.loads(lines[-1][len("WAVE_TIMELINE "):]))
        if r.returncode != 0:   # a failed or timed-out step ends the tool: nothing more is started on the GPU
            sys.stderr.write(r.stdout[-3000:] + r.stderr[-3000:])
            print("wave_timeline: batch %s ended with status %d; stopping" % (name, r.returncode))
            break
    if results:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out + ".json", "w") as f:
            json.dump({"tool": "tools/wave_timeline.py", "batches": results}, f, indent=1)
            f.write("\n")
        with open(a.out + ".txt", "w") as f:
            f.write(text(results))
        print(text(results))
    return 0 if len(results) == len(a.batches.split(",")) and all(all(b["summaries_equal_after_each_run"]) and b["result_words_equal"] for b in results) else 1


if __name__ == "__main__":
    sys.exit(main())
