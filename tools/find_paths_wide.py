"""bt_find_paths_sample on a batch with wide clusters: the lane kernel alone against wide clusters on a wavefront each, and several samples per call
(bt_find_paths_samples) against one call per sample (profiles/find_paths_wide.txt, profiles/find_paths_samples.txt).

  find_paths_wide.py prepare --cache DIR [--small 50000] [--wide 150,400,1000]
      generate the parts (CPU only): DIR/small.npz — clusters of 1-3 variants — and DIR/wide_<variants>.npz, one cluster each
      (synth_graphs.random_cluster, 6 sampled haplotypes, in-degree <= 3)
  find_paths_wide.py run --cache DIR [--tree CHECKOUT] [--wide 150,400] [--wave-min T[,T...]] [--runs 3] [--limit-s 20] [--label TEXT]
                         [--repeat R] [--samples S [--batched]]
      one JSON line per (batch, threshold): the batch = small + the named wide clusters (none: the lane-only batch), one sample, fpr 0.05,
      max_sample_haplotypes 32; `runs` timed bt_find_paths_sample calls on a fresh object each (the first call of the process is a warm-up on the
      lane-only batch), their median.  --tree: import bayestyper_amd from another built checkout (the parent commit's); a build without
      BT_FIND_PATHS_WAVE_MIN ignores --wave-min.  --limit-s: a batch whose first call took longer is not repeated and ends the run (the sizes after it
      are reported as left out).
      --repeat R: the small clusters R times over (the lane-only batch long enough to time).  --samples S: S samples with a filter of their own each (the
      same k-mers in filters of different sizes, so their false positives differ) and a seed row each; a timed call is then the S searches of one object:
      S bt_find_paths_sample calls, or with --batched one bt_find_paths_samples call (profiles/find_paths_samples.txt).  --check-rows counts the rows
      after the last sample: the two routes must agree.
Every GPU step of a measurement session is one process of this tool under its own `timeout`, chained with &&; nothing is retried."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, MAX_HAPS, FPR, HAPS = 55, 32, 0.05, 6
OFFSETS = {"vertex_off": np.uint32, "seq_off": np.uint64, "refvar_off": np.uint32, "path_off": np.uint64, "var_off": np.uint32, "in_off": np.uint32}


def concat(flats):
    """flattened batches one after the other (offset arrays re-based, everything else appended)"""
    out = {"num_clusters": int(sum(f["num_clusters"] for f in flats))}
    for name in flats[0]:
        if name == "num_clusters":
            continue
        if name in OFFSETS:
            parts, base = [np.zeros(1, OFFSETS[name])], 0
            for f in flats:
                parts.append((f[name][1:].astype(np.uint64) + base).astype(OFFSETS[name]))
                base += int(f[name][-1])
            out[name] = np.concatenate(parts)
        else:
            out[name] = np.concatenate([f[name] for f in flats])
    return out


def load(path):
    z = np.load(path)
    f = {n: z[n] for n in z.files}
    f["num_clusters"] = int(f["num_clusters"])
    return f


def prepare(args):
    sys.path.insert(0, ROOT)
    from bayestyper_amd import synth_graphs

    os.makedirs(args.cache, exist_ok=True)
    rng = np.random.default_rng(11)
    t = time.perf_counter()
    gs = [synth_graphs.random_cluster(rng, K, int(rng.integers(1, 4)), HAPS, kinds=("snv", "snv", "snv", "ins", "del")) for _ in range(args.small)]
    np.savez(os.path.join(args.cache, "small.npz"), **synth_graphs.flatten(gs))
    print(f"small.npz: {args.small} clusters, {time.perf_counter() - t:.1f} s")
    for n in args.wide:
        t = time.perf_counter()
        g = synth_graphs.random_cluster(np.random.default_rng(1000 + n), K, n, HAPS)
        np.savez(os.path.join(args.cache, f"wide_{n}.npz"), **synth_graphs.flatten([g]))
        print(f"wide_{n}.npz: {len(g.seq)} vertices, {time.perf_counter() - t:.1f} s")


def run(args):
    sys.path.insert(0, os.path.abspath(args.tree) if args.tree else ROOT)
    from bayestyper_amd import lib

    ctx = lib.Ctx(0)
    small = load(os.path.join(args.cache, "small.npz"))
    if args.repeat > 1:
        small = concat([small] * args.repeat)
    wides = [load(os.path.join(args.cache, f"wide_{n}.npz")) for n in args.wide]
    whole = concat([small] + wides)
    # the sample's filter: the k-mers of the sampled haplotypes (the batch's path rows) of every cluster, wide ones included
    gp = lib.Paths(ctx, whole, K)
    blooms = []
    for s in range(args.samples):
        blooms.append(lib.Bloom.create(ctx, gp.num_windows + 1000 * (s + 1), FPR, K, threaded=True))
        gp.count_kmers(blooms[-1])
    gp.close()
    ctx.sync()

    def once(flat):
        gf = lib.FindPaths(ctx, flat, K, MAX_HAPS, args.samples)
        seeds = np.stack([np.arange(flat["num_clusters"], dtype=np.uint32) + np.uint32(7 + 1000003 * s) for s in range(args.samples)])
        ctx.sync()
        t = time.perf_counter()
        if args.batched:
            gf.samples(blooms, seeds)
        else:
            for s in range(args.samples):
                gf.sample(blooms[s], seeds[s])
        ctx.sync()
        dt = time.perf_counter() - t
        st = gf.info() if hasattr(gf, "info") else None
        rows = int(sum(len(b) for b in gf.best_paths())) if args.check_rows else None
        gf.close()
        return dt, st, rows

    os.environ["BT_FIND_PATHS_WAVE_MIN"] = "0"
    once(small)   # warm-up: code objects, allocator
    batches = [("lane-only", small, [])] if not args.wide else [(f"small + {n} variants", concat([small, w]), [n]) for n, w in zip(args.wide, wides)]
    if args.all_wide and len(wides) > 1:
        batches = [("small + " + " + ".join(str(n) for n in args.wide) + " variants", whole, list(args.wide))]
    for bi, (name, flat, sizes) in enumerate(batches):
        nv = flat["vertex_off"][1:] - flat["vertex_off"][:-1]
        for wave_min in args.wave_min:
            if wave_min is None:
                os.environ.pop("BT_FIND_PATHS_WAVE_MIN", None)
            else:
                os.environ["BT_FIND_PATHS_WAVE_MIN"] = str(wave_min)
            times, st, rows = [], None, None
            for r in range(args.runs):
                dt, st, rows = once(flat)
                times.append(dt)
                if dt > args.limit_s:
                    break
            rec = {"label": args.label, "batch": name, "clusters": int(flat["num_clusters"]), "max_vertices": int(nv.max()), "wave_min_env": wave_min,
                   "seconds": [round(x, 4) for x in times], "median_s": round(float(np.median(times)), 4)}
            if st is not None:
                rec.update(num_wave_clusters=st.num_wave_clusters, wave_min=st.wave_min_vertices, max_candidate_paths=st.max_candidate_paths)
            if args.samples > 1 or args.batched:
                rec.update(samples=args.samples, batched=bool(args.batched))
            if rows is not None:
                rec["best_rows"] = rows
            print(json.dumps(rec), flush=True)
            if times[-1] > args.limit_s:
                left = [b[0] for b in batches[bi + 1:]]
                print(json.dumps({"label": args.label, "stopped_after": name, "limit_s": args.limit_s, "left_out": left}), flush=True)
                return


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["prepare", "run"])
    ap.add_argument("--cache", required=True)
    ap.add_argument("--tree", default=None)
    ap.add_argument("--small", type=int, default=50_000)
    ap.add_argument("--wide", type=lambda s: [int(x) for x in s.split(",") if x], default=[])
    ap.add_argument("--wave-min", type=lambda s: [None if x == "default" else int(x) for x in s.split(",")], default=[None])
    ap.add_argument("--all-wide", action="store_true", help="one batch with every wide cluster instead of one batch per size")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--limit-s", type=float, default=20.0)
    ap.add_argument("--label", default="")
    ap.add_argument("--check-rows", action="store_true")
    ap.add_argument("--repeat", type=int, default=1, help="the small clusters this many times over")
    ap.add_argument("--samples", type=int, default=1, help="samples searched per timed call, a filter each")
    ap.add_argument("--batched", action="store_true", help="one bt_find_paths_samples call instead of one bt_find_paths_sample call per sample")
    args = ap.parse_args()
    prepare(args) if args.mode == "prepare" else run(args)


if __name__ == "__main__":
    main()
