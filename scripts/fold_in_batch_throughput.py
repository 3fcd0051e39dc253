"""Throughput of batched fold-in recommendations (Engine.recommend_for_batch, csrc/foldin.hip) at the ml-25m shape,
next to the host loop of single recommend_for calls.

The workload is that of scripts/fold_in_latency.py: syn-25m, k = 300, the same `_queries` draw with seed 11,
recommend(n = 3).  One child process fits once, warms up, and times `--repeats` passes over the `--queries` queries for
every leg: the single-call loop (the baseline: it uses only entry points that exist without the batch calls, so
`--baseline-only` runs unchanged on a tree that lacks them) and recommend_for_batch issued B = 1, 8, 64 and 200 at a time.
Each figure is the median over the repeats with min and standard deviation beside it.  Then the B = 64 work is repeated
under `rocprofv3 --kernel-trace --stats` in two child processes of their own — the fit alone, and the fit plus the batch
calls — and the per-query device time of each kernel is their difference over the number of queries.  Prints one JSON line.

    python scripts/fold_in_batch_throughput.py [--queries 200] [--repeats 5] [--baseline-only] [--no-profile] [--out DIR]

Every GPU step runs in its own child process under `timeout -k 10`; a failing step ends the run."""
import argparse
import csv
import importlib
import importlib.util
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "movie-recommender-system_amd"
BATCHES = (1, 8, 64, 200)
SIM_KERNEL = "k_query_sim_dual"


def _latency_script():
    spec = importlib.util.spec_from_file_location("fold_in_latency", os.path.join(ROOT, "scripts", "fold_in_latency.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _summary(seconds, n_queries):
    import numpy as np

    us = np.array(seconds) * 1e6 / n_queries
    return {"us_per_query_median": float(np.median(us)), "us_per_query_min": float(us.min()), "us_per_query_sigma": float(us.std()),
            "queries_per_s": float(1e6 / np.median(us)), "repeats": len(seconds)}


def inner(args):
    """runs on the GPU: fit, warm up, time every leg (or just run the B = 64 leg once, under the profiler)"""
    kn = importlib.import_module(PKG + ".knncf")
    synth = importlib.import_module(PKG + ".synth")
    d = synth.syn_25m()
    e = kn.Engine(k=300)
    e.fit(d.train.users, d.train.items, d.train.ratings)
    U, I, nnz = e.num_users, e.num_items, len(d.train.users)
    qs = _latency_script()._queries(d, args.queries, seed=11)
    res = {"U": U, "I": I, "train_ratings": nnz, "queries": len(qs), "k": 300, "n": 3,
           "query_ratings_total": int(sum(len(it) for _, it, _ in qs))}
    if args.profile_batch >= 0:
        if args.profile_batch > 0:
            for a in range(0, len(qs), args.profile_batch):
                e.recommend_for_batch(qs[a:a + args.profile_batch], 3)
        e.close()
        print(json.dumps(res), flush=True)
        return
    for q, it, rt in qs[:20]:  # warm-up: every launch shape and the scratch sizes
        e.recommend_for(q, it, rt, 3)
    runs = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        for q, it, rt in qs:
            e.recommend_for(q, it, rt, 3)
        runs.append(time.perf_counter() - t0)
    res["single_loop"] = _summary(runs, len(qs))
    if not args.baseline_only:
        res["batch"] = {}
        for B in BATCHES:
            chunks = [qs[a:a + B] for a in range(0, len(qs), B)]
            for c in chunks[:2]:
                e.recommend_for_batch(c, 3)
            runs = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                for c in chunks:
                    e.recommend_for_batch(c, 3)
                runs.append(time.perf_counter() - t0)
            res["batch"][str(B)] = _summary(runs, len(qs))
    e.close()
    print(json.dumps(res), flush=True)


def _child(argv, timeout_s, log):
    cmd = ["timeout", "-k", "10", str(timeout_s)] + argv
    with open(log, "w") as f:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=f, text=True, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit(f"step failed with status {r.returncode}: {' '.join(argv)} (log: {log})")
    return json.loads(r.stdout.strip().splitlines()[-1])


def _stats(path):
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            out[row["Name"]] = (int(row["Calls"]), float(row["TotalDurationNs"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--commit", default="", help="label written into the result")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "fold_in_batch"))
    ap.add_argument("--inner", action="store_true")
    ap.add_argument("--profile-batch", type=int, default=-1)
    args = ap.parse_args()
    if args.inner:
        return inner(args)
    os.makedirs(args.out, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__), "--inner", "--queries", str(args.queries), "--repeats", str(args.repeats)]
    res = _child(me + (["--baseline-only"] if args.baseline_only else []), 900, os.path.join(args.out, "timing.log"))
    res["commit"] = args.commit
    if not (args.baseline_only or args.no_profile):
        B = 64
        prof = {}
        for tag, batch in (("fit", 0), ("calls", B)):
            d = os.path.join(args.out, "prof_" + tag)
            _child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "fb", "--"] + me +
                   ["--profile-batch", str(batch)], 900, os.path.join(args.out, f"prof_{tag}.log"))
            found = [os.path.join(r, f) for r, _, fs in os.walk(d) for f in fs if f.endswith("kernel_stats.csv")]
            prof[tag] = _stats(found[0])
        per_kernel = {}
        for name, (calls, ns) in prof["calls"].items():
            c0, ns0 = prof["fit"].get(name, (0, 0.0))
            if calls > c0:
                per_kernel[name[:120]] = {"calls_per_query": (calls - c0) / args.queries, "us_per_query": (ns - ns0) / args.queries / 1e3}
        res["profile_batch"] = B
        res["device_us_per_query"] = sum(v["us_per_query"] for v in per_kernel.values())
        res["kernels"] = per_kernel
        # the similarity pass on its algorithmic bytes: every chunk reads s_col and u_ptr once (4 n + 16 U) and writes one
        # fp64 per (query, user)
        sim = [v for name, v in per_kernel.items() if SIM_KERNEL in name]
        if sim:
            n_chunks = round(sim[0]["calls_per_query"] * args.queries)  # (a last chunk below 32 queries runs k_query_sim)
            sim_bytes = n_chunks * (4 * res["train_ratings"] + 16 * res["U"]) + min(args.queries, n_chunks * B) * 8 * res["U"]
            res["similarity_bytes"] = sim_bytes
            res["similarity_bytes_per_s"] = sim_bytes / (sim[0]["us_per_query"] * args.queries * 1e-6)
    with open(os.path.join(args.out, "fold_in_batch_throughput.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
