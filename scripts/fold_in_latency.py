"""Latency of a fold-in recommendation (Engine.recommend_for, csrc/foldin.hip) at the ml-25m shape.

Fits syn-25m (k = 300) once, warms up, and times `--calls` recommend_for(n = 3) calls whose query rows are those of train
users drawn uniformly (so the query sizes follow the train row-length distribution), each under a fresh user id.  Then
repeats the work under `rocprofv3 --kernel-trace --stats` in two child processes — the fit alone, and the fit plus the
profiled calls — and reports the per-call device time of each kernel as the difference over the number of calls (the
radix-sort kernels are shared with the fit).  Prints one JSON line.

    python scripts/fold_in_latency.py [--calls 200] [--prof-calls 50] [--out bench_out/fold_in]

Every GPU step runs in its own child process under `timeout -k 10`."""
import argparse
import csv
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "movie-recommender-system_amd"


def _queries(d, count, seed):
    import numpy as np

    u = d.train.users
    order = np.argsort(u, kind="stable")
    su = u[order]
    users, starts, counts = np.unique(su, return_index=True, return_counts=True)
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(users), count)
    fresh = int(users.max()) + 1
    out = []
    for j, x in enumerate(pick):
        rows = order[starts[x]:starts[x] + counts[x]]
        out.append((fresh + j, d.train.items[rows], d.train.ratings[rows]))
    return out


def inner(args):
    """runs on the GPU: fit, warm up, time (or just run, under the profiler)"""
    import numpy as np

    kn = importlib.import_module(PKG + ".knncf")
    synth = importlib.import_module(PKG + ".synth")
    d = synth.syn_25m()
    e = kn.Engine(k=300)
    e.fit(d.train.users, d.train.items, d.train.ratings)
    U, I, nnz = e.num_users, e.num_items, len(d.train.users)
    qs = _queries(d, max(args.calls, args.prof_calls) + 20, seed=11)
    res = {"calls": args.calls}
    if args.calls > 0:
        for q, it, rt in qs[args.calls:]:  # warm-up: every launch shape and the scratch sizes
            e.recommend_for(q, it, rt, 3)
        times = []
        for q, it, rt in qs[:args.calls]:
            t0 = time.perf_counter()
            e.recommend_for(q, it, rt, 3)
            times.append(time.perf_counter() - t0)
        ms = np.array(times) * 1e3
        sizes = np.array([len(it) for _, it, _ in qs[:args.calls]])
        nbr_ratings = nnz / U * 300  # expected ratings of 300 neighbours at the mean row length
        res.update({
            "median_ms": float(np.median(ms)), "p90_ms": float(np.percentile(ms, 90)), "mean_ms": float(ms.mean()),
            "query_ratings_median": int(np.median(sizes)), "query_ratings_max": int(sizes.max()),
            # algorithmic bytes of one call: the similarity pass (s_col + u_ptr read, one fp64 per user written), the top-k
            # sort (8 radix passes over U 12-byte pairs, read + write), the neighbours' rows (s_col, s_t, s_dev gathered,
            # 28-byte records written, sorted: 6 passes) and the per-item prediction pass (num, den, pred, rated)
            "bytes_similarity": 4 * nnz + 8 * (U + 1) + 8 * U,
            "bytes_topk_sort": 8 * 2 * 12 * U,
            "bytes_prediction": int(nbr_ratings * (16 + 28 + 6 * 2 * 12)) + I * (8 + 8 + 8 + 1),
        })
        res["bytes_per_call"] = res["bytes_similarity"] + res["bytes_topk_sort"] + res["bytes_prediction"]
    else:
        for q, it, rt in qs[:args.prof_calls]:  # (the same queries as the timed run's first ones)
            e.recommend_for(q, it, rt, 3)
        res["calls"] = args.prof_calls
    res.update({"U": U, "I": I, "train_ratings": nnz})
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
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--prof-calls", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "fold_in"))
    ap.add_argument("--inner", action="store_true")
    args = ap.parse_args()
    if args.inner:
        return inner(args)
    os.makedirs(args.out, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__), "--inner"]
    res = _child(me + ["--calls", str(args.calls)], 900, os.path.join(args.out, "timing.log"))
    prof = {}
    for tag, calls in (("fit", 0), ("calls", args.prof_calls)):
        d = os.path.join(args.out, "prof_" + tag)
        _child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "fl", "--"] + me +
               ["--calls", "0", "--prof-calls", str(calls)], 900, os.path.join(args.out, f"prof_{tag}.log"))
        found = [os.path.join(r, f) for r, _, fs in os.walk(d) for f in fs if f.endswith("kernel_stats.csv")]
        prof[tag] = _stats(found[0])
    per_kernel = {}
    for name, (calls, ns) in prof["calls"].items():
        c0, ns0 = prof["fit"].get(name, (0, 0.0))
        if calls > c0:
            per_kernel[name[:120]] = {"calls_per_query": (calls - c0) / args.prof_calls,
                                            "us_per_query": (ns - ns0) / args.prof_calls / 1e3}
    res["device_us_per_call"] = sum(v["us_per_query"] for v in per_kernel.values())
    res["kernels"] = per_kernel
    res["bytes_per_s_at_device_time"] = res["bytes_per_call"] / (res["device_us_per_call"] * 1e-6)
    with open(os.path.join(args.out, "fold_in_latency.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
