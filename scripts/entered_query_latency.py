"""Latency of entered queries (EnteredQueries.entered / entered_batch, csrc/entered.hip) at the ml-25m shape: which fitted
users' neighbour lists a newcomer joins, without a refit.

Takes 64 users of syn-25m out of train entirely (the newcomers), fits the rest once (k = 300) and times, as medians of wall
time with the profiler off and every list built before the timed region,
  * one query per call and a batch of 64 queries per call (time per query), each as a count-only call (cap = 0) and with a
    cap that holds every entered user,
beside them, in the same run,
  (a) what a query replaces: fit(train ++ the newcomer's rows) followed by neighbors_batch over all users of the fit, timed
      for `--baseline-calls` newcomers.  It uses nothing but Engine.fit / Engine.neighbors_batch, so `--baseline-only` runs
      unchanged on a tree that lacks the entered calls;
  (b) separately, the first call's one-off build of the missing lists on a fresh handle (all of them).
Then it repeats the single-query shape under `rocprofv3 --kernel-trace --stats` in a child process of its own and reports the
device time per launch of the three kernels of entered.hip.  Prints one JSON line.

    python scripts/entered_query_latency.py [--reps 20] [--baseline-calls 2] [--baseline-only] [--prof-calls 20]
                                            [--out bench_out/entered_query]

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
NEWCOMERS = 64
KERNELS = ("k_en_pair", "k_en_flag", "k_en_compact", "k_en_place")


def _split(d, seed):
    """(train without the newcomers' rows, [(user, items, ratings)] of the newcomers): 64 users of 10 .. 400 ratings"""
    import numpy as np

    u = d.train.users
    users, counts = np.unique(u, return_counts=True)
    rng = np.random.default_rng(seed)
    pick = rng.choice(users[(counts >= 10) & (counts <= 400)], NEWCOMERS, replace=False)
    out = np.isin(u, pick)
    queries = [(int(q), d.train.items[u == q], d.train.ratings[u == q]) for q in pick]
    return (u[~out], d.train.items[~out], d.train.ratings[~out]), queries


def _stats(ms):
    import numpy as np

    ms = np.asarray(ms)
    return {"median_ms": float(np.median(ms)), "p90_ms": float(np.percentile(ms, 90)), "mean_ms": float(ms.mean())}


def inner(args):
    """runs on the GPU"""
    import numpy as np

    kn = importlib.import_module(PKG + ".knncf")
    synth = importlib.import_module(PKG + ".synth")
    d = synth.syn_25m()
    train, queries = _split(d, seed=17)
    fitted = np.unique(train[0]).astype(np.int32)
    res = {"k": 300, "newcomer_ratings_mean": float(np.mean([len(q[1]) for q in queries]))}
    e = kn.Engine(k=300)
    en = kn.EnteredQueries(e)
    if args.prof_calls >= 0:  # under the profiler: the fit, the build of every list, then that many single queries
        e.fit(*train)
        en.entered(*queries[0], cap=0)
        for j in range(args.prof_calls):
            en.entered(*queries[j % NEWCOMERS], cap=args.cap)
        e.close()
        print(json.dumps({"calls": args.prof_calls}), flush=True)
        return
    # (a) the refit and the full neighbour build that a query replaces
    times = []
    for j in range(args.baseline_calls + 1):  # (the first one warms up)
        q, it, rt = queries[j]
        aug = (np.concatenate([train[0], np.full(len(it), q, dtype=np.int32)]), np.concatenate([train[1], it]),
               np.concatenate([train[2], rt]))
        users = np.concatenate([fitted, np.asarray([q], dtype=np.int32)])
        t0 = time.perf_counter()
        e.fit(*aug)
        e.neighbors_batch(users)
        times.append(time.perf_counter() - t0)
    res["baseline_refit_and_neighbors_batch"] = dict(_stats(np.array(times[1:]) * 1e3), calls=args.baseline_calls)
    if not args.baseline_only:
        # (b) the first call on a fresh fit builds every list
        e.fit(*train)
        res.update({"U": e.num_users, "I": e.num_items, "train_ratings": len(train[0])})
        t0 = time.perf_counter()
        en.entered(*queries[0], cap=0)
        res["first_call_builds_every_list_ms"] = (time.perf_counter() - t0) * 1e3
        counts = [len(en.entered(*q)[0]) for q in queries]  # (also the warm-up of every launch shape and scratch size)
        res["entered_users"] = {"mean": float(np.mean(counts)), "min": int(min(counts)), "max": int(max(counts))}
        full = max(args.cap, max(counts))  # (holds every entered user of every newcomer)
        res["cap"] = full
        for cap, key in ((0, "count_only"), (full, "with_entries")):
            en.entered(*queries[0], cap=cap)
            times = []
            for j in range(args.reps):
                t0 = time.perf_counter()
                en.entered(*queries[j % NEWCOMERS], cap=cap)
                times.append(time.perf_counter() - t0)
            res.setdefault("single_query", {})[key] = {"per_query": _stats(np.array(times) * 1e3)}
            en.entered_batch(queries, cap=cap)
            times = []
            for _ in range(max(3, args.reps // 4)):
                t0 = time.perf_counter()
                _, st = en.entered_batch(queries, cap=cap)
                times.append((time.perf_counter() - t0) / NEWCOMERS)
                assert not st.any()
            res.setdefault("batch_64", {})[key] = {"per_query": _stats(np.array(times) * 1e3)}
        refit = res["baseline_refit_and_neighbors_batch"]["median_ms"]
        for shape in ("single_query", "batch_64"):
            for r in res[shape].values():
                r["refit_over_query"] = refit / r["per_query"]["median_ms"]
        res["query_cheaper_than_refit"] = all(r["refit_over_query"] > 1.0 for s in ("single_query", "batch_64") for r in res[s].values())
    e.close()
    print(json.dumps(res), flush=True)


def _child(argv, timeout_s, log):
    cmd = ["timeout", "-k", "10", str(timeout_s)] + argv
    with open(log, "w") as f:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=f, text=True, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit(f"step failed with status {r.returncode}: {' '.join(argv)} (log: {log})")
    return json.loads(r.stdout.strip().splitlines()[-1])


def _kernel_stats(path):
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            out[row["Name"]] = (int(row["Calls"]), float(row["TotalDurationNs"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--baseline-calls", type=int, default=2)
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--cap", type=int, default=4096, help="cells per query of the calls that ask for the entries")
    ap.add_argument("--prof-calls", type=int, default=20, help="calls under the profiler (0: no profiler run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "entered_query"))
    ap.add_argument("--inner", type=int, default=None, help=argparse.SUPPRESS)  # -1: the timed run, n >= 0: n profiled calls
    args = ap.parse_args()
    if args.inner is not None:
        args.prof_calls = args.inner
        return inner(args)
    os.makedirs(args.out, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__)]
    res = _child(me + ["--inner", "-1", "--reps", str(args.reps), "--baseline-calls", str(args.baseline_calls), "--cap", str(args.cap)] +
                 (["--baseline-only"] if args.baseline_only else []), 900, os.path.join(args.out, "timing.log"))
    if not args.baseline_only and args.prof_calls > 0:
        d = os.path.join(args.out, "prof")
        _child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "en", "--"] + me +
               ["--inner", str(args.prof_calls), "--cap", str(args.cap)], 900, os.path.join(args.out, "prof.log"))
        found = [os.path.join(r, f) for r, _, fs in os.walk(d) for f in fs if f.endswith("kernel_stats.csv")]
        per_kernel = {}
        for name, (calls, ns) in _kernel_stats(found[0]).items():
            for k in KERNELS:
                if k in name:
                    per_kernel[k] = {"launches": calls, "us_per_launch": ns / calls / 1e3}
        res["profiled_shape"] = f"one query per call, cap = {args.cap} (k_en_pair runs only for a newcomer of <= 4 ratings: none here)"
        res["kernels"] = per_kernel
    with open(os.path.join(args.out, "entered_query_latency.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
