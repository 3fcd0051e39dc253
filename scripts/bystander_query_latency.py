"""Latency of bystander queries (BystanderQueries.predict_for, csrc/bystander.hip) at the ml-25m shape: the kNN prediction of
a FITTED user once a newcomer has joined the data, without a refit.

Takes 64 users of syn-25m out of train entirely (the newcomers), fits the rest once (k = 300), warms up and times
  * one query with 1, 8 and 63 bystanders (one row each: a random fitted user and a random train item),
  * a batch of 64 queries x 4 bystanders,
as wall time per row.  Beside them
  (a) what the call replaces: fit(train ++ the newcomer's rows) followed by predict(PRED_KNN, v, i), timed for
      `--baseline-calls` newcomers.  It uses nothing but Engine.fit / Engine.predict, so `--baseline-only` runs unchanged on a
      tree that lacks the bystander calls;
  (b) predict_with(v, [], [], [i]) for the same bystanders on the same build: the update query without rows that a bystander
      slot extends by the pair, the merge and the newcomer's share of the fold.  The ratio to (b) is reported, not judged.
Then it repeats the 8-bystander shape under `rocprofv3 --kernel-trace --stats` in two child processes — the fit alone, and the
fit plus the profiled calls — and reports the device time of each kernel per call as the difference over the number of calls
(the radix-sort kernels are shared with the fit).  Prints one JSON line.

    python scripts/bystander_query_latency.py [--reps 20] [--baseline-calls 3] [--baseline-only] [--prof-calls 20]
                                              [--out bench_out/bystander_query]

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
SHAPES = (1, 8, 63)
NEWCOMERS, BATCH_ROWS = 64, 4


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
    rng = np.random.default_rng(5)
    fitted, items = np.unique(train[0]), np.unique(train[1])
    rows = [(rng.choice(fitted, 63, replace=False).astype(np.int32), rng.choice(items, 63).astype(np.int32)) for _ in queries]
    res = {"k": 300, "newcomer_ratings_mean": float(np.mean([len(q[1]) for q in queries]))}
    e = kn.Engine(k=300)
    by = kn.BystanderQueries(e)
    if args.prof_calls >= 0:  # under the profiler: the fit, then that many calls of the 8-bystander shape
        e.fit(*train)
        for j in range(args.prof_calls):
            q, (vs, its) = queries[j % NEWCOMERS], rows[j % NEWCOMERS]
            by.predict_for(*q, vs[:8], its[:8])
        e.close()
        print(json.dumps({"calls": args.prof_calls}), flush=True)
        return
    # (a) the refit that a row replaces
    times = []
    for j in range(args.baseline_calls + 1):  # (the first one warms up)
        (q, it, rt), (vs, its) = queries[j], rows[j]
        aug = (np.concatenate([train[0], np.full(len(it), q, dtype=np.int32)]), np.concatenate([train[1], it]),
               np.concatenate([train[2], rt]))
        t0 = time.perf_counter()
        e.fit(*aug)
        e.predict(kn.PRED_KNN, int(vs[0]), int(its[0]))
        times.append(time.perf_counter() - t0)
    res["baseline_refit_and_predict"] = dict(_stats(np.array(times[1:]) * 1e3), calls=args.baseline_calls)
    if not args.baseline_only:
        e.fit(*train)
        res.update({"U": e.num_users, "I": e.num_items, "train_ratings": len(train[0])})
        res["single_query"] = {}
        for m in SHAPES:
            for j in range(3):  # warm-up: every launch shape and the scratch sizes
                by.predict_for(*queries[j], rows[j][0][:m], rows[j][1][:m])
            times = []
            for j in range(args.reps):
                q, (vs, its) = queries[j % NEWCOMERS], rows[j % NEWCOMERS]
                t0 = time.perf_counter()
                by.predict_for(*q, vs[:m], its[:m])
                times.append((time.perf_counter() - t0) / m)
            res["single_query"][str(m)] = {"per_row": _stats(np.array(times) * 1e3)}
        others, pis = [r[0][:BATCH_ROWS] for r in rows], [r[1][:BATCH_ROWS] for r in rows]
        by.predict_for_batch(queries, others, pis)
        times = []
        for _ in range(max(3, args.reps // 4)):
            t0 = time.perf_counter()
            _, st = by.predict_for_batch(queries, others, pis)
            times.append((time.perf_counter() - t0) / (NEWCOMERS * BATCH_ROWS))
            assert not st.any()
        res["batch_64x4"] = {"per_row": _stats(np.array(times) * 1e3)}
        # (b) the same bystanders as update queries without rows
        none_i, none_r = np.empty(0, dtype=np.int32), np.empty(0)
        for j in range(3):
            e.predict_with(int(rows[0][0][j]), none_i, none_r, rows[0][1][j:j + 1])
        times = []
        for j in range(args.reps):
            vs, its = rows[j % NEWCOMERS]
            t0 = time.perf_counter()
            e.predict_with(int(vs[0]), none_i, none_r, its[:1])
            times.append(time.perf_counter() - t0)
        res["predict_with_no_rows"] = {"per_row": _stats(np.array(times) * 1e3)}
        refit = res["baseline_refit_and_predict"]["median_ms"]
        base = res["predict_with_no_rows"]["per_row"]["median_ms"]
        for key, r in list(res["single_query"].items()) + [("batch", res["batch_64x4"])]:
            r["refit_over_row"] = refit / r["per_row"]["median_ms"]
            r["row_over_predict_with"] = r["per_row"]["median_ms"] / base
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
    ap.add_argument("--baseline-calls", type=int, default=3)
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--prof-calls", type=int, default=20, help="calls under the profiler (0: no profiler runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "bystander_query"))
    ap.add_argument("--inner", type=int, default=None, help=argparse.SUPPRESS)  # -1: the timed run, n >= 0: n profiled calls
    args = ap.parse_args()
    if args.inner is not None:
        args.prof_calls = args.inner
        return inner(args)
    os.makedirs(args.out, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__)]
    res = _child(me + ["--inner", "-1", "--reps", str(args.reps), "--baseline-calls", str(args.baseline_calls)] +
                 (["--baseline-only"] if args.baseline_only else []), 900, os.path.join(args.out, "timing.log"))
    if not args.baseline_only and args.prof_calls > 0:
        prof = {}
        for tag, calls in (("fit", 0), ("calls", args.prof_calls)):
            d = os.path.join(args.out, "prof_" + tag)
            _child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "by", "--"] + me +
                   ["--inner", str(calls)], 900, os.path.join(args.out, f"prof_{tag}.log"))
            found = [os.path.join(r, f) for r, _, fs in os.walk(d) for f in fs if f.endswith("kernel_stats.csv")]
            prof[tag] = _kernel_stats(found[0])
        per_kernel = {}
        for name, (calls, ns) in prof["calls"].items():
            c0, ns0 = prof["fit"].get(name, (0, 0.0))
            if calls > c0:
                per_kernel[name[:120]] = {"launches_per_call": (calls - c0) / args.prof_calls, "us_per_call": (ns - ns0) / args.prof_calls / 1e3}
        res["profiled_shape"] = "one query, 8 bystanders"
        res["device_us_per_call"] = sum(v["us_per_call"] for v in per_kernel.values())
        res["kernels"] = per_kernel
    with open(os.path.join(args.out, "bystander_query_latency.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
