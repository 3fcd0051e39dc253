"""Latency of the entered queries of revise queries (EnteredQueries.entered_with(..., removed=...) / entered_with_batch,
csrc/entered.hip) at the ml-25m shape: whose kNN lists change when a FITTED user removes or re-rates items, without a refit.

Fits syn-25m once (k = 300) and takes the 64 fitted changers of scripts/revise_bystander_latency.py — changer j takes out its
last a + b file rows, a = 1 + j % 5 for good and b = 1 + (j // 5) % 5 given again with another value — and times, as medians of
wall time with the profiler off and every list built before the timed region,
  * one query per call and a batch of 64 queries per call (time per query), each as a count-only call (cap = 0) and with
    cap = 4096 (raised to the largest count if one is larger),
with the reported users per query and the tail rows per query that phase 2 resolved (min / mean / max) and phase 2's share of
the wall time, read from the `knncf-dispatch entered_update tails` lines of KNNCF_DEBUG_TRACE_DISPATCH in a pass of its own.
Beside them, in the same run on the same tree:
  (a) what a query replaces: fit(aug) followed by neighbors_batch over all users, timed for `--baseline-calls` changers;
  (b) entered_with WITHOUT removals for the same changers (the update queries of revise_bystander_latency.py: b additional rows
      on items they have not rated), the same four shapes.
Prints one JSON line.  No profiler pass: the kernels are those of scripts/update_entered_latency.py.

    python scripts/revise_entered_latency.py [--reps 64] [--baseline-calls 2] [--out bench_out/revise_entered]

The GPU step runs in a child process of its own under `timeout -k 10`."""
import argparse
import importlib
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
PKG = "movie-recommender-system_amd"

from revise_bystander_latency import CHANGERS, _aug, _queries  # noqa: E402
from update_entered_latency import _spread, _stats, _traced  # noqa: E402


def _shapes(np, reps, single, batch, queries, caps):
    """{shape: {cap key: per-query stats}} of single(q, cap) and batch(queries, cap)"""
    res = {"single_query": {}, "batch_64": {}}
    for cap, key in caps:
        single(queries[0], cap)
        times = []
        for j in range(reps):
            t0 = time.perf_counter()
            single(queries[j % CHANGERS], cap)
            times.append(time.perf_counter() - t0)
        res["single_query"][key] = {"per_query": _stats(np.array(times) * 1e3)}
        batch(queries, cap)
        times = []
        for _ in range(max(3, reps // 8)):
            t0 = time.perf_counter()
            st = batch(queries, cap)
            times.append((time.perf_counter() - t0) / CHANGERS)
            assert not st.any()
        res["batch_64"][key] = {"per_query": _stats(np.array(times) * 1e3)}
    return res


def _tails(en_single, en_batch, queries, cap):
    """the tail rows and phase 2's share, from the dispatch hook"""
    pat = re.compile(r"entered_update tails queries=(\d+) rows=(\d+) ms=([0-9.]+)")
    tails, wall, phase2 = [], 0.0, 0.0
    for q in queries:
        ms, text = _traced(lambda: en_single(q, cap))
        found = pat.findall(text)
        tails.append(sum(int(m[1]) for m in found))
        wall += ms
        phase2 += sum(float(m[2]) for m in found)
    ms, text = _traced(lambda: en_batch(queries, cap))
    found = pat.findall(text)
    return (dict(_spread(tails), batch_64_total=sum(int(m[1]) for m in found)),
            {"single_query": phase2 / wall, "batch_64": sum(float(m[2]) for m in found) / ms})


def inner(args):
    """runs on the GPU"""
    import numpy as np

    kn = importlib.import_module(PKG + ".knncf")
    synth = importlib.import_module(PKG + ".synth")
    d = synth.syn_25m()
    train = (d.train.users, d.train.items, d.train.ratings)
    revise, update = _queries(train, seed=23)
    fitted = np.unique(train[0]).astype(np.int32)
    res = {"k": 300, "changers": CHANGERS, "removed_items_mean": float(np.mean([len(q[1]) for q in revise])),
           "re_rated_items_mean": float(np.mean([len(q[2]) for q in revise]))}
    e = kn.Engine(k=300)
    en = kn.EnteredQueries(e)
    # (a) the refit and the full neighbour build that a query replaces
    times = []
    for j in range(args.baseline_calls + 1):  # (the first one warms up)
        aug = _aug(train, revise[j])
        t0 = time.perf_counter()
        e.fit(*aug)
        e.neighbors_batch(fitted)
        times.append(time.perf_counter() - t0)
    res["baseline_refit_and_neighbors_batch"] = dict(_stats(np.array(times[1:]) * 1e3), calls=args.baseline_calls)
    e.fit(*train)
    res.update({"U": e.num_users, "I": e.num_items, "train_ratings": len(train[0])})
    t0 = time.perf_counter()
    en.entered_with(revise[0][0], revise[0][2], revise[0][3], cap=0, removed=revise[0][1])
    res["first_call_builds_every_list_ms"] = (time.perf_counter() - t0) * 1e3

    rv_single = lambda q, cap: en.entered_with(q[0], q[2], q[3], cap=cap, removed=q[1])
    rv_batch = lambda qs, cap: en.entered_with_batch([(q[0], q[2], q[3]) for q in qs], cap=cap, removed=[q[1] for q in qs])[1]
    up_single = lambda q, cap: en.entered_with(*q, cap=cap)
    up_batch = lambda qs, cap: en.entered_with_batch(qs, cap=cap)[1]
    refit = res["baseline_refit_and_neighbors_batch"]["median_ms"]
    for name, single, batch, queries in (("revise", rv_single, rv_batch, revise), ("update_same_changers", up_single, up_batch, update)):
        counts = [len(single(q, None)[0]) for q in queries]  # (also the warm-up of every launch shape and scratch size)
        full = max(args.cap, max(counts))
        leg = {"reported_users_per_query": _spread(counts), "cap": full}
        leg.update(_shapes(np, args.reps, single, batch, queries, ((0, "count_only"), (full, "with_entries"))))
        leg["tail_rows_per_query"], leg["phase2_share_of_wall_time"] = _tails(single, batch, queries, full)
        for shape in ("single_query", "batch_64"):
            for r in leg[shape].values():
                r["refit_over_query"] = refit / r["per_query"]["median_ms"]
        res[name] = leg
    for shape in ("single_query", "batch_64"):
        for key, r in res["revise"][shape].items():
            r["over_update_same_changers"] = r["per_query"]["median_ms"] / res["update_same_changers"][shape][key]["per_query"]["median_ms"]
    res["query_cheaper_than_refit"] = all(r["refit_over_query"] > 1.0 for s in ("single_query", "batch_64") for r in res["revise"][s].values())
    e.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=64)
    ap.add_argument("--baseline-calls", type=int, default=2)
    ap.add_argument("--cap", type=int, default=4096, help="cells per query of the calls that ask for the entries")
    ap.add_argument("--timeout", type=int, default=900, help="seconds for the GPU step")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "revise_entered"))
    ap.add_argument("--inner", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.inner:
        return inner(args)
    os.makedirs(args.out, exist_ok=True)
    log = os.path.join(args.out, "timing.log")
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--inner", "--reps", str(args.reps),
           "--baseline-calls", str(args.baseline_calls), "--cap", str(args.cap)]
    with open(log, "w") as f:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=f, text=True, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit(f"step failed with status {r.returncode} (log: {log})")
    res = json.loads(r.stdout.strip().splitlines()[-1])
    with open(os.path.join(args.out, "revise_entered_latency.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
