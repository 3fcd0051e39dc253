"""Time of explaining what a Personalized fold-in query recommends (Engine.explain_for_batch(..., predictor=PRED_PERSONALIZED),
csrc/foldin.hip k_qb_explain_all) at the ml-25m shape, next to Engine.predict_for_batch(PRED_PERSONALIZED) on the same rows of
the same handle.

The workload is that of scripts/query_explain_throughput.py: syn-25m, the 200 queries of fold_in_latency._queries seed 11.  What
a serving layer does: recommend_for_batch(n = 3, PRED_PERSONALIZED), then explain_for_batch of each query's three recommended
items with cap = 16 by weight.  One child process fits once and, for B = 1, 8, 64 and 200 queries per call, warms up and times
`--repeats` passes over the queries for every leg: the recommendations, their explanation, and predict_for_batch on the same
(query, item) rows.  The explain call and the predict call pay the same chunk fold (k_qb_fold_all); what differs is
k_qb_explain_all and the copy of the terms against k_qb_pick_all and the copy of one number per row.  Each figure is the median
over the repeats, in µs per query, with min and standard deviation beside it; the figures to read are explain over predict on
the same rows and the absolute time per explained row.  Unless --no-profile is given, one pass at B = 64 of the explain leg
is repeated under `rocprofv3 --kernel-trace --stats` in a child process of its own for the device time of k_qb_fold_all and
k_qb_explain_all.  Writes one JSON file and prints it.

    python scripts/personalized_query_explain_throughput.py [--queries 200] [--repeats 5]
        [--out profiles/personalized_query_explain_syn25m_1gpu.json]

The GPU work runs in child processes under `timeout -k 10`; a failing step ends the run."""
import argparse
import csv
import importlib
import importlib.util
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "movie-recommender-system_amd"
K, N, CAP = 300, 3, 16
BATCHES = (1, 8, 64, 200)
PROFILE_B = 64
KERNELS = ("k_qb_fold_all", "k_qb_explain_all")


def _latency_script():
    spec = importlib.util.spec_from_file_location("fold_in_latency", os.path.join(ROOT, "scripts", "fold_in_latency.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _summary(seconds, n_queries):
    import numpy as np

    us = np.array(seconds) * 1e6 / n_queries
    return {"us_per_query_median": float(np.median(us)), "us_per_query_min": float(us.min()), "us_per_query_sigma": float(us.std()),
            "repeats": len(seconds)}


def inner(args):
    import numpy as np

    sys.path.insert(0, ROOT)
    kn = importlib.import_module(PKG + ".knncf")
    synth = importlib.import_module(PKG + ".synth")
    P = kn.PRED_PERSONALIZED
    d = synth.syn_25m()
    e = kn.Engine(k=K)
    e.fit(d.train.users, d.train.items, d.train.ratings)
    qs = _latency_script()._queries(d, args.queries, seed=11)
    answers, st = e.recommend_for_batch(qs, N, predictor=P)
    assert (st == kn.OK).all()
    rows = [items for items, _ in answers]  # the recommended items of every query
    explain = lambda c, r: e.explain_for_batch(c, r, CAP, order=kn.EXPLAIN_BY_WEIGHT, predictor=P)
    if args.profile:  # under the profiler: one pass of the explain leg at B = PROFILE_B
        for a in range(0, len(qs), PROFILE_B):
            explain(qs[a:a + PROFILE_B], rows[a:a + PROFILE_B])
        e.close()
        print(json.dumps({"queries": len(qs), "rows": int(sum(len(r) for r in rows))}), flush=True)
        return
    res = {"U": e.num_users, "I": e.num_items, "train_ratings": len(d.train.users), "queries": len(qs), "n": N, "cap": CAP,
           "order": "KNNCF_EXPLAIN_BY_WEIGHT", "rows": int(sum(len(r) for r in rows)), "batch": {}}
    # the explanations against the predict call, once, outside the timing
    explained, st = explain(qs, rows)
    predicted, _ = e.predict_for_batch(qs, rows, predictor=P)
    counts = np.concatenate([x[3] for x in explained])
    assert (st == kn.OK).all() and all(np.array_equal(x[5].view(np.int64), p.view(np.int64)) for x, p in zip(explained, predicted))
    res["terms_per_row_mean"], res["terms_per_row_max"] = float(counts.mean()), int(counts.max())
    res["rows_with_more_terms_than_cap"] = int((counts > CAP).sum())
    n_rows = res["rows"]
    for B in BATCHES:
        chunks = [(qs[a:a + B], rows[a:a + B]) for a in range(0, len(qs), B)]
        legs = {"recommend": lambda c, r: e.recommend_for_batch(c, N, predictor=P),
                "explain_by_weight": explain,
                "predict": lambda c, r: e.predict_for_batch(c, r, predictor=P)}
        for call in legs.values():  # warm-up: every launch shape and the scratch sizes
            for c, r in chunks[:2]:
                call(c, r)
        runs = {tag: [] for tag in legs}
        for _ in range(args.repeats):
            for tag, call in legs.items():  # alternating
                t0 = time.perf_counter()
                for c, r in chunks:
                    call(c, r)
                runs[tag].append(time.perf_counter() - t0)
        out = {tag: _summary(runs[tag], len(qs)) for tag in legs}
        x = out["explain_by_weight"]
        x["over_predict_us_per_query"] = x["us_per_query_median"] - out["predict"]["us_per_query_median"]
        x["ratio_to_predict"] = x["us_per_query_median"] / out["predict"]["us_per_query_median"]
        x["us_per_explained_row"] = x["us_per_query_median"] * len(qs) / n_rows
        x["with_recommend_us_per_query"] = x["us_per_query_median"] + out["recommend"]["us_per_query_median"]
        res["batch"][str(B)] = out
    e.close()
    print(json.dumps(res), flush=True)


def _child(argv, timeout_s):
    r = subprocess.run(["timeout", "-k", "10", str(timeout_s)] + argv, stdout=subprocess.PIPE, text=True, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit(f"the GPU step failed with status {r.returncode}: {' '.join(argv)}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "personalized_query_explain_syn25m_1gpu.json"))
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--commit", default="", help="the commit the library was built from, recorded in the output")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--inner", action="store_true")
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    if args.inner:
        return inner(args)
    me = [sys.executable, os.path.abspath(__file__), "--inner", "--queries", str(args.queries), "--repeats", str(args.repeats)]
    res = _child(me, args.timeout)
    res["measured_on"] = args.commit
    if not args.no_profile:
        with tempfile.TemporaryDirectory() as d:
            shape = _child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "pqx", "--"] + me + ["--profile"],
                           args.timeout)
            found = [os.path.join(r, f) for r, _, fs in os.walk(d) for f in fs if f.endswith("kernel_stats.csv")]
            kernels = {}
            with open(found[0]) as f:
                for row in csv.DictReader(f):
                    for name in KERNELS:
                        if name in row["Name"]:
                            # (k_qb_fold_all also ran in the recommend pass that picked the rows, over chunks of the same sizes:
                            # the explain pass is `chunks` of its calls)
                            calls, ns = int(row["Calls"]), float(row["TotalDurationNs"])
                            chunks = -(-shape["queries"] // PROFILE_B)
                            kernels[name] = {"calls": calls, "us_per_call": ns / calls / 1e3,
                                             "explain_pass_us_per_query": ns / calls * chunks / shape["queries"] / 1e3,
                                             "explain_pass_us_per_row": ns / calls * chunks / shape["rows"] / 1e3}
        res["profile_batch"] = PROFILE_B
        res["kernels"] = kernels
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
