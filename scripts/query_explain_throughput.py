"""Time of explaining what a fold-in query recommends (Engine.explain_for_batch, csrc/foldin.hip k_qb_explain) at the ml-25m
shape, next to Engine.predict_for_batch on the same rows of the same tree.

The workload is that of scripts/fold_in_batch_throughput.py: syn-25m, k = 300, the 200 queries of fold_in_latency._queries
seed 11.  What a serving layer does: recommend_for_batch(n = 3), then explain_for_batch of each query's three recommended items
with cap = 16.  One child process fits once and, for B = 1, 8, 64 and 200 queries per call, warms up and times `--repeats`
passes over the queries for every leg: the recommendations, their explanation in both orders of the terms, and
predict_for_batch on the same (query, item) rows — the explain call is the predict call plus one small launch and the copy of
the terms.  Each figure is the median over the repeats, in µs per query, with min and standard deviation beside it.  Writes one
JSON file, prints it, and prints the table of DESIGN.md ("Explanations of query predictions") on stderr.

    python scripts/query_explain_throughput.py [--queries 200] [--repeats 5] [--out profiles/query_explain_syn25m_1gpu.json]

The GPU work runs in a child process under `timeout -k 10`; a failing step ends the run."""
import argparse
import importlib
import importlib.util
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "movie-recommender-system_amd"
K, N, CAP = 300, 3, 16
BATCHES = (1, 8, 64, 200)
LEGS = ("recommend", "explain_sum_order", "explain_by_weight", "predict")


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
    d = synth.syn_25m()
    e = kn.Engine(k=K)
    e.fit(d.train.users, d.train.items, d.train.ratings)
    qs = _latency_script()._queries(d, args.queries, seed=11)
    answers, st = e.recommend_for_batch(qs, N)
    assert (st == kn.OK).all()
    rows = [items for items, _ in answers]  # the recommended items of every query
    res = {"U": e.num_users, "I": e.num_items, "train_ratings": len(d.train.users), "queries": len(qs), "k": K, "n": N, "cap": CAP,
           "rows": int(sum(len(r) for r in rows)), "batch": {}}
    # the explanations against the predict call, once, outside the timing
    explained, st = e.explain_for_batch(qs, rows, CAP)
    predicted, _ = e.predict_for_batch(qs, rows)
    counts = np.concatenate([x[3] for x in explained])
    assert (st == kn.OK).all() and all(np.array_equal(x[5].view(np.int64), p.view(np.int64)) for x, p in zip(explained, predicted))
    res["terms_per_row_mean"], res["terms_per_row_max"] = float(counts.mean()), int(counts.max())
    res["rows_with_more_terms_than_cap"] = int((counts > CAP).sum())
    for B in BATCHES:
        chunks = [(qs[a:a + B], rows[a:a + B]) for a in range(0, len(qs), B)]
        legs = {"recommend": lambda c, r: e.recommend_for_batch(c, N),
                "explain_sum_order": lambda c, r: e.explain_for_batch(c, r, CAP, order=kn.EXPLAIN_SUM_ORDER),
                "explain_by_weight": lambda c, r: e.explain_for_batch(c, r, CAP, order=kn.EXPLAIN_BY_WEIGHT),
                "predict": lambda c, r: e.predict_for_batch(c, r)}
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
        for tag in ("explain_sum_order", "explain_by_weight"):
            out[tag]["over_predict_us_per_query"] = out[tag]["us_per_query_median"] - out["predict"]["us_per_query_median"]
            out[tag]["ratio_to_predict"] = out[tag]["us_per_query_median"] / out["predict"]["us_per_query_median"]
            out[tag]["with_recommend_us_per_query"] = out[tag]["us_per_query_median"] + out["recommend"]["us_per_query_median"]
        res["batch"][str(B)] = out
    e.close()
    print(json.dumps(res), flush=True)


def design_table(res):
    """the rows of DESIGN.md's table: µs per query, median (min, σ)"""
    cell = lambda s: f"{s['us_per_query_median']:.1f} ({s['us_per_query_min']:.1f}, {s['us_per_query_sigma']:.1f})"
    lines = ["| B | `recommend_for_batch` | `predict_for_batch` on the 3 items | `explain_for_batch`, `SUM_ORDER` | over predict | `BY_WEIGHT` | over predict |",
             "|---|---|---|---|---|---|---|"]
    for B in BATCHES:
        o = res["batch"][str(B)]
        lines.append(f"| {B} | {cell(o['recommend'])} | {cell(o['predict'])} | {cell(o['explain_sum_order'])} | "
                     f"{o['explain_sum_order']['over_predict_us_per_query']:+.1f} | {cell(o['explain_by_weight'])} | "
                     f"{o['explain_by_weight']['over_predict_us_per_query']:+.1f} |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_explain_syn25m_1gpu.json"))
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--inner", action="store_true")
    args = ap.parse_args()
    if args.inner:
        return inner(args)
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--inner", "--queries", str(args.queries),
           "--repeats", str(args.repeats)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit(f"the GPU step failed with status {r.returncode}")
    res = json.loads(r.stdout.strip().splitlines()[-1])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    print(design_table(res), file=sys.stderr)


if __name__ == "__main__":
    main()
