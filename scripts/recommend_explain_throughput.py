"""Time of recommending and explaining in one pass (Engine.recommend_explain_for_batch, knncf_query_recommend_explain_batch)
at the ml-25m shape, next to the two calls it replaces on the same tree: recommend_for_batch, then explain_for_batch of the
recommended items.

The workload is that of scripts/query_explain_throughput.py: syn-25m, k = 300, the 200 queries of fold_in_latency._queries
seed 11, n = 3 recommendations per query, cap = 16 terms per row.  One child process fits once.  Before any timing it asserts,
once per predictor and order, that the fused answer equals the two calls' on bit views.  Then, for PRED_KNN at B = 1, 8, 64 and
200 queries per call and for PRED_PERSONALIZED at B = 1 and 64, in both orders of the terms, it warms up and times `--repeats`
passes over the queries for two legs:

  recommend_then_explain  recommend_for_batch, then explain_for_batch with pred_items = the items just returned
  recommend_explain       the fused call

Each figure is the median over the repeats, in µs per query, with min and standard deviation beside it.  `--baseline-only`
runs the first leg alone: it uses no entry point of the fused call, so it runs unchanged on a tree that lacks it.  Writes one
JSON file, prints it, and prints the table of DESIGN.md ("Recommendations with their explanations") on stderr.

    python scripts/recommend_explain_throughput.py [--queries 200] [--repeats 5] [--baseline-only] [--commit LABEL]
                                                   [--out profiles/recommend_explain_syn25m_1gpu.json]

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
BATCHES = {"knn": (1, 8, 64, 200), "personalized": (1, 64)}
ORDERS = ("sum_order", "by_weight")
LEGS = ("recommend_then_explain", "recommend_explain")


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


def _bits(a):
    import numpy as np

    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _assert_fused_equals_two_calls(kn, e, qs, predictor, order):
    """once, outside the timing: items, predictions, terms, counts and sums of every query, == on bit views"""
    import numpy as np

    reco, st = e.recommend_for_batch(qs, N, predictor=predictor)
    expl, st2 = e.explain_for_batch(qs, [items for items, _ in reco], CAP, order=order, predictor=predictor)
    fused, st3 = e.recommend_explain_for_batch(qs, N, CAP, order=order, predictor=predictor)
    assert (st == kn.OK).all() and (st2 == kn.OK).all() and (st3 == kn.OK).all()
    for (items, preds), terms, got in zip(reco, expl, fused):
        assert np.array_equal(got[0], items) and np.array_equal(_bits(got[1]), _bits(preds)) and np.array_equal(_bits(terms[5]), _bits(preds))
        for g, w in zip(got[2:], terms[:5]):  # (the padding is nan on both sides: bit views compare it too)
            assert g.shape == w.shape and np.array_equal(_bits(g), _bits(w))


def inner(args):
    sys.path.insert(0, ROOT)
    kn = importlib.import_module(PKG + ".knncf")
    synth = importlib.import_module(PKG + ".synth")
    d = synth.syn_25m()
    e = kn.Engine(k=K)
    e.fit(d.train.users, d.train.items, d.train.ratings)
    qs = _latency_script()._queries(d, args.queries, seed=11)
    predictors = {"knn": kn.PRED_KNN, "personalized": kn.PRED_PERSONALIZED}
    orders = {"sum_order": kn.EXPLAIN_SUM_ORDER, "by_weight": kn.EXPLAIN_BY_WEIGHT}
    res = {"U": e.num_users, "I": e.num_items, "train_ratings": len(d.train.users), "queries": len(qs), "k": K, "n": N, "cap": CAP,
           "baseline_only": bool(args.baseline_only), "legs": {}}
    for pname, predictor in predictors.items():
        if not args.baseline_only:
            for order in orders.values():
                _assert_fused_equals_two_calls(kn, e, qs, predictor, order)
        res["legs"][pname] = {}
        for B in BATCHES[pname]:
            chunks = [qs[a:a + B] for a in range(0, len(qs), B)]
            res["legs"][pname][str(B)] = {}
            for oname, order in orders.items():
                def two_calls(c):
                    reco, _ = e.recommend_for_batch(c, N, predictor=predictor)
                    e.explain_for_batch(c, [items for items, _ in reco], CAP, order=order, predictor=predictor)

                legs = {"recommend_then_explain": two_calls}
                if not args.baseline_only:
                    legs["recommend_explain"] = lambda c: e.recommend_explain_for_batch(c, N, CAP, order=order, predictor=predictor)
                for call in legs.values():  # warm-up: every launch shape and the scratch sizes
                    for c in chunks[:2]:
                        call(c)
                runs = {tag: [] for tag in legs}
                for _ in range(args.repeats):
                    for tag, call in legs.items():  # alternating
                        t0 = time.perf_counter()
                        for c in chunks:
                            call(c)
                        runs[tag].append(time.perf_counter() - t0)
                res["legs"][pname][str(B)][oname] = {tag: _summary(runs[tag], len(qs)) for tag in legs}
    e.close()
    print(json.dumps(res), flush=True)


def design_table(res):
    """the rows of DESIGN.md's table: µs per query, median (min, σ)"""
    cell = lambda s: f"{s['us_per_query_median']:.1f} ({s['us_per_query_min']:.1f}, {s['us_per_query_sigma']:.1f})"
    lines = ["| predictor | B | order | `recommend_for_batch` then `explain_for_batch` | `recommend_explain_for_batch` |", "|---|---|---|---|---|"]
    for pname, by_batch in res["legs"].items():
        for B, by_order in by_batch.items():
            for oname, legs in by_order.items():
                fused = cell(legs["recommend_explain"]) if "recommend_explain" in legs else "-"
                lines.append(f"| {pname} | {B} | {oname} | {cell(legs['recommend_then_explain'])} | {fused} |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--commit", default="", help="label written into the result")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recommend_explain_syn25m_1gpu.json"))
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--inner", action="store_true")
    args = ap.parse_args()
    if args.inner:
        return inner(args)
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--inner", "--queries", str(args.queries),
           "--repeats", str(args.repeats)] + (["--baseline-only"] if args.baseline_only else [])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit(f"the GPU step failed with status {r.returncode}")
    res = json.loads(r.stdout.strip().splitlines()[-1])
    res["commit"] = args.commit
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    print(design_table(res), file=sys.stderr)


if __name__ == "__main__":
    main()
