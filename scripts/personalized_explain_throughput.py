"""Time of Engine.explain_personalized_batch (knncf_explain_personalized_batch, csrc/explain_all.hip) at the ml-25m shape next
to Engine.predict_batch(PRED_PERSONALIZED) on the same rows of the same handle: syn-25m, cap = 16.

Two settings over `--users` fitted users: their top-3 Personalized recommendations (recommend_batch(PRED_PERSONALIZED, users,
3)) — what a serving layer would ask to have explained; such items have few raters — and the three most-rated items of train
for every one of them, the long segments the select is built for.  One child process fits once; per setting a warm-up call of
each leg builds the rater copies and sizes every scratch buffer, then the three legs — predict, explain in summation order,
explain by weight — alternate `--repeats` times.  A call returns with the handle's streams drained, so the host clock around
it is the call's time; beside it stand the handle's rerank_ms (the exact similarity rows, the same work in every leg) and
predict_ms (row sort and fold for predict; row sort and k_explain_all for explain) of the call.  Medians, minima and standard
deviations; the cost of KNNCF_EXPLAIN_BY_WEIGHT over KNNCF_EXPLAIN_SUM_ORDER is the figure of interest.  Writes one JSON file
and prints it.

    python scripts/personalized_explain_throughput.py [--repeats 5] [--out profiles/personalized_explain_syn25m_1gpu.json]

The GPU work runs in a child process under `timeout -k 10`; a failing step ends the run."""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "movie-recommender-system_amd"
K, CAP = 300, 16


def _summary(values):
    import numpy as np

    v = np.asarray(values, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "sigma": float(v.std()), "repeats": len(v)}


def inner(args):
    import numpy as np

    sys.path.insert(0, ROOT)
    kn = importlib.import_module(PKG + ".knncf")
    synth = importlib.import_module(PKG + ".synth")
    note = lambda text: print(f"[personalized_explain_throughput] {text}", file=sys.stderr, flush=True)
    d = synth.syn_25m()
    note("data ready")
    e = kn.Engine(k=K)
    e.fit(d.train.users, d.train.items, d.train.ratings)
    known = np.unique(d.train.users).astype(np.int32)
    users = known[::max(1, len(known) // args.users)][:args.users].copy()
    items, _, counts = e.recommend_batch(kn.PRED_PERSONALIZED, users, 3)
    assert (counts == 3).all()
    ids, raters_of = np.unique(d.train.items, return_counts=True)
    heavy = ids[np.argsort(-raters_of, kind="stable")[:3]].astype(np.int32)
    settings = {"top3_recommendations": (np.repeat(users, 3), items.reshape(-1).astype(np.int32)),
                "three_most_rated_items": (np.repeat(users, 3), np.tile(heavy, len(users)))}
    res = {"U": e.num_users, "I": e.num_items, "train_ratings": len(d.train.users), "cap": CAP, "users": len(users), "settings": {}}
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.int64)

    def timed(call):
        before = e.timings()
        t0 = time.perf_counter()
        call()
        wall = (time.perf_counter() - t0) * 1e3
        after = e.timings()
        return wall, after["rerank_ms"] - before["rerank_ms"], after["predict_ms"] - before["predict_ms"]

    for name, (u, i) in settings.items():
        n = len(u)
        note(f"{name}: {n} rows")
        got = {}
        legs = {"predict": lambda: got.__setitem__("predict", e.predict_batch(kn.PRED_PERSONALIZED, u, i))}
        for tag, order in (("explain_sum_order", kn.EXPLAIN_SUM_ORDER), ("explain_by_weight", kn.EXPLAIN_BY_WEIGHT)):
            legs[tag] = lambda tag=tag, order=order: got.__setitem__(tag, e.explain_personalized_batch(u, i, CAP, order=order))
        for call in legs.values():  # warm-up: the rater copies, the scratch sizes, the code objects
            call()
        for tag in ("explain_sum_order", "explain_by_weight"):  # the same predictions, bit for bit
            assert np.array_equal(bits(got[tag][5]), bits(got["predict"]))
        wall, rows_ms, rest_ms = ({t: [] for t in legs} for _ in range(3))
        for _ in range(args.repeats):
            for tag, call in legs.items():  # alternating
                w, r, p = timed(call)
                wall[tag].append(w)
                rows_ms[tag].append(r)
                rest_ms[tag].append(p)
        c = got["explain_by_weight"][3]
        out = {"rows": n, "terms_per_row_mean": float(c.mean()), "terms_per_row_max": int(c.max()),
               "rows_with_more_terms_than_cap": int((c > CAP).sum())}
        for tag in legs:
            out[tag] = {"call_ms": _summary(wall[tag]), "rerank_ms": _summary(rows_ms[tag]), "predict_ms": _summary(rest_ms[tag]),
                        "us_per_row": float(np.median(wall[tag])) * 1e3 / n}
        for tag in ("explain_sum_order", "explain_by_weight"):
            out[tag]["ratio_to_predict_call"] = out[tag]["call_ms"]["median"] / out["predict"]["call_ms"]["median"]
        out["by_weight_over_sum_order_call_ms"] = out["explain_by_weight"]["call_ms"]["median"] - out["explain_sum_order"]["call_ms"]["median"]
        out["by_weight_over_sum_order_predict_ms"] = (out["explain_by_weight"]["predict_ms"]["median"]
                                                      - out["explain_sum_order"]["predict_ms"]["median"])
        res["settings"][name] = out
    e.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--users", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "personalized_explain_syn25m_1gpu.json"))
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--inner", action="store_true")
    args = ap.parse_args()
    if args.inner:
        return inner(args)
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--inner", "--repeats", str(args.repeats),
           "--users", str(args.users)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit(f"the GPU step failed with status {r.returncode}")
    res = json.loads(r.stdout.strip().splitlines()[-1])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
