"""Latency of the bystanders of update queries (BystanderQueries.predict_with, csrc/bystander.hip) at the ml-25m shape: the kNN
prediction of a FITTED user once ANOTHER fitted user has added ratings, without a refit.

Holds the last 1 .. 20 ratings of 64 users of syn-25m out of train (the changers and their additional rows), fits the rest once
(k = 300), warms up and times
  * one query with 1, 8 and 63 bystanders (one row each: a random fitted user and a random train item),
  * a batch of 64 queries x 4 bystanders,
as wall time per row.  Beside them, in the same run,
  (a) what a row replaces: fit(train ++ the changer's additional rows) followed by predict(PRED_KNN, v, i), timed for
      `--baseline-calls` changers.  CHECKED: a row is cheaper than that at every shape (exit status 1 otherwise);
  (b) the fold-in bystander row of the same shape: predict_for with the same additional rows under an id that is absent from
      train.  The ratio is reported, not judged.
Prints one JSON line.

    python scripts/update_bystander_latency.py [--reps 20] [--baseline-calls 3] [--out bench_out/update_bystander]

The GPU work runs in a child process under `timeout -k 10`."""
import argparse
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
CHANGERS, BATCH_ROWS = 64, 4


def _split(d, seed):
    """(train without the held-out rows, [(user, items, ratings)]): the last 1 .. 20 file rows of 64 users of 30 .. 400 ratings"""
    import numpy as np

    u = d.train.users
    users, counts = np.unique(u, return_counts=True)
    rng = np.random.default_rng(seed)
    pick = rng.choice(users[(counts >= 30) & (counts <= 400)], CHANGERS, replace=False)
    out = np.zeros(len(u), dtype=bool)
    queries = []
    for j, c in enumerate(pick):
        idx = np.flatnonzero(u == c)[-(1 + (j * 7) % 20):]
        out[idx] = True
        queries.append((int(c), d.train.items[idx], d.train.ratings[idx]))
    return (u[~out], d.train.items[~out], d.train.ratings[~out]), queries


def _stats(ms):
    import numpy as np

    ms = np.asarray(ms)
    return {"median_ms": float(np.median(ms)), "p90_ms": float(np.percentile(ms, 90)), "mean_ms": float(ms.mean())}


def _time_shapes(np, reps, single, batch, queries, rows):
    """per-row wall statistics of single(query, others, items) at SHAPES and of batch(queries, others, items) at 64 x 4"""
    res = {"single_query": {}}
    for m in SHAPES:
        for j in range(3):  # warm-up: every launch shape and the scratch sizes
            single(queries[j], rows[j][0][:m], rows[j][1][:m])
        times = []
        for j in range(reps):
            q, (vs, its) = queries[j % CHANGERS], rows[j % CHANGERS]
            t0 = time.perf_counter()
            single(q, vs[:m], its[:m])
            times.append((time.perf_counter() - t0) / m)
        res["single_query"][str(m)] = {"per_row": _stats(np.array(times) * 1e3)}
    others, pis = [r[0][:BATCH_ROWS] for r in rows], [r[1][:BATCH_ROWS] for r in rows]
    batch(queries, others, pis)
    times = []
    for _ in range(max(3, reps // 4)):
        t0 = time.perf_counter()
        _, st = batch(queries, others, pis)
        times.append((time.perf_counter() - t0) / (CHANGERS * BATCH_ROWS))
        assert not st.any()
    res["batch_64x4"] = {"per_row": _stats(np.array(times) * 1e3)}
    return res


def inner(args):
    """runs on the GPU"""
    import numpy as np

    kn = importlib.import_module(PKG + ".knncf")
    synth = importlib.import_module(PKG + ".synth")
    d = synth.syn_25m()
    train, queries = _split(d, seed=23)
    rng = np.random.default_rng(5)
    fitted, items = np.unique(train[0]), np.unique(train[1])
    rows = []
    for q in queries:  # 63 bystanders other than the changer
        vs = rng.choice(fitted[fitted != q[0]], 63, replace=False).astype(np.int32)
        rows.append((vs, rng.choice(items, 63).astype(np.int32)))
    res = {"k": 300, "additional_ratings_mean": float(np.mean([len(q[1]) for q in queries]))}
    e = kn.Engine(k=300)
    by = kn.BystanderQueries(e)
    # (a) the refit that a row replaces
    times = []
    for j in range(args.baseline_calls + 1):  # (the first one warms up)
        (c, it, rt), (vs, its) = queries[j], rows[j]
        aug = (np.concatenate([train[0], np.full(len(it), c, dtype=np.int32)]), np.concatenate([train[1], it]),
               np.concatenate([train[2], rt]))
        t0 = time.perf_counter()
        e.fit(*aug)
        e.predict(kn.PRED_KNN, int(vs[0]), int(its[0]))
        times.append(time.perf_counter() - t0)
    res["baseline_refit_and_predict"] = dict(_stats(np.array(times[1:]) * 1e3), calls=args.baseline_calls)
    e.fit(*train)
    res.update({"U": e.num_users, "I": e.num_items, "train_ratings": len(train[0])})
    res["update_bystander"] = _time_shapes(np, args.reps, lambda q, vs, its: by.predict_with(*q, vs, its), by.predict_with_batch, queries, rows)
    # (b) the same additional rows under ids that train does not know: fold-in bystander rows
    new_id = int(fitted.max()) + 1
    newcomers = [(new_id + j, q[1], q[2]) for j, q in enumerate(queries)]
    res["fold_in_bystander"] = _time_shapes(np, args.reps, lambda q, vs, its: by.predict_for(*q, vs, its), by.predict_for_batch, newcomers, rows)
    refit = res["baseline_refit_and_predict"]["median_ms"]
    ok = True
    for key in [str(m) for m in SHAPES] + ["batch"]:
        pick = lambda r: (r["batch_64x4"] if key == "batch" else r["single_query"][key])
        r, f = pick(res["update_bystander"]), pick(res["fold_in_bystander"])
        r["refit_over_row"] = refit / r["per_row"]["median_ms"]
        r["row_over_fold_in_row"] = r["per_row"]["median_ms"] / f["per_row"]["median_ms"]
        ok = ok and r["per_row"]["median_ms"] < refit
    res["every_row_cheaper_than_the_refit"] = ok
    e.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--baseline-calls", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "update_bystander"))
    ap.add_argument("--inner", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.inner:
        return inner(args)
    os.makedirs(args.out, exist_ok=True)
    cmd = ["timeout", "-k", "10", "900", sys.executable, os.path.abspath(__file__), "--inner", "--reps", str(args.reps),
           "--baseline-calls", str(args.baseline_calls)]
    log = os.path.join(args.out, "timing.log")
    with open(log, "w") as f:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=f, text=True, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit(f"the timed run failed with status {r.returncode} (log: {log})")
    res = json.loads(r.stdout.strip().splitlines()[-1])
    with open(os.path.join(args.out, "update_bystander_latency.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    if not res["every_row_cheaper_than_the_refit"]:
        raise SystemExit("a bystander row costs more than the refit it replaces")


if __name__ == "__main__":
    main()
