"""Latency of the bystanders of revise queries (BystanderQueries.predict_with(..., removed=...), csrc/bystander.hip) at the ml-25m shape: the kNN
prediction of a FITTED user once ANOTHER fitted user has removed and re-rated items, without a refit.

Fits syn-25m once (k = 300).  64 fitted changers each take out the last 2 .. 10 of their train ratings in file order: 1 .. 5 of
them for good, 1 .. 5 given again with another value.  Warms up and times
  * one query with 1, 8 and 63 bystanders (one row each: a random fitted user and a random train item),
  * a batch of 64 queries x 4 bystanders,
as wall time per row.  Beside them, in the same run,
  (a) what a row replaces: fit(aug) followed by predict(PRED_KNN, v, i), timed for `--baseline-calls` changers.  CHECKED: a row
      is cheaper than that at every shape (exit status 1 otherwise);
  (b) the update-bystander row of the same shape: predict_with for the same changer with as many additional rows on items it has
      not rated.  The ratio is reported, not judged.
  (c) on an off-scale copy of the data (ratings round(0.93 r + 0.1, 2): not dyadic, so the fit sums sequentially and average(aug)
      of a query with removals is folded anew): one query of one fitted bystander, with and without a second row that names a user
      unknown to aug — the row answered with average(aug).  The difference of the medians is the re-fold.
Prints one JSON line.

    python scripts/revise_bystander_latency.py [--reps 20] [--baseline-calls 3] [--out bench_out/revise_bystander]
    python scripts/revise_bystander_latency.py --inner --off-scale-only     (the leg (c) alone, for a kernel trace of its own)

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
UNKNOWN_USER = 2**30


def _queries(train, seed):
    """[(user, removed items, additional items, additional ratings)] of 64 users of 30 .. 400 ratings: changer j takes out its last
    a + b file rows, a = 1 + j % 5 for good and b = 1 + (j // 5) % 5 given again with another value; and [(user, items, ratings)],
    the update queries of the same users with b additional rows on items they have not rated"""
    import numpy as np

    u, i, r = train
    users, counts = np.unique(u, return_counts=True)
    rng = np.random.default_rng(seed)
    pick = rng.choice(users[(counts >= 30) & (counts <= 400)], CHANGERS, replace=False)
    all_items = np.unique(i)
    revise, update = [], []
    for j, c in enumerate(pick):
        a, b = 1 + j % 5, 1 + (j // 5) % 5
        idx = np.flatnonzero(u == c)
        gone, again = idx[-(a + b):], idx[-b:]
        vals = r[again]
        other = np.where(vals >= 3, vals - 2, vals + 2)  # (another value on the same scale)
        revise.append((int(c), i[gone].astype(np.int32), i[again].astype(np.int32), other))
        free = np.setdiff1d(all_items, i[idx])
        update.append((int(c), rng.choice(free, b, replace=False).astype(np.int32), other))
    return revise, update


def _aug(train, q):
    import numpy as np

    u, i, r = train
    c, removed, items, ratings = q
    keep = ~((u == c) & np.isin(i, removed))
    return (np.concatenate([u[keep], np.full(len(items), c, dtype=np.int32)]), np.concatenate([i[keep], items]),
            np.concatenate([r[keep], ratings]))


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


def _off_scale_leg(np, kn, train, revise, rows, reps):
    """(c): the re-fold of average(aug) on a fit that is not dyadic"""
    off = (train[0], train[1], np.round(train[2] * 0.93 + 0.1, 2))
    e = kn.Engine(k=300)
    t0 = time.perf_counter()
    e.fit(*off)
    fit_ms = (time.perf_counter() - t0) * 1e3
    by = kn.BystanderQueries(e)
    res = {"fit_wall_ms": fit_ms, "prep_ms": float(e.timings().get("prep_ms", 0.0))}
    legs = {}
    for name, extra in (("fitted_row_only", []), ("with_an_average_row", [UNKNOWN_USER])):
        times = []
        for j in range(reps + 2):  # (two warm-up calls)
            c, removed, items, ratings = revise[j % CHANGERS]
            ratings = np.round(ratings * 0.93 + 0.1, 2)
            vs, its = rows[j % CHANGERS]
            others = np.concatenate([vs[:1], np.asarray(extra, dtype=np.int32)]).astype(np.int32)
            pis = its[:len(others)]
            t0 = time.perf_counter()
            out = by.predict_with(c, items, ratings, others, pis, removed=removed)
            times.append((time.perf_counter() - t0) * 1e3)
            assert np.isfinite(out).all()
        legs[name] = _stats(times[2:])
    res["per_call"] = legs
    res["refold_ms"] = legs["with_an_average_row"]["median_ms"] - legs["fitted_row_only"]["median_ms"]
    e.close()
    return res


def inner(args):
    """runs on the GPU"""
    import numpy as np

    kn = importlib.import_module(PKG + ".knncf")
    synth = importlib.import_module(PKG + ".synth")
    d = synth.syn_25m()
    train = (d.train.users, d.train.items, d.train.ratings)
    revise, update = _queries(train, seed=23)
    rng = np.random.default_rng(5)
    fitted, items = np.unique(train[0]), np.unique(train[1])
    rows = []
    for q in revise:  # 63 bystanders other than the changer
        vs = rng.choice(fitted[fitted != q[0]], 63, replace=False).astype(np.int32)
        rows.append((vs, rng.choice(items, 63).astype(np.int32)))
    if args.off_scale_only:
        print(json.dumps({"off_scale": _off_scale_leg(np, kn, train, revise, rows, args.reps)}), flush=True)
        return
    res = {"k": 300, "removed_mean": float(np.mean([len(q[1]) for q in revise])), "re_rated_mean": float(np.mean([len(q[2]) for q in revise]))}
    e = kn.Engine(k=300)
    by = kn.BystanderQueries(e)
    # (a) the refit that a row replaces
    times = []
    for j in range(args.baseline_calls + 1):  # (the first one warms up)
        vs, its = rows[j]
        aug = _aug(train, revise[j])
        t0 = time.perf_counter()
        e.fit(*aug)
        e.predict(kn.PRED_KNN, int(vs[0]), int(its[0]))
        times.append(time.perf_counter() - t0)
    res["baseline_refit_and_predict"] = dict(_stats(np.array(times[1:]) * 1e3), calls=args.baseline_calls)
    e.fit(*train)
    res.update({"U": e.num_users, "I": e.num_items, "train_ratings": len(train[0])})
    removed = [q[1] for q in revise]
    triples = [(q[0], q[2], q[3]) for q in revise]
    res["revise_bystander"] = _time_shapes(np, args.reps, lambda q, vs, its: by.predict_with(q[0], q[2], q[3], vs, its, removed=q[1]),
                                           lambda qs, others, pis: by.predict_with_batch(triples, others, pis, removed=removed), revise, rows)
    # (b) the same changers adding as many rows as they re-rate: update-bystander rows
    res["update_bystander"] = _time_shapes(np, args.reps, lambda q, vs, its: by.predict_with(*q, vs, its), by.predict_with_batch, update, rows)
    refit = res["baseline_refit_and_predict"]["median_ms"]
    ok = True
    for key in [str(m) for m in SHAPES] + ["batch"]:
        pick = lambda r: (r["batch_64x4"] if key == "batch" else r["single_query"][key])
        r, f = pick(res["revise_bystander"]), pick(res["update_bystander"])
        r["refit_over_row"] = refit / r["per_row"]["median_ms"]
        r["row_over_update_row"] = r["per_row"]["median_ms"] / f["per_row"]["median_ms"]
        ok = ok and r["per_row"]["median_ms"] < refit
    res["every_row_cheaper_than_the_refit"] = ok
    e.close()
    res["off_scale"] = _off_scale_leg(np, kn, train, revise, rows, args.reps)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--baseline-calls", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "revise_bystander"))
    ap.add_argument("--off-scale-only", action="store_true", help="the leg (c) alone")
    ap.add_argument("--inner", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.inner:
        return inner(args)
    os.makedirs(args.out, exist_ok=True)
    cmd = ["timeout", "-k", "10", "1000", sys.executable, os.path.abspath(__file__), "--inner", "--reps", str(args.reps),
           "--baseline-calls", str(args.baseline_calls)] + (["--off-scale-only"] if args.off_scale_only else [])
    log = os.path.join(args.out, "timing.log")
    with open(log, "w") as f:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=f, text=True, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit(f"the timed run failed with status {r.returncode} (log: {log})")
    res = json.loads(r.stdout.strip().splitlines()[-1])
    with open(os.path.join(args.out, "revise_bystander_latency.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    if not res.get("every_row_cheaper_than_the_refit", True):
        raise SystemExit("a bystander row costs more than the refit it replaces")


if __name__ == "__main__":
    main()
