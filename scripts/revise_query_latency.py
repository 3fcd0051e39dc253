"""Latency of a revise query (Engine.recommend_revised, csrc/foldin.hip) at the ml-25m shape: recommendations for a user of
the fit that re-rated some of its train items and deleted others, without a refit.

Takes `--calls` users of syn-25m, fits train once (k = 300), warms up, and times recommend_revised(n = 3) per user, each
re-rating 1-3 of its train items and deleting 1-2 more; then recommend_revised_batch issued B = 1, 8, 64 and 200 at a time.
The baseline is what a tree without the revise calls must do for the same answer: fit(aug) followed by recommend(user, 3),
where aug is the edited file, timed for `--baseline-calls` of the same users.  It uses nothing but Engine.fit /
Engine.recommend, so `--baseline-only` runs unchanged on a tree that lacks the revise calls.  Prints one JSON line.

    python scripts/revise_query_latency.py [--calls 200] [--baseline-calls 10] [--baseline-only] [--out bench_out/revise_query]

The GPU work runs in its own child process under `timeout -k 10`."""
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
BATCHES = (1, 8, 64, 200)


def _edits(d, count, seed):
    """[(user, removed items, additional items, additional ratings)]: `count` users with at least 10 train rows, each
    re-rating 1-3 of its train items (removed and given again with another value) and deleting 1-2 more"""
    import numpy as np

    u = d.train.users
    order = np.argsort(u, kind="stable")
    users, starts, counts = np.unique(u[order], return_index=True, return_counts=True)
    rng = np.random.default_rng(seed)
    pick = rng.choice(np.flatnonzero(counts >= 10), count, replace=False)
    queries = []
    for x in pick:
        n_re, n_del = int(rng.integers(1, 4)), int(rng.integers(1, 3))
        rows = order[starts[x] + rng.choice(counts[x], n_re + n_del, replace=False)]
        items, old = d.train.items[rows], d.train.ratings[rows[:n_re]]
        queries.append((int(users[x]), items.astype(np.int32), items[:n_re].astype(np.int32), np.where(old >= 3, old - 2, old + 2)))
    return queries


def _aug(train, q, removed, items, ratings):
    """the edited file: train in file order without q's removed rows, then the additional rows"""
    import numpy as np

    keep = ~((train[0] == q) & np.isin(train[1], removed))
    return (np.concatenate([train[0][keep], np.full(len(items), q, dtype=np.int32)]), np.concatenate([train[1][keep], items]),
            np.concatenate([train[2][keep], ratings]))


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
    train = (d.train.users, d.train.items, d.train.ratings)
    queries = _edits(d, args.calls, seed=13)
    res = {"calls": args.calls, "k": 300, "removed_items_mean": float(np.mean([len(q[1]) for q in queries])),
           "rerated_items_mean": float(np.mean([len(q[2]) for q in queries]))}
    e = kn.Engine(k=300)
    # baseline: a refit of the edited file, then the user's recommendations (building the edited file is not timed)
    times, answers = [], []
    for q, rm, it, rt in queries[:args.baseline_calls + 1]:  # (the first one warms up)
        aug = _aug(train, q, rm, it, rt)
        t0 = time.perf_counter()
        e.fit(*aug)
        answers.append(e.recommend(kn.PRED_KNN, q, 3))
        times.append(time.perf_counter() - t0)
    res["baseline_refit"] = dict(_stats(np.array(times[1:]) * 1e3), calls=args.baseline_calls)
    if not args.baseline_only:
        e.fit(*train)
        res.update({"U": e.num_users, "I": e.num_items, "train_ratings": len(train[0])})
        for q, rm, it, rt in queries[:20]:  # warm-up: every launch shape and the scratch sizes
            e.recommend_revised(q, rm, it, rt, 3)
        times, same = [], 0
        for j, (q, rm, it, rt) in enumerate(queries):
            t0 = time.perf_counter()
            got = e.recommend_revised(q, rm, it, rt, 3)
            times.append(time.perf_counter() - t0)
            if j < len(answers):  # (the refit's closures are not fresh, so its values may differ in the last bits: ids only)
                same += got[0].tolist() == answers[j][0].tolist()
        res["recommend_revised"] = _stats(np.array(times) * 1e3)
        res["same_items_as_refit"] = [same, len(answers)]
        res["batched"] = {}
        for B in BATCHES:
            chunks = [queries[a:a + B] for a in range(0, len(queries), B)]
            e.recommend_revised_batch(chunks[0], 3)
            t0 = time.perf_counter()
            for c in chunks:
                _, st = e.recommend_revised_batch(c, 3)
                assert not st.any()
            dt = time.perf_counter() - t0
            res["batched"][str(B)] = {"ms_per_query": dt / len(queries) * 1e3, "queries_per_s": len(queries) / dt}
    e.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--baseline-calls", type=int, default=10)
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "revise_query"))
    ap.add_argument("--inner", action="store_true")
    args = ap.parse_args()
    if args.inner:
        return inner(args)
    os.makedirs(args.out, exist_ok=True)
    cmd = ["timeout", "-k", "10", "900", sys.executable, os.path.abspath(__file__), "--inner", "--calls", str(args.calls),
           "--baseline-calls", str(args.baseline_calls)] + (["--baseline-only"] if args.baseline_only else [])
    log = os.path.join(args.out, "timing.log")
    with open(log, "w") as f:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=f, text=True, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit(f"step failed with status {r.returncode} (log: {log})")
    res = json.loads(r.stdout.strip().splitlines()[-1])
    with open(os.path.join(args.out, "revise_query_latency.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
