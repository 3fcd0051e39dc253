"""Latency of knncf_append (Appends.append, csrc/append.hip) at the ml-25m shape: new ratings go into the fit and the kNN lists
they cannot change are kept, against the refit it replaces.

Fits syn-25m once (k = 300) and builds every list.  A step appends the rows of C changers — users of the fit with 10 .. 400 train
ratings that each add 1 .. 20 half-star ratings on train items they have not rated, every changer used once — and then runs
mae(PRED_KNN) over the test set, which rebuilds the lists the append dropped; every list is built again before the next step
(the fit grows from step to step).  Timed per step, wall time with the profiler off:
  * append: knncf_append alone, with the lists it carried and dropped and the prep_ms it charged;
  * append + mae;
  * plain: the same append under KNNCF_DEBUG_APPEND_MAX_CHANGERS=0 (nothing carried) + mae, on a second engine that holds the
    same fit: the path knncf_append itself takes beyond KNNCF_APPEND_MAX_CHANGERS;
  * refit: that second engine's fit(aug) + the same mae call, aug = what the first engine now holds — same process, same job.
(Two engines, not three: a whole-matrix build keeps a 53 GB similarity panel per engine.)
C = 1, 8, 64 and APPEND_MAX_CHANGERS are the headline rows (--reps steps each, medians, with the [min, max] of the sums); the sweep then takes C upward in
powers of two with the limit lifted (--sweep-reps steps each) until append + mae is no cheaper than plain + mae, and reports that
crossover (interpolated between the two C around it) — the measurement behind the constant.  One more row has half of 64
changers NEW to the fit (5 .. 20 rows each), so that the table moves.  Prints one JSON line.

    python scripts/append_latency.py [--reps 5] [--sweep-reps 2] [--sweep-max 8192] [--out bench_out/append]

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
LIMIT = "KNNCF_DEBUG_APPEND_MAX_CHANGERS"


class Pool:
    """changers of the fit, each used once, with rows on train items they have not rated; newcomers get fresh ids"""

    def __init__(self, train, seed):
        import numpy as np

        self.np = np
        u, i, _ = train
        order = np.argsort(u, kind="stable")
        self.users, start, counts = np.unique(u[order], return_index=True, return_counts=True)
        self.rows = {int(c): i[order[s:s + n]] for c, s, n in zip(self.users, start, counts) if 10 <= n <= 400}
        self.items = np.unique(i)
        self.rng = np.random.default_rng(seed)
        self.fitted = self.rng.permutation(np.asarray(sorted(self.rows), dtype=np.int64)).tolist()
        self.next_id = int(self.users.max()) + 1

    def take(self, n_fitted, n_new=0):
        """(users, items, ratings) of one append, the changers' rows interleaved in blocks"""
        np, rng = self.np, self.rng
        parts = []
        for _ in range(n_fitted):
            c = self.fitted.pop()
            free = np.setdiff1d(self.items, self.rows[c])
            n = int(rng.integers(1, 21))
            parts.append((c, rng.choice(free, n, replace=False), rng.integers(1, 11, n) / 2.0))
        for _ in range(n_new):
            n = int(rng.integers(5, 21))
            parts.append((self.next_id, rng.choice(self.items, n, replace=False), rng.integers(1, 11, n) / 2.0))
            self.next_id += 1
        u = np.concatenate([np.full(len(p[1]), p[0]) for p in parts]).astype(np.int32)
        it = np.concatenate([p[1] for p in parts]).astype(np.int32)
        rt = np.concatenate([p[2] for p in parts]).astype(np.float64)
        mix = rng.permutation(len(u))  # rows of several users interleave
        return u[mix], it[mix], rt[mix]


def _ms(call):
    t0 = time.perf_counter()
    out = call()
    return (time.perf_counter() - t0) * 1e3, out


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2] if len(xs) % 2 else 0.5 * (xs[len(xs) // 2 - 1] + xs[len(xs) // 2])


def inner(args):
    """runs on the GPU"""
    import numpy as np

    kn = importlib.import_module(PKG + ".knncf")
    synth = importlib.import_module(PKG + ".synth")
    d = synth.syn_25m()
    train = [d.train.users, d.train.items, d.train.ratings]
    test = (d.test.users, d.test.items, d.test.ratings)
    pool = Pool(train, seed=23)
    e, other = kn.Engine(k=300), kn.Engine(k=300)
    first_user = int(train[0][0])
    build_all = lambda eng: kn.EnteredQueries(eng).entered_with(first_user, [], [], cap=0)  # (builds every missing list)
    for eng in (e, other):
        eng.fit(*train)
        eng.mae(kn.PRED_KNN, *test)
        build_all(eng)
    res = {"k": 300, "U": e.num_users, "I": e.num_items, "train_ratings": len(train[0]), "test_ratings": len(test[0]),
           "max_changers": kn.APPEND_MAX_CHANGERS}

    def step(n_fitted, n_new, lifted):
        rows = pool.take(n_fitted, n_new)
        if lifted:
            os.environ[LIMIT] = str(1 << 30)
        before = e.timings()["prep_ms"]
        t_append, (carried, dropped) = _ms(lambda: kn.Appends(e).append(*rows))
        prep = e.timings()["prep_ms"] - before
        os.environ.pop(LIMIT, None)
        t_mae, mae = _ms(lambda: e.mae(kn.PRED_KNN, *test))
        os.environ[LIMIT] = "0"
        t_plain, (c0, _) = _ms(lambda: kn.Appends(other).append(*rows))
        os.environ.pop(LIMIT, None)
        t_plain_mae, mae_plain = _ms(lambda: other.mae(kn.PRED_KNN, *test))
        for j in range(3):
            train[j] = np.concatenate([train[j], rows[j]])
        t_fit, _ = _ms(lambda: other.fit(*train))
        t_fit_mae, mae_refit = _ms(lambda: other.mae(kn.PRED_KNN, *test))
        assert c0 == 0 and mae == mae_plain == mae_refit, (mae, mae_plain, mae_refit)
        build_all(e)
        return {"rows": len(rows[0]), "carried": carried, "dropped": dropped, "append_ms": t_append, "append_prep_ms": prep,
                "mae_after_append_ms": t_mae, "append_plus_mae_ms": t_append + t_mae, "plain_append_ms": t_plain,
                "plain_plus_mae_ms": t_plain + t_plain_mae, "refit_ms": t_fit, "refit_plus_mae_ms": t_fit + t_fit_mae}

    def row(n_fitted, n_new, reps, lifted=False):
        steps = [step(n_fitted, n_new, lifted) for _ in range(reps)]
        out = {k: _median([s[k] for s in steps]) for k in steps[0]}
        # (a step whose rebuild needs more rows than any before it grows the row-block panels: the spread says how often)
        out["spread"] = {k: [min(s[k] for s in steps), max(s[k] for s in steps)]
                         for k in ("append_ms", "append_plus_mae_ms", "plain_plus_mae_ms", "refit_plus_mae_ms")}
        out.update({"changers": n_fitted + n_new, "newcomers": n_new, "steps": reps})
        return out

    step(1, 0, False)  # warm-up: every launch shape and scratch size
    res["headline"] = [row(c, 0, args.reps) for c in (1, 8, 64, kn.APPEND_MAX_CHANGERS)]
    res["table_moves"] = row(32, 32, args.reps)
    sweep, c = [], 64
    while c <= args.sweep_max and len(pool.fitted) >= c * args.sweep_reps:
        sweep.append(row(c, 0, args.sweep_reps, lifted=True))
        if sweep[-1]["append_plus_mae_ms"] >= sweep[-1]["plain_plus_mae_ms"]:
            break
        c *= 2
    res["sweep"] = sweep
    gain = [s["plain_plus_mae_ms"] - s["append_plus_mae_ms"] for s in sweep]
    if gain[-1] <= 0 and len(sweep) > 1:
        a, b = sweep[-2]["changers"], sweep[-1]["changers"]
        res["crossover_changers"] = a + (b - a) * gain[-2] / (gain[-2] - gain[-1])
    else:
        res["crossover_changers"] = None  # (not reached below --sweep-max, or already behind at the first C)
        res["crossover_note"] = "behind at the first sweep point" if gain[-1] <= 0 else f"not reached up to {sweep[-1]['changers']} changers"
    for eng in (e, other):
        eng.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep-reps", type=int, default=2)
    ap.add_argument("--sweep-max", type=int, default=8192)
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "append"))
    ap.add_argument("--inner", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.inner:
        return inner(args)
    os.makedirs(args.out, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--inner", "--reps", str(args.reps),
           "--sweep-reps", str(args.sweep_reps), "--sweep-max", str(args.sweep_max)]
    log = os.path.join(args.out, "timing.log")
    with open(log, "w") as f:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=f, text=True, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit(f"the timed run failed with status {r.returncode} (log: {log})")
    res = json.loads(r.stdout.strip().splitlines()[-1])
    with open(os.path.join(args.out, "append_latency.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
