"""Latency of knncf_remove_users (csrc/append.hip) at the ml-25m shape: fitted users leave the fit with every row they have, and the
kNN lists that hold none of them are kept — against the plain refit that knncf_amend makes of the same deletion, and against
fit(aug).  amend_latency.py for whole users.

Fits syn-25m (k = 300) and builds every list.  A step takes C users of the fit (15 .. 400 train ratings, every user used once)
out of it and then runs mae(PRED_KNN) over the test set, which rebuilds the lists the call dropped; every list is built again
before the next step.  The same steps run three times, one leg after the other with one engine alive at a time (two handles in
one process pay for each other's panel releases in their next allocation).  Timed per step, wall time with the profiler off:
  * remove: knncf_remove_users alone, with the lists it carried and dropped, the holders of its trace line and the prep_ms it
    charged (removal stage, refit and carry);
  * remove + mae;
  * amend: Appends.amend given every (user, item) row of those users, on a second engine that starts from the same fit with every
    list built — a user leaves, so knncf_amend refits plainly: this tree's own baseline for the old behaviour — + the same mae;
  * refit: that engine's fit(aug) + the same mae call.
C = 1, 8, 64 and 128 are the rows (--reps steps each, medians, with the [min, max] of the sums and the lists dropped per step).
Unless --no-profile is given, one step of every C is repeated under `rocprofv3 --kernel-trace --stats` in a child process of its
own for the device time of k_ap_holders and k_am_flag_users.  Prints one JSON line and writes it to --out.

    python scripts/remove_users_latency.py [--reps 5] [--out profiles/remove_users_syn25m_1gpu.json]

The GPU work runs in child processes under `timeout -k 10`."""
import argparse
import csv
import importlib
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "movie-recommender-system_amd"
TRACE = "KNNCF_DEBUG_TRACE_DISPATCH"
KERNELS = ("k_ap_holders", "k_am_flag_users")
COUNTS = (1, 8, 64, 128)


def _ms(call):
    t0 = time.perf_counter()
    out = call()
    return (time.perf_counter() - t0) * 1e3, out


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2] if len(xs) % 2 else 0.5 * (xs[len(xs) // 2 - 1] + xs[len(xs) // 2])


def _remove_line(read_fd):
    """the fields of the `remove` trace line that the call just wrote to stderr (redirected into a pipe around the call)"""
    text = os.read(read_fd, 1 << 16).decode(errors="replace")
    m = re.search(r"knncf-dispatch remove (.*)", text)
    return dict(re.findall(r"(\w+)=(\w+)", m.group(1))) if m else {}


def inner(args):
    """runs on the GPU"""
    import numpy as np

    kn = importlib.import_module(PKG + ".knncf")
    synth = importlib.import_module(PKG + ".synth")
    d = synth.syn_25m()
    train = [d.train.users, d.train.items, d.train.ratings]
    test = (d.test.users, d.test.items, d.test.ratings)
    users, counts = np.unique(train[0], return_counts=True)
    rng = np.random.default_rng(31)
    pool = rng.permutation(users[(counts >= 15) & (counts <= 400)]).tolist()
    build_all = lambda eng: kn.EnteredQueries(eng).entered_with(int(train[0][0]), [], [], cap=0)  # (builds every missing list)

    def fresh_engine():
        eng = kn.Engine(k=300)
        eng.fit(*train)
        eng.mae(kn.PRED_KNN, *test)
        build_all(eng)
        return eng

    def traced_remove(e, leavers):
        """remove_users with the trace on and stderr in a pipe for the length of the call: (ms, (carried, dropped), trace fields)"""
        r, w = os.pipe()
        saved = os.dup(2)
        os.environ[TRACE] = "1"
        os.dup2(w, 2)
        try:
            t, out = _ms(lambda: kn.remove_users(e, leavers))
        finally:
            os.dup2(saved, 2)
            os.close(saved); os.close(w)
            os.environ.pop(TRACE, None)
        line = _remove_line(r)
        os.close(r)
        return t, out, line

    # the steps: a warm-up of one leaver (every launch shape and scratch size), then --reps steps of every C
    plan = [1] + ([c for c in COUNTS] if args.profile else [c for c in COUNTS for _ in range(args.reps)])
    plan = [np.asarray([pool.pop() for _ in range(c)], dtype=np.int32) for c in plan]
    first = [a.copy() for a in train]

    # ---- leg 1: knncf_remove_users, alone on the device (one engine at a time: a second handle's panel releases would land in
    # this handle's next hipMalloc — the first form of this script measured 4.5 s removals right after the other engine's refits)
    e = fresh_engine()
    res = {"k": 300, "U": e.num_users, "I": e.num_items, "train_ratings": len(train[0]), "test_ratings": len(test[0]),
           "max_leavers": kn.APPEND_MAX_CHANGERS, "tile": kn.AMEND_TILE}
    steps = []
    for leavers in plan:
        gone = np.isin(train[0], leavers)
        before = e.timings()["prep_ms"]
        t_remove, (carried, dropped), line = traced_remove(e, leavers)
        prep = e.timings()["prep_ms"] - before
        t_mae, mae = _ms(lambda: e.mae(kn.PRED_KNN, *test))
        train = [a[~gone] for a in train]
        build_all(e)
        steps.append({"leavers": len(leavers), "removed_rows": int(gone.sum()), "carried": carried, "dropped": dropped,
                      "holders": int(line.get("holders", -1)), "bitmap": line.get("bitmap", ""), "remove_ms": t_remove,
                      "remove_prep_ms": prep, "mae_after_remove_ms": t_mae, "remove_plus_mae_ms": t_remove + t_mae, "mae": mae,
                      "shape": (e.num_users, e.num_items)})
    e.close()
    if args.profile:  # the new call's leg alone: the kernels' device time comes from the profiler's table
        res["profile_steps"] = [{k: v for k, v in s.items() if k != "shape"} for s in steps[1:]]
        print(json.dumps(res), flush=True)
        return

    # ---- leg 2: knncf_amend given every row of the same users (a user leaves: the plain refit), on a fresh engine
    train = [a.copy() for a in first]
    other = fresh_engine()
    for leavers, s in zip(plan, steps):
        gone = np.isin(train[0], leavers)
        ru, ri = train[0][gone], train[1][gone]
        t_amend, (c0, _) = _ms(lambda: kn.Appends(other).amend(ru, ri, [], [], []))
        t_mae, mae = _ms(lambda: other.mae(kn.PRED_KNN, *test))
        train = [a[~gone] for a in train]
        assert c0 == 0 and mae == s["mae"] and (other.num_users, other.num_items) == s["shape"], (mae, s["mae"])
        build_all(other)
        s.update({"amend_ms": t_amend, "amend_plus_mae_ms": t_amend + t_mae})

    # ---- leg 3: fit(aug) on that engine
    train = [a.copy() for a in first]
    for leavers, s in zip(plan, steps):
        train = [a[~np.isin(train[0], leavers)] for a in train]
        t_fit, _ = _ms(lambda: other.fit(*train))
        t_mae, mae = _ms(lambda: other.mae(kn.PRED_KNN, *test))
        assert mae == s["mae"], (mae, s["mae"])
        s.update({"refit_ms": t_fit, "refit_plus_mae_ms": t_fit + t_mae})
    other.close()

    def row(c):
        mine = [s for s in steps[1:] if s["leavers"] == c]
        out = {k: _median([s[k] for s in mine]) for k in mine[0] if k not in ("bitmap", "shape")}
        out["spread"] = {k: [min(s[k] for s in mine), max(s[k] for s in mine)]
                         for k in ("remove_ms", "remove_plus_mae_ms", "amend_plus_mae_ms", "refit_plus_mae_ms")}
        out["dropped_per_step"] = [s["dropped"] for s in mine]
        out["holders_per_step"] = [s["holders"] for s in mine]
        out["ms_per_step"] = {k: [round(s[k], 3) for s in mine] for k in ("remove_ms", "remove_prep_ms", "mae_after_remove_ms", "amend_ms",
                                                                         "amend_plus_mae_ms", "refit_ms", "refit_plus_mae_ms")}
        out.update({"steps": len(mine), "bitmap": mine[0]["bitmap"]})
        return out

    res["headline"] = [row(c) for c in COUNTS]
    print(json.dumps(res), flush=True)


def _child(argv, timeout_s):
    r = subprocess.run(["timeout", "-k", "10", str(timeout_s)] + argv, stdout=subprocess.PIPE, text=True, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit(f"the GPU step failed with status {r.returncode}: {' '.join(argv)}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "remove_users_syn25m_1gpu.json"))
    ap.add_argument("--commit", default="", help="the commit the library was built from, recorded in the output")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--inner", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--profile", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.inner:
        return inner(args)
    me = [sys.executable, os.path.abspath(__file__), "--inner", "--reps", str(args.reps)]
    res = _child(me, args.timeout)
    res["measured_on"] = args.commit
    if not args.no_profile:
        with tempfile.TemporaryDirectory() as d:
            shape = _child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "ru", "--"] + me + ["--profile"],
                           args.timeout)
            found = [os.path.join(r, f) for r, _, fs in os.walk(d) for f in fs if f.endswith("kernel_stats.csv")]
            kernels = {}
            with open(found[0]) as f:
                for row in csv.DictReader(f):
                    for name in KERNELS:
                        if name in row["Name"]:
                            calls, ns = int(row["Calls"]), float(row["TotalDurationNs"])
                            k = kernels.setdefault(name, {"calls": 0, "total_us": 0.0})
                            k["calls"] += calls; k["total_us"] += ns / 1e3
                            for col, key in (("MinNs", "min_us"), ("MaxNs", "max_us")):
                                if row.get(col):
                                    v = float(row[col]) / 1e3
                                    k[key] = v if key not in k else (min if key == "min_us" else max)(k[key], v)
            for k in kernels.values():
                k["us_per_call"] = k["total_us"] / k["calls"]
        res["profile_steps"] = shape["profile_steps"]
        res["kernels"] = kernels
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
