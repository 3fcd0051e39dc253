"""Throughput of Engine.recommend_batch (knncf_recommend_batch, csrc/reco_batch.hip) at the ml-25m shape next to the host loop
of single Engine.recommend calls (the same call over one user): syn-25m, k = 300, n = 3, KNNCF_PRED_KNN.

Every leg runs in a child process that fits once and builds the neighbour table of ALL users first (neighbors_batch), so the
legs time recommendation, not the fit.  Legs: the single-call loop over 256 users — with `--parent-tree DIR` also on a
checkout of the parent commit built in DIR (`single_loop_parent`; it uses only entry points that exist there) — and
recommend_batch issued 1, 2, 4, ... 512, 1024, 16 384 and all users at a time.  Each figure is the median over `--repeats` passes with
min and standard deviation beside it.  Then one batch of 1024 users is repeated under `rocprofv3 --kernel-trace --stats` in
two child processes of their own — set-up alone, and set-up plus the batch — and the per-user device time of each kernel is
their difference over 1024.  Prints one JSON line.

    python scripts/recommend_batch_throughput.py [--repeats 5] [--parent-tree DIR] [--no-profile] [--out DIR]

Every GPU step runs in its own child process under `timeout -k 10`; a failing step ends the run."""
import argparse
import csv
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "movie-recommender-system_amd"
LOOP_USERS = 256
# (users per call, users per pass); 0 = all
BATCHES = ((1, 256), (2, 256), (4, 256), (8, 256), (16, 256), (32, 256), (64, 1024), (128, 1024), (256, 1024), (512, 2048),
           (1024, 4096), (16384, 16384), (0, 0))
PROFILE_BATCH = 1024


def _summary(seconds, n_users):
    import numpy as np

    us = np.array(seconds) * 1e6 / n_users
    return {"us_per_user_median": float(np.median(us)), "us_per_user_min": float(us.min()), "us_per_user_sigma": float(us.std()),
            "users_per_s": float(1e6 / np.median(us)), "users_per_pass": int(n_users), "repeats": len(seconds)}


def inner(args):
    """runs on the GPU: fit, build every neighbourhood, then time the legs (or run one batch, under the profiler)"""
    import numpy as np

    sys.path.insert(0, args.tree)
    kn = importlib.import_module(PKG + ".knncf")
    synth = importlib.import_module(PKG + ".synth")
    d = synth.syn_25m()
    e = kn.Engine(k=300)
    e.fit(d.train.users, d.train.items, d.train.ratings)
    known = np.unique(d.train.users).astype(np.int32)
    e.neighbors_batch(known)
    U, I = e.num_users, e.num_items
    res = {"U": U, "I": I, "train_ratings": len(d.train.users), "k": 300, "n": 3}
    stride = lambda m: known[::max(1, len(known) // m)][:m].copy()
    if args.profile_batch >= 0:
        if args.profile_batch > 0:
            users = stride(args.profile_batch)
            e.recommend_batch(kn.PRED_KNN, users, 3)
        e.close()
        print(json.dumps(res), flush=True)
        return
    users = stride(LOOP_USERS)
    for u in users[:16]:
        e.recommend(kn.PRED_KNN, int(u), 3)
    runs = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        for u in users:
            e.recommend(kn.PRED_KNN, int(u), 3)
        runs.append(time.perf_counter() - t0)
    res["single_loop"] = _summary(runs, len(users))
    if not args.baseline_only:
        res["batch"] = {}
        for B, per_pass in BATCHES:
            us = stride(per_pass) if per_pass else known
            step = B if B else len(us)
            e.recommend_batch(kn.PRED_KNN, us[:step], 3)  # warm-up: the launch shapes and the scratch sizes
            runs = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                for a in range(0, len(us), step):
                    e.recommend_batch(kn.PRED_KNN, us[a:a + step], 3)
                runs.append(time.perf_counter() - t0)
            res["batch"][str(B) if B else "all"] = _summary(runs, len(us))
    e.close()
    print(json.dumps(res), flush=True)


def _child(argv, timeout_s, log):
    cmd = ["timeout", "-k", "10", str(timeout_s)] + argv
    with open(log, "w") as f:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=f, text=True, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit(f"step failed with status {r.returncode}: {' '.join(argv)} (log: {log})")
    return json.loads(r.stdout.strip().splitlines()[-1])


def _stats(path):
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            out[row["Name"]] = (int(row["Calls"]), float(row["TotalDurationNs"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-tree", default="", help="a built checkout of the parent commit: adds the single_loop_parent leg")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--commit", default="", help="label written into the result")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "recommend_batch"))
    ap.add_argument("--inner", action="store_true")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--profile-batch", type=int, default=-1)
    args = ap.parse_args()
    if args.inner:
        return inner(args)
    os.makedirs(args.out, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__), "--inner", "--repeats", str(args.repeats)]
    res = {"commit": args.commit}
    if args.parent_tree:
        parent = _child(me + ["--baseline-only", "--tree", os.path.abspath(args.parent_tree)], 600, os.path.join(args.out, "parent.log"))
        res["single_loop_parent"] = parent["single_loop"]
    res.update(_child(me, 900, os.path.join(args.out, "timing.log")))
    if not args.no_profile:
        prof = {}
        for tag, batch in (("setup", 0), ("calls", PROFILE_BATCH)):
            d = os.path.join(args.out, "prof_" + tag)
            _child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "rb", "--"] + me +
                   ["--profile-batch", str(batch)], 600, os.path.join(args.out, f"prof_{tag}.log"))
            found = [os.path.join(r, f) for r, _, fs in os.walk(d) for f in fs if f.endswith("kernel_stats.csv")]
            prof[tag] = _stats(found[0])
        per_kernel = {}
        for name, (calls, ns) in prof["calls"].items():
            c0, ns0 = prof["setup"].get(name, (0, 0.0))
            if calls > c0:
                per_kernel[name[:120]] = {"calls": calls - c0, "us_per_user": (ns - ns0) / PROFILE_BATCH / 1e3}
        res["profile_batch"] = PROFILE_BATCH
        res["device_us_per_user"] = sum(v["us_per_user"] for v in per_kernel.values())
        res["kernels"] = per_kernel
    with open(os.path.join(args.out, "recommend_batch_throughput.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
