"""Throughput of the bulk similarities (Engine.similarity_batch, Engine.knn_similarity_batch; csrc/similarity_batch.hip) at the
ml-25m shape, next to host loops of the single calls.

syn-25m, k = 300, seed 17.  Two pair lists of `--pairs` (10^6) pairs: uniformly random (u, v) over the fitted users, and
(user, one of its neighbours) drawn from the lists of `--sample-users` random users.  One child process per similarity
(adjusted cosine, then Jaccard; the neighbour pairs are those of the cosine lists for both) fits once, warms up and times
`--repeats` calls of every leg; each figure is the median with min and standard deviation beside it:

  similarity_batch      wall time per pair; the pair kernel's device time (rerank_ms of knncf_get_timings: HIP events around the
                        launch) and its algorithmic bytes per second, 12 B x (|row u| + |row v|) per pair, the convention of
                        rerank_row_bytes, against the 8 TB/s HBM figure of DESIGN.md
  knn_similarity_batch  wall time per pair with every list built (the call that builds them is timed apart), the lookup's
                        device time (predict_ms)
  loops                 `--loop` single knncf_similarity / knncf_knn_similarity calls over the head of the same lists (lists
                        built beforehand).  `--baseline-only` runs only these: it uses no entry point of the batch, so it runs
                        unchanged on a tree that lacks them.

    python scripts/similarity_batch_throughput.py [--pairs 1000000] [--repeats 5] [--loop 3000] [--baseline-only] [--out DIR] [--json FILE]

Writes the result to --json (default profiles/similarity_batch_syn25m_1gpu.json; with --baseline-only
similarity_batch_baseline.json in --out, so that a run on another tree leaves the profile alone) and prints it as one JSON line;
the children's logs go to --out.  Every GPU step runs in its own child
process under `timeout -k 10`; a failing step ends the run."""
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
HBM_BYTES_PER_S = 8e12
K = 300


def _summary(seconds, n, unit):
    import numpy as np

    ns = np.array(seconds) * 1e9 / n
    return {f"ns_per_{unit}_median": float(np.median(ns)), f"ns_per_{unit}_min": float(ns.min()), f"ns_per_{unit}_sigma": float(ns.std()),
            "repeats": len(seconds)}


def _timed(repeats, call):
    runs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        runs.append(time.perf_counter() - t0)
    return runs


def _note(text):
    print(f"[{time.strftime('%H:%M:%S')}] {text}", file=sys.stderr, flush=True)


def inner(args):
    """runs on the GPU: one similarity; fit, pair lists, every leg"""
    import numpy as np

    kn = importlib.import_module(PKG + ".knncf")
    synth = importlib.import_module(PKG + ".synth")
    d = synth.syn_25m()
    sim = kn.SIM_JACCARD if args.similarity == "jaccard" else kn.SIM_COSINE
    e = kn.Engine(k=K, similarity=sim)
    e.fit(d.train.users, d.train.items, d.train.ratings)
    _note("fitted")
    users = np.unique(d.train.users).astype(np.int32)
    row_len = np.bincount(d.train.users, minlength=int(users.max()) + 1)
    rng = np.random.default_rng(17)
    n = args.pairs
    sample = rng.choice(users, size=min(args.sample_users, len(users)), replace=False).astype(np.int32)
    # the neighbour pairs come from the adjusted-cosine lists whichever similarity is timed (one list of pairs for both)
    lister = e if sim == kn.SIM_COSINE else kn.Engine(k=K).fit(d.train.users, d.train.items, d.train.ratings)
    ids, _, counts = lister.neighbors_batch(sample)
    if lister is not e:
        lister.close()
    pick = rng.integers(0, len(sample), size=n)
    lists = {"random": (rng.choice(users, size=n), rng.choice(users, size=n)),
             "neighbours": (sample[pick], ids[pick, rng.integers(0, counts.min(), size=n)])}
    lists = {name: (np.ascontiguousarray(u, dtype=np.int32), np.ascontiguousarray(v, dtype=np.int32)) for name, (u, v) in lists.items()}
    res = {"similarity": args.similarity, "U": e.num_users, "I": e.num_items, "train_ratings": len(d.train.users), "k": K, "pairs": n,
           "loop_calls": args.loop, "hbm_bytes_per_s": HBM_BYTES_PER_S, "lists": {}}
    e.neighbors_batch(sample)  # the lists that the kNN loop reads exist (a missing one would be built alone, per call)
    _note("pair lists drawn, sample lists built")
    for name, (us, vs) in lists.items():
        out = {"algorithmic_bytes": int(12 * (row_len[us].sum() + row_len[vs].sum())),
               "mean_row": float((row_len[us].mean() + row_len[vs].mean()) / 2)}
        m = args.loop
        in_sample = np.isin(us, sample)
        lu, lv = us[in_sample][:m], vs[in_sample][:m]  # (the kNN loop stays on built lists)
        for u, v in zip(lu[:50].tolist(), lv[:50].tolist()):
            e.similarity(u, v)
            e.knn_similarity(u, v)
        out["similarity_loop"] = _summary(_timed(args.repeats, lambda: [e.similarity(u, v) for u, v in zip(lu.tolist(), lv.tolist())]), len(lu), "pair")
        out["knn_similarity_loop"] = _summary(_timed(args.repeats, lambda: [e.knn_similarity(u, v) for u, v in zip(lu.tolist(), lv.tolist())]),
                                              len(lu), "pair")
        res["lists"][name] = out
        _note(f"loops over {name} done")
    if not args.baseline_only:
        for name, (us, vs) in lists.items():
            out = res["lists"][name]
            e.similarity_batch(us, vs)  # warm-up: the scratch
            e.reset_timings()
            runs = _timed(args.repeats, lambda: e.similarity_batch(us, vs))
            dev_s = e.timings()["rerank_ms"] * 1e-3 / args.repeats
            out["similarity_batch"] = _summary(runs, n, "pair")
            out["similarity_batch"].update(device_ns_per_pair=dev_s * 1e9 / n, bytes_per_s=out["algorithmic_bytes"] / dev_s,
                                           hbm_fraction=out["algorithmic_bytes"] / dev_s / HBM_BYTES_PER_S)
            out["similarity_batch"]["speedup_over_loop"] = out["similarity_loop"]["ns_per_pair_median"] / out["similarity_batch"]["ns_per_pair_median"]
            _note(f"similarity_batch over {name} done")
        for name, (us, vs) in lists.items():
            out = res["lists"][name]
            t0 = time.perf_counter()
            e.knn_similarity_batch(us, vs)
            out["knn_similarity_batch_first_call_s"] = time.perf_counter() - t0  # with the builds of the lists still missing
            _note(f"knn_similarity_batch over {name}: first call done")
            e.reset_timings()
            runs = _timed(args.repeats, lambda: e.knn_similarity_batch(us, vs))
            out["knn_similarity_batch"] = _summary(runs, n, "pair")
            out["knn_similarity_batch"]["device_ns_per_pair"] = e.timings()["predict_ms"] * 1e6 / args.repeats / n
            out["knn_similarity_batch"]["speedup_over_loop"] = (out["knn_similarity_loop"]["ns_per_pair_median"] /
                                                                out["knn_similarity_batch"]["ns_per_pair_median"])
    e.close()
    print(json.dumps(res), flush=True)


def _child(argv, timeout_s, log):
    cmd = ["timeout", "-k", "10", str(timeout_s)] + argv
    with open(log, "w") as f:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=f, text=True, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit(f"step failed with status {r.returncode}: {' '.join(argv)} (log: {log})")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--sample-users", type=int, default=20_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop", type=int, default=3000)
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--commit", default="", help="label written into the result")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "similarity_batch"))
    ap.add_argument("--json", default="")
    ap.add_argument("--inner", action="store_true")
    ap.add_argument("--similarity", default="cosine", choices=["cosine", "jaccard"])
    args = ap.parse_args()
    if args.inner:
        return inner(args)
    os.makedirs(args.out, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__), "--inner", "--pairs", str(args.pairs), "--sample-users", str(args.sample_users),
          "--repeats", str(args.repeats), "--loop", str(args.loop)] + (["--baseline-only"] if args.baseline_only else [])
    res = {"commit": args.commit, "baseline_only": args.baseline_only}
    for sim in ("cosine", "jaccard"):
        res[sim] = _child(me + ["--similarity", sim], 540, os.path.join(args.out, f"timing_{sim}.log"))
    path = args.json or (os.path.join(args.out, "similarity_batch_baseline.json") if args.baseline_only
                         else os.path.join(ROOT, "profiles", "similarity_batch_syn25m_1gpu.json"))
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
