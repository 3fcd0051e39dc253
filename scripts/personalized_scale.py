"""Seconds per full-test-set PERSONALIZED MAE (adjusted cosine and Jaccard, no neighbourhood cut) at four shapes.

Per shape and similarity: fit (not timed), one warm-up `mae(PRED_PERSONALIZED)` over the whole test set, then 3 timed calls,
each ended by a device synchronise (the C entry point returns after draining its streams).  Reports the wall time, the
call's rerank_ms (the exact similarity rows, csrc/personalized.hip: k_sim_rows) and predict_ms (the file-order folds,
k_fold_rows, plus the row sort), and the rates over the counted work: row-build updates sum_u sum_{i in I(u)} |U(i)| over the
users with a test row, fold terms sum_test |U(i)|, and the bytes of similarity rows written (U x 8 B per built user).
syn-100k takes the U x U table path (U <= 2048), for contrast.  One JSON object per (shape, similarity) on stdout.

    python scripts/personalized_scale.py [--shapes syn-100k,ml-1m-like,ml-10m-like,syn-25m] [--sims cosine,jaccard]

Kernel times: run the same under `rocprofv3 --kernel-trace --stats -- python scripts/personalized_scale.py --shapes syn-25m`."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "movie-recommender-system_amd"

SHAPES = {
    "syn-100k": lambda s: s.syn_100k(),
    "ml-1m-like": lambda s: s.syn_scaled(6_040, 3_706, 1_000_209, seed=1),
    "ml-10m-like": lambda s: s.syn_scaled(69_878, 10_677, 10_000_054, seed=10),
    "syn-25m": lambda s: s.syn_25m(),
}


def work(d):
    """(row-build updates, fold terms, users with a test row on a train item) of the streamed form"""
    raters = np.bincount(d.train.items).astype(np.float64)
    per_user = np.bincount(d.train.users, weights=raters[d.train.items])
    known = np.isin(d.test.items, d.train.items)
    users = np.unique(d.test.users[known])
    fold = float(raters[d.test.items[known]].sum())
    return float(per_user[users].sum()), fold, len(users)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--sims", default="cosine,jaccard")
    ap.add_argument("--calls", type=int, default=3)
    a = ap.parse_args()
    synth = importlib.import_module(PKG + ".synth")
    kn = importlib.import_module(PKG + ".knncf")
    kn.load_library()
    sims = {"cosine": kn.SIM_COSINE, "jaccard": kn.SIM_JACCARD}
    for shape in a.shapes.split(","):
        d = SHAPES[shape](synth)
        tr = (d.train.users, d.train.items, d.train.ratings)
        te = (d.test.users, d.test.items, d.test.ratings)
        updates, fold, built = work(d)
        U = len(np.unique(d.train.users))
        for sim in a.sims.split(","):
            e = kn.Engine(k=10, similarity=sims[sim])
            e.fit(*tr)
            mae = e.mae(kn.PRED_PERSONALIZED, *te)  # warm-up: the first-use copies (prep_ms)
            runs = []
            for _ in range(a.calls):
                e.reset_timings()
                t0 = time.perf_counter()
                got = e.mae(kn.PRED_PERSONALIZED, *te)
                wall = time.perf_counter() - t0
                t = e.timings()
                assert got == mae
                runs.append((wall, t["rerank_ms"], t["predict_ms"]))
            e.close()
            wall, rr, pp = (float(np.median([r[j] for r in runs])) for j in range(3))
            streamed = U > 2048
            out = {
                "shape": shape, "similarity": sim, "users": U, "train": len(tr[0]), "test": len(te[0]),
                "path": "streamed rows" if streamed else "U x U table", "mae": mae,
                "seconds_per_mae": [round(r[0], 4) for r in runs], "median_s": round(wall, 4),
                "rerank_ms": round(rr, 2), "predict_ms": round(pp, 2),
                "row_build_updates": updates, "fold_terms": fold, "users_built": built,
                "row_bytes_written": float(built) * U * 8,
            }
            if streamed and rr > 0 and pp > 0:
                out["row_build_updates_per_s"] = updates / (rr * 1e-3)
                out["row_write_GB_per_s"] = built * U * 8 / (rr * 1e-3) / 1e9
                out["fold_terms_per_s"] = fold / (pp * 1e-3)
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
