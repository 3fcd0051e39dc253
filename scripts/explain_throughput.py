"""Time of Engine.explain_batch_device (knncf_explain_batch_device, csrc/explain.hip) at the ml-25m shape next to
Engine.predict_batch_device (KNNCF_PRED_KNN) on the same rows of the same build: syn-25m, k = 300, cap = 16.

Two settings: 12 288 rows — the top-3 recommendations of 4096 users, what a serving layer would ask to have explained — and
the first 1 000 000 test rows.  One child process fits once; per setting a warm-up call of each entry point builds the
neighbourhoods the rows need and sizes every scratch buffer, then the two calls alternate `--repeats` times.  A call returns
with the handle's streams drained, so the host clock around it is the call's time; beside it stands the handle's predict_ms of
the call (device events around the dense-id lookup and the kernels: for predict the row sort and k_predict_knn_items, for
explain k_explain).  Medians, minima and standard deviations; the ratio is explain over predict.  Both orders of the terms are
timed.  Writes one JSON file and prints it.

    python scripts/explain_throughput.py [--repeats 7] [--out profiles/explain_batch_syn25m_1gpu.json]

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
K, CAP, TOP_USERS, TEST_ROWS = 300, 16, 4096, 1_000_000


def _summary(values):
    import numpy as np

    v = np.asarray(values, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "sigma": float(v.std()), "repeats": len(v)}


def inner(args):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    kn = importlib.import_module(PKG + ".knncf")
    synth = importlib.import_module(PKG + ".synth")
    note = lambda text: print(f"[explain_throughput] {text}", file=sys.stderr, flush=True)
    d = synth.syn_25m()
    note("data ready")
    e = kn.Engine(k=K)
    e.fit(d.train.users, d.train.items, d.train.ratings)
    known = np.unique(d.train.users).astype(np.int32)
    top_users = known[::max(1, len(known) // TOP_USERS)][:TOP_USERS].copy()
    items, _, counts = e.recommend_batch(kn.PRED_KNN, top_users, 3)
    assert (counts == 3).all()
    settings = {"top3_of_4096_users": (np.repeat(top_users, 3), items.reshape(-1)),
                "first_1m_test_rows": (d.test.users[:TEST_ROWS], d.test.items[:TEST_ROWS])}
    res = {"U": e.num_users, "I": e.num_items, "train_ratings": len(d.train.users), "k": K, "cap": CAP, "settings": {}}
    dev = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, dtype=t)).cuda()

    def timed(call):
        before = e.timings()["predict_ms"]
        t0 = time.perf_counter()
        call()
        return (time.perf_counter() - t0) * 1e3, e.timings()["predict_ms"] - before

    for name, (u, i) in settings.items():
        n = len(u)
        tu, ti = dev(u, np.int32), dev(i, np.int32)
        raters = torch.empty((n, CAP), dtype=torch.int32, device="cuda")
        sims, devs = (torch.empty((n, CAP), dtype=torch.float64, device="cuda") for _ in range(2))
        cnt = torch.empty(n, dtype=torch.int32, device="cuda")
        sums = torch.empty((n, 2), dtype=torch.float64, device="cuda")
        pred_x, pred_p = (torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(2))
        legs = {"predict": lambda: e._check(e._lib.knncf_predict_batch_device(e._h, kn.PRED_KNN, kn._dev_ptr(tu, "int32"),
                                                                             kn._dev_ptr(ti, "int32"), n, kn._dev_ptr(pred_p, "float64")))}
        for tag, order in (("explain_sum_order", kn.EXPLAIN_SUM_ORDER), ("explain_by_weight", kn.EXPLAIN_BY_WEIGHT)):
            legs[tag] = lambda order=order: e.explain_batch_device(tu, ti, CAP, raters, sims, devs, cnt, sums, pred_x, order=order)
        note(f"{name}: {n} rows")
        for call in legs.values():  # warm-up: the builds, the scratch sizes, the code objects
            call()
        assert torch.equal(pred_x.view(torch.int64), pred_p.view(torch.int64))  # the same predictions, bit for bit
        wall, device = {t: [] for t in legs}, {t: [] for t in legs}
        for _ in range(args.repeats):
            for tag, call in legs.items():  # alternating
                w, dv = timed(call)
                wall[tag].append(w)
                device[tag].append(dv)
        c = cnt.cpu().numpy()
        out = {"rows": n, "terms_per_row_mean": float(c.mean()), "terms_per_row_max": int(c.max()),
               "rows_with_more_terms_than_cap": int((c > CAP).sum())}
        for tag in legs:
            out[tag] = {"call_ms": _summary(wall[tag]), "predict_ms": _summary(device[tag])}
        for tag in ("explain_sum_order", "explain_by_weight"):
            out[tag]["ratio_to_predict_call"] = out[tag]["call_ms"]["median"] / out["predict"]["call_ms"]["median"]
            out[tag]["ratio_to_predict_device"] = out[tag]["predict_ms"]["median"] / out["predict"]["predict_ms"]["median"]
            out[tag]["us_per_row"] = out[tag]["call_ms"]["median"] * 1e3 / n
        res["settings"][name] = out
    e.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "explain_batch_syn25m_1gpu.json"))
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--inner", action="store_true")
    args = ap.parse_args()
    if args.inner:
        return inner(args)
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--inner", "--repeats", str(args.repeats)]
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
