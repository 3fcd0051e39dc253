"""bench.py's options around the headline line: --steps / --warmup as given, the lean default run, what --full adds, and
--dump-outputs (the arrays of the last timed step, checked here bit for bit against the oracle)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (6000, 1500, 400_000)
K = 40
WORKLOAD = ["--workload", "syn-scaled:%d:%d:%d" % SHAPE, "--k", str(K)]


def _bench(args, timeout=600):
    r = subprocess.run([sys.executable, "bench.py"] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_bench_options_without_a_gpu():
    h = subprocess.run([sys.executable, "bench.py", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert h.returncode == 0 and "--full" in h.stdout and "--dump-outputs" in h.stdout
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        r = subprocess.run([sys.executable, "bench.py"] + bad, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "--steps must be >= 1" in r.stderr


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step_outputs(tmp_path, synth, oracle):
    a = _bench(WORKLOAD + ["--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "a")])
    assert a["steps"] == 3 and a["warmup"] == 1 and a["ms_per_step"] > 0 and a["higher_is_better"] is True
    assert not {"cpu_baseline", "cpu_baseline_all_cores", "bf16_filter"} & set(a)   # the lean default: only the steps
    out = _load(tmp_path / "a")
    assert set(out) == {"mae", "predictions", "neighbor_users", "neighbor_ids", "neighbor_sims"}
    assert all(v.dtype == np.float64 for v in out.values()) and sum(v.nbytes for v in out.values()) <= 64_000_000
    d = synth.syn_scaled(*SHAPE, seed=25)
    assert out["mae"].tolist() == [a["mae"], len(d.test)]
    # every prediction and the sampled neighbour lists, bit for bit against the oracle's bulk form
    m = oracle.Model(d.train.users, d.train.items, d.train.ratings)
    _, want = m.knn_table(K).mae(d.test.users, d.test.items, d.test.ratings)
    assert np.array_equal(out["predictions"].view(np.int64), want.view(np.int64))
    users = out["neighbor_users"].astype(np.int32)
    assert len(users) == 1024 and out["neighbor_ids"].shape == (1024, K)
    table = m.knn_table(K, users=users)
    assert np.array_equal(table.row_user, users)
    assert np.array_equal(out["neighbor_ids"], table.ids.astype(np.float64))
    assert np.array_equal(out["neighbor_sims"].view(np.int64), table.sims.view(np.int64))
    # another number of steps, the same inputs: the same outputs
    b = _bench(WORKLOAD + ["--steps", "1", "--warmup", "0", "--dump-outputs", str(tmp_path / "b")])
    assert b["steps"] == 1 and b["mae"] == a["mae"]
    again = _load(tmp_path / "b")
    assert set(again) == set(out) and all(np.array_equal(again[n].view(np.int64), out[n].view(np.int64)) for n in out)


@pytest.mark.gpu
def test_full_adds_the_bf16_leg_and_the_cpu_baselines():
    f = _bench(WORKLOAD + ["--steps", "2", "--warmup", "1", "--full", "--cpu-baseline-seconds", "0.5"])
    assert f["steps"] == 2 and f["ms_per_step"] > 0
    assert f["bf16_filter"]["mae"] == f["mae"] and f["bf16_filter"]["value"] > 0
    assert f["cpu_baseline"]["value"] > 0 and f["cpu_baseline"]["cores"] == 1
