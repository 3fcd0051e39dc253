"""Randomised call sequences on one handle against the stateful model (run on an MI355X): the hand-run companion of
scripts/fuzz_parity.py for tests/test_gpu_call_sequences.py.  Fresh seeds beyond the committed ones go through the same
generator and model (tests/call_sequences.py): per seed an order-sensitive fit (40 users, 18 of them with <= 4 ratings), a
similarity, a first k and cs.N_OPS ops over every kind of cs.KINDS — those of the classes beside Engine among them: appends
and amends (which replace the fit and keep lists; an amend also takes a user or an item out of it, and num_users / num_items
are compared after each), entered calls (which build every missing list, with and without removals) and bystander calls of the
three families.  Stops at the first
mismatch or unexpected status and prints the seed and the op to replay; nothing is started after an error and nothing is tried
twice.
usage: python scripts/fuzz_sequences.py [first_seed] [count]"""
import importlib
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import call_sequences as cs  # noqa: E402

kn = importlib.import_module("movie-recommender-system_amd.knncf")
oracle = importlib.import_module("oracle.knncf_oracle")
kn.load_library()

first = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
count = int(sys.argv[2]) if len(sys.argv) > 2 else 200
tmp = tempfile.mkdtemp(prefix="fuzz_sequences_")
done = 0
for seed in range(first, first + count):
    sim = ("cosine", "jaccard")[seed % 3 == 2]
    case = cs.Case(f"seed{seed}", seed, (2, 6, cs.K_ALL)[seed % 3 if seed % 3 < 2 else (seed // 3) % 3], seed)
    ops = case.ops(oracle)
    model = case.model(oracle, sim)
    e = kn.Engine(k=case.k, similarity={"cosine": kn.SIM_COSINE, "jaccard": kn.SIM_JACCARD}[sim]).fit(*case.train())
    player = cs.Player(kn, e, tmp, "fuzz", case.train())
    for j, op in enumerate(ops):
        try:
            got, want = player.play(op), model.call(op)
        except Exception as ex:  # noqa: BLE001  (an unexpected status or error: report how to replay it, then stop)
            print(f"ERROR seed {seed} (fit and sequence), {sim}, first k {case.k}, op {j}: {op!r}\n  {ex!r}", flush=True)
            sys.exit(2)
        if not cs.same(got, want):
            print(f"MISMATCH seed {seed} (fit and sequence), {sim}, first k {case.k}, op {j}: {op!r}", flush=True)
            print(f"  engine {got!r}\n  model  {want!r}", flush=True)
            print(f"fuzz sequences: {done} cases without a mismatch, stopped at seed {seed}", flush=True)
            sys.exit(1)
        if op.kind in cs.REFITS and (e.num_users, e.num_items) != (len(model.known_users), len(model.known_items)):
            print(f"MISMATCH seed {seed} (fit and sequence), {sim}, first k {case.k}, op {j}: {op!r}", flush=True)
            print(f"  engine users, items {(e.num_users, e.num_items)}\n  model  {(len(model.known_users), len(model.known_items))}", flush=True)
            print(f"fuzz sequences: {done} cases without a mismatch, stopped at seed {seed}", flush=True)
            sys.exit(1)
    e.close()
    done += 1
    if done % 20 == 0:
        print(f"... {done} cases, no mismatch so far", flush=True)  # (a silent GPU command is taken to be hung)
print(f"fuzz sequences: {done} cases of {cs.N_OPS} ops (seeds {first}..{first + count - 1}), 0 mismatches", flush=True)
