"""Hard-negative mining and the descriptor-cache refresh with the cloud bank on: host arrays against record ids, in ONE process.
  (a) the Trainer loop with mining on (bank-fed replayed step, 18 clouds x 4096 points, a descriptor table of --set-clouds >= 4000
      rows, 4000 sampled negatives per key):  arm H  Trainer(bank=True)  -- the query's descriptor from the host array through the
      whole inference pipeline at batch 1, 4000 rows of the host table gathered and uploaded, epc_pairwise_topk_ws with one query;
      arm D  Trainer(bank=True, device_mining=True)  -- forward_bank on the key's record, one 16 KB id upload, epc_mine_topk.
      Wall time per iteration, and per call of the mining alone (`_hard_negatives`, its read-back included).
  (b) a refresh of the descriptor table for 2048 clouds: get_latent_vectors on the host array against latent_vectors_bank.
  (c) the two launches of epc_mine_topk alone (one query, 4000 candidates), back to back between two events; beside it the
      one-query search over the same rows already gathered on the device (retrieval.knn_search).
The arms alternate, `--regions` timed regions, every region between device synchronisations; the median region.  Both arms of (a)
draw from the same seeds.  Exits non-zero on a non-finite loss.
One JSON line.
Usage (GPU box): python scripts/time_bank_mining.py [--iters K] [--regions R] [--set-clouds T] [--out FILE]"""
import argparse
import gc
import json
import logging
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20)          # iterations per region (below 29: no cache refresh inside a region)
ap.add_argument("--regions", type=int, default=7)
ap.add_argument("--set-clouds", type=int, default=4200)
ap.add_argument("--refresh-clouds", type=int, default=2048)
ap.add_argument("--arch", default="epc-net")
ap.add_argument("--out", default=None)
args = ap.parse_args()

TR, TL, R = bench.pkg("training"), bench.pkg("train_loop"), bench.pkg("retrieval")
dev = torch.device("cuda:0")
N = bench.N_POINTS
T_SET = args.set_clouds
failed = []
quiet = logging.getLogger("time_bank_mining")
quiet.setLevel(logging.WARNING)

rs = np.random.default_rng(0)
set_np = rs.uniform(-1, 1, (T_SET, N, 3)).astype(np.float32)


def make_queries():
    return {i: {"query": "%d.bin" % i, "positives": [j for j in range(T_SET) if j != i and abs(j - i) <= 2],
                "negatives": [j for j in range(T_SET) if abs(j - i) > 4]} for i in range(T_SET)}


def sync():
    torch.cuda.synchronize()
    return time.perf_counter()


# ---- (a) the loop with mining on ------------------------------------------------------------------------------------------------------
arms = {}
# one store, two steps (each with its own captured graph and Adam moments over the same variables, as scripts/time_train_bank.py):
# the arms train the same weights in turn, so their losses are not comparable -- equality is what tests/test_gpu_bank_mining.py holds
store = bench.build_store(args.arch, dev, 0)
params = dict(bench.PARAMS, ARCH=args.arch, TRAIN_PRECISION="bf16", BATCH_NUM_QUERIES=1, POSITIVES_PER_QUERY=2,
              NEGATIVES_PER_QUERY=14, NUM_POINTS=N, BASE_LEARNING_RATE=5e-5)
for name, on_device in (("H", False), ("D", True)):
    ts = TR.TrainStep(params, store, outer=bench.OUTER)
    tr = TL.Trainer(ts, make_queries(), set_np, logger=quiet, graph=True, bank=True, device_mining=on_device)
    arms[name] = tr
table_np = arms["H"].get_latent_vectors()                  # both arms mine against the same numpy cache (D uploads it once)
state = {}
for name, tr in arms.items():
    tr.TRAINING_LATENT_VECTORS = table_np
    state[name] = (random.Random(0).getstate(), np.random.RandomState(0).get_state())


def run_loop(name, iters):
    """`iters` iterations of the arm's loop, continuing ITS OWN random streams (so both arms draw the same tuples)."""
    tr = arms[name]
    random.setstate(state[name][0])
    np.random.set_state(state[name][1])
    losses = tr.train_one_epoch(1, max_iters=iters)
    state[name] = (random.getstate(), np.random.get_state())
    return losses


all_losses = {"H": [], "D": []}
for name in arms:
    all_losses[name] += run_loop(name, args.iters)         # warm-up: code objects, the captured step, the packed weights
times = {"H": [], "D": []}
steps = {"H": 0, "D": 0}
for _ in range(args.regions):
    for name in arms:
        t0 = sync()
        got = run_loop(name, args.iters)
        times[name].append(sync() - t0)
        steps[name] = len(got)
        all_losses[name] += got
loop_ms = {a: statistics.median(v) / args.iters * 1e3 for a, v in times.items()}
for name in arms:
    if not all(np.isfinite(all_losses[name])):
        failed.append("loop arm %s: non-finite loss" % name)

# the mining alone, per key (wall time: every call ends with its read-back)
mine_ms = {}
keys = list(range(100, 100 + 40))
for name, tr in arms.items():
    per = []
    for rep in range(args.regions):
        np.random.seed(rep)
        t0 = sync()
        for k in keys:
            tr._hard_negatives(k)
        per.append((sync() - t0) / len(keys) * 1e3)
    mine_ms[name] = statistics.median(per)

# ---- (b) the refresh of the descriptor table ------------------------------------------------------------------------------------------
RC = min(args.refresh_clouds, T_SET)
trD = arms["D"]
trD.step._ensure_built(N)
ids = torch.arange(RC, dtype=torch.int32, device=dev)
refresh = {"host_arrays": [], "bank": []}
ref_h = trD.get_latent_vectors(set_np[:RC])                # (warm-up of both forms)
ref_d = R.latent_vectors_bank(trD._engine(), trD.bank, ids)
same_refresh = bool(np.array_equal(ref_h.view(np.uint32), ref_d.cpu().numpy().view(np.uint32)))
for _ in range(args.regions):
    t0 = sync()
    trD.get_latent_vectors(set_np[:RC])
    refresh["host_arrays"].append(sync() - t0)
    t0 = sync()
    R.latent_vectors_bank(trD._engine(), trD.bank, ids)
    refresh["bank"].append(sync() - t0)
refresh_ms = {k: statistics.median(v) * 1e3 for k, v in refresh.items()}

# ---- (c) the mining launches alone ------------------------------------------------------------------------------------------------------
table = torch.from_numpy(table_np).to(dev)
cand = torch.from_numpy(np.random.RandomState(1).permutation(T_SET)[:4000].astype(np.int32)).to(dev).view(1, 4000)
count = torch.full((1,), 4000, dtype=torch.int32, device=dev)
query = table[7:8].contiguous()
rows = table[cand[0].long()].contiguous()
ws = torch.empty(int(bench.pkg("lib").lib().epc_mine_topk_workspace_bytes(1, 4000)), dtype=torch.uint8, device=dev)
launch_us = {}
for what, fn in (("mine_topk_two_launches", lambda: R.mine_topk(table, query, cand, count, 10, workspace=ws)),
                 ("knn_search_on_gathered_rows", lambda: R.knn_search(rows, query, 10))):
    for _ in range(20):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    per, reps = [], 200
    for _ in range(5):
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        per.append(e0.elapsed_time(e1) * 1e3 / reps)
    launch_us[what] = round(statistics.median(per), 2)

line = {"workload": "%s: Trainer(bank=True) with hard-negative mining on, 18 x %d clouds per replayed step, %d-row descriptor table, "
                    "4000 sampled negatives; arm H = host mining, arm D = device_mining=True" % (args.arch, N, T_SET),
        "loop_ms_per_iteration": {a: round(v, 4) for a, v in loop_ms.items()}, "D_over_H": round(loop_ms["D"] / loop_ms["H"], 4),
        "loop_regions_s": {a: [round(t, 5) for t in v] for a, v in times.items()},
        "steps_per_region": steps,
        "mining_ms_per_key": {a: round(v, 4) for a, v in mine_ms.items()},
        "refresh_ms_%d_clouds" % RC: {k: round(v, 3) for k, v in refresh_ms.items()}, "refresh_equal_bits": same_refresh,
        "launches_us_one_query_4000_candidates": launch_us,
        "iterations_per_region": args.iters, "regions": args.regions, "failed": failed, "lib_sha256": bench.lib_sha256()}
text = json.dumps(line)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
del arms
gc.collect()
sys.exit(1 if failed else 0)
