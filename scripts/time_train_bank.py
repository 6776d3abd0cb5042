"""The training step fed from a device-resident cloud bank against the step fed with device tensors, in ONE process.
  arm A  TrainStep.step(..., graph=True) on clouds picked by torch indexing from a device-resident array (today's best case: what
         bench.py's training leg times) -- the replayed graph sorts, searches and transposes the tuple's clouds every step;
  arm B  TrainStep.step_ids(bank, ..., graph=True) -- the replayed graph assembles them from the bank (epc_bank_assemble).
Cells: 18 and 22 clouds x 4096 points, TRAIN_PRECISION "bf16" and "bf16x6"; a different tuple every step, the same tuples in both arms.
The arms alternate, `--regions` timed regions of `--steps` steps each, every region between device synchronisations; the median region.
Also: the bank's build time per 1000 clouds and bytes per cloud, the assemble kernel's own time and GB/s (back-to-back launches between
two events), and the wall time per iteration of the Trainer loop (host tuple assembly + upload included) with and without the bank.
Exits non-zero on a non-finite loss, a set ops.chain_persist_check() word or a bad id.  One JSON line.
Usage (GPU box): python scripts/time_train_bank.py [--steps K] [--regions R] [--warmup W] [--out FILE]"""
import argparse
import gc
import json
import logging
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--regions", type=int, default=7)
ap.add_argument("--warmup", type=int, default=40)
ap.add_argument("--bank-clouds", type=int, default=256)
ap.add_argument("--arch", default="epc-net")
ap.add_argument("--out", default=None)
args = ap.parse_args()

TR, ops, TL = bench.pkg("training"), bench.pkg("ops"), bench.pkg("train_loop")
dev = torch.device("cuda:0")
N, CAP = bench.N_POINTS, 32
g = torch.Generator().manual_seed(7)
data = (torch.rand((args.bank_clouds, N, 3), generator=g) * 2.0 - 1.0).to(dev)
M = int(data.shape[0])

# ---- the bank: build cost, bytes ----------------------------------------------------------------------------------------------
ops.CloudBank(N, 64, dev).add(data[:64])          # (first launches: code objects)
torch.cuda.synchronize()
t0 = time.perf_counter()
bank = ops.CloudBank(N, M, dev)
bank.add(data)
torch.cuda.synchronize()
build_s = time.perf_counter() - t0

# ---- the assemble kernel alone ---------------------------------------------------------------------------------------------------
rng = np.random.RandomState(0)
assemble = {}
for T in (18, 22):
    ids = torch.from_numpy(rng.permutation(M)[:T].astype(np.int32)).to(dev)
    out = bank.buffers(T)
    for _ in range(20):
        bank.assemble(ids, out=out)
    reps = 200
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    per = []
    for _ in range(5):
        e0.record()
        for _ in range(reps):
            bank.assemble(ids, out=out)
        e1.record()
        torch.cuda.synchronize()
        per.append(e0.elapsed_time(e1) * 1e3 / reps)
    used = (out["roff"].view(T, N)[:, -1] + out["rdeg"].view(T, N)[:, -1] - torch.arange(T, device=dev) * (N * CAP)).cpu().numpy()
    oc = out["ovf_cnt"].cpu().numpy()
    chunks = lambda v: int(((v + 7) // 8).sum())
    rd = T * (16 + N * 28 + N * CAP * 2) + 16 * (chunks(used) + chunks(oc))
    wr = T * (N * 28 + N * CAP * 4 + 4) + 32 * (chunks(used) + chunks(oc))
    us = statistics.median(per)
    assemble[str(T)] = {"us_per_launch": round(us, 2), "bytes_read": rd, "bytes_written": wr,
                        "GB_per_s": round((rd + wr) / us / 1e3, 1), "rlist_slots_used": round(float(used.mean()) / (N * CAP), 3)}
bank.check()

# ---- the step: arm A (device tensors) against arm B (ids) ---------------------------------------------------------------------
cells = {}
failed = []
for prec in ("bf16", "bf16x6"):
    for neg in (14, 18):
        T = 1 + 2 + neg + 1
        store = bench.build_store(args.arch, dev, 0)
        params = dict(bench.PARAMS, ARCH=args.arch, TRAIN_PRECISION=prec, BATCH_NUM_QUERIES=1, DECAY_STEP=200000,
                      BASE_LEARNING_RATE=5e-5, MARGIN_1=0.5, MARGIN_2=0.2)
        # one store, two steps: each holds its own captured graph (and Adam moments) over the same variables
        step = {"A": TR.TrainStep(params, store, outer=bench.OUTER), "B": TR.TrainStep(params, store, outer=bench.OUTER)}
        total = args.warmup + args.regions * args.steps
        tuples = [rng.permutation(M)[:T].reshape(1, T) for _ in range(total)]
        tuples_dev = [torch.from_numpy(t.reshape(-1)).to(dev) for t in tuples]
        split = lambda f: (f[:, :1], f[:, 1:3], f[:, 3:3 + neg], f[:, T - 1:])
        cursor = {"A": 0, "B": 0}

        def run(arm, k):
            loss = None
            for _ in range(k):
                i = cursor[arm]
                cursor[arm] += 1
                if arm == "A":
                    t = data[tuples_dev[i]][None]             # (1, T, n, 3): one gather; its four slices are copied as one tensor
                    loss, _, _ = step[arm].step(*split(t), epoch=0, graph=True)
                else:
                    loss, _, _ = step[arm].step_ids(bank, *split(tuples[i]), epoch=0, graph=True)
            return loss

        last = {}
        for arm in ("A", "B"):
            last[arm] = run(arm, args.warmup)
        torch.cuda.synchronize()
        times = {"A": [], "B": []}
        for _ in range(args.regions):
            for arm in ("A", "B"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                last[arm] = run(arm, args.steps)
                torch.cuda.synchronize()
                times[arm].append(time.perf_counter() - t0)
        ms = {a: statistics.median(v) / args.steps * 1e3 for a, v in times.items()}
        for arm in ("A", "B"):
            if not bool(torch.isfinite(last[arm]).all()):
                failed.append("%s/%d/%s: non-finite loss" % (prec, T, arm))
        try:
            ops.chain_persist_check()
            bank.check()
        except Exception as exc:      # noqa: BLE001  (reported, then a non-zero exit)
            failed.append("%s/%d: %s" % (prec, T, exc))
        cells["%s/%d" % (prec, T)] = {"ms_per_step": {a: round(v, 4) for a, v in ms.items()}, "B_over_A": round(ms["B"] / ms["A"], 4),
                                      "saved_us": round((ms["A"] - ms["B"]) * 1e3, 1),
                                      "regions_s": {a: [round(t, 5) for t in v] for a, v in times.items()}}
        del step, store
        gc.collect()
        torch.cuda.empty_cache()

# ---- the Trainer loop: wall time per iteration, host work included ------------------------------------------------------------
loop = {}
T_SET = 60
rs = np.random.default_rng(0)
set_np = rs.uniform(-1, 1, (T_SET, N, 3)).astype(np.float32)
quiet = logging.getLogger("time_train_bank")
quiet.setLevel(logging.WARNING)
for use_bank in (False, True):
    queries = {i: {"query": "%d.bin" % i, "positives": [j for j in range(T_SET) if j != i and abs(j - i) <= 2],
                   "negatives": [j for j in range(T_SET) if abs(j - i) > 4]} for i in range(T_SET)}
    store = bench.build_store(args.arch, dev, 0)
    params = dict(bench.PARAMS, ARCH=args.arch, TRAIN_PRECISION="bf16", BATCH_NUM_QUERIES=1, POSITIVES_PER_QUERY=2,
                  NEGATIVES_PER_QUERY=14, NUM_POINTS=N)
    ts = TR.TrainStep(params, store, outer=bench.OUTER)
    tr = TL.Trainer(ts, queries, set_np, logger=quiet, graph=True, bank=use_bank)
    import random
    random.seed(0)
    np.random.seed(0)
    tr.train_one_epoch(1, max_iters=30)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    losses = tr.train_one_epoch(1, max_iters=50)
    torch.cuda.synchronize()
    loop["bank" if use_bank else "arrays"] = round((time.perf_counter() - t0) / max(len(losses), 1) * 1e3, 4)
    if not all(np.isfinite(losses)):
        failed.append("trainer loop (bank=%s): non-finite loss" % use_bank)
    del tr, ts, store
    gc.collect()
    torch.cuda.empty_cache()

line = {"workload": "%s training step, 18 / 22 x %d clouds, HIP graph replay; arm A = step on device tensors, arm B = step_ids on the "
                    "cloud bank" % (args.arch, N),
        "cells": cells, "assemble_kernel": assemble,
        "bank": {"clouds": M, "bytes_per_cloud": bank.bytes_per_cloud, "int32_bytes_per_cloud": N * 28 + N * CAP * 8 + N * 4 + 4,
                 "build_s_per_1000_clouds": round(build_s / M * 1000, 3)},
        "trainer_loop_ms_per_iteration_18x4096_bf16": loop,
        "steps_per_region": args.steps, "regions": args.regions, "failed": failed, "lib_sha256": bench.lib_sha256()}
text = json.dumps(line)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
sys.exit(1 if failed else 0)
