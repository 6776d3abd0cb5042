"""Training tuples from poses at the Oxford training-set size (T = 21 711 records, a synthetic loop trajectory with about 41 positives per
record), ONE process, one MI355X, 18-cloud tuples (P = 2, Nn = 14), bf16, the step replayed as a HIP graph, a descriptor cache present
so that the hard-negative mining runs:
  (a) the Trainer loop, wall time per iteration between device synchronisations, the arms alternating:
        arm H  Trainer(bank=True, device_mining=True) on a reference-format dict (the host path as it was: per tuple
               get_query_tuple_ids shuffles the ~21 000-entry negatives list, builds set(QUERY_DICT.keys()) - set(neighbors) and shuffles
               that; per key one upload of the sampled ids and one read-back of the mined ones);
        arm P  the same with poses=: candidates -> forward_bank -> mine_topk -> sample -> step_ids, nothing read but the loss.
      The dict is what ``query_dict_from_poses`` returns (checked here on the first 300 records), except that a record's negatives list
      is built when the loop first asks for it -- before the timed region: all 21 711 lists at once are 4.7 x 10^8 Python ints.
  (b) the GPU time of ``PoseTuples.candidates`` (C = 4000) and ``PoseTuples.sample`` (H = 10 mined ids) alone, per key: one pair of
      events around each call, the median over --keys keys.
The two arms share the bank and the descriptor cache and train the same weights in turn (their losses are not comparable; what the
device draw computes is held to tests/tuples_ref.py by tests/test_gpu_pose_tuples.py).  Exits non-zero on a non-finite loss.
One JSON line.
Usage (GPU box): python scripts/time_pose_tuples.py [--records T] [--iters K] [--regions R] [--keys Q] [--out FILE]"""
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
ap.add_argument("--records", type=int, default=21711)
ap.add_argument("--iters", type=int, default=20)          # iterations per region (below 29: no cache refresh inside a region)
ap.add_argument("--regions", type=int, default=7)
ap.add_argument("--keys", type=int, default=64)
ap.add_argument("--points", type=int, default=bench.N_POINTS)
ap.add_argument("--arch", default="epc-net")
ap.add_argument("--out", default=None)
args = ap.parse_args()

T, N, P, NN = args.records, args.points, 2, 14
R_POS, R_NEG = 10.0, 50.0


def loop_poses(count, spacing=0.4878):
    """A closed loop driven once, a record every `spacing` metres (20 m / 0.4878 m = 41 positives), +-0.25 m of lateral noise."""
    rng = np.random.default_rng(0)
    radius = count * spacing / (2 * np.pi)
    t = np.arange(count) * (2 * np.pi / count)
    r = radius + rng.uniform(-0.25, 0.25, count)
    return np.stack([5735000.0 + r * np.cos(t), 620000.0 + r * np.sin(t)], 1)


class _Entry(dict):
    """One record of the training dict; its 'negatives' list (every record farther than R_NEG, ascending) is built on first use."""

    def __init__(self, poses, key, positives):
        super().__init__(query="%d.bin" % key, positives=positives)
        self._poses, self._key = poses, key

    def __missing__(self, name):
        if name != "negatives":
            raise KeyError(name)
        d = self._poses - self._poses[self._key]
        self["negatives"] = np.nonzero(~(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] <= R_NEG * R_NEG))[0].tolist()
        return self["negatives"]


def lazy_queries(poses):
    ops = bench.pkg("ops")
    near, near_len = (t.cpu().numpy() for t in ops.pose_radius_lists(poses, poses, R_POS))
    out = {}
    for i in range(len(poses)):
        row = near[i, :near_len[i]]
        out[i] = _Entry(poses, i, row[row != i].tolist())
    return out, float(near_len.mean() - 1.0)


def sync():
    torch.cuda.synchronize()
    return time.perf_counter()


if not torch.cuda.is_available():
    sys.exit("time_pose_tuples.py measures on an MI355X: no ROCm device visible")
TR, TL, RT, LP, ops = (bench.pkg(m) for m in ("training", "train_loop", "retrieval", "utils.loading_pointclouds", "ops"))
dev = torch.device("cuda:0")
failed = []
quiet = logging.getLogger("time_pose_tuples")
quiet.setLevel(logging.WARNING)

poses = loop_poses(T)
small, _ = lazy_queries(poses[:300])
want = LP.query_dict_from_poses(poses[:300], R_POS, R_NEG)
if any(small[i]["positives"] != want[i]["positives"] or small[i]["negatives"] != want[i]["negatives"] for i in range(300)):
    failed.append("the lazily built dict differs from query_dict_from_poses")
queries, mean_positives = lazy_queries(poses)

rs = np.random.default_rng(0)
data = np.empty((T, N, 3), dtype=np.float32)
for a in range(0, T, 2048):
    data[a:a + 2048] = rs.uniform(-1, 1, (min(2048, T - a), N, 3)).astype(np.float32)

store = bench.build_store(args.arch, dev, 0)
params = dict(bench.PARAMS, ARCH=args.arch, TRAIN_PRECISION="bf16", BATCH_NUM_QUERIES=1, POSITIVES_PER_QUERY=P,
              NEGATIVES_PER_QUERY=NN, NUM_POINTS=N, BASE_LEARNING_RATE=5e-5)
arms = {}
shared = {}
build_bank = TL.Trainer._build_bank
TL.Trainer._build_bank = lambda self, d: shared["bank"] if "bank" in shared else shared.setdefault("bank", build_bank(self, d))   # ONE bank
t0 = time.perf_counter()
for name in ("H", "P"):
    ts = TR.TrainStep(params, store, outer=bench.OUTER)
    arms[name] = TL.Trainer(ts, queries if name == "H" else None, data, logger=quiet, graph=True, bank=True, device_mining=True,
                            poses=poses if name == "P" else None, tuple_seed=0)
TL.Trainer._build_bank = build_bank
setup_s = time.perf_counter() - t0
arms["H"].step._ensure_built(N)
table = RT.latent_vectors_bank(arms["H"]._engine(), arms["H"].bank)        # the descriptor cache, on the device, for both arms
for tr in arms.values():
    tr.TRAINING_LATENT_VECTORS = table
state = {name: (random.Random(0).getstate(), np.random.RandomState(0).get_state()) for name in arms}


def run_loop(name, iters):
    """`iters` iterations of the arm's loop, continuing ITS OWN random streams.  Arm H: the negatives lists of the keys the epoch will
    visit are built first (the permutation is drawn ahead from a copy of the stream), outside the timed region."""
    tr = arms[name]
    random.setstate(state[name][0])
    np.random.set_state(state[name][1])
    if name == "H":
        ahead = np.arange(T)
        np.random.shuffle(ahead)
        for k in ahead[:iters]:
            queries[int(k)]["negatives"]
        np.random.set_state(state[name][1])
    t0 = sync()
    losses = tr.train_one_epoch(1, max_iters=iters)
    dt = sync() - t0
    state[name] = (random.getstate(), np.random.get_state())
    return losses, dt


all_losses = {"H": [], "P": []}
for name in arms:
    all_losses[name] += run_loop(name, args.iters)[0]         # warm-up: code objects, the captured step, the packed weights
times = {"H": [], "P": []}
steps = {"H": 0, "P": 0}
for _ in range(args.regions):
    for name in arms:
        got, dt = run_loop(name, args.iters)
        times[name].append(dt)
        steps[name] = len(got)
        all_losses[name] += got
loop_ms = {a: statistics.median(v) / args.iters * 1e3 for a, v in times.items()}
for name in arms:
    if not all(np.isfinite(all_losses[name])) or steps[name] != args.iters:
        failed.append("loop arm %s: non-finite loss or skipped iterations (%d of %d)" % (name, steps[name], args.iters))
arms["P"].tuples.check()

# the host path's sampling alone, per key (wall time; no GPU work in it): what arm H pays on the host for every tuple
host_ms = []
random.seed(1)
for k in np.random.RandomState(1).permutation(T)[:20]:
    k = int(k)
    queries[k]["negatives"]
    t0 = time.perf_counter()
    LP.get_query_tuple_ids(k, queries[k], P, NN, queries, hard_neg=[], other_neg=True)
    host_ms.append((time.perf_counter() - t0) * 1e3)

# ---- (b) the two sampler launches alone ------------------------------------------------------------------------------------------------------
pt = arms["P"].tuples
keys = torch.from_numpy(np.random.RandomState(2).permutation(T)[:args.keys].astype(np.int32)).to(dev)
cand = (torch.empty((1, TL.SAMPLED_NEG), dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev))
ws = torch.empty(int(bench.pkg("lib").lib().epc_mine_topk_workspace_bytes(1, TL.SAMPLED_NEG)), dtype=torch.uint8, device=dev)
e0, e1, e2, e3 = (torch.cuda.Event(enable_timing=True) for _ in range(4))
cand_us, sample_us = [], []
for rep in range(2):                                        # (the first sweep warms both kernels up)
    cand_us, sample_us = [], []
    for i in range(args.keys):
        key = keys[i:i + 1]
        e0.record()
        pt.candidates(key, 1000 + i, TL.SAMPLED_NEG, out=cand)
        e1.record()
        _, _, mined = RT.mine_topk(table, table[key.long()].contiguous(), cand[0], cand[1], TL.NUM_TO_TAKE, workspace=ws)
        e2.record()
        pt.sample(key, 1000 + i, P, NN, hard=mined)
        e3.record()
        torch.cuda.synchronize()
        cand_us.append(e0.elapsed_time(e1) * 1e3)
        sample_us.append(e2.elapsed_time(e3) * 1e3)
pt.check()
sampler_us = statistics.median(cand_us) + statistics.median(sample_us)
STEP_MS = 1.72                                              # the replayed bank-fed step these launches feed (README.md, profiles/r08_train_bank_time.json)

line = {"workload": "%s: Trainer(bank=True, device_mining=True), mining on, %d records (loop trajectory, %.1f positives per record), 18 x %d "
                    "clouds per replayed step, bf16; arm H = reference-format dict on the host path, arm P = poses=" % (args.arch, T, mean_positives, N),
        "loop_ms_per_iteration": {a: round(v, 4) for a, v in loop_ms.items()}, "P_over_H": round(loop_ms["P"] / loop_ms["H"], 4),
        "loop_regions_s": {a: [round(t, 5) for t in v] for a, v in times.items()},
        "host_get_query_tuple_ids_ms_per_key": {"median": round(statistics.median(host_ms), 3), "min": round(min(host_ms), 3)},
        "gpu_us_per_key": {"candidates_C4000": round(statistics.median(cand_us), 2), "sample_H10": round(statistics.median(sample_us), 2),
                           "candidates_min_max": [round(min(cand_us), 2), round(max(cand_us), 2)],
                           "sample_min_max": [round(min(sample_us), 2), round(max(sample_us), 2)], "keys": args.keys},
        "sampler_us_per_key": round(sampler_us, 2), "replayed_step_ms": STEP_MS, "sampler_below_step": bool(sampler_us < STEP_MS * 1e3),
        "poses_faster_than_host_path": bool(loop_ms["P"] < loop_ms["H"]),
        "iterations_per_region": args.iters, "regions": args.regions, "setup_s": round(setup_s, 2), "failed": failed,
        "lib_sha256": bench.lib_sha256()}
text = json.dumps(line)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
del arms
gc.collect()
sys.exit(1 if failed else 0)
