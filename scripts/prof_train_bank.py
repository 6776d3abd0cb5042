"""Kernel-level view of the two ways to feed the training step (scripts/time_train_bank.py's arms), for a run under
`rocprofv3 --kernel-trace`: ARM=A steps on device tensors (sort, kNN and transposition inside the step), ARM=B on ids of a cloud bank
(one assemble launch instead).  Eager steps, so that every launch is a kernel record of its own; 18 clouds x 4096 by default.
Usage (GPU box): ARM=A|B [PRECISION=bf16x6] [NEG=14] [STEPS=40] rocprofv3 --kernel-trace -d DIR -o run -- python scripts/prof_train_bank.py
then scripts/rocpd_stats.py DIR/*.db <WARM + STEPS>"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402

arm, neg = os.environ.get("ARM", "B"), int(os.environ.get("NEG", "14"))
steps, warm = int(os.environ.get("STEPS", "40")), int(os.environ.get("WARM", "10"))
TR, ops = bench.pkg("training"), bench.pkg("ops")
dev = torch.device("cuda:0")
T, M = 1 + 2 + neg + 1, 64
data = (torch.rand((M, bench.N_POINTS, 3), generator=torch.Generator().manual_seed(7)) * 2.0 - 1.0).to(dev)
store = bench.build_store("epc-net", dev, 0)
params = dict(bench.PARAMS, ARCH="epc-net", TRAIN_PRECISION=os.environ.get("PRECISION", "bf16x6"), BATCH_NUM_QUERIES=1)
ts = TR.TrainStep(params, store, outer=bench.OUTER)
bank = None
if arm == "B":
    bank = ops.CloudBank(bench.N_POINTS, M, dev)
    bank.add(data)
rng = np.random.RandomState(0)
split = lambda f: (f[:, :1], f[:, 1:3], f[:, 3:3 + neg], f[:, T - 1:])
for _ in range(warm + steps):
    ids = rng.permutation(M)[:T].reshape(1, T)
    if arm == "A":
        loss, _, _ = ts.step(*split(data[torch.from_numpy(ids.reshape(-1)).to(dev)][None]), epoch=0)
    else:
        loss, _, _ = ts.step_ids(bank, *split(ids), epoch=0)
torch.cuda.synchronize()
ops.chain_persist_check()
if bank is not None:
    bank.check()
print("arm %s: %d eager steps at %d clouds, loss %.4f" % (arm, warm + steps, T, float(loss)))
sys.exit(0 if bool(torch.isfinite(loss).all()) else 1)
