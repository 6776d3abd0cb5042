"""Pair registration against the torch pass it replaces, at n = 1024 and 4096 rows per cloud and P = 5, 320 and 4096 pairs (H = 8 seeds,
16 iterations, max_dist 1 m): per (n, P) (a) the median time of one retrieval.register_pairs call -- 8 + 16 correspondence passes --, (b)
the median time of ONE correspondence pass through the entry (one seed, no iteration: its three launches, the pass among them) and (c) in
the same process one correspondence pass done the way a user would do it without this kernel: torch.cdist + argmin per pair, as a Python
loop over the pairs and, the stronger form, batched over as many pairs as keep the distance matrix below 1 GiB.  HIP events around
`--steps` calls, `--regions` regions, the median region, the arms alternating; everything runs eagerly on one stream.  The bar set in
advance: the kernel's pass is not slower than the faster torch pass at any of these sizes; the JSON says which way it came out.

Without --one the script touches no device itself: it starts one child process per (n, P) (`--one n,P`) under a time limit of its own,
stops at the first child that fails, and writes the children's lines as one JSON document, stamped with the SHA-256 of the loaded library.
Usage (GPU box): python scripts/time_register.py [--sizes 1024,4096] [--pairs 5,320,4096] [--steps K] [--regions R] [--warmup W]
[--limit SECONDS] [--out FILE]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _timing  # noqa: E402

DEFAULT_OUT = os.path.join(ROOT, "profiles", "r14_register_time.json")

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="1024,4096")
ap.add_argument("--pairs", default="5,320,4096")
ap.add_argument("--seeds", type=int, default=8)
ap.add_argument("--iterations", type=int, default=16)
ap.add_argument("--steps", type=int, default=2)
ap.add_argument("--regions", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--limit", type=int, default=240, help="seconds one child may take")
ap.add_argument("--one", default="", help="(child) measure this n,P and print its JSON line")
ap.add_argument("--out", default=DEFAULT_OUT)
args = ap.parse_args()

if not args.one:
    lines = _timing.children(__file__, ["%s,%s" % (n, P) for n in args.sizes.split(",") for P in args.pairs.split(",")],
                             ["--steps", args.steps, "--regions", args.regions, "--warmup", args.warmup, "--seeds", args.seeds,
                              "--iterations", args.iterations], args.limit)
    slower = [(l["n"], l["P"]) for l in lines if l["pass_over_torch"] > 1.0]
    _timing.emit({"workload": "P pairs among 64 views of a structured scene of n rows, %d seeds per pair a few degrees apart, %d iterations, max_dist "
                              "1 m, min_pairs 32" % (args.seeds, args.iterations),
                  "timer": "HIP events around %d calls; median of %d regions, the arms alternating; eager, one stream; one process per (n, P)"
                           % (args.steps, args.regions),
                  "bar": "one correspondence pass through the entry is not slower than the faster torch.cdist + argmin pass",
                  "verdict": "met at every size" if not slower else "MISSED at (n, P) = %s" % slower,
                  "sizes": lines, "lib_sha256": lines[0]["lib_sha256"]}, args.out)
    raise SystemExit(0)

sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import register_ref as R  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("time_register.py measures on the device: no ROCm device is visible")
RT, L = bench.pkg("retrieval"), bench.pkg("lib")
dev = torch.device("cuda:0")
n, P = (int(v) for v in args.one.split(","))
Hs, C = args.seeds, 64
rng = np.random.default_rng([n, P])
scene = R.structured_scene(1, n)
views = []
for c in range(C):
    m = R.pose_of(rng.uniform(-8, 8), rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(-0.8, 0.8, size=3))
    views.append((R.apply_pose(m, scene) + 0.02 * rng.normal(size=scene.shape))[rng.permutation(n)])
clouds = torch.from_numpy(np.stack(views).astype(np.float32)).to(dev)
pairs_h = np.stack([rng.integers(0, C, size=P), rng.integers(0, C, size=P)], 1).astype(np.int32)
pairs = torch.from_numpy(pairs_h).to(dev)
base = np.stack([R.pose_of(a, b, 0.0, (0.1 * a, 0.0, 0.0)) for a, b in ((0, 0), (4, 0), (-4, 0), (8, 0), (-8, 0), (0, 3), (0, -3), (12, 0))][:Hs])
seeds = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(base, (P, Hs, 12)))).to(dev)
ws = torch.empty(int(L.lib().epcnet_pair_register_workspace_bytes(P, Hs, n)), dtype=torch.uint8, device=dev)
kw = dict(max_dist=1.0, min_pairs=32, workspace=ws)

# the timed calls compute what they should: the first pairs against the restatement, bit for bit
few = min(P, 2 if n > 1024 else 4)
got = RT.register_pairs(clouds, pairs[:few].contiguous(), seeds[:few].contiguous(), iterations=2, **kw)
torch.cuda.synchronize()
want = R.register_reference(np.stack(views).astype(np.float32), pairs_h[:few], seeds[:few].cpu().numpy(), 1.0, 2, 32)
assert got[0].cpu().numpy().tobytes() == want[0].tobytes() and got[3].cpu().tolist() == want[3].tolist(), "the entry equals its restatement"

src_of, tgt_of = pairs[:, 0].long(), pairs[:, 1].long()
batch = max(1, min(P, (1 << 28) // (n * n)))


def torch_pass_loop():
    out = []
    for i in range(P):
        out.append(torch.cdist(clouds[pairs_h[i, 0]], clouds[pairs_h[i, 1]]).argmin(1))
    return out


def torch_pass_batched():
    out = []
    for a in range(0, P, batch):
        out.append(torch.cdist(clouds[src_of[a:a + batch]], clouds[tgt_of[a:a + batch]]).argmin(2))
    return out


arms = {"register_pairs": lambda: RT.register_pairs(clouds, pairs, seeds, iterations=args.iterations, **kw),
        "one_pass_entry": lambda: RT.register_pairs(clouds, pairs, None, iterations=0, **kw),
        "torch_pass_loop": torch_pass_loop,
        "torch_pass_batched": torch_pass_batched}
times = {name: [1e3 * t / args.steps for t in v]                             # seconds per region -> ms per call
         for name, v in _timing.alternate(arms, args.steps, args.regions, args.warmup, events=True).items()}
ms = {name: statistics.median(v) for name, v in times.items()}
ratio = ms["one_pass_entry"] / min(ms["torch_pass_loop"], ms["torch_pass_batched"])
passes = Hs + args.iterations
_timing.emit({"n": n, "P": P, "seeds": Hs, "iterations": args.iterations, "passes_per_call": passes,
              "ms_per_call": {k: round(v, 4) for k, v in ms.items()},
              "regions_ms": {k: [round(t, 4) for t in v] for k, v in times.items()},
              "ms_per_pass_in_call": round(ms["register_pairs"] / passes, 4),
              "pass_over_torch": round(ratio, 3),
              "verdict": "not slower than the torch pass" if ratio <= 1.0 else "SLOWER than the torch pass"})
