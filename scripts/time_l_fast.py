"""EPC-Net-L at 256 x 4096 synthetic clouds: clouds/s of the two arithmetics (EPC_PRECISION_F32, EPC_PRECISION_FAST) in ONE process,
each as InferenceEngine.forward runs it by default (f32: two 128-cloud halves in flight; fast: one 256-cloud pass), plus the fast arithmetic
as two halves in flight (the f32 default's form: whether it pays in fast).  The arms alternate, `--regions` timed regions of `--steps` calls each, every region between
device synchronisations; the median region.  One JSON line, stamped with the SHA-256 of the loaded library.
Usage (GPU box): python scripts/time_l_fast.py [--steps K] [--regions R] [--warmup W]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--regions", type=int, default=7)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--in-flight", type=int, default=None, help="lanes of the f32 and fast arms (default: the engine's own default)")
args = ap.parse_args()

E = bench.pkg("engine")
dev = torch.device("cuda:0")
store = bench.build_store("epc-net-l", dev, 0)
arms = {"f32": E.InferenceEngine("epc-net-l", bench.PARAMS, store, outer=bench.OUTER, precision="f32", in_flight=args.in_flight),
        "fast": E.InferenceEngine("epc-net-l", bench.PARAMS, store, outer=bench.OUTER, precision="fast", in_flight=args.in_flight),
        "fast_two_lanes": E.InferenceEngine("epc-net-l", bench.PARAMS, store, outer=bench.OUTER, precision="fast", in_flight=2)}
g = torch.Generator().manual_seed(100)
xyz = (torch.rand((256, bench.N_POINTS, 3), generator=g) * 2.0 - 1.0).to(dev)
outs = {k: torch.empty((256, 256), dtype=torch.float32, device=dev) for k in arms}
for k, eng in arms.items():
    for _ in range(args.warmup):
        eng.forward(xyz, out=outs[k])
torch.cuda.synchronize()
times = {k: [] for k in arms}
for _ in range(args.regions):
    for k, eng in arms.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            eng.forward(xyz, out=outs[k])
        torch.cuda.synchronize()
        times[k].append(time.perf_counter() - t0)
rate = {k: 256 * args.steps / statistics.median(v) for k, v in times.items()}
line = {"workload": "EPC-Net-L inference, 256 x %d x 3 synthetic clouds, InferenceEngine.forward" % bench.N_POINTS,
        "clouds_per_s": {k: round(v, 1) for k, v in rate.items()},
        "ms_per_batch": {k: round(statistics.median(v) / args.steps * 1e3, 4) for k, v in times.items()},
        "fast_over_f32": round(rate["fast"] / rate["f32"], 4),
        "fast_two_lanes_over_default": round(rate["fast_two_lanes"] / rate["fast"], 4),
        "in_flight": {k: e.in_flight for k, e in arms.items()},
        "fast_same_bits_on_two_lanes": bool(torch.equal(outs["fast"], outs["fast_two_lanes"])),
        "fast_vs_f32_descriptor_l2_max": float((outs["fast"] - outs["f32"]).norm(dim=1).max()),
        "regions_s": {k: [round(t, 5) for t in v] for k, v in times.items()},
        "steps_per_region": args.steps,
        "lib_sha256": bench.lib_sha256()}
print(json.dumps(line))
