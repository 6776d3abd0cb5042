"""The raw-scan front end against the extractor it feeds: ops.grid_downsample on 64 LiDAR-like scans of 32 768 points -> 4096 points each
(the seeded scene of tests/downsample_ref.py), and InferenceEngine.forward (EPC-Net, the default arithmetic) on the 64 results, in ONE
process.  The two arms alternate, `--regions` timed regions of `--steps` calls each, every region between device synchronisations; the
median region.  Also the kernel's registers / LDS / scratch as the compiler reports them (the Makefile's flags; skipped with
--no-resources).  One JSON line, stamped with the SHA-256 of the loaded library.
Usage (GPU box): python scripts/time_downsample.py [--steps K] [--regions R] [--warmup W] [--out FILE]"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import bench  # noqa: E402
import downsample_ref as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scans", type=int, default=64)
ap.add_argument("--points", type=int, default=32768)
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--regions", type=int, default=7)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--no-resources", action="store_true")
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
args = ap.parse_args()


def kernel_resources():
    """Registers, static LDS and scratch of grid_downsample_kernel from hipcc's resource remarks; the dynamic LDS from the launch's own
    formula (csrc/downsample.hip: table of T = pow2 >= 4n slots, then pairs + kept keys, counts and sums)."""
    csrc = os.path.join(ROOT, "epc-net_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=on", "-fno-slp-vectorize",
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "downsample.hip"), "-o", os.devnull]
    text = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    grab = lambda name: int(re.search(r"\b%s:\s*(\d+)" % re.escape(name), text).group(1))
    T = 4096
    while T < 4 * args.n:
        T *= 2
    return {"vgprs": grab("VGPRs"), "sgprs": grab("TotalSGPRs"), "scratch_bytes_per_lane": grab("ScratchSize [bytes/lane]"),
            "vgpr_spills": grab("VGPRs Spill"), "lds_static_bytes": grab("LDS Size [bytes/block]"),
            "lds_dynamic_bytes": max(8 * T, 4 * T + 20 * args.n), "threads": 1024}


ops, E = bench.pkg("ops"), bench.pkg("engine")
dev = torch.device("cuda:0")
scans = [R.scene(args.points, 1000 + i) for i in range(args.scans)]
points, offsets = ops.pack_scans(scans, dev)
eng = E.InferenceEngine("epc-net", bench.PARAMS, bench.build_store("epc-net", dev, 0), outer=bench.OUTER)
xyz, status, info = ops.grid_downsample(points, offsets, args.n)
out = torch.empty((args.scans, 256), dtype=torch.float32, device=dev)
arms = {"downsample": lambda: ops.grid_downsample(points, offsets, args.n, out=xyz),
        "forward": lambda: eng.forward(xyz, out=out)}
for fn in arms.values():
    for _ in range(args.warmup):
        fn()
torch.cuda.synchronize()
times = {k: [] for k in arms}
for _ in range(args.regions):
    for k, fn in arms.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        times[k].append(time.perf_counter() - t0)
ms = {k: statistics.median(v) / args.steps * 1e3 for k, v in times.items()}
info_h = info.cpu()
line = {"workload": "%d scenes x %d points -> %d (ops.grid_downsample), then InferenceEngine.forward (EPC-Net, f32) on the %d results"
                    % (args.scans, args.points, args.n, args.scans),
        "ms_per_batch": {k: round(v, 4) for k, v in ms.items()},
        "clouds_per_s": {k: round(args.scans / v * 1e3, 1) for k, v in ms.items()},
        "downsample_over_forward_time": round(ms["downsample"] / ms["forward"], 4),
        "status_nonzero": int((status != 0).sum()),
        "r_star_min_max": [int(info_h[:, 1].min()), int(info_h[:, 1].max())],
        "cells_over_n_max": round(float(info_h[:, 2].max()) / args.n, 4),
        "descriptors_finite": bool(torch.isfinite(out).all()),
        "regions_s": {k: [round(t, 5) for t in v] for k, v in times.items()},
        "steps_per_region": args.steps,
        "kernel": None if args.no_resources else kernel_resources(),
        "lib_sha256": bench.lib_sha256()}
text = json.dumps(line)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
