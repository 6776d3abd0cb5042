"""The raw-scan front end against the extractor it feeds: ops.grid_downsample on 64 LiDAR-like scans of 32 768 points -> 4096 points each
(the seeded scene of tests/downsample_ref.py), and InferenceEngine.forward (EPC-Net, the default arithmetic) on the 64 results, in ONE
process.  The two arms alternate, `--regions` timed regions of `--steps` calls each, every region between device synchronisations; the
median region.  Also the kernel's registers / LDS / scratch as the compiler reports them (the Makefile's flags; skipped with
--no-resources).  One JSON line, stamped with the SHA-256 of the loaded library.
Usage (GPU box): python scripts/time_downsample.py [--steps K] [--regions R] [--warmup W] [--out FILE]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import _timing  # noqa: E402
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
    k = _timing.kernel_resources("downsample.hip", r"grid_downsample_kernel")["grid_downsample_kernel"]
    T = 4096
    while T < 4 * args.n:
        T *= 2
    return {"vgprs": k["vgprs"], "sgprs": k["sgprs"], "scratch_bytes_per_lane": k["scratch_bytes_per_lane"], "vgpr_spills": k["vgpr_spills"],
            "lds_static_bytes": k["lds_bytes"], "lds_dynamic_bytes": max(8 * T, 4 * T + 20 * args.n), "threads": 1024}


ops, E = bench.pkg("ops"), bench.pkg("engine")
dev = torch.device("cuda:0")
scans = [R.scene(args.points, 1000 + i) for i in range(args.scans)]
points, offsets = ops.pack_scans(scans, dev)
eng = E.InferenceEngine("epc-net", bench.PARAMS, bench.build_store("epc-net", dev, 0), outer=bench.OUTER)
xyz, status, info = ops.grid_downsample(points, offsets, args.n)
out = torch.empty((args.scans, 256), dtype=torch.float32, device=dev)
arms = {"downsample": lambda: ops.grid_downsample(points, offsets, args.n, out=xyz),
        "forward": lambda: eng.forward(xyz, out=out)}
times = _timing.alternate(arms, args.steps, args.regions, args.warmup)
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
        "kernel": None if args.no_resources else kernel_resources()}
_timing.emit(line, args.out)
