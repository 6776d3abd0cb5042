"""Ground removal against the raw-scan path it precedes: ops.remove_ground on 64 LiDAR-like scans of 32 768 rows (the seeded scene of
tests/downsample_ref.py, the batch of scripts/time_downsample.py) and on ONE scan of 100 000 rows, ops.grid_downsample on the same 64
scans, and InferenceEngine.forward_scans (EPC-Net, the default arithmetic, 4096 points) with and without ``ground=True``, in ONE process.
The arms alternate, `--regions` timed regions of `--steps` calls each, every region between device synchronisations; the median region.
Also the kernels' registers / LDS / scratch as the compiler reports them (the Makefile's flags; skipped with --no-resources), and the
scorer's cost model: 9 non-fused lane operations per (row, hypothesis) against half the 157.3 TFLOP/s vector peak.  One JSON line,
stamped with the SHA-256 of the loaded library.
Usage (GPU box): python scripts/time_ground.py [--steps K] [--regions R] [--warmup W] [--out FILE]"""
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
ap.add_argument("--single", type=int, default=100000, help="rows of the one scan of the B = 1 arm")
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--hypotheses", type=int, default=256)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--regions", type=int, default=7)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--only", default=None, help="comma-separated arms (a profiler's run: ground_batch,ground_single)")
ap.add_argument("--no-resources", action="store_true")
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
args = ap.parse_args()


def kernel_resources():
    """Registers, LDS and scratch of the four kernels of csrc/ground.hip from hipcc's resource remarks."""
    out = _timing.kernel_resources("ground.hip", r"ground_\w+_kernel")
    for name, k in out.items():
        k["threads"] = 1024 if name == "ground_score_kernel" else 256
    return out


ops, E = bench.pkg("ops"), bench.pkg("engine")
dev = torch.device("cuda:0")
points, offsets = ops.pack_scans([R.scene(args.points, 1000 + i) for i in range(args.scans)], dev)
one, one_offsets = ops.pack_scans([R.scene(args.single, 999)], dev)
eng = E.InferenceEngine("epc-net", bench.PARAMS, bench.build_store("epc-net", dev, 0), outer=bench.OUTER)
kept, g_status, plane, g_info = ops.remove_ground(points, offsets, hypotheses=args.hypotheses)
one_kept, one_status, _, one_info = ops.remove_ground(one, one_offsets, hypotheses=args.hypotheses)
xyz, status, info = ops.grid_downsample(points, offsets, args.n)
out = torch.empty((args.scans, 256), dtype=torch.float32, device=dev)
ground = dict(hypotheses=args.hypotheses)
arms = {"ground_batch": lambda: ops.remove_ground(points, offsets, hypotheses=args.hypotheses, out=kept),
        "ground_single": lambda: ops.remove_ground(one, one_offsets, hypotheses=args.hypotheses, out=one_kept),
        "downsample": lambda: ops.grid_downsample(points, offsets, args.n, out=xyz),
        "downsample_after_ground": lambda: ops.grid_downsample(kept, offsets, args.n, out=xyz),
        "forward_scans": lambda: eng.forward_scans(points, offsets, num_points=args.n, out=out),
        "forward_scans_ground": lambda: eng.forward_scans(points, offsets, num_points=args.n, out=out, ground=ground)}
if args.only:
    arms = {k: arms[k] for k in args.only.split(",")}
times = _timing.alternate(arms, args.steps, args.regions, args.warmup)
ms = {k: statistics.median(v) / args.steps * 1e3 for k, v in times.items()}
pairs = float(args.scans) * args.points * args.hypotheses
model_ms = pairs * 9 / 78.6e12 * 1e3
g_info_h = g_info.cpu()
line = {"workload": "%d scenes x %d rows and 1 scene x %d rows (ops.remove_ground, %d hypotheses), ops.grid_downsample -> %d, "
                    "InferenceEngine.forward_scans (EPC-Net, f32) with and without ground=True"
                    % (args.scans, args.points, args.single, args.hypotheses, args.n),
        "ms_per_call": {k: round(v, 4) for k, v in ms.items()},
        "ground_adds_to_forward_scans_ms": round(ms["forward_scans_ground"] - ms["forward_scans"], 4) if "forward_scans" in ms and "forward_scans_ground" in ms else None,
        "scorer_model": {"row_hypothesis_pairs": pairs, "lane_ops_per_pair": 9, "lane_ops_per_s": 78.6e12, "floor_ms": round(model_ms, 4)},
        "ground_status_nonzero": int((g_status != 0).sum()) + int((one_status != 0).sum()),
        "removed_share_min_max": [round(float(x), 4) for x in ((g_info_h[:, 3].float() / g_info_h[:, 0].float()).min(),
                                                               (g_info_h[:, 3].float() / g_info_h[:, 0].float()).max())],
        "downsample_status_nonzero": int((status != 0).sum()),
        "descriptors_finite": bool(torch.isfinite(out).all()),
        "regions_s": {k: [round(t, 5) for t in v] for k, v in times.items()},
        "steps_per_region": args.steps,
        "kernels": None if args.no_resources else kernel_resources()}
_timing.emit(line, args.out)
