"""De-skewing against its byte floor and inside the engine: (a) epcnet_scan_deskew on 64 sweeps of 65 536 rows and 1000 poses, with and
without point_dt -- without it only the check and the per-scan launch run, so the difference is the row kernel -- against a
device-to-device copy measured in the same process (the row kernel moves 28 bytes per row: 12 in, 4 of point_dt, 12 out); (b)
InferenceEngine.forward_stamped against forward_trajectory on the same scans with the poses precomputed, whose difference is the whole
cost of the stamps stage.  HIP events around `--steps` calls, `--regions` regions, the arms alternating; the median region.  Everything
runs eagerly on one stream.  One JSON line, stamped with the SHA-256 of the loaded library.
Usage (GPU box): python scripts/time_deskew.py [--steps K] [--regions R] [--warmup W] [--out FILE]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import _timing  # noqa: E402
import bench  # noqa: E402
import downsample_ref as D  # noqa: E402
import helpers as H  # noqa: E402
import stamps_ref as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--regions", type=int, default=7)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--sweeps", type=int, default=64)
ap.add_argument("--rows", type=int, default=65536)
ap.add_argument("--poses", type=int, default=1000)
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("time_deskew.py measures on the device: no ROCm device is visible")
ops, L = bench.pkg("ops"), bench.pkg("lib")
dev = torch.device("cuda:0")
GAP = 0.5
SWEEP_NS = 100_000_000

# ---- the workload: sweeps 0.1 s apart at 10 m/s and 0.5 rad/s, odometry every 10 ms ------------------------------------------------------
pose_time_np, pose_np = R.odometry(5, args.poses, jitter_ns=200_000, wobble=0.005)
span = int(pose_time_np[-1] - pose_time_np[0]) - 2 * SWEEP_NS
scan_time_np = (pose_time_np[0] + SWEEP_NS // 2 + (np.arange(args.sweeps) * (span // args.sweeps))).astype(np.int64)
base = [D.scene(args.rows, 1000 + i) for i in range(min(args.sweeps, 8))]
points, offsets = ops.pack_scans([base[i % len(base)] for i in range(args.sweeps)], dev)
rows = int(points.shape[0])
rng = np.random.default_rng(7)
dt_np = np.sort(rng.integers(0, SWEEP_NS, size=(args.sweeps, rows // args.sweeps)), axis=1).reshape(-1).astype(np.int32)
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
scan_time, pose_time, pose, point_dt = up(scan_time_np), up(pose_time_np), up(pose_np), up(dt_np)
out = torch.empty_like(points)
scan_pose = torch.empty((args.sweeps, 12), dtype=torch.float64, device=dev)
status = torch.empty(args.sweeps, dtype=torch.int32, device=dev)
need = int(L.lib().epcnet_deskew_workspace_bytes(args.sweeps, args.poses, rows))
ws = torch.empty(need, dtype=torch.uint8, device=dev)
gap_ns = int(GAP * 1e9)
copy_src, copy_dst = torch.empty((rows, 7), dtype=torch.float32, device=dev), torch.empty((rows, 7), dtype=torch.float32, device=dev)
copy_src.normal_()


def deskew(dt):
    L.run.epcnet_scan_deskew(points, offsets, rows, args.sweeps, dt, scan_time, pose_time, pose, args.poses, gap_ns,
                             None if dt is None else out, scan_pose, status, ws, need)


deskew(point_dt)
torch.cuda.synchronize()
assert not bool(status.any()) and bool(torch.isfinite(out).all()), "the timed workload must be one without drop-outs"

# ---- (b): the engine, the poses precomputed for forward_trajectory ---------------------------------------------------------------------
arch = "epc-net-l"
eng, _ = H.make_engine(arch, H.O.seeded_weights(arch, 0), dev, in_flight=1)
sub = dict(length=20.0, spacing=10.0, max_submaps=8, out_rows=4 * rows)
moved, poses12, st = ops.deskew_scans(points, offsets, scan_time, pose_time, pose, point_dt=point_dt, max_gap=GAP)
along = ops.travel_along(poses12, st)
moved, poses12, along = moved.clone(), poses12.clone(), along.clone()
desc = torch.empty((8, 256), dtype=torch.float32, device=dev)
stamped = eng.forward_stamped(points, offsets, scan_time, pose_time, pose, point_dt=point_dt, max_gap=GAP, num_points=args.n, submaps=sub)
plain = eng.forward_trajectory(moved, offsets, poses12, along=along, num_points=args.n, submaps=sub)
torch.cuda.synchronize()
assert torch.equal(stamped[0].view(torch.int32), plain[0].view(torch.int32)), "forward_stamped is forward_trajectory behind the stamps stage"
submaps = int(stamped[3][0])

arms = {
    "deskew": lambda: deskew(point_dt),
    "poses_only": lambda: deskew(None),
    "copy_28B_per_row": lambda: copy_dst.copy_(copy_src),
    "forward_stamped": lambda: eng.forward_stamped(points, offsets, scan_time, pose_time, pose, point_dt=point_dt, max_gap=GAP,
                                                   num_points=args.n, submaps=sub, out=desc),
    "forward_trajectory": lambda: eng.forward_trajectory(moved, offsets, poses12, along=along, num_points=args.n, submaps=sub, out=desc),
}
times = {k: [t * 1e3 / args.steps for t in v]
         for k, v in _timing.alternate(arms, args.steps, args.regions, args.warmup, events=True).items()}
ms = {k: statistics.median(v) for k, v in times.items()}
row_ms = ms["deskew"] - ms["poses_only"]
copy_gb_s = 2 * 28 * rows / ms["copy_28B_per_row"] / 1e6           # a copy reads and writes its bytes
floor_ms = 28 * rows / copy_gb_s / 1e6
line = {"workload": "epcnet_scan_deskew on %d sweeps x %d rows, %d poses; forward_stamped and forward_trajectory (epc-net-l, %d points, "
                    "20 m every 10 m: %d submaps) on the same scans" % (args.sweeps, rows // args.sweeps, args.poses, args.n, submaps),
        "timer": "HIP events around %d calls; median of %d regions; eager, one stream" % (args.steps, args.regions),
        "ms_per_call": {k: round(v, 4) for k, v in ms.items()},
        "regions_ms": {k: [round(t, 4) for t in v] for k, v in times.items()},
        "row_kernel": {"rows": rows, "bytes_per_row": 28, "ms": round(row_ms, 4), "how": "deskew minus poses_only (the call without point_dt)",
                       "copy_gb_per_s": round(copy_gb_s, 1), "byte_floor_ms": round(floor_ms, 4), "over_floor": round(row_ms / floor_ms, 3),
                       "gb_per_s": round(28 * rows / row_ms / 1e6, 1)},
        "engine": {"forward_stamped_ms": round(ms["forward_stamped"], 4), "forward_trajectory_ms": round(ms["forward_trajectory"], 4),
                   "difference_ms": round(ms["forward_stamped"] - ms["forward_trajectory"], 4)}}
_timing.emit(line, args.out)
