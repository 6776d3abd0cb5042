"""Submap building against its floor and against the stages behind it: ops.build_submaps on 64 posed scans of 32 768 rows with overlap 2
(length 4 m every 2 m at 0.5 m per scan: 14 submaps of 8 scans) and on ONE long trajectory of 2000 scans of 2000 rows (length 20 m every
10 m: 98 submaps of 40 scans), a device-to-device copy of as many bytes as the gather reads and writes (12 B in and 12 B out per output
row: the floor of such a kernel), and ops.remove_ground and ops.grid_downsample on the result -- what share of a forward_trajectory
batch in front of the network the new stage is -- in ONE process.  The arms alternate, `--regions` timed regions of `--steps` calls each,
every region between device synchronisations; the median region.  Also the kernels' registers / LDS / scratch as the compiler reports them
(the Makefile's flags; skipped with --no-resources).  One JSON line, stamped with the SHA-256 of the loaded library.
Usage (GPU box): python scripts/time_submap.py [--steps K] [--regions R] [--warmup W] [--out FILE]"""
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
import submap_ref as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--regions", type=int, default=7)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--no-resources", action="store_true")
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
args = ap.parse_args()


ops = bench.pkg("ops")
dev = torch.device("cuda:0")


def drive(name, scans, rows, length, spacing):
    """One workload: the packed scans, a seeded drive of 0.5 m per scan (small roll and pitch: z stays up), the exact capacities."""
    base = [D.scene(rows, 1000 + i) for i in range(min(scans, 64))]
    points, offsets = ops.pack_scans([base[i % len(base)] for i in range(scans)], dev)
    poses, along = R.trajectory(3, scans, step=0.5, wobble=0.01, general=False)
    is_submap, lo, hi, ref = R.segment(along, length, spacing, scans)
    count = int(is_submap.sum())
    sub_offsets, status, _ = R.layout(offsets.cpu().numpy(), is_submap, lo, hi, 2 ** 31 - 1)
    total = int(sub_offsets[-1])
    w = dict(name=name, points=points, offsets=offsets, poses=torch.from_numpy(poses).to(dev), along=torch.from_numpy(along).to(dev),
             kw=dict(length=length, spacing=spacing, max_submaps=count, out_rows=total), submaps=count, out_rows=total,
             scans_per_submap=int((hi - lo)[:count].max()))
    w["out"] = torch.empty((total, 3), dtype=torch.float32, device=dev)
    res = ops.build_submaps(points, offsets, w["poses"], along=w["along"], out=w["out"], **w["kw"])
    w["sub_offsets"], w["status"] = res[1], res[2]
    assert res[5].tolist() == [count, 0] and int(res[1][-1]) == total and not bool(res[2].any())
    # the floor: a copy of as many bytes as the gather moves (read 12 B, write 12 B per output row)
    w["copy_src"], w["copy_dst"] = torch.empty_like(w["out"]), torch.empty_like(w["out"])
    w["copy_src"].copy_(w["out"])
    w["kept"] = torch.empty_like(w["out"])
    g = ops.remove_ground(w["out"], w["sub_offsets"], out=w["kept"])
    w["ground_status_nonzero"] = int((g[1] != 0).sum())
    x = ops.grid_downsample(w["kept"], w["sub_offsets"], args.n)
    w["xyz"], w["downsample_status_nonzero"] = x[0], int((x[1] != 0).sum())
    return w


loads = [drive("batch", 64, 32768, 4.0, 2.0), drive("long", 2000, 2000, 20.0, 10.0)]
arms = {}
for w in loads:
    n = w["name"]
    arms["build_" + n] = lambda w=w: ops.build_submaps(w["points"], w["offsets"], w["poses"], along=w["along"], out=w["out"], **w["kw"])
    arms["copy_" + n] = lambda w=w: w["copy_dst"].copy_(w["copy_src"])
    arms["ground_" + n] = lambda w=w: ops.remove_ground(w["out"], w["sub_offsets"], out=w["kept"])
    arms["downsample_" + n] = lambda w=w: ops.grid_downsample(w["kept"], w["sub_offsets"], args.n, out=w["xyz"])
times = _timing.alternate(arms, args.steps, args.regions, args.warmup)
ms = {k: statistics.median(v) / args.steps * 1e3 for k, v in times.items()}
line = {"workload": "ops.build_submaps on 64 scans x 32768 rows (4 m every 2 m) and 2000 scans x 2000 rows (20 m every 10 m), a "
                    "device-to-device copy of the output's bytes, ops.remove_ground and ops.grid_downsample -> %d on the result" % args.n,
        "ms_per_call": {k: round(v, 4) for k, v in ms.items()},
        "steps_per_region": args.steps,
        "regions_s": {k: [round(t, 5) for t in v] for k, v in times.items()}}
for w in loads:
    n = w["name"]
    front = ms["build_" + n] + ms["ground_" + n] + ms["downsample_" + n]
    line[n] = {"submaps": w["submaps"], "scans_per_submap": w["scans_per_submap"], "out_rows": w["out_rows"],
               "bytes_moved": 24 * w["out_rows"],
               "build_gb_per_s": round(24 * w["out_rows"] / ms["build_" + n] / 1e6, 1),
               "copy_gb_per_s": round(24 * w["out_rows"] / ms["copy_" + n] / 1e6, 1),
               "build_over_copy": round(ms["build_" + n] / ms["copy_" + n], 3),
               "share_of_build_ground_downsample": round(ms["build_" + n] / front, 4),
               "ground_status_nonzero": w["ground_status_nonzero"], "downsample_status_nonzero": w["downsample_status_nonzero"]}
line["kernels"] = None if args.no_resources else _timing.kernel_resources("submap.hip", r"submap_\w+_kernel")
_timing.emit(line, args.out)
