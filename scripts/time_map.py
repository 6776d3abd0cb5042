"""Map fusion against the same map written with torch: ops.fuse_map at voxel 0.2 m on the two outputs of scripts/time_submap.py -- 14
submaps of 8 scans of 32 768 rows (3.67 M rows) and 98 submaps of 40 scans of 2000 rows (7.84 M rows), each with its sub_pose -- and on ONE
streaming-sized submap of 40 scans of 2000 rows (80 000 rows; a drive of 41 scans), against a torch composition of the same map on the device in the same
process: the float64 transform, floor, torch.unique(keys, return_inverse=True, return_counts=True) and index_add_ (float64 sums: its
means differ from the entry's in the last bits and from run to run; its voxel set and counts are compared with the entry's before
anything is timed).  Arms: `fuse` (the wrapper's defaults: max_voxels = rows, its own workspace), `fuse_tight` (max_voxels = V rounded up
to a multiple of 4096, a caller's workspace) and `torch`.  The arms alternate, `--regions` timed regions of `--steps` calls each, every
region between device synchronisations; the median region.  Also the kernels' registers / LDS / scratch as the compiler reports them
(skipped with --no-resources).  One JSON line, stamped with the SHA-256 of the loaded library.
Usage (GPU box): python scripts/time_map.py [--steps K] [--regions R] [--warmup W] [--out FILE]"""
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
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--regions", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--voxel", type=float, default=0.2)
ap.add_argument("--no-resources", action="store_true")
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
args = ap.parse_args()

ops, L = bench.pkg("ops"), bench.pkg("lib")
dev = torch.device("cuda:0")


def torch_map(points, offsets, poses, origin, voxel):
    """The same map with torch on the device: (keys (V,), counts (V,), mean (V, 3) float64), the voxels in key order."""
    rows, C = points.shape[0], poses.shape[0]
    index = torch.arange(rows, device=points.device, dtype=torch.int32)
    cloud = torch.bucketize(index, offsets[1:], right=True).clamp(max=C - 1).long()
    inside = (index >= offsets[0]) & (index < offsets[-1])
    P = poses.reshape(C, 3, 4)[cloud]
    q = (P[:, :, :3] @ points.double().unsqueeze(-1)).squeeze(-1) + (P[:, :, 3] - origin)
    f = torch.floor(q / voxel)
    ok = inside & torch.isfinite(f).all(1) & (f.abs() < 2.0 ** 20).all(1)
    g = torch.where(ok[:, None], f, torch.zeros_like(f)).long() + (1 << 20)
    keys = torch.where(ok, (g[:, 2] << 42) | (g[:, 1] << 21) | g[:, 0], torch.full_like(g[:, 0], -1))
    uniq, inverse, counts = torch.unique(keys, return_inverse=True, return_counts=True)
    sums = torch.zeros((uniq.numel(), 3), dtype=torch.float64, device=points.device)
    q = torch.where(ok[:, None], q, torch.zeros_like(q))
    for a in range(3):
        sums[:, a].index_add_(0, inverse, q[:, a])
    return uniq, counts, sums / counts[:, None]


def drive(name, scans, rows, length, spacing):
    """One workload: time_submap.py's drive, built into submaps once; the map's inputs are its outputs."""
    base = [D.scene(rows, 1000 + i) for i in range(min(scans, 64))]
    points, offsets = ops.pack_scans([base[i % len(base)] for i in range(scans)], dev)
    poses, along = R.trajectory(3, scans, step=0.5, wobble=0.01, general=False)
    is_submap, lo, hi, ref = R.segment(along, length, spacing, scans)
    count = int(is_submap.sum())
    sub_offsets, _, _ = R.layout(offsets.cpu().numpy(), is_submap, lo, hi, 2 ** 31 - 1)
    total = int(sub_offsets[-1])
    res = ops.build_submaps(points, offsets, torch.from_numpy(poses).to(dev), along=torch.from_numpy(along).to(dev), length=length,
                            spacing=spacing, max_submaps=count, out_rows=total)
    assert res[5].tolist() == [count, 0] and int(res[1][-1]) == total
    w = dict(name=name, points=res[0], offsets=res[1], poses=res[3], rows=total, clouds=count)
    w["origin"] = w["poses"][0, 3::4].clone()
    out = ops.fuse_map(w["points"], w["offsets"], w["poses"], voxel=args.voxel, origin=w["origin"])
    w["num_out"] = out[2].tolist()
    V = w["num_out"][0]
    assert 0 < V <= total
    # the torch composition holds the same voxels with the same counts (one more key, -1, for the rows that are not kept)
    uniq, counts, mean = torch_map(w["points"], w["offsets"], w["poses"], w["origin"], args.voxel)
    kept = uniq >= 0
    w["torch_agrees"] = bool(int(kept.sum()) == V and int(counts[kept].sum()) == w["num_out"][1]
                             and torch.equal(torch.sort(counts[kept]).values, torch.sort(out[1][:V].long()).values))
    w["max_count"] = int(out[1].max())
    w["tight"] = (V + 4095) // 4096 * 4096
    w["ws"] = torch.empty(int(L.lib().epcnet_map_fuse_workspace_bytes(total, count, w["tight"])), dtype=torch.uint8, device=dev)
    w["ws_default_bytes"] = int(L.lib().epcnet_map_fuse_workspace_bytes(total, count, max(total, 1)))
    return w


loads = [drive("batch", 64, 32768, 4.0, 2.0), drive("long", 2000, 2000, 20.0, 10.0), drive("stream", 41, 2000, 20.0, 20.0)]
arms = {}
for w in loads:
    n = w["name"]
    arms["fuse_" + n] = lambda w=w: ops.fuse_map(w["points"], w["offsets"], w["poses"], voxel=args.voxel, origin=w["origin"])
    arms["fuse_tight_" + n] = lambda w=w: ops.fuse_map(w["points"], w["offsets"], w["poses"], voxel=args.voxel, origin=w["origin"],
                                                       max_voxels=w["tight"], workspace=w["ws"])
    arms["torch_" + n] = lambda w=w: torch_map(w["points"], w["offsets"], w["poses"], w["origin"], args.voxel)
times = _timing.alternate(arms, args.steps, args.regions, args.warmup)
ms = {k: statistics.median(v) / args.steps * 1e3 for k, v in times.items()}
line = {"workload": "ops.fuse_map at voxel %g m on the submaps of 64 scans x 32768 rows (4 m every 2 m), of 2000 scans x 2000 rows (20 m "
                    "every 10 m) and on one submap of 40 scans x 2000 rows, against the same map with torch (float64 transform, floor, "
                    "torch.unique, index_add_)" % args.voxel,
        "ms_per_call": {k: round(v, 4) for k, v in ms.items()},
        "steps_per_region": args.steps,
        "regions_s": {k: [round(t, 5) for t in v] for k, v in times.items()}}
for w in loads:
    n = w["name"]
    line[n] = {"rows": w["rows"], "clouds": w["clouds"], "num_out": w["num_out"], "max_count": w["max_count"], "torch_holds_the_same_voxels_and_counts": w["torch_agrees"],
               "max_voxels_tight": w["tight"], "workspace_bytes_default": w["ws_default_bytes"], "workspace_bytes_tight": int(w["ws"].numel()),
               "fuse_over_torch": round(ms["fuse_" + n] / ms["torch_" + n], 4),
               "fuse_tight_over_torch": round(ms["fuse_tight_" + n] / ms["torch_" + n], 4),
               "fuse_mrows_per_s": round(w["rows"] / ms["fuse_" + n] / 1e3, 1)}
line["kernels"] = None if args.no_resources else _timing.kernel_resources("map.hip", r"map_\w+_kernel")
_timing.emit(line, args.out)
