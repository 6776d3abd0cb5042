"""The map that grows against the only route there was: ops.SurfelMap.add of ONE streaming-sized submap (80 000 rows) into (a) an empty
map, (b) the map of the `batch` workload of scripts/time_surfels.py (3.67 M rows) and (c) the map of its `long` workload (7.84 M rows),
all three at the same max_voxels, against ops.fuse_surfels over ALL rows so far -- the same seven outputs, which the script compares bit
for bit before anything is timed.  At (a) the other arm is ops.fuse_surfels of that one submap at the same max_voxels: the one-shot entry
pays the table's clear on every call.  Besides init (SurfelMap.reset), the one call that scales with max_voxels.

Adding the same rows twice would change the map's fill, so THE STATE IS RESTORED before every timed add: the state's bytes are copied back
from a snapshot taken behind the base map (a device copy of the whole table: what it leaves in the caches is its tail, so the add finds
the table as cold as a table of that size is), and a pair of device events around the add alone is the clock -- for every arm, the
restore outside the pair.  The arms alternate, `--regions` regions of `--steps` timed calls each; the median region.  Also the kernels'
registers / LDS / scratch as the compiler reports them (skipped with --no-resources).  One JSON line, stamped with the SHA-256 of the
loaded library.
Usage (GPU box): python scripts/time_growmap.py [--steps K] [--regions R] [--warmup W] [--out FILE] [--only NAME]"""
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
import downsample_ref as D  # noqa: E402
import submap_ref as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--regions", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--voxel", type=float, default=0.2)
ap.add_argument("--max-voxels", type=int, default=1 << 22)
ap.add_argument("--only", default=None, help="one base map (empty, batch, long) and its add arm alone, no comparison: for a profiler")
ap.add_argument("--no-resources", action="store_true")
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
args = ap.parse_args()

ops, L = bench.pkg("ops"), bench.pkg("lib")
dev = torch.device("cuda:0")
NAMES = ("map_points", "count", "centroid", "normal", "eigen", "support", "num_out")


def drive(name, scans, rows, length, spacing):
    """One workload of scripts/time_surfels.py: time_submap.py's drive, built into submaps once."""
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
    return dict(name=name, points=res[0], offsets=res[1], poses=res[3], rows=total, clouds=count)


def timed(arms, steps, regions, warmup):
    """{arm: [seconds per region]}: every arm is (prepare, call); a pair of device events around ``call`` alone, ``prepare`` in front of
    the pair; the arms alternate."""
    for prepare, call in arms.values():
        for _ in range(warmup):
            prepare()
            call()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(regions):
        for k, (prepare, call) in arms.items():
            total = 0.0
            for _ in range(steps):
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                prepare()
                torch.cuda.synchronize()
                start.record()
                call()
                end.record()
                end.synchronize()
                total += start.elapsed_time(end) * 1e-3
            times[k].append(total)
    return times


shapes = {"batch": (64, 32768, 4.0, 2.0), "long": (2000, 2000, 20.0, 10.0)}
stream = drive("stream", 41, 2000, 20.0, 20.0)
origin = stream["poses"][0, 3::4].clone()
kw = dict(voxel=args.voxel, origin=origin, max_voxels=args.max_voxels)
add_ws = torch.empty(L.lib().epcnet_surfel_map_add_workspace_bytes(stream["rows"], stream["clouds"], 1), dtype=torch.uint8, device=dev)
arms, facts = {}, {}
nothing = lambda: None
for base in ("empty", "batch", "long"):
    if args.only not in (None, base):
        continue
    m = ops.SurfelMap(**kw)
    w = None if base == "empty" else drive(base, *shapes[base])
    if w is not None:
        # the base map's poses are taken as they are against the stream submap's origin: both drives start within metres of each other
        m.add(w["points"], w["offsets"], w["poses"])
    before = m.num_out.tolist()
    snapshot = m.state.clone()
    restore = lambda m=m, snapshot=snapshot: m.state.copy_(snapshot)
    add = lambda m=m: m.add(stream["points"], stream["offsets"], stream["poses"], workspace=add_ws)
    arms["add_" + base] = (restore, add)
    facts[base] = {"rows_before": 0 if w is None else w["rows"], "num_out_before": before}
    if args.only:
        continue
    if w is None:
        every = (stream["points"], stream["offsets"], stream["poses"])
    else:
        every = (torch.cat([w["points"], stream["points"]]), torch.cat([w["offsets"], stream["offsets"][1:] + w["offsets"][-1]]),
                 torch.cat([w["poses"], stream["poses"]]))
    ws = torch.empty(L.lib().epcnet_map_surfels_workspace_bytes(int(every[0].shape[0]), int(every[2].shape[0]), args.max_voxels),
                     dtype=torch.uint8, device=dev)
    one_shot = lambda every=every, ws=ws: ops.fuse_surfels(*every, workspace=ws, **kw)
    arms["fuse_surfels_all_rows_" + base] = (nothing, one_shot)
    num_call = add().tolist()
    want = one_shot()
    facts[base].update(num_call=num_call, num_out_after=m.num_out.tolist(), rows_all=int(every[0].shape[0]),
                       add_equals_fuse_surfels_of_all_rows=all(torch.equal(getattr(m, n).view(torch.int32), t.view(torch.int32))
                                                               for n, t in zip(NAMES, want[:7])))
    assert facts[base]["add_equals_fuse_surfels_of_all_rows"] and facts[base]["num_out_after"][0] > 0, facts[base]
    restore()
    del want
    if base == "empty":
        arms["init"] = (nothing, m.reset)
times = timed(arms, args.steps, args.regions, args.warmup)
ms = {k: statistics.median(v) / args.steps * 1e3 for k, v in times.items()}
line = {"workload": "ops.SurfelMap.add of one submap of 40 scans x 2000 rows (%d rows) at voxel %g m, ring 1, min_support 8, max_voxels %d, into an "
                    "empty map, the map of 64 scans x 32768 rows (4 m every 2 m) and the map of 2000 scans x 2000 rows (20 m every 10 m), "
                    "against ops.fuse_surfels over all rows so far at the same max_voxels" % (stream["rows"], args.voxel, args.max_voxels),
        "clock": "a pair of device events around every call; before every add the state is copied back from a snapshot, outside the pair",
        "ms_per_call": {k: round(v, 4) for k, v in ms.items()},
        "steps_per_region": args.steps,
        "regions_s": {k: [round(t, 6) for t in v] for k, v in times.items()}}
line.update(facts)
if not args.only:
    for base in ("empty", "batch", "long"):
        line[base]["add_over_fuse_surfels_of_all_rows"] = round(ms["add_" + base] / ms["fuse_surfels_all_rows_" + base], 4)
    line["add_batch_over_add_empty"] = round(ms["add_batch"] / ms["add_empty"], 4)
    line["add_long_over_add_empty"] = round(ms["add_long"] / ms["add_empty"], 4)
line["kernels"] = None if args.no_resources else _timing.kernel_resources("growmap.hip", r"growmap_\w+_kernel")
_timing.emit(line, args.out)
