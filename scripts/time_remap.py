"""A loop closure applied to the map that grows: ops.SurfelMap.repose against the only route there was, a rebuild.  The maps are those of
scripts/time_growmap.py -- the `batch` workload (3.67 M rows) and the `long` one (7.84 M rows) with one streaming-sized submap (80 000
rows) added, at the same max_voxels -- and the closure is a correction of 0.3 m and one degree of yaw.
  (a) repose of THE ONE 80 000-row submap inside each map, against ops.fuse_surfels over all rows at the corrected poses and against
      reset() plus add of all rows;
  (b) repose of the first 1/8, 1/4, 1/2 and all of the map's clouds, against the same rebuild: the fraction of moved rows at which the
      rebuild becomes cheaper is interpolated between the measured fractions;
  (c) add of the same 80 000 rows into the map without them, for scale.
Before anything is timed every repose is checked against ops.fuse_surfels at the corrected poses: the row counts, the number of voxels
that hold rows and a sorted 64-bit digest of their six output rows (the numbers differ, the cells' contents do not).

THE STATE IS RESTORED before every timed repose or add, as time_growmap.py does it: the state's bytes are copied back from a snapshot,
outside the pair of device events that is the clock (for the timed calls the arrays are not restored: which rows a call writes follows
from the state and the rows; for the comparisons they are).  The arms alternate, `--regions` regions of `--steps` timed calls each; the
median region, and the spread between regions.  max_voxels is 2^24, four times time_growmap.py's: the voxels a repose empties keep their
slots, so a map whose every row moves needs room for twice its voxels (and the one-shot rebuild clears a table of that size).  One JSON
line, stamped with the SHA-256 of the loaded library.
Usage (GPU box): python scripts/time_remap.py [--steps K] [--regions R] [--warmup W] [--out FILE] [--only batch|long]"""
import argparse
import math
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
ap.add_argument("--max-voxels", type=int, default=1 << 24)
ap.add_argument("--only", default=None, help="one base map (batch, long)")
ap.add_argument("--no-resources", action="store_true")
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
args = ap.parse_args()

ops, L = bench.pkg("ops"), bench.pkg("lib")
dev = torch.device("cuda:0")
NAMES = ("map_points", "count", "centroid", "normal", "eigen", "support", "num_out")
FRACTIONS = (0.125, 0.25, 0.5, 1.0)


def drive(name, scans, rows, length, spacing):
    """One workload of scripts/time_surfels.py: time_submap.py's drive, built into submaps once (as scripts/time_growmap.py does)."""
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


def corrected(poses):
    """What a closure makes of ``poses`` (C, 12): one degree of yaw about the world's z in front, 0.3 m on the translation."""
    a = math.radians(1.0)
    turn = torch.tensor([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64, device=dev)
    out = poses.reshape(-1, 3, 4).clone()
    out[:, :, :3] = turn @ out[:, :, :3]
    out[:, :, 3] += torch.tensor([0.2, -0.2, 0.1], dtype=torch.float64, device=dev)
    return out.reshape(-1, 12).contiguous()


def digest(arrays):
    """The voxels that hold rows -> (how many, their 64-bit digests sorted): the six output rows' words under odd multipliers."""
    count = arrays[1]
    words = torch.cat([t.view(torch.int32).reshape(len(count), -1) for t in arrays[:6]], 1)[count > 0].to(torch.int64)
    mult = torch.arange(words.shape[1], device=dev, dtype=torch.int64) * 0x9E3779B1 + 0x85EBCA6B
    h = (words * mult).sum(1)
    h = (h ^ (h >> 29)) * 0x165667B19E3779F9
    return int(words.shape[0]), torch.sort(h).values


def timed(arms, steps, regions, warmup):
    """{arm: [seconds per region]}: every arm is (prepare, call); a pair of device events around ``call`` alone, ``prepare`` in front of
    the pair; the arms alternate (the clock of scripts/time_growmap.py)."""
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
stream_new = corrected(stream["poses"])
nothing = lambda: None
line = {"workload": "ops.SurfelMap.repose at voxel %g m, ring 1, min_support 8, max_voxels %d, in the map of 64 scans x 32768 rows (4 m every "
                    "2 m) and in the map of 2000 scans x 2000 rows (20 m every 10 m), each with one submap of 40 scans x 2000 rows (%d rows) "
                    "added; the correction is one degree of yaw and 0.3 m" % (args.voxel, args.max_voxels, stream["rows"]),
        "clock": "a pair of device events around every call; before every repose or add the state is copied back from a snapshot, outside the pair",
        "steps_per_region": args.steps}
for base in ("batch", "long"):
    if args.only not in (None, base):
        continue
    w = drive(base, *shapes[base])
    every = (torch.cat([w["points"], stream["points"]]), torch.cat([w["offsets"], stream["offsets"][1:] + w["offsets"][-1]]),
             torch.cat([w["poses"], stream["poses"]]))
    rows_all, clouds_all = int(every[0].shape[0]), int(every[2].shape[0])
    m = ops.SurfelMap(**kw)
    m.add(w["points"], w["offsets"], w["poses"])
    without = m.state.clone()                            # the map without the submap: arm (c)
    m.add(stream["points"], stream["offsets"], stream["poses"])
    snapshot, before = m.state.clone(), m.num_out.tolist()
    restore = lambda m=m, snapshot=snapshot: m.state.copy_(snapshot)
    arrays = [getattr(m, n).clone() for n in NAMES]

    def restore_all(m=m, arrays=arrays):                 # for the comparisons: the arrays too are what they were behind the adds
        restore()
        for n, a in zip(NAMES, arrays):
            getattr(m, n).copy_(a)

    fuse_ws = torch.empty(L.lib().epcnet_map_surfels_workspace_bytes(rows_all, clouds_all, args.max_voxels), dtype=torch.uint8, device=dev)
    move_ws = torch.empty(L.lib().epcnet_surfel_map_move_workspace_bytes(rows_all, clouds_all, 1), dtype=torch.uint8, device=dev)
    add_ws = torch.empty(L.lib().epcnet_surfel_map_add_workspace_bytes(rows_all, clouds_all, 1), dtype=torch.uint8, device=dev)
    facts = {"rows": rows_all, "clouds": clouds_all, "num_out_before": before}
    arms = {}
    # (a) the one submap
    one_new = torch.cat([w["poses"], stream_new])
    repose_one = lambda m=m: m.repose(stream["points"], stream["offsets"], stream["poses"], stream_new, workspace=move_ws)
    fuse_one = lambda every=every, one_new=one_new, ws=fuse_ws: ops.fuse_surfels(every[0], every[1], one_new, workspace=ws, **kw)

    def rebuild_one(m=m, every=every, one_new=one_new, ws=add_ws):
        m.reset()
        return m.add(every[0], every[1], one_new, workspace=ws)

    restore_all()
    call = repose_one().tolist()
    want = fuse_one()
    (n_mine, h_mine), (n_theirs, h_theirs) = digest([getattr(m, n) for n in NAMES]), digest(want)
    facts["one_submap"] = {"rows_moved": stream["rows"], "num_call": call, "num_out_after": m.num_out.tolist(), "voxels_with_rows": n_mine,
                           "equals_fuse_surfels_by_cell": n_mine == n_theirs == int(want[6][0]) and bool(torch.equal(h_mine, h_theirs))
                           and m.num_out.tolist()[1:] == want[6].tolist()[1:]}
    assert facts["one_submap"]["equals_fuse_surfels_by_cell"] and call[0] > 0 and call[3] == 0, facts
    del want
    arms["repose_one_submap"] = (restore, repose_one)
    arms["fuse_surfels_all_rows"] = (nothing, fuse_one)
    arms["reset_and_add_all_rows"] = (nothing, rebuild_one)
    arms["add_one_submap"] = (lambda m=m, without=without: m.state.copy_(without),
                              lambda m=m: m.add(stream["points"], stream["offsets"], stream["poses"],
                                                workspace=add_ws))
    # (b) a growing share of the map's clouds, the first ones of the drive
    all_new = corrected(every[2])
    for fraction in FRACTIONS:
        k = max(1, int(round(fraction * clouds_all)))
        end = int(every[1][k])
        part = (every[0][:end], every[1][:k + 1].contiguous(), every[2][:k].contiguous(), all_new[:k].contiguous())
        repose_part = lambda m=m, part=part: m.repose(*part, workspace=move_ws)
        restore_all()
        call = repose_part().tolist()
        want = ops.fuse_surfels(every[0], every[1], torch.cat([all_new[:k], every[2][k:]]), workspace=fuse_ws, **kw)
        (n_mine, h_mine), (n_theirs, h_theirs) = digest([getattr(m, n) for n in NAMES]), digest(want)
        ok = n_mine == n_theirs == int(want[6][0]) and bool(torch.equal(h_mine, h_theirs)) and m.num_out.tolist()[1:] == want[6].tolist()[1:]
        facts["share_%g" % fraction] = {"clouds_moved": k, "rows_moved": end, "share_of_rows": round(end / rows_all, 4), "num_call": call,
                                        "num_out_after": m.num_out.tolist(), "equals_fuse_surfels_by_cell": ok}
        assert ok and call[3] == 0, facts
        del want
        arms["repose_share_%g" % fraction] = (restore, repose_part)
    times = timed(arms, args.steps, args.regions, args.warmup)
    ms = {k: statistics.median(v) / args.steps * 1e3 for k, v in times.items()}
    spread = {k: (max(v) - min(v)) / args.steps * 1e3 for k, v in times.items()}
    rebuild = min(ms["fuse_surfels_all_rows"], ms["reset_and_add_all_rows"])
    facts["ms_per_call"] = {k: round(v, 4) for k, v in ms.items()}
    facts["spread_between_regions_ms"] = {k: round(v, 4) for k, v in spread.items()}
    facts["regions_s"] = {k: [round(t, 6) for t in v] for k, v in times.items()}
    facts["repose_one_over_cheaper_rebuild"] = round(ms["repose_one_submap"] / rebuild, 4)
    facts["repose_one_over_add_one"] = round(ms["repose_one_submap"] / ms["add_one_submap"], 4)
    facts["rebuild_minus_repose_one_ms"] = round(rebuild - ms["repose_one_submap"], 4)
    facts["repose_one_beats_rebuild_by_more_than_the_spread"] = bool(
        rebuild - ms["repose_one_submap"] > max(spread["repose_one_submap"], spread["fuse_surfels_all_rows"], spread["reset_and_add_all_rows"]))
    # where the rebuild becomes cheaper: between the measured shares, linearly in the share of rows
    pts = [(stream["rows"] / rows_all, ms["repose_one_submap"])] + [(facts["share_%g" % f]["share_of_rows"], ms["repose_share_%g" % f]) for f in FRACTIONS]
    cross = None
    for (x0, y0), (x1, y1) in zip(pts[:-1], pts[1:]):
        if y0 <= rebuild < y1:
            cross = x0 + (rebuild - y0) * (x1 - x0) / (y1 - y0)
    facts["share_of_rows_at_which_a_rebuild_is_cheaper"] = None if cross is None else round(cross, 3)
    facts["repose_of_all_rows_over_cheaper_rebuild"] = round(ms["repose_share_1"] / rebuild, 4)
    line[base] = facts
    del m, snapshot, without, every, w, fuse_ws, move_ws, add_ws, arrays
    torch.cuda.empty_cache()
line["kernels"] = None if args.no_resources else _timing.kernel_resources("growmap.hip", r"growmap_\w+_kernel")
_timing.emit(line, args.out)
