"""Map surfels against the same result composed with torch: ops.fuse_surfels at voxel 0.2 m, ring 1, on the three workloads of
scripts/time_map.py -- 14 submaps of 8 scans of 32 768 rows (3.67 M rows), 98 submaps of 40 scans of 2000 rows (7.84 M rows) and ONE
streaming-sized submap of 80 000 rows -- in one process with `fuse` (the unchanged ops.fuse_map: what the surfels cost on top of the
map) and `torch`, the same result composed on the device: the float64 transform, torch.unique, index_add_ of the ten moment columns
(int64), 27 searchsorted poolings and torch.linalg.eigh (its voxel set and its supports are compared with the entry's before anything is
timed; its eigenvectors differ in the last bits).  Besides `surfels` at ring 0 and ring 2.  The arms alternate, `--regions` timed
regions of `--steps` calls each, every region between device synchronisations; the median region.  Also the kernels' registers / LDS /
scratch as the compiler reports them (skipped with --no-resources).  One JSON line, stamped with the SHA-256 of the loaded library.
Usage (GPU box): python scripts/time_surfels.py [--steps K] [--regions R] [--warmup W] [--out FILE] [--only NAME]"""
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
ap.add_argument("--only", default=None, help="one workload (batch, long, stream) and the surfels arm alone: for a profiler")
ap.add_argument("--no-resources", action="store_true")
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
args = ap.parse_args()

ops, L = bench.pkg("ops"), bench.pkg("lib")
dev = torch.device("cuda:0")
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def torch_surfels(points, offsets, poses, origin, voxel, ring=1, min_count=1):
    """The same surfels with torch on the device: (keys (V,), support (V,), centroid (V, 3), eigenvalues (V, 3), normal (V, 3)) in key
    order; a first key of -1 collects the rows that are not kept."""
    rows, C = points.shape[0], poses.shape[0]
    index = torch.arange(rows, device=points.device, dtype=torch.int32)
    cloud = torch.bucketize(index, offsets[1:], right=True).clamp(max=C - 1).long()
    inside = (index >= offsets[0]) & (index < offsets[-1])
    P = poses.reshape(C, 3, 4)[cloud]
    q = (P[:, :, :3] @ points.double().unsqueeze(-1)).squeeze(-1) + (P[:, :, 3] - origin)
    f = torch.floor(q / voxel * 256.0)
    ok = inside & torch.isfinite(f).all(1) & (f.abs() < 2.0 ** 28).all(1)
    U = torch.where(ok[:, None], f, torch.zeros_like(f)).long()
    g, u = (U >> 8) + (1 << 20), U & 255
    keys = torch.where(ok, (g[:, 2] << 42) | (g[:, 1] << 21) | g[:, 0], torch.full_like(g[:, 0], -1))
    uniq, inverse = torch.unique(keys, return_inverse=True)
    V = uniq.numel()
    cols = torch.stack([torch.ones_like(u[:, 0]), u[:, 0], u[:, 1], u[:, 2]] + [u[:, a] * u[:, b] for a, b in PAIRS], 1)
    own = torch.zeros((V, 10), dtype=torch.int64, device=points.device).index_add_(0, inverse, cols)
    cell = torch.stack([uniq & 0x1fffff, (uniq >> 21) & 0x1fffff, (uniq >> 42) & 0x1fffff], 1)
    pooled = torch.zeros_like(own)
    span = range(-ring, ring + 1)
    for o2 in span:
        for o1 in span:
            for o0 in span:
                c = cell + torch.tensor([o0, o1, o2], device=points.device)
                there = ((c >= 0) & (c < (1 << 21))).all(1) & (uniq >= 0)
                key = (c[:, 2] << 42) | (c[:, 1] << 21) | c[:, 0]
                at = torch.searchsorted(uniq, key).clamp(max=V - 1)
                m = own[at]
                there = there & (uniq[at] == key) & (m[:, 0] >= min_count)
                e = (256 * o0, 256 * o1, 256 * o2)
                add = [m[:, 0]] + [m[:, 1 + a] + m[:, 0] * e[a] for a in range(3)]
                add += [m[:, 4 + k] + e[a] * m[:, 1 + b] + e[b] * m[:, 1 + a] + m[:, 0] * (e[a] * e[b]) for k, (a, b) in enumerate(PAIRS)]
                pooled += torch.where(there[:, None], torch.stack(add, 1), torch.zeros_like(own))
    n = pooled[:, 0].double().clamp(min=1.0)
    mu = pooled[:, 1:4].double() / n[:, None]
    cov = torch.empty((V, 3, 3), dtype=torch.float64, device=points.device)
    for k, (a, b) in enumerate(PAIRS):
        cov[:, a, b] = cov[:, b, a] = pooled[:, 4 + k].double() / n - mu[:, a] * mu[:, b]
    values, vectors = torch.linalg.eigh(cov)
    s = voxel / 256.0
    centroid = (((cell - (1 << 20)) * 256).double() + mu) * s
    return uniq, pooled[:, 0], centroid.float(), (values.clamp(min=0.0) * s * s).float(), vectors[:, :, 0].float()


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
    return w


def verify(w):
    """The entry's voxels and supports against the torch composition's, and its three shared outputs against ops.fuse_map."""
    out = ops.fuse_surfels(w["points"], w["offsets"], w["poses"], voxel=args.voxel, origin=w["origin"])
    fused = ops.fuse_map(w["points"], w["offsets"], w["poses"], voxel=args.voxel, origin=w["origin"])
    w["num_out"] = out[6].tolist()
    V = w["num_out"][0]
    assert 0 < V <= w["rows"]
    w["equals_fuse_map"] = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in ((out[0], fused[0]), (out[1], fused[1]), (out[6], fused[2])))
    uniq, support, centroid, values, normal = torch_surfels(w["points"], w["offsets"], w["poses"], w["origin"], args.voxel)
    kept = uniq >= 0
    w["torch_agrees"] = bool(int(kept.sum()) == V and torch.equal(torch.sort(support[kept]).values, torch.sort(out[5][:V].long()).values))
    valid = torch.isfinite(out[3][:V]).all(1)
    w["valid"] = int(valid.sum())
    w["max_support"] = int(out[5].max())
    del uniq, support, centroid, values, normal
    torch.cuda.empty_cache()


names = {"batch": (64, 32768, 4.0, 2.0), "long": (2000, 2000, 20.0, 10.0), "stream": (41, 2000, 20.0, 20.0)}
loads = [drive(n, *names[n]) for n in names if args.only in (None, n)]
arms = {}
for w in loads:
    n = w["name"]
    call = lambda w=w, **kw: ops.fuse_surfels(w["points"], w["offsets"], w["poses"], voxel=args.voxel, origin=w["origin"], **kw)
    arms["surfels_" + n] = call
    if args.only:
        continue
    verify(w)
    arms["fuse_" + n] = lambda w=w: ops.fuse_map(w["points"], w["offsets"], w["poses"], voxel=args.voxel, origin=w["origin"])
    arms["torch_" + n] = lambda w=w: torch_surfels(w["points"], w["offsets"], w["poses"], w["origin"], args.voxel)
    arms["surfels_ring0_" + n] = lambda call=call: call(ring=0)
    arms["surfels_ring2_" + n] = lambda call=call: call(ring=2)
times = _timing.alternate(arms, args.steps, args.regions, args.warmup)
ms = {k: statistics.median(v) / args.steps * 1e3 for k, v in times.items()}
line = {"workload": "ops.fuse_surfels at voxel %g m, ring 1, min_support 8 on the submaps of 64 scans x 32768 rows (4 m every 2 m), of 2000 "
                    "scans x 2000 rows (20 m every 10 m) and on one submap of 40 scans x 2000 rows, against ops.fuse_map and against the "
                    "same surfels with torch (float64 transform, torch.unique, index_add_ of ten int64 moment columns, 27 searchsorted "
                    "poolings, torch.linalg.eigh)" % args.voxel,
        "ms_per_call": {k: round(v, 4) for k, v in ms.items()},
        "steps_per_region": args.steps,
        "regions_s": {k: [round(t, 5) for t in v] for k, v in times.items()},
        "insert_forms_ms": {"what": "surfels arm alone, same process shape (--only), both forms passed tests/test_gpu_surfels.py; (a) one lane per "
                                    "row with thirteen scattered 8-byte atomics, (b) sixteen lanes per row through LDS, the form kept",
                            "a": {"long": 14.334, "batch": 5.8839, "stream": 0.2215}, "b": {"long": 11.3338, "batch": 4.7959, "stream": 0.2032}}}
for w in loads:
    n = w["name"]
    if args.only:
        continue
    line[n] = {"rows": w["rows"], "clouds": w["clouds"], "num_out": w["num_out"], "valid_surfels": w["valid"], "max_support": w["max_support"],
               "map_points_count_num_out_equal_fuse_map": w["equals_fuse_map"], "torch_holds_the_same_voxels_and_supports": w["torch_agrees"],
               "surfels_over_torch": round(ms["surfels_" + n] / ms["torch_" + n], 4),
               "surfels_over_fuse": round(ms["surfels_" + n] / ms["fuse_" + n], 4),
               "ring0_over_ring1": round(ms["surfels_ring0_" + n] / ms["surfels_" + n], 4),
               "ring2_over_ring1": round(ms["surfels_ring2_" + n] / ms["surfels_" + n], 4),
               "surfels_mrows_per_s": round(w["rows"] / ms["surfels_" + n] / 1e3, 1)}
line["kernels"] = None if args.no_resources else _timing.kernel_resources("surfel.hip", r"surfel_\w+_kernel")
_timing.emit(line, args.out)
