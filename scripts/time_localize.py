"""Scan-to-map localisation against the same iteration composed with torch, and against today's detour: ops.localize_scans at voxel 0.2 m,
16 iterations, on the surfel maps of two workloads of scripts/time_surfels.py -- `batch` (14 submaps of 8 scans of 32 768 rows, 1.43 M
voxels) and `long` (98 submaps of 40 scans of 2000 rows, 3.76 M voxels) -- for (Q, n) = (1, 4096), (64, 4096) and (320, 1024).  A scan
is n rows drawn from one submap's cloud in its own frame; its truth is that submap's pose (held out: the seed is the truth moved by up to
1.5 degrees and 0.1 m).  In one process, the arms alternating:
  entry_*   (a) ops.localize_scans on a prebuilt index
  torch_*   (b) the same iteration with torch on the device: sorted keys + 27 searchsorted, gathers, einsum for the 29 sums,
            torch.linalg.solve_ex, the same retraction (its poses are compared with the entry's before anything is timed)
  detour_*  (c) retrieval.register_pairs on [the scans, grid_downsample(map, n)] from the same seeds: point-to-point against n rows
            thinned from the map (its first 2^20 voxels: the down-sampler takes no more per cloud and refuses these maps whole).  Another
            metric: reported with its own residual against the truth, never as a ratio
  build_* / sort_*   ops.index_surfels against a torch.sort of the map's precomputed keys
`--regions` timed regions of `--steps` calls each, every region between device synchronisations; the median region.  Also the kernels'
registers / LDS / scratch as the compiler reports them (skipped with --no-resources).  One JSON line, stamped with the SHA-256 of the
loaded library.  The bar, set before anything was measured: entry <= torch at every size, build <= sort on both maps.
Usage (GPU box): python scripts/time_localize.py [--steps K] [--regions R] [--warmup W] [--out FILE] [--only NAME]"""
import argparse
import math
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
import register_ref as RR  # noqa: E402
import submap_ref as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--regions", type=int, default=7)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--voxel", type=float, default=0.2)
ap.add_argument("--iterations", type=int, default=16)
ap.add_argument("--only", default=None, help="one workload (batch, long) and the entry arms alone: for a profiler")
ap.add_argument("--no-resources", action="store_true")
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
args = ap.parse_args()

ops, L, retrieval = bench.pkg("ops"), bench.pkg("lib"), bench.pkg("retrieval")
dev = torch.device("cuda:0")
SIZES = ((1, 4096), (64, 4096), (320, 1024))
MAX_CELL = 1 << 20
OFFSETS = [(o0, o1, o2) for o2 in (-1, 0, 1) for o1 in (-1, 0, 1) for o0 in (-1, 0, 1)]


def drive(name, scans, rows, length, spacing):
    """One workload of time_surfels.py: its drive, built into submaps once, and the surfel map of the submaps."""
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
    out = ops.fuse_surfels(w["points"], w["offsets"], w["poses"], voxel=args.voxel, origin=w["origin"])
    V = int(out[6][0])
    assert 0 < V
    w["V"], w["anchor"], w["centroid"], w["normal"] = V, out[0][:V].contiguous(), out[2][:V].contiguous(), out[3][:V].contiguous()
    w["valid"] = int(torch.isfinite(w["normal"]).all(1).sum())
    return w


def scans_of(w, Q, n, seed):
    """(scans (Q, n, 3) float32, truth (Q, 12) float64 relative to the origin, seeds (Q, 1, 12) float64): n rows of submap q % C each."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    off = w["offsets"].cpu().numpy()
    rel = w["poses"].clone()
    rel[:, 3::4] -= w["origin"]
    rel = rel.cpu().numpy()
    rng = np.random.default_rng(seed)
    clouds, truth, seeds = [], [], []
    for q in range(Q):
        c = q % w["clouds"]
        pick = torch.randint(int(off[c]), int(off[c + 1]), (n,), generator=g).to(dev)
        clouds.append(w["points"][pick])
        truth.append(rel[c])
        a = rng.uniform(-1.5, 1.5, size=3)
        d = RR.pose_of(a[0], a[1] / 3, a[2] / 3, rng.uniform(-0.06, 0.06, size=3)).reshape(3, 4)
        m = rel[c].reshape(3, 4)
        seeds.append(np.concatenate([d[:, :3] @ m[:, :3], (m[:, 3] + d[:, 3])[:, None]], 1).reshape(12))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)
    return torch.stack(clouds).contiguous(), up(np.stack(truth)), up(np.stack(seeds)).reshape(Q, 1, 12)


def keys_of(cell):
    c = cell + MAX_CELL
    return (c[..., 2] << 42) | (c[..., 1] << 21) | c[..., 0]


def torch_index(anchor, centroid, normal, voxel):
    """(sorted keys, the lowest present surfel of every key)."""
    present = torch.isfinite(anchor).all(1) & torch.isfinite(centroid).all(1) & torch.isfinite(normal).all(1)
    cell = torch.floor(torch.where(present[:, None], anchor, torch.zeros_like(anchor)).double() / voxel).long()
    j = torch.nonzero(present)[:, 0]
    keys, inverse = torch.unique(keys_of(cell[j]), return_inverse=True)
    first = torch.full_like(keys, anchor.shape[0]).scatter_reduce_(0, inverse, j, "amin")
    return keys, first


def torch_localize(scans, seeds, keys, first, centroid, normal, voxel, gate2, iterations):
    """The header's iteration with torch: (pose (Q, 12), H (Q, 6, 6), mean e^2 (Q,), accepted (Q,))."""
    Q = scans.shape[0]
    pose = seeds.reshape(Q, 3, 4).clone()
    there = torch.isfinite(scans).all(-1)                          # an absent row is accepted nowhere
    x = torch.where(there[..., None], scans, torch.zeros_like(scans)).double()
    K = keys.numel()
    for it in range(iterations + 1):
        r = torch.einsum("qij,qnj->qni", pose[:, :, :3], x)
        p = (r + pose[:, None, :, 3]).float()
        k = torch.floor(p.double() / voxel).long().clamp(-MAX_CELL - 1, MAX_CELL)
        best = torch.full(p.shape[:2], float("inf"), dtype=torch.float32, device=p.device)
        bj = torch.zeros(p.shape[:2], dtype=torch.int64, device=p.device)
        for o in OFFSETS:
            c = k + torch.tensor(o, device=p.device)
            inside = ((c >= -MAX_CELL) & (c < MAX_CELL)).all(-1)
            key = keys_of(torch.where(inside[..., None], c, torch.zeros_like(c)))
            at = torch.searchsorted(keys, key).clamp(max=K - 1)
            j = first[at]
            d = p - centroid[j]
            d2 = torch.where(inside & (keys[at] == key), (d * d).sum(-1), torch.full_like(best, float("inf")))
            take = d2 < best
            best, bj = torch.where(take, d2, best), torch.where(take, j, bj)
        took = (best <= gate2) & there                              # (a row that took nothing gathers surfel 0, which may be NaN)
        acc = took.double()
        nrm = normal[bj].double()
        e = torch.where(took, ((p.double() - centroid[bj].double()) * nrm).sum(-1), torch.zeros_like(acc))
        J = torch.cat([torch.linalg.cross(r, nrm), nrm], -1)
        J = torch.where(took[..., None], J, torch.zeros_like(J))
        Hm, b = torch.einsum("qni,qnj->qij", J, J), torch.einsum("qni,qn->qi", J, e)
        if it == iterations:
            break
        delta = torch.linalg.solve_ex(Hm, -b[..., None])[0][..., 0]
        h = 0.5 * delta[:, :3]
        qx, qy, qz = h[:, 0], h[:, 1], h[:, 2]
        u = 2.0 / (1.0 + (h * h).sum(1))
        C = torch.stack([1 - u * (qy * qy + qz * qz), u * (qx * qy - qz), u * (qx * qz + qy),
                         u * (qx * qy + qz), 1 - u * (qx * qx + qz * qz), u * (qy * qz - qx),
                         u * (qx * qz - qy), u * (qy * qz + qx), 1 - u * (qx * qx + qy * qy)], 1).reshape(Q, 3, 3)
        pose = torch.cat([C @ pose[:, :, :3], (pose[:, :, 3] + delta[:, 3:])[..., None]], 2)
    count = acc.sum(1)
    return pose.reshape(Q, 12), Hm, (e * e).sum(1) / count, count


def errors(pose, truth):
    """Median and worst (rotation in radians, translation in metres) of poses (Q, 12) against the truth; NaN poses count as missing."""
    a, b = pose.reshape(-1, 3, 4), truth.reshape(-1, 3, 4)
    ok = torch.isfinite(a).all(2).all(1)
    chord = torch.linalg.matrix_norm(a[:, :, :3] - b[:, :, :3]) / (2.0 * math.sqrt(2.0))
    angle, dist = 2.0 * torch.asin(chord.clamp(max=1.0)), torch.linalg.vector_norm(a[:, :, 3] - b[:, :, 3], dim=1)
    if not bool(ok.any()):
        return {"solved": 0}
    return {"solved": int(ok.sum()), "median_rad": float(angle[ok].median()), "max_rad": float(angle[ok].max()),
            "median_m": float(dist[ok].median()), "max_m": float(dist[ok].max())}


names = {"batch": (64, 32768, 4.0, 2.0), "long": (2000, 2000, 20.0, 10.0)}
gate2 = float(np.float32(1.0))
arms, report = {}, {}
for name in names:
    if args.only not in (None, name):
        continue
    w = drive(name, *names[name])
    print("time_localize: %s: %d voxels" % (name, w["V"]), file=sys.stderr, flush=True)
    index, num = ops.index_surfels(w["anchor"], w["centroid"], w["normal"], args.voxel)
    keys, first = torch_index(w["anchor"], w["centroid"], w["normal"], args.voxel)
    cell = torch.floor(torch.nan_to_num(w["anchor"]).double() / args.voxel).long()
    raw_keys = keys_of(cell).contiguous()
    rep = report[name] = {"rows": w["rows"], "submaps": w["clouds"], "voxels": w["V"], "valid_surfels": w["valid"], "num": num.tolist(),
                          "torch_holds_the_same_keys": bool(keys.numel() == int(num[0])), "index_bytes": int(index.numel())}
    arms["build_" + name] = lambda w=w, index=index: ops.index_surfels(w["anchor"], w["centroid"], w["normal"], args.voxel, index=index)
    if not args.only:
        arms["sort_" + name] = lambda raw_keys=raw_keys: torch.sort(raw_keys)
    for Q, n in SIZES:
        tag = "%s_%dx%d" % (name, Q, n)
        scans, truth, seeds = scans_of(w, Q, n, 7 * Q + n)
        ws = torch.empty(int(L.lib().epcnet_scan_localize_workspace_bytes(Q, 1, n)), dtype=torch.uint8, device=dev)
        entry = lambda scans=scans, seeds=seeds, index=index, w=w, ws=ws: ops.localize_scans(
            scans, index, w["centroid"], w["normal"], seeds, voxel=args.voxel, iterations=args.iterations, workspace=ws)
        arms["entry_" + tag] = entry
        if args.only:
            continue
        pose, fit, hessian, info, status = entry()
        tpose, tH, tfit, tcount = torch_localize(scans, seeds, keys, first, w["centroid"], w["normal"], args.voxel, gate2, args.iterations)
        ok = status == 0
        size = rep["%dx%d" % (Q, n)] = {
            "status_ok": int(ok.sum()), "accepted_rows_median": float(info[:, 1].double().median()),
            "entry_against_truth": errors(pose, truth), "seed_against_truth": errors(seeds.reshape(Q, 12), truth),
            "torch_against_entry_max_abs_pose_word": float((tpose[ok] - pose[ok]).abs().max()) if bool(ok.any()) else None,
            "fit_msr_m2_median": float(fit[ok, 0].median()) if bool(ok.any()) else None}
        arms["torch_" + tag] = lambda scans=scans, seeds=seeds, keys=keys, first=first, w=w: torch_localize(
            scans, seeds, keys, first, w["centroid"], w["normal"], args.voxel, gate2, args.iterations)
        # today's detour: the scans and the map thinned to n rows as clouds of one register_pairs call.  grid_downsample takes at most
        # 2^20 rows per cloud and refuses these maps whole (recorded): the detour gets the map's first 2^20 voxels, the start of the drive
        whole = ops.grid_downsample(w["anchor"], torch.tensor([0, w["V"]], dtype=torch.int32, device=dev), n, normalize=False)[1]
        size["detour_thinning_status_on_the_whole_map"] = int(whole[0])
        head = min(w["V"], 1 << 20)
        size["detour_map_voxels"] = head
        thin, thin_status, _ = ops.grid_downsample(w["anchor"], torch.tensor([0, head], dtype=torch.int32, device=dev), n, normalize=False)
        clouds = torch.cat([scans, thin], 0).contiguous()
        pairs = torch.stack([torch.arange(Q, dtype=torch.int32, device=dev), torch.full((Q,), Q, dtype=torch.int32, device=dev)], 1).contiguous()
        detour = lambda clouds=clouds, pairs=pairs, seeds=seeds: retrieval.register_pairs(clouds, pairs, seeds, max_dist=1.0,
                                                                                         iterations=args.iterations)
        dpose, dfit, dinfo, dstatus = detour()
        size["detour_thinning_status"] = int(thin_status[0])
        size["detour_status_ok"] = int((dstatus == 0).sum())
        size["detour_against_truth"] = errors(dpose, truth)
        arms["detour_" + tag] = detour
        print("time_localize: %s verified" % tag, file=sys.stderr, flush=True)
times = _timing.alternate(arms, args.steps, args.regions, args.warmup)
ms = {k: statistics.median(v) / args.steps * 1e3 for k, v in times.items()}
line = {"workload": "ops.localize_scans at voxel %g m, max_dist 1 m, %d iterations, one seed per scan (the truth moved by up to 1.5 degrees "
                    "and 0.1 m), against the surfel maps of time_surfels.py's batch and long workloads; (b) torch_*: the same iteration "
                    "with torch (27 searchsorted, gathers, einsum, linalg.solve_ex); (c) detour_*: register_pairs against "
                    "grid_downsample(map, n), point-to-point: another metric, see *_against_truth; build_* against a torch.sort of the "
                    "map's keys" % (args.voxel, args.iterations),
        "ms_per_call": {k: round(v, 4) for k, v in ms.items()},
        "steps_per_region": args.steps,
        "regions_s": {k: [round(t, 5) for t in v] for k, v in times.items()},
        "pass_and_solve_split": "this script takes no profile; where one was taken (rocprofv3 --kernel-trace --stats -- python "
                                "scripts/time_localize.py --only long --no-resources) it is profiles/r21_localize_kernel_stats.csv"}
if not args.only:
    bar = {}
    for name in report:
        bar["build_over_sort_" + name] = round(ms["build_" + name] / ms["sort_" + name], 4)
        for Q, n in SIZES:
            tag = "%s_%dx%d" % (name, Q, n)
            bar["entry_over_torch_" + tag] = round(ms["entry_" + tag] / ms["torch_" + tag], 4)
            report[name]["%dx%d" % (Q, n)]["entry_scans_per_s"] = round(Q / ms["entry_" + tag] * 1e3, 1)
    line["bar"] = {"set_in_advance": "every ratio <= 1", "ratios": bar, "met": all(v <= 1.0 for v in bar.values())}
line.update(report)
line["kernels"] = None if args.no_resources else _timing.kernel_resources("localize.hip", r"lz_\w+_kernel")
_timing.emit(line, args.out)
