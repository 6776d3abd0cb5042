"""numpy restatement of include/epcnet_maps.h (epcnet_map_fuse), operation for operation, written from the header's text: elementwise
float64 in the stated association (numpy fuses nothing), ``np.floor``, int64 shifts, ``np.unique(..., return_index, return_inverse,
return_counts)`` for the voxels and their leaders, ``np.add.at`` for the integer sums, ``//`` for the mean and ONE ``astype(float32)``
at the end.  The device's outputs are compared with these on bit patterns.  Also the seeded scenes the tests share."""
import numpy as np

import submap_ref as SR

NAN_WORD = 0x7FC00000
MAX_CELL = 1 << 20
KEPT, ABSENT, OUT_OF_RANGE, NO_CLOUD = 0, 1, 2, 3


# ---- the definition ----------------------------------------------------------------------------------------------------------------------
def valid(offsets, num_rows):
    offsets = np.asarray(offsets, np.int64)
    return bool(offsets[0] >= 0 and offsets[-1] <= num_rows and not (np.diff(offsets) < 0).any())


def lattice(points, offsets, poses, origin, voxel):
    """``(kind (rows,) int, w (rows, 3) int64)`` of every row of ``points``: KEPT, ABSENT, OUT_OF_RANGE or NO_CLOUD (a row outside
    [offsets[0], offsets[-1])); w is the row's lattice position where it is kept, 0 elsewhere.  The offsets are valid."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    offsets = np.asarray(offsets, np.int64)
    C = len(offsets) - 1
    poses = np.asarray(poses, np.float64).reshape(C, 3, 4)
    origin, voxel = np.asarray(origin, np.float64), np.float64(voxel)
    rows = len(points)
    cloud = np.repeat(np.arange(C), np.diff(offsets))
    inside = np.arange(offsets[0], offsets[-1])
    kind = np.full(rows, NO_CLOUD)
    w = np.zeros((rows, 3), np.int64)
    x, y, z = (points[inside, c].astype(np.float64) for c in range(3))
    R, t = poses[cloud, :, :3], poses[cloud, :, 3]
    s = np.empty((len(inside), 3))
    with np.errstate(all="ignore"):
        for a in range(3):
            d = t[:, a] - origin[a]
            q = ((R[:, a, 0] * x + R[:, a, 1] * y) + R[:, a, 2] * z) + d
            s[:, a] = (q / voxel) * 4096.0
        finite = np.isfinite(s).all(1)
        f = np.floor(s)
        ranged = ((f >= -4294967296.0) & (f < 4294967296.0)).all(1)
    k = np.where(~finite, ABSENT, np.where(ranged, KEPT, OUT_OF_RANGE))
    kind[inside] = k
    w[inside[k == KEPT]] = f[k == KEPT].astype(np.int64)
    return kind, w


def keys_of(w):
    g = w >> 12
    return ((g[:, 2] + MAX_CELL) << 42) | ((g[:, 1] + MAX_CELL) << 21) | (g[:, 0] + MAX_CELL)


def reference(points, offsets, poses, origin, voxel, max_voxels, min_count=1, num_rows=None):
    """Every output of epcnet_map_fuse as a dict: ``map_points`` (max_voxels, 3) float32, ``count`` (max_voxels,) int32, ``num_out`` (4,)
    int32; besides ``V`` (the number of voxels, also on overflow) and ``leader`` (V,) for the tests."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    num_rows = len(points) if num_rows is None else num_rows
    out = np.zeros((max_voxels, 3), np.float32)
    out.view(np.uint32)[:] = NAN_WORD
    count = np.zeros(max_voxels, np.int32)
    if not valid(offsets, num_rows):
        return dict(map_points=out, count=count, num_out=np.int32([-1, 0, 0, 0]), V=0, leader=np.zeros(0, np.int64))
    kind, w = lattice(points, offsets, poses, origin, voxel)
    tally = [int((kind == k).sum()) for k in (KEPT, ABSENT, OUT_OF_RANGE)]
    rows = np.nonzero(kind == KEPT)[0]                  # ascending: the first occurrence of a key is its leader
    uniq, first, inverse, cnt = np.unique(keys_of(w[rows]), return_index=True, return_inverse=True, return_counts=True)
    V = len(uniq)
    order = np.argsort(first, kind="stable")           # the voxels by ascending leader
    leader = rows[first[order]]
    if V > max_voxels:
        return dict(map_points=out, count=count, num_out=np.int32([-1] + tally), V=V, leader=leader)
    number = np.empty(V, np.int64)
    number[order] = np.arange(V)
    j = number[inverse.reshape(-1)]                     # the voxel of every kept row
    S = np.zeros((V, 3), np.int64)
    np.add.at(S, j, w[rows] & 4095)
    cnt_j = cnt[order].astype(np.int64)
    m = S // cnt_j[:, None]
    g = w[leader] >> 12
    step = np.float64(voxel) / np.float64(4096.0)
    value = ((g * 4096 + m).astype(np.float64) * step).astype(np.float32)
    value.view(np.uint32)[cnt_j < min_count] = NAN_WORD
    out[:V] = value
    count[:V] = cnt_j
    return dict(map_points=out, count=count, num_out=np.int32([V] + tally), V=V, leader=leader)


# ---- a second formulation: Python integers and fractions (tests/test_map_cpu.py) ----------------------------------------------------------
def exact_row(row, pose, origin, voxel):
    """One row with ``fractions.Fraction``: valid where every operation of the definition is exact (the lattice scenes: identity or signed
    permutation rotations, values on a binary grid) -> ``(kind, w)`` with w a tuple of Python ints, from floor(q / voxel * 4096) in
    rationals."""
    from fractions import Fraction as F
    import math
    pose = np.asarray(pose, np.float64).reshape(3, 4)
    w = []
    for a in range(3):
        q = sum(F(float(pose[a, b])) * F(float(np.float32(row[b]))) for b in range(3)) + (F(float(pose[a, 3])) - F(float(origin[a])))
        w.append(math.floor(q / F(float(voxel)) * 4096))
    if any(not -(1 << 32) <= v < (1 << 32) for v in w):
        return OUT_OF_RANGE, None
    return KEPT, tuple(w)


def exact_map(points, offsets, poses, origin, voxel):
    """The voxels of an exact scene with dictionaries and Python integers: ``[(cell, count, mean), ...]`` by ascending leader, and the
    rows' kinds."""
    voxels, order, kinds = {}, [], []
    for c in range(len(offsets) - 1):
        for r in range(offsets[c], offsets[c + 1]):
            kind, w = exact_row(points[r], poses[c], origin, voxel)
            kinds.append(kind)
            if kind != KEPT:
                continue
            cell = tuple(v // 4096 for v in w)          # Python's floor division: floor(q / voxel)
            if cell not in voxels:
                voxels[cell] = [0, [0, 0, 0]]
                order.append(cell)
            voxels[cell][0] += 1
            for a in range(3):
                voxels[cell][1][a] += w[a] % 4096
    return [(cell, voxels[cell][0], tuple(s // voxels[cell][0] for s in voxels[cell][1])) for cell in order], kinds


# ---- seeded scenes ------------------------------------------------------------------------------------------------------------------------
def identity_poses(num, t=(0.0, 0.0, 0.0)):
    poses = np.zeros((num, 3, 4))
    poses[:, :, :3] = np.eye(3)
    poses[:, :, 3] = np.asarray(t, np.float64)
    return poses.reshape(num, 12)


def drive(seed, sizes, step=2.0, extent=12.0):
    """``(points, offsets, poses (C, 12), origin (3,))``: clouds of ``sizes`` rows along a seeded drive of ``step`` metres per cloud with
    general rotations and translations near (5.7e6, 6.2e5, 1e2) (submap_ref.trajectory); consecutive clouds overlap, so most voxels at
    0.5 m hold rows of several clouds.  The origin is the first translation."""
    poses, _ = SR.trajectory(seed, max(len(sizes), 1), step=step)
    poses = poses[:len(sizes)]
    points, offsets = SR.pack([SR.scan(500 + seed + i, m, extent=extent) for i, m in enumerate(sizes)])
    origin = poses[0].reshape(3, 4)[:, 3].copy() if len(sizes) else SR.ORIGIN.copy()
    return points, offsets, poses, origin


def lattice_scene():
    """Every value exact: rows on a grid of 1/4 m over [-2, 2]^3 (so a third of them lies exactly on a cell face of voxel 0.5, on both
    sides of the origin, -0.0 among them), two clouds with identity rotations and integer translations."""
    axis = np.arange(-8, 9) / 4.0
    grid = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    grid[grid == 0] = np.float32(-0.0)
    points, offsets = SR.pack([grid, grid[::-1][::3]])
    poses = np.concatenate([identity_poses(1, (100.0, 200.0, 10.0)), identity_poses(1, (101.0, 199.0, 10.0))])
    return points, offsets, poses, np.array([100.0, 200.0, 10.0])


def contracted(R, row):
    """fma(R2, z, fma(R0, x, fl(R1 y))): what a compiler that contracts makes of fl(fl(fl(R0 x) + fl(R1 y)) + fl(R2 z)), each fused
    operation rounded once (Fraction -> float rounds to nearest even)."""
    from fractions import Fraction as F
    R0, R1, R2 = (float(v) for v in R)
    x, y, z = (float(np.float32(v)) for v in row)
    inner = float(F(R0) * F(x) + F(float(np.float64(R1) * np.float64(y))))
    return float(F(R2) * F(z) + F(inner))


def face_scene(seed=5, clouds=16, rows=48):
    """A scene whose kept-or-which-cell decision sits in float64's last bit: general rotations from seeded quaternions, local
    translations, origin 0, voxel 1.  For every cloud c and axis a one row r = 3 i + a is TUNED: its t_a is N - max(p, p') with p the
    definition's fl(fl(fl(R0 x) + fl(R1 y)) + fl(R2 z)), p' the contracted one (they differ in the last bit for the rows chosen) and N
    an integer just above, so that fl(p + t_a) is exactly N for one of the two and the double below N for the other: the two fall into
    different cells.  ``(points, offsets, poses, origin, voxel, tuned)``; ``tuned``: the rows (global indices) whose cell a contraction
    moves, verified with the restatement and ``contracted``."""
    rng = np.random.default_rng([seed, clouds, rows])
    scans, poses, tuned = [], np.zeros((clouds, 3, 4)), []
    for c in range(clouds):
        R = SR.quat_matrix(rng.normal(size=4))
        pts = (rng.uniform(-20.0, 20.0, size=(rows, 3))).astype(np.float32)
        t = rng.integers(-5, 6, size=3).astype(np.float64)
        for a in range(3):
            for r in range(a, rows, 3):
                x, y, z = (np.float64(v) for v in pts[r])
                p = (np.float64(R[a, 0]) * x + np.float64(R[a, 1]) * y) + np.float64(R[a, 2]) * z
                pc = contracted(R[a], pts[r])
                if pc == p:
                    continue
                N = np.ceil(max(p, pc)) + 2.0
                d = N - max(p, pc)
                cells = {float(np.floor(np.float64(v) + d)) for v in (p, pc)}
                if len(cells) == 2 and float(np.float64(max(p, pc)) + d) == N:
                    t[a] = d
                    tuned.append(c * rows + r)
                    break
        poses[c, :, :3], poses[c, :, 3] = R, t
        scans.append(pts)
    points, offsets = SR.pack(scans)
    return points, offsets, poses.reshape(clouds, 12), np.zeros(3), 1.0, tuned
