"""numpy restatement of include/epcnet_localize.h (epcnet_surfel_index, epcnet_scan_localize), written from the header's text: the index
is the sorted keys of the indexed surfels (``np.unique`` keeps the lowest j of a key); a correspondence pass is 27 shifted
``searchsorted`` lookups in elementwise float32 / float64 in the stated association (numpy fuses nothing); the 29 sums are the two-line
pairing loop over 4096 leaves; the Cholesky, the solve and the retraction are scalar float64 Python (a Python float is an IEEE double and
every operator rounds once; ``math.sqrt`` is correctly rounded).  Nothing here calls the library."""
import math

import numpy as np

import register_ref as RR

NO_PAIR, NO_FIT = RR.NO_PAIR, RR.NO_FIT
MAX_CELL = 1 << 20
LEAVES = 4096
SUMS = 29
IDENTITY = RR.IDENTITY
UPPER = [(i, j) for i in range(6) for j in range(i, 6)]          # sums[1 + k] = sum J_i J_j


# ---- the index ------------------------------------------------------------------------------------------------------------------------------
def cells_of(rows, voxel):
    """float32 rows (k, 3) -> (k_a as float64 (k, 3), inside (k,)): floor(fl((double)row / voxel)) and whether every k_a is in range."""
    with np.errstate(all="ignore"):
        f = np.floor(np.asarray(rows, np.float32).astype(np.float64) / np.float64(voxel))
    return f, ((f >= -MAX_CELL) & (f < MAX_CELL)).all(1)


def keys_of(cells):
    """int64 cells (k, 3), each in range -> the key of map_common.h."""
    c = np.asarray(cells, np.int64) + MAX_CELL
    return (c[:, 2] << 42) | (c[:, 1] << 21) | c[:, 0]


def index_reference(anchor, centroid, normal, voxel):
    """dict: ``keys`` (sorted), ``j`` (the indexed surfel of every key), ``num`` [indexed, not present, duplicates, out of range],
    ``kind`` per surfel (0 indexed, 1 not present, 2 duplicate, 3 out of range), and the arrays."""
    anchor, centroid, normal = (np.asarray(a, np.float32).reshape(-1, 3) for a in (anchor, centroid, normal))
    M = len(anchor)
    present = np.isfinite(anchor).all(1) & np.isfinite(centroid).all(1) & np.isfinite(normal).all(1)
    f, inside = cells_of(anchor, voxel)
    kind = np.where(~present, 1, np.where(~inside, 3, 2))
    rows = np.nonzero(present & inside)[0]
    keys, first = np.unique(keys_of(f[rows].astype(np.int64)), return_index=True) if rows.size else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    j = rows[first]                                                   # np.unique: the first occurrence, rows ascending = the lowest j
    kind[j] = 0
    num = [int((kind == v).sum()) for v in (0, 1, 2, 3)]
    assert sum(num) == M
    return dict(keys=keys, j=j, num=num, kind=kind, centroid=centroid, normal=normal, voxel=float(voxel), M=M)


# ---- the correspondence pass ------------------------------------------------------------------------------------------------------------------
def transform(m, rows):
    """(r (k, 3) float64, p (k, 3) float32) of float32 rows under the pose m."""
    x, y, z = (rows[:, c].astype(np.float64) for c in range(3))
    with np.errstate(all="ignore"):
        r = np.stack([(m[4 * c] * x + m[4 * c + 1] * y) + m[4 * c + 2] * z for c in range(3)], 1)
        p = np.stack([(r[:, c] + m[4 * c + 3]).astype(np.float32) for c in range(3)], 1)
    return r, p


def correspond(p, index):
    """float32 places p (k, 3) -> (surfel j (k,), -1 without a candidate; float32 d2 (k,), +Inf without one)."""
    n = len(p)
    best = np.full(n, np.inf, np.float32)
    bj = np.full(n, -1, np.int64)
    keys, js, cen = index["keys"], index["j"], index["centroid"]
    if n == 0 or len(keys) == 0:
        return bj, best
    f, _ = cells_of(p, index["voxel"])
    for o2 in (-1, 0, 1):
        for o1 in (-1, 0, 1):
            for o0 in (-1, 0, 1):
                with np.errstate(all="ignore"):
                    cell = f + np.array([o0, o1, o2], np.float64)
                    inside = ((cell >= -MAX_CELL) & (cell < MAX_CELL)).all(1)            # False for a NaN
                key = keys_of(np.where(inside[:, None], cell, 0.0).astype(np.int64))
                at = np.minimum(np.searchsorted(keys, key), len(keys) - 1)
                hit = inside & (keys[at] == key)
                j = js[at]
                c = cen[j]
                with np.errstate(all="ignore"):
                    dx, dy, dz = p[:, 0] - c[:, 0], p[:, 1] - c[:, 1], p[:, 2] - c[:, 2]
                    d2 = (dx * dx + dy * dy) + dz * dz
                d2 = np.where(np.isnan(d2) | ~hit, np.float32(np.inf), d2).astype(np.float32)
                take = d2 < best                                                          # ties keep the earlier candidate
                best = np.where(take, d2, best)
                bj = np.where(take, j, bj)
    return bj, best


def residuals(r, p, index, j):
    """(e (k,), J (k, 6)) float64 of rows with their surfels j."""
    c, nrm = index["centroid"][j].astype(np.float64), index["normal"][j].astype(np.float64)
    q = p.astype(np.float64)
    e = (nrm[:, 0] * (q[:, 0] - c[:, 0]) + nrm[:, 1] * (q[:, 1] - c[:, 1])) + nrm[:, 2] * (q[:, 2] - c[:, 2])
    J = np.stack([r[:, 1] * nrm[:, 2] - r[:, 2] * nrm[:, 1], r[:, 2] * nrm[:, 0] - r[:, 0] * nrm[:, 2], r[:, 0] * nrm[:, 1] - r[:, 1] * nrm[:, 0],
                  nrm[:, 0], nrm[:, 1], nrm[:, 2]], 1)
    return e, J


def pass_sums(m, scan, index, gate2, detail=False):
    """One correspondence pass under the pose m[12] -> the 29 sums (float64)."""
    scan = np.asarray(scan, np.float32)
    leaves = np.zeros((SUMS, LEAVES), np.float64)
    rows = np.nonzero(RR.present(scan))[0]
    r, p = transform(m, scan[rows])
    j, d2 = correspond(p, index)
    acc = d2 <= gate2
    rows, r, p, j = rows[acc], r[acc], p[acc], j[acc]
    e, J = residuals(r, p, index, j)
    leaves[0, rows] = 1.0
    for k, (a, b) in enumerate(UPPER):
        leaves[1 + k, rows] = J[:, a] * J[:, b]
    for a in range(6):
        leaves[22 + a, rows] = J[:, a] * e
    leaves[28, rows] = e * e
    sums = RR.tree_sum(leaves)
    return (sums, rows, j, e, J, r, p) if detail else sums


# ---- the solve ------------------------------------------------------------------------------------------------------------------------------
def cholesky(sums):
    """The lower factor L (6 x 6 lists) of H = sums[1 .. 21], or None at a pivot that is not > 0."""
    H = [[0.0] * 6 for _ in range(6)]
    for k, (a, b) in enumerate(UPPER):
        H[a][b] = H[b][a] = float(sums[1 + k])
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        s = H[j][j]
        for k in range(j):
            s = s - L[j][k] * L[j][k]
        if not s > 0.0:
            return None
        L[j][j] = math.sqrt(s)
        for i in range(j + 1, 6):
            s = H[i][j]
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            L[i][j] = s / L[j][j]
    return L


def step(sums, pose):
    """One Gauss-Newton step -> the new pose (12,) float64, or None (a failed pivot, a non-finite word)."""
    try:
        L = cholesky(sums)
        if L is None:
            return None
        y, d = [0.0] * 6, [0.0] * 6
        for i in range(6):
            s = -float(sums[22 + i])
            for k in range(i):
                s = s - L[i][k] * y[k]
            y[i] = s / L[i][i]
        for i in range(5, -1, -1):
            s = y[i]
            for k in range(i + 1, 6):
                s = s - L[k][i] * d[k]
            d[i] = s / L[i][i]
        C = RR.rotation_of((1.0, 0.5 * d[0], 0.5 * d[1], 0.5 * d[2]))
        m = [float(v) for v in pose]
        out = []
        for i in range(3):
            out += [(C[3 * i] * m[j] + C[3 * i + 1] * m[4 + j]) + C[3 * i + 2] * m[8 + j] for j in range(3)] + [m[4 * i + 3] + d[3 + i]]
    except (OverflowError, ZeroDivisionError, ValueError):
        return None
    out = np.array(out, np.float64)
    return out if np.isfinite(out).all() else None


def localize_scan(scan, seeds, index, gate2, iterations, min_pairs):
    """One scan -> (pose (12,), fit (2,), hessian (21,), info [4], status)."""
    rows = int(RR.present(scan).sum())

    def flagged(bit):
        return np.full(12, np.nan), np.full(2, np.nan), np.full(21, np.nan), [-1, 0, rows, 0], bit

    best, best_sums = -1, None
    for h, seed in enumerate(seeds):
        if not np.isfinite(seed).all():
            continue
        s = pass_sums(seed, scan, index, gate2)
        if best < 0 or s[0] > best_sums[0] or (s[0] == best_sums[0] and s[28] < best_sums[28]):
            best, best_sums = h, s
    if best < 0:
        return flagged(NO_PAIR)
    pose, sums = np.array(seeds[best], np.float64), best_sums
    for it in range(iterations):
        if it:
            sums = pass_sums(pose, scan, index, gate2)
        if sums[0] < min_pairs:
            return flagged(NO_FIT)
        pose = step(sums, pose)
        if pose is None:
            return flagged(NO_FIT)
    if iterations:
        sums = pass_sums(pose, scan, index, gate2)
    if sums[0] < min_pairs:
        return flagged(NO_FIT)
    m = float(sums[0])
    return pose, np.array([float(sums[28]) / m, m / rows]), np.array(sums[1:22]), [best, int(m), rows, 0], 0


def localize_reference(scans, seeds, index, max_dist=1.0, iterations=16, min_pairs=32):
    """The whole entry: scans (Q, n, 3) float32, seeds (Q, H, 12) float64 or None, ``index`` from index_reference -> pose (Q, 12), fit
    (Q, 2), hessian (Q, 21) float64, info (Q, 4), status (Q,) int32."""
    scans = np.asarray(scans, np.float32)
    Q = len(scans)
    gate2 = RR.gate2_of(max_dist)
    pose, fit, hessian = np.full((Q, 12), np.nan), np.full((Q, 2), np.nan), np.full((Q, 21), np.nan)
    info, status = np.zeros((Q, 4), np.int32), np.zeros(Q, np.int32)
    for q in range(Q):
        hyp = IDENTITY[None] if seeds is None else np.asarray(seeds[q], np.float64).reshape(-1, 12)
        pose[q], fit[q], hessian[q], info[q], status[q] = localize_scan(scans[q], hyp, index, gate2, iterations, min_pairs)
    return pose, fit, hessian, info, status


def hessian_matrix(h21):
    H = np.zeros((6, 6))
    for k, (a, b) in enumerate(UPPER):
        H[a, b] = H[b, a] = h21[k]
    return H


# ---- scenes for the tests ------------------------------------------------------------------------------------------------------------------
def plane_patches(seed, normals, offsets, per_patch, half=1.5):
    """Rows exactly (in float64) on the planes n . x = d, ``per_patch`` each, within ``half`` metres of the plane's foot point."""
    rng = np.random.default_rng(seed)
    parts = []
    for nrm, d in zip(normals, offsets):
        nrm = np.asarray(nrm, np.float64) / np.linalg.norm(nrm)
        a = np.cross(nrm, [0.3, -0.5, 0.8])
        a /= np.linalg.norm(a)
        b = np.cross(nrm, a)
        uv = rng.uniform(-half, half, size=(per_patch, 2))
        parts.append(nrm * d + uv[:, :1] * a + uv[:, 1:] * b)
    return parts


THREE_PLANES = (((0.1, 0.2, 1.0), (1.0, 0.15, 0.1), (0.2, 1.0, -0.1)), (-1.0, 2.0, -2.5))


def plane_map(seed, normals, offsets, per_patch=6000, voxel=0.2, half=1.5):
    """The surfel map (through surfel_ref, at the origin, ring 1, min_support 8) of rows on the given planes -> ``(anchor, centroid,
    normal)`` (V, 3) float32, ready for index_reference."""
    import map_ref as M
    import surfel_ref as S
    pts = np.concatenate(plane_patches(seed, normals, offsets, per_patch, half)).astype(np.float32)
    ref = S.reference(pts, [0, len(pts)], M.identity_poses(1), np.zeros(3), voxel, len(pts), 1, 1, 8)
    V = ref["V"]
    return ref["map_points"][:V].copy(), ref["centroid"][:V].copy(), ref["normal"][:V].copy()


def plane_scan(seed, normals, offsets, n, truth, half=1.3):
    """n float32 rows of other samples of the same planes, seen from the sensor at ``truth`` ([R | t] sensor -> map)."""
    world = np.concatenate(plane_patches(seed, normals, offsets, n // len(normals) + 1, half))[:n]
    return RR.apply_pose(RR.invert_pose(truth), world).astype(np.float32)
