"""numpy restatement of include/epcnet_submaps.h (epcnet_submap_build), operation for operation: elementwise float64 in the stated
association (numpy fuses nothing), ``searchsorted(..., 'left')`` for the three lower bounds, an integer cumsum for the layout and ONE
``astype(float32)`` at the end.  The device's outputs are compared with these on bit patterns.  Also the seeded trajectories and scans the
tests share: general rotations from seeded quaternions (not yaw alone), translations near (5.7e6, 6.2e5, 1e2)."""
import numpy as np

NO_SUBMAP, NO_ROOM = 16, 32
MAX_ROWS = 1 << 20
NAN_WORD = 0x7FC00000
ORIGIN = np.array([5.7e6, 6.2e5, 1.0e2])


# ---- the definition ----------------------------------------------------------------------------------------------------------------------
def valid(offsets, along, num_rows):
    """The whole-call rule: offsets valid by the third header's rule, along finite and non-decreasing, at least one scan."""
    offsets, along = np.asarray(offsets, np.int64), np.asarray(along, np.float64)
    if len(along) == 0:
        return False
    if offsets[0] < 0 or offsets[-1] > num_rows or (np.diff(offsets) < 0).any():
        return False
    return bool(np.isfinite(along).all() and not (along[:-1] > along[1:]).any())


def segment(along, length, spacing, max_submaps):
    """Slots 0 .. max_submaps (one more than the caller's: the last says whether the trajectory goes on):
    ``(is_submap, lo, hi, ref)``; lo, hi, ref are -1 for a slot that is no submap."""
    along = np.asarray(along, np.float64)
    h = np.float64(length) * 0.5
    k = np.arange(max_submaps + 1).astype(np.float64)
    with np.errstate(all="ignore"):
        c = (along[0] + h) + k * np.float64(spacing)
        s, e = c - h, c + h
        is_submap = e <= along[-1]
    lo = np.searchsorted(along, s, "left")
    hi = np.searchsorted(along, e, "left")
    ref = np.searchsorted(along, c, "left")
    return is_submap, np.where(is_submap, lo, -1), np.where(is_submap, hi, -1), np.where(is_submap, ref, -1)


def layout(offsets, is_submap, lo, hi, out_rows):
    """``(sub_offsets (max_submaps + 1) int32, status (max_submaps) int32, rows (max_submaps) int64)`` of the caller's slots from the
    segmentation of slots 0 .. max_submaps."""
    offsets = np.asarray(offsets, np.int64)
    is_submap, lo, hi = is_submap[:-1], lo[:-1], hi[:-1]
    raw = np.where(is_submap, offsets[np.maximum(hi, 0)] - offsets[np.maximum(lo, 0)], 0)
    big = raw > MAX_ROWS
    rows = np.where(big, 0, raw)
    P = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    fits = is_submap & (P[1:] <= out_rows)
    k_fit = int(fits.sum())
    assert fits[:k_fit].all()                          # (P is monotone: the submaps that do not fit are the last ones)
    sub_offsets = np.minimum(P, P[k_fit]).astype(np.int32)
    status = np.where(~is_submap, NO_SUBMAP, np.where(big | ~fits, NO_ROOM, 0)).astype(np.int32)
    return sub_offsets, status, rows


def pair(Ri, Rr):
    """M (3, 3) and u (3) of a scan's pose Ri and the frame's pose Rr, both (12,) float64 [R | t] row-major."""
    Ri, Rr = np.asarray(Ri, np.float64).reshape(3, 4), np.asarray(Rr, np.float64).reshape(3, 4)
    with np.errstate(all="ignore"):
        d = Ri[:, 3] - Rr[:, 3]
        M = np.empty((3, 3))
        u = np.empty(3)
        for a in range(3):
            for b in range(3):
                M[a, b] = (Rr[0, a] * Ri[0, b] + Rr[1, a] * Ri[1, b]) + Rr[2, a] * Ri[2, b]
            u[a] = (Rr[0, a] * d[0] + Rr[1, a] * d[1]) + Rr[2, a] * d[2]
    return M, u


def transform64(rows, M, u):
    """q (n, 3) float64 of float32 rows (n, 3): the header's association."""
    x, y, z = (np.asarray(rows, np.float32)[:, c].astype(np.float64) for c in range(3))
    with np.errstate(all="ignore"):
        return np.stack([((M[a, 0] * x + M[a, 1] * y) + M[a, 2] * z) + u[a] for a in range(3)], 1)


def transform(rows, M, u, min_range=0.0, max_range=100.0, z_min=-np.inf, z_max=np.inf):
    """The output words (n, 3) float32 of a scan's rows: (float)q for a kept row, three words 0x7fc00000 for every other."""
    x, y, z = (np.asarray(rows, np.float32)[:, c].astype(np.float64) for c in range(3))
    q = transform64(rows, M, u)
    with np.errstate(all="ignore"):
        rr = (x * x + y * y) + z * z
        keep = ((rr >= np.float64(min_range) * np.float64(min_range))
                & ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) <= np.float64(max_range) * np.float64(max_range))
                & (np.float64(z_min) <= q[:, 2]) & (q[:, 2] <= np.float64(z_max)))
        out = q.astype(np.float32)
    out.view(np.uint32)[~keep] = NAN_WORD
    return out


def reference(points, offsets, poses, along, length=20.0, spacing=10.0, min_range=0.0, max_range=100.0, z_min=-np.inf, z_max=np.inf,
              max_submaps=None, out_rows=None):
    """Every output of epcnet_submap_build as a dict: ``points_out`` (sub_offsets[-1], 3) float32 -- the rows the call writes --,
    ``sub_offsets``, ``status``, ``sub_info``, ``num_out``, ``sub_pose``."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    offsets = np.asarray(offsets, np.int64)
    S = len(offsets) - 1
    poses = np.asarray(poses, np.float64).reshape(S, 12)
    along = np.asarray(along, np.float64)
    max_submaps = min(max(S, 1), 65535) if max_submaps is None else max_submaps
    out_rows = len(points) * (int(np.ceil(length / spacing)) + 1) if out_rows is None else out_rows
    if not valid(offsets, along, len(points)):
        return dict(points_out=np.zeros((0, 3), np.float32), sub_offsets=np.zeros(max_submaps + 1, np.int32),
                    status=np.full(max_submaps, NO_SUBMAP, np.int32), sub_info=np.tile(np.int32([-1, -1, -1, 0]), (max_submaps, 1)),
                    num_out=np.zeros(2, np.int32), sub_pose=np.full((max_submaps, 12), np.nan))
    is_submap, lo, hi, ref = segment(along, length, spacing, max_submaps)
    sub_offsets, status, rows = layout(offsets, is_submap, lo, hi, out_rows)
    sub_pose = np.full((max_submaps, 12), np.nan)
    out = np.zeros((int(sub_offsets[-1]), 3), np.float32)
    for k in range(max_submaps):
        if not is_submap[k]:
            continue
        sub_pose[k] = poses[ref[k]]
        if sub_offsets[k + 1] == sub_offsets[k]:
            continue
        at = int(sub_offsets[k])
        for i in range(lo[k], hi[k]):
            n = int(offsets[i + 1] - offsets[i])
            if n:
                M, u = pair(poses[i], poses[ref[k]])
                out[at:at + n] = transform(points[offsets[i]:offsets[i + 1]], M, u, min_range, max_range, z_min, z_max)
                at += n
        assert at == sub_offsets[k + 1]
    info = np.stack([lo[:-1], hi[:-1], ref[:-1], rows], 1).astype(np.int32)
    num_out = np.int32([int(is_submap[:-1].sum()), int(is_submap[-1])])
    return dict(points_out=out, sub_offsets=sub_offsets, status=status, sub_info=info, num_out=num_out, sub_pose=sub_pose)


# ---- seeded scenes ------------------------------------------------------------------------------------------------------------------------
def quat_matrix(q):
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def trajectory(seed, num_scans, step=0.5, wobble=0.05, general=True):
    """``(poses (S, 12) float64, along (S,) float64)``: a seeded drive of ``step`` metres per scan from ORIGIN.  The rotations come
    from seeded quaternions: a general one for the whole drive (``general=False``: the identity, so that only roll, pitch and yaw of
    size ``wobble`` remain) perturbed per scan.  ``along`` is exactly ``step * i``; the translations follow a heading that wanders."""
    rng = np.random.default_rng([seed, num_scans])
    q0 = rng.normal(size=4) if general else np.array([1.0, 0.0, 0.0, 0.0])
    q0 = q0 / np.linalg.norm(q0)
    poses = np.zeros((num_scans, 3, 4))
    t = ORIGIN + rng.normal(size=3)
    heading = rng.uniform(0, 2 * np.pi)
    for i in range(num_scans):
        poses[i, :, :3] = quat_matrix(q0 + wobble * rng.normal(size=4))
        poses[i, :, 3] = t
        heading += 0.05 * rng.normal()
        t = t + step * np.array([np.cos(heading), np.sin(heading), 0.02 * rng.normal()])
    return poses.reshape(num_scans, 12), step * np.arange(num_scans, dtype=np.float64)


def identity_poses(num_scans, step=0.0):
    """Identity rotations, translations (step * i, 0, 0): the lattice scenes, where every q is exact."""
    poses = np.zeros((num_scans, 3, 4))
    poses[:, :, :3] = np.eye(3)
    poses[:, 0, 3] = step * np.arange(num_scans)
    return poses.reshape(num_scans, 12)


def scan(seed, rows, extent=30.0):
    """(rows, 3) float32 in the sensor's frame: x, y in [-extent, extent], z in [-2, 5]."""
    rng = np.random.default_rng([seed, rows, 77])
    p = rng.uniform(-1.0, 1.0, size=(rows, 3)) * np.array([extent, extent, 3.5]) + np.array([0.0, 0.0, 1.5])
    return p.astype(np.float32)


def pack(scans):
    """``(points (total, 3) float32, offsets (S + 1) int32)`` of a list of scans."""
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int32)
    points = np.concatenate([np.asarray(s, np.float32).reshape(-1, 3) for s in scans]) if len(scans) else np.zeros((0, 3), np.float32)
    return points.reshape(-1, 3), offsets


def direct64(rows, Ri, Rr):
    """((p Ri^T + ti) - tr) Rr in float64: the textbook form the header's M | u form is tested against."""
    Ri, Rr = np.asarray(Ri, np.float64).reshape(3, 4), np.asarray(Rr, np.float64).reshape(3, 4)
    p = np.asarray(rows, np.float32).astype(np.float64)
    return ((p @ Ri[:, :3].T + Ri[:, 3]) - Rr[:, 3]) @ Rr[:, :3]
