"""numpy restatement of include/epcnet_stamps.h (epcnet_pose_interp, epcnet_scan_deskew), operation for operation: int64 and uint64
arithmetic for the bracket and the fraction, elementwise float64 in the stated association (one operation per numpy call: numpy fuses
nothing), ``searchsorted(..., 'right')`` for the bracket index and ONE ``astype(float32)`` at the end.  The device's outputs are compared
with these on bit patterns.  Also the seeded scenes the tests share: odometry near submap_ref.ORIGIN on a 10 ms clock, and a vehicle on a
straight line with a constant yaw rate that sees static world points."""
import numpy as np

import submap_ref as SR

NO_POSE, PART_POSE = 64, 128
NAN_WORD = 0x7FC00000
NAN64_WORD = 0x7FF8000000000000


# ---- the definition ----------------------------------------------------------------------------------------------------------------------
def fraction(num, den):
    """fi = floor(num * 2^32 / den) in unsigned 64-bit integers, for arrays with 0 <= num <= den, 1 <= den < 2^31."""
    num, den = np.asarray(num).astype(np.uint64), np.asarray(den).astype(np.uint64)
    return (num << np.uint64(32)) // den


def bracket(pose_time, tau, max_gap_ns):
    """``(j, num, den, valid)`` of the times ``tau``: j as the header defines it (-1 before the first pose time), int64 num and den
    (0 and 1 where j is -1), and whether the bracket is valid."""
    pose_time, tau = np.asarray(pose_time, np.int64), np.asarray(tau, np.int64)
    P = len(pose_time)
    j = np.minimum(np.searchsorted(pose_time, tau, "right") - 1, P - 2)
    jc = np.maximum(j, 0)
    num = np.where(j >= 0, tau - pose_time[jc], 0)
    den = np.where(j >= 0, pose_time[jc + 1] - pose_time[jc], 1)
    valid = (j >= 0) & (num >= 0) & (num <= den) & (den <= np.int64(max_gap_ns))
    return j, num, den, valid


def blend(p0, p1, f):
    """The pose [R | t] (n, 12), n and t's finiteness of the knots ``p0``, ``p1`` (n, 7) and the exact fractions ``f`` (n,): the
    header's float64 operations one by one.  Returns ``(m, ok)``."""
    p0, p1, f = np.asarray(p0, np.float64), np.asarray(p1, np.float64), np.asarray(f, np.float64)
    with np.errstate(all="ignore"):
        g = 1.0 - f
        t = [p0[:, a] + f * (p1[:, a] - p0[:, a]) for a in range(3)]
        w0, x0, y0, z0 = (p0[:, 3 + c] for c in range(4))
        w1, x1, y1, z1 = (p1[:, 3 + c] for c in range(4))
        d = ((w0 * w1 + x0 * x1) + y0 * y1) + z0 * z1
        neg = d < 0
        w1, x1, y1, z1 = (np.where(neg, -c, c) for c in (w1, x1, y1, z1))
        w = g * w0 + f * w1
        x = g * x0 + f * x1
        y = g * y0 + f * y1
        z = g * z0 + f * z1
        n = ((w * w + x * x) + y * y) + z * z
        s = 2.0 / n
        m = np.empty((len(f), 12))
        m[:, 0] = 1.0 - s * (y * y + z * z)
        m[:, 1] = s * (x * y - w * z)
        m[:, 2] = s * (x * z + w * y)
        m[:, 3] = t[0]
        m[:, 4] = s * (x * y + w * z)
        m[:, 5] = 1.0 - s * (x * x + z * z)
        m[:, 6] = s * (y * z - w * x)
        m[:, 7] = t[1]
        m[:, 8] = s * (x * z - w * y)
        m[:, 9] = s * (y * z + w * x)
        m[:, 10] = 1.0 - s * (x * x + y * y)
        m[:, 11] = t[2]
        ok = np.isfinite(n) & (n > 0) & np.isfinite(t[0]) & np.isfinite(t[1]) & np.isfinite(t[2])
    return m, ok


def pose_at(pose_time, pose, tau, max_gap_ns):
    """``(m (n, 12) float64, valid (n,) bool)``: the pose at each integer time of ``tau``; an invalid pose is twelve words
    0x7ff8000000000000."""
    pose_time, tau = np.asarray(pose_time, np.int64), np.asarray(tau, np.int64).reshape(-1)
    pose = np.asarray(pose, np.float64).reshape(len(pose_time), 7)
    j, num, den, valid = bracket(pose_time, tau, max_gap_ns)
    jc = np.maximum(j, 0)
    fi = fraction(np.where(valid, num, 0), np.where(valid, den, 1))
    f = fi.astype(np.float64) * 2.0 ** -32
    m, ok = blend(pose[jc], pose[jc + 1], f)
    valid = valid & ok
    m.view(np.uint64)[~valid] = NAN64_WORD
    return m, valid


def times_valid(pose_time):
    pose_time = np.asarray(pose_time, np.int64)
    return bool(len(pose_time) >= 2 and (pose_time[:-1] < pose_time[1:]).all())


def offsets_valid(offsets, num_rows):
    offsets = np.asarray(offsets, np.int64)
    return bool(offsets[0] >= 0 and offsets[-1] <= num_rows and not (np.diff(offsets) < 0).any())


def interp_reference(pose_time, pose, query_time, max_gap_ns):
    """``(pose_out (Q, 12), status (Q,) int32)`` of epcnet_pose_interp."""
    query_time = np.asarray(query_time, np.int64).reshape(-1)
    if not times_valid(pose_time):
        out = np.empty((len(query_time), 12))
        out.view(np.uint64)[:] = NAN64_WORD
        return out, np.full(len(query_time), NO_POSE, np.int32)
    m, valid = pose_at(pose_time, pose, query_time, max_gap_ns)
    return m, np.where(valid, 0, NO_POSE).astype(np.int32)


def row_transform(rows, mp, ms):
    """(n, 3) float64 q of float32 rows (n, 3), their own poses mp (n, 12) and their scan's pose ms (12,) or (n, 12)."""
    x, y, z = (np.asarray(rows, np.float32)[:, c].astype(np.float64) for c in range(3))
    ms = np.broadcast_to(np.asarray(ms, np.float64), mp.shape)
    with np.errstate(all="ignore"):
        w = [((mp[:, 4 * a] * x + mp[:, 4 * a + 1] * y) + mp[:, 4 * a + 2] * z) + (mp[:, 4 * a + 3] - ms[:, 4 * a + 3]) for a in range(3)]
        return np.stack([(ms[:, a] * w[0] + ms[:, 4 + a] * w[1]) + ms[:, 8 + a] * w[2] for a in range(3)], 1)


def deskew_reference(points, offsets, scan_time, pose_time, pose, point_dt, max_gap_ns, num_rows=None):
    """Every output of epcnet_scan_deskew as a dict: ``scan_pose`` (S, 12), ``status`` (S,) int32, ``failed``, and -- with ``point_dt``
    -- ``points_out``: the rows [offsets[0], offsets[S]) the call writes (a whole-call failure writes none: an empty array) and
    ``first``, the row they begin at."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    offsets = np.asarray(offsets, np.int64)
    scan_time = np.asarray(scan_time, np.int64).reshape(-1)
    S = len(offsets) - 1
    num_rows = len(points) if num_rows is None else num_rows
    if not (times_valid(pose_time) and offsets_valid(offsets, num_rows)):
        sp = np.empty((S, 12))
        sp.view(np.uint64)[:] = NAN64_WORD
        return dict(scan_pose=sp, status=np.full(S, NO_POSE, np.int32), failed=True, points_out=np.zeros((0, 3), np.float32), first=0)
    sp, s_ok = pose_at(pose_time, pose, scan_time, max_gap_ns)
    status = np.where(s_ok, 0, NO_POSE).astype(np.int32)
    out = dict(scan_pose=sp, status=status, failed=False)
    if point_dt is None:
        return out
    first, last = int(offsets[0]), int(offsets[-1])
    rows = points[first:last]
    scan_of = np.repeat(np.arange(S), np.diff(offsets))
    tau = scan_time[scan_of] + np.asarray(point_dt, np.int32)[first:last].astype(np.int64)
    mp, p_ok = pose_at(pose_time, pose, tau, max_gap_ns)
    q = row_transform(rows, mp, sp[scan_of])
    with np.errstate(all="ignore"):
        res = q.astype(np.float32)
    keep = s_ok[scan_of] & p_ok & np.isfinite(rows).all(1)
    res.view(np.uint32)[~keep] = NAN_WORD
    part = np.zeros(S, bool)
    np.logical_or.at(part, scan_of, ~p_ok)
    status[s_ok & part] |= PART_POSE
    out.update(points_out=res, first=first)
    return out


# ---- seeded scenes ------------------------------------------------------------------------------------------------------------------------
def quat_of_yaw(yaw):
    yaw = np.asarray(yaw, np.float64)
    zero = np.zeros_like(yaw)
    return np.stack([np.cos(yaw / 2), zero, zero, np.sin(yaw / 2)], -1)


def odometry(seed, num_poses, period_ns=10_000_000, t_start=1_700_000_000_000_000_000, speed=10.0, yaw_rate=0.5, wobble=0.02, jitter_ns=0):
    """``(pose_time (P,) int64, pose (P, 7) float64)``: a seeded drive near submap_ref.ORIGIN, ``period_ns`` between poses (plus a seeded
    jitter below ``jitter_ns``), general rotations: a seeded quaternion for the whole drive turned by the yaw and perturbed per pose.  The
    quaternions are unit only up to ``wobble``-sized terms on purpose: the definition never normalises."""
    rng = np.random.default_rng([seed, num_poses, 5])
    steps = np.full(num_poses, period_ns, np.int64)
    if jitter_ns:
        steps = steps + rng.integers(0, jitter_ns, size=num_poses)
    pose_time = t_start + np.cumsum(steps) - steps[0]
    secs = (pose_time - pose_time[0]).astype(np.float64) * 1e-9
    q0 = rng.normal(size=4)
    q0 /= np.linalg.norm(q0)
    yaw = yaw_rate * secs
    heading = rng.uniform(0, 2 * np.pi)
    pose = np.zeros((num_poses, 7))
    pose[:, 0] = SR.ORIGIN[0] + speed * secs * np.cos(heading) + 0.01 * rng.normal(size=num_poses)
    pose[:, 1] = SR.ORIGIN[1] + speed * secs * np.sin(heading) + 0.01 * rng.normal(size=num_poses)
    pose[:, 2] = SR.ORIGIN[2] + 0.01 * rng.normal(size=num_poses)
    qy = quat_of_yaw(yaw)
    # q = q0 * qy (Hamilton), then the perturbation
    w0, x0, y0, z0 = q0
    pose[:, 3] = w0 * qy[:, 0] - z0 * qy[:, 3]
    pose[:, 4] = x0 * qy[:, 0] + y0 * qy[:, 3]
    pose[:, 5] = y0 * qy[:, 0] - x0 * qy[:, 3]
    pose[:, 6] = z0 * qy[:, 0] + w0 * qy[:, 3]
    pose[:, 3:] += wobble * rng.normal(size=(num_poses, 4))
    return pose_time.astype(np.int64), pose


def sweep_dt(seed, rows, sweep_ns=100_000_000):
    """(rows,) int32: stamps that rise over one sweep, as a spinning sensor's do, with seeded sub-steps."""
    rng = np.random.default_rng([seed, rows, 9])
    return np.sort(rng.integers(0, sweep_ns, size=rows)).astype(np.int32)


def quat_matrix_exact(q):
    """Rotation of a quaternion, normalised in float64 (the tests' textbook form; not the definition)."""
    return SR.quat_matrix(q)


def physical_scene(seed, rows, yaw_per_interval, speed=10.0, period_ns=10_000_000, sweep_ns=100_000_000, extent=40.0):
    """A sensor on a straight line with a constant yaw rate sees static world points, each in the sensor frame of its own time.
    Poses are sampled exactly every ``period_ns``.  Returns a dict: pose_time, pose, scan_time (1,), offsets, point_dt, points (the
    observations, float32), truth (the points in the sweep-start frame, float64), ranges."""
    rng = np.random.default_rng([seed, rows, 13])
    P = sweep_ns // period_ns + 3
    t_start = 1_700_000_000_000_000_000
    pose_time = t_start + period_ns * np.arange(P, dtype=np.int64)
    rate = yaw_per_interval / (period_ns * 1e-9)

    def state(ns):
        s = np.asarray(ns, np.float64) * 1e-9
        t = np.stack([SR.ORIGIN[0] + speed * s, SR.ORIGIN[1] + 0 * s, SR.ORIGIN[2] + 0 * s], -1)
        return t, rate * s

    t_k, yaw_k = state(pose_time - t_start)
    pose = np.concatenate([t_k, quat_of_yaw(yaw_k)], 1)
    scan_ns = period_ns                                 # the sweep starts on the second knot
    dt = np.sort(rng.integers(0, sweep_ns, size=rows)).astype(np.int32)
    dt[0] = 0
    # in the sweep-start frame, 2 m to `extent` away: the float64 knots are rounded at 5.7e6 (1e-9 m), which the bound's range terms cover
    radius, angle = rng.uniform(2.0, extent, size=rows), rng.uniform(0, 2 * np.pi, size=rows)
    truth = np.stack([radius * np.cos(angle), radius * np.sin(angle), rng.uniform(-3.0, 3.0, size=rows)], 1)
    t_s, yaw_s = state(scan_ns)
    c, s = np.cos(yaw_s), np.sin(yaw_s)
    t_p, yaw_p = state(scan_ns + dt.astype(np.int64))
    cp, spn = np.cos(yaw_p), np.sin(yaw_p)
    # world - t_p, with the UTM-sized translations subtracted first (the world point itself is never rounded at 5.7e6)
    rel = truth @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]).T + (t_s - t_p)
    obs = np.stack([cp * rel[:, 0] + spn * rel[:, 1], -spn * rel[:, 0] + cp * rel[:, 1], rel[:, 2]], 1)      # R_p^T (world - t_p)
    return dict(pose_time=pose_time, pose=pose, scan_time=np.array([t_start + scan_ns], np.int64), offsets=np.array([0, rows], np.int32),
                point_dt=dt, points=obs.astype(np.float32), truth=truth, ranges=np.linalg.norm(truth, axis=1))
