"""numpy restatement of epcnet_ground_remove (include/epcnet_scans.h) -- the kernels' contract -- and the seeded scenes its tests and
scripts/time_ground.py share.  float32 with every operation rounded once, integer counts: the kernels' output equals this bit for bit."""
import numpy as np

F = np.float32
NO_GROUND = 8
NAN_WORD = 0x7fc00000
DEFAULTS = dict(threshold=0.2, max_tilt_deg=15.0, hypotheses=256, draws=8, min_share=0.05, max_z=float("inf"), seed=0)


def mix(x):
    """mix of include/epcnet_poses.h on a uint32 array."""
    x = np.asarray(x, np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def cos2_of(max_tilt_deg):
    """cos^2 of the largest tilt: computed in double, rounded once."""
    return F(np.cos(np.deg2rad(np.float64(max_tilt_deg))) ** 2)


def candidate_rows(M, hypotheses, draws, seed):
    """(H, 3, K) int64: the candidate rows of every vertex of every hypothesis in a scan of M rows."""
    seed = int(seed) & 0xffffffffffffffff
    s = mix(np.uint32(seed & 0xffffffff))
    s = mix(s ^ np.uint32(seed >> 32))
    sh = mix(s ^ np.arange(hypotheses, dtype=np.uint32))
    c = np.arange(3 * draws, dtype=np.uint32).reshape(3, draws)
    return ((mix(sh[:, None, None] ^ c[None]).astype(np.uint64) * np.uint64(M)) >> np.uint64(32)).astype(np.int64)


def planes(p, hypotheses, draws, threshold, cos2_tilt, max_z, seed):
    """-> n (H, 3), d0 (H,), thr (H,) float32 and valid (H,) bool for the scan p (M, 3) float32, M > 0."""
    rows = candidate_rows(len(p), hypotheses, draws, seed)
    cand = p[rows]                                                   # (H, 3, K, 3)
    fin = np.isfinite(cand).all(-1)
    k = np.argmin(np.where(fin, cand[..., 2], F(np.inf)), axis=-1)   # the first of the smallest: ties to the smaller k
    v = np.take_along_axis(cand, k[..., None, None], axis=2)[:, :, 0, :]
    valid = fin.any(-1).all(-1)
    v = np.where(valid[:, None, None], v, F(0))
    with np.errstate(all="ignore"):
        u, w = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
        n = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
        nn = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        n = np.where((n[:, 2] < 0)[:, None], -n, n)
        d0 = (n[:, 0] * v[:, 0, 0] + n[:, 1] * v[:, 0, 1]) + n[:, 2] * v[:, 0, 2]
        valid = valid & (nn >= F(1e-12)) & (nn <= F(3e38)) & (n[:, 2] * n[:, 2] >= F(cos2_tilt) * nn) & (d0 <= F(max_z) * n[:, 2])
        thr = (F(threshold) * F(threshold)) * nn
    assert n.dtype == F and d0.dtype == F and thr.dtype == F
    return n, d0, thr, valid


def residual(n, d0, p):
    """e of every row of p (M, 3) for the planes n (H, 3), d0 (H,): (H, M) float32."""
    with np.errstate(all="ignore"):
        return ((n[:, 0:1] * p[None, :, 0] + n[:, 1:2] * p[None, :, 1]) + n[:, 2:3] * p[None, :, 2]) - d0[:, None]


def remove_ground_ref(scan, threshold=0.2, max_tilt_deg=15.0, hypotheses=256, draws=8, min_share=0.05, max_z=float("inf"), seed=0):
    """-> (out (M, 3) float32, status, plane (4,) float32, info [4])"""
    p = np.ascontiguousarray(np.asarray(scan, F).reshape(-1, 3))
    nan_plane = np.full(4, np.nan, F)
    M = len(p)
    if M > (1 << 20):
        return p.copy(), NO_GROUND, nan_plane, [0, 0, 0, 0]
    finite = np.isfinite(p).all(1)
    info = [int(finite.sum()), 0, -1, 0]
    if M == 0:
        return p.copy(), NO_GROUND, nan_plane, info
    n, d0, thr, valid = planes(p, hypotheses, draws, threshold, cos2_of(max_tilt_deg), max_z, seed)
    info[1] = int(valid.sum())
    if not valid.any():
        return p.copy(), NO_GROUND, nan_plane, info
    pf = p[finite]
    score = np.zeros(hypotheses, np.int64)
    with np.errstate(all="ignore"):
        for a in range(0, len(pf), 8192):                            # (row chunks: the temporaries stay in cache)
            e = residual(n, d0, pf[a:a + 8192])
            score += (e * e <= thr[:, None]).sum(1)
    score = np.where(valid, score, -1)
    h = int(np.argmax(score))                                        # the first of the largest: ties to the smaller h
    info[2:] = [h, int(score[h])]
    if not (score[h] >= 3 and F(score[h]) >= F(min_share) * F(info[0])):
        return p.copy(), NO_GROUND, nan_plane, info
    with np.errstate(all="ignore"):
        e = residual(n[h:h + 1], d0[h:h + 1], p)[0]
        gone = finite & ((e < 0) | (e * e <= thr[h]))
    out = p.copy()
    out.view(np.uint32)[gone] = NAN_WORD
    return out, 0, np.array([n[h, 0], n[h, 1], n[h, 2], d0[h]], F), info


def reference_batch(scans, **kw):
    """The restatement on every scan: (out (total, 3) float32, status (B,) int32, plane (B, 4) float32, info (B, 4) int32)."""
    res = [remove_ground_ref(s, **kw) for s in scans]
    out = np.concatenate([r[0] for r in res], 0) if res else np.zeros((0, 3), F)
    return (out, np.array([r[1] for r in res], np.int32), np.stack([r[2] for r in res]).astype(F).reshape(-1, 4),
            np.array([r[3] for r in res], np.int32).reshape(-1, 4))


def family(seed, with_truth=False):
    """A seeded raw scan over +-40 m: 4 000-20 000 ground rows on a plane through z = -1.8 tilted up to +-5 degrees about both axes (sigma
    3 cm), 15 000-40 000 object rows 0.5-12 m above that plane, 0-25 000 rows on a vertical wall, 1 % of all rows pushed 1-6 m down, 10 %
    of all rows with one coordinate NaN, randomly permuted.  with_truth: also the unit normal and offset (n, d) of the true plane
    (float64)."""
    rng = np.random.default_rng(seed)
    g, o, w = int(rng.integers(4000, 20001)), int(rng.integers(15000, 40001)), int(rng.integers(0, 25001))
    ta, tb = np.tan(np.deg2rad(rng.uniform(-5, 5, 2)))
    height = lambda xy: -1.8 + ta * xy[:, 0] + tb * xy[:, 1]
    gxy = rng.uniform(-40, 40, (g, 2))
    ground = np.column_stack([gxy, height(gxy) + rng.normal(0.0, 0.03, g)])
    oxy = rng.uniform(-40, 40, (o, 2))
    objects = np.column_stack([oxy, height(oxy) + rng.uniform(0.5, 12.0, o)])
    wy = rng.uniform(-40, 40, w)
    wxy = np.column_stack([np.full(w, rng.uniform(-30, 30)) + rng.normal(0.0, 0.03, w), wy])
    wall = np.column_stack([wxy, height(wxy) + rng.uniform(0.0, 8.0, w)])
    p = np.concatenate([ground, objects, wall], 0)
    M = len(p)
    down = rng.choice(M, M // 100, replace=False)
    p[down, 2] -= rng.uniform(1.0, 6.0, len(down))
    bad = rng.choice(M, M // 10, replace=False)
    p[bad, rng.integers(0, 3, len(bad))] = np.nan
    p = p[rng.permutation(M)].astype(F)
    if not with_truth:
        return p
    n = np.array([-ta, -tb, 1.0])
    s = np.linalg.norm(n)
    return p, n / s, -1.8 / s


def wall_only(M, seed):
    """M rows on one exactly vertical wall (x = 7): every normal has n_z = 0, no hypothesis is valid."""
    rng = np.random.default_rng(seed)
    return np.column_stack([np.full(M, 7.0), rng.uniform(-40, 40, M), rng.uniform(0, 8, M)]).astype(F)


def cube(M, seed):
    """M rows uniform in a 40 m cube: no slab of 0.4 m holds a twentieth of them."""
    return np.random.default_rng(seed).uniform(-20, 20, (M, 3)).astype(F)


def roofed(seed):
    """A ground plane at z = -1.8 (2 500 rows) under a much larger roof plane at z = +3 (30 000 rows), 500 rows above the roof: the roof
    is the largest near-horizontal plane, the ground the largest one below the sensor."""
    rng = np.random.default_rng(seed)
    flat = lambda m, z: np.column_stack([rng.uniform(-30, 30, (m, 2)), np.full(m, z) + rng.normal(0.0, 0.03, m)])
    above = np.column_stack([rng.uniform(-30, 30, (500, 2)), rng.uniform(3.5, 6.0, 500)])
    p = np.concatenate([flat(2500, -1.8), flat(30000, 3.0), above], 0).astype(F)
    return p[rng.permutation(len(p))]
