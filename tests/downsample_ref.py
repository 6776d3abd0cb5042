"""numpy restatement of epc_grid_downsample (include/epcnet.h) -- the kernel's contract -- and the seeded scenes its tests and
scripts/time_downsample.py share.  Integer arithmetic behind the quantisation: the kernel's output equals this bit for bit."""
import numpy as np

F = np.float32


def _u(p, lo, e, R):
    t = (p - lo) * (F(R) / e)
    return np.minimum((t * F(4096)).astype(np.int64), R * 4096 - 1)


def _keys(u):
    c = u >> 12
    return (c[:, 2] * 1024 + c[:, 1]) * 1024 + c[:, 0]


def grid_downsample_ref(p, N, normalize=True):
    """-> (out (N,3) float32 or None, status, info[4])"""
    p = np.asarray(p, F).reshape(-1, 3)
    p = p[np.isfinite(p).all(1)]
    info = [len(p), 0, 0, 0]
    if len(p) < N:
        return None, 4, info
    lo = p.min(0)
    e = (p.max(0) - lo).max()
    D = lambda R: np.unique(_keys(_u(p, lo, e, R))).size
    if not e > 0 or D(1024) < N:
        return None, 4, info
    a, b = 1, 1024
    while b - a > 1:
        m = (a + b) // 2
        if D(m) >= N:
            b = m
        else:
            a = m
    u = _u(p, lo, e, b)
    keys, inv, cnt = np.unique(_keys(u), return_inverse=True, return_counts=True)
    info[1:3] = [b, keys.size]
    if keys.size > 2 * N:
        return None, 4, info
    S = np.zeros((keys.size, 3), np.int64)
    np.add.at(S, inv, u & 4095)
    order = np.lexsort((keys, -cnt))[:N]
    keep = np.sort(order)
    info[3] = int(cnt[order[-1]])
    k = keys[keep]
    c = np.stack([k & 1023, (k >> 10) & 1023, k >> 20], 1)
    q = c * 4096 + S[keep] // cnt[keep][:, None]
    if normalize:
        d = q - q.sum(0) // N
        return d.astype(F) * (F(1) / F(np.abs(d).max())), 0, info
    return lo + q.astype(F) * (e / F(b * 4096)), 0, info


def scene(M, seed):
    """A LiDAR-like scan of M points in metres over +-40 m: half of them on a ground plane (sigma 3 cm), a quarter each on two
    walls.  Seeded."""
    rng = np.random.default_rng(seed)
    g, w = M // 2, M // 4
    ground = np.stack([rng.uniform(-40, 40, g), rng.uniform(-40, 40, g), rng.normal(0.0, 0.03, g)], 1)
    wall1 = np.stack([rng.uniform(-40, 40, w), np.full(w, 12.0) + rng.normal(0.0, 0.03, w), rng.uniform(0, 8, w)], 1)
    w2 = M - g - w
    wall2 = np.stack([np.full(w2, -15.0) + rng.normal(0.0, 0.03, w2), rng.uniform(-40, 40, w2), rng.uniform(0, 8, w2)], 1)
    p = np.concatenate([ground, wall1, wall2], 0).astype(F)
    return p[rng.permutation(M)]


def lattice(k):
    """The k x k x k unit lattice, (k^3, 3) float32."""
    a = np.arange(k, dtype=F)
    return np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)


def reference_batch(scans, N, normalize=True):
    """The restatement on every scan: (xyz (B, N, 3) float32 with NaN rows for a failed scan, status (B,) int32, info (B, 4) int32)."""
    xyz = np.full((len(scans), N, 3), np.nan, F)
    status = np.zeros(len(scans), np.int32)
    info = np.zeros((len(scans), 4), np.int32)
    for i, s in enumerate(scans):
        out, status[i], info[i] = grid_downsample_ref(s, N, normalize)
        if out is not None:
            xyz[i] = out
    return xyz, status, info


def split_clusters(seed=0):
    """Tight 8-corner clusters on a 1/16 lattice inside the unit cube: a grid too coarse to split them sees one cell per cluster
    (fewer than 32), the next probe of the bisection splits them all at once -- with seed 0, D(R*) = 190 > 2 * 32 at N = 32."""
    rng = np.random.default_rng(seed)
    k = int(rng.integers(10, 31))
    delta = float(rng.choice([0.01, 0.02, 0.03, 0.05]))
    cen = np.unique(rng.integers(0, 16, (k, 3)).astype(F) / 16, axis=0)
    corners = np.stack(np.meshgrid([0, 1], [0, 1], [0, 1], indexing="ij"), -1).reshape(-1, 3) * delta
    p = (cen[:, None, :] + corners[None]).reshape(-1, 3)
    return np.concatenate([p, [[0, 0, 0], [1, 1, 1]]]).astype(F)
