"""The definition of include/epcnet_pairs.h in numpy, written from the header's text: the correspondence pass in elementwise float32 in
the stated association, the 17 sums by the two-line pairing loop over 4096 leaves, Horn's matrix, cyclic Jacobi and the quaternion in
scalar float64 Python (a Python float is an IEEE double and every operator rounds once; ``math.sqrt`` is correctly rounded).  Nothing
here calls the library.  ``register_reference`` is the whole entry; the pieces are public for tests/test_register_cpu.py."""
import math

import numpy as np

NO_PAIR, NO_FIT = 256, 512
LEAVES = 4096
SWEEPS = 6                       # the header's count
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
F32_MAX = np.float32(np.finfo(np.float32).max)
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64)


def present(cloud):
    """The rows without a non-finite word."""
    return np.isfinite(np.asarray(cloud, np.float32)).all(1)


def gate2_of(max_dist):
    with np.errstate(over="ignore"):
        g = np.float32(float(max_dist) * float(max_dist))
    return min(g, F32_MAX)


def transform(m, rows):
    """p = fl32(((m[4c] x + m[4c+1] y) + m[4c+2] z) + m[4c+3]) of float32 rows (k, 3), the arithmetic in float64."""
    x, y, z = (rows[:, c].astype(np.float64) for c in range(3))
    with np.errstate(all="ignore"):
        return np.stack([(((m[4 * c] * x + m[4 * c + 1] * y) + m[4 * c + 2] * z) + m[4 * c + 3]).astype(np.float32) for c in range(3)], 1)


def nearest(p, target, t_ok, block=256):
    """For float32 rows p (k, 3): (row of the nearest present target row, its float32 d2); NaN counts as +Inf, ties go to the lower row."""
    j = np.zeros(len(p), np.int64)
    best = np.full(len(p), np.inf, np.float32)
    q = np.asarray(target, np.float32)
    for a in range(0, len(p), block):
        b = p[a:a + block]
        with np.errstate(all="ignore"):
            dx, dy, dz = (b[:, None, c] - q[None, :, c] for c in range(3))
            d2 = (dx * dx + dy * dy) + dz * dz
        d2[np.isnan(d2)] = np.inf
        d2[:, ~t_ok] = np.inf
        j[a:a + block] = d2.argmin(1)                                   # the first of equal minima
        best[a:a + block] = d2[np.arange(len(b)), j[a:a + block]]
    return j, best


def tree_sum(v):
    """The normative order: adjacent pairing until one value is left.  v (..., 2^k) float64."""
    v = np.asarray(v, np.float64)
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def pass_sums(m, source, target, gate2):
    """One correspondence pass under the pose m[12] -> the 17 sums (float64)."""
    source, target = np.asarray(source, np.float32), np.asarray(target, np.float32)
    s_ok, t_ok = present(source), present(target)
    leaves = np.zeros((17, LEAVES), np.float64)
    rows = np.nonzero(s_ok)[0]
    if rows.size:
        j, d2 = nearest(transform(m, source[rows]), target, t_ok)
        acc = d2 <= gate2
        rows, j, d2 = rows[acc], j[acc], d2[acc]
        s, q = source[rows].astype(np.float64), target[j].astype(np.float64)
        leaves[0, rows] = 1.0
        for a in range(3):
            leaves[1 + a, rows] = s[:, a]
            leaves[4 + a, rows] = q[:, a]
            for b in range(3):
                leaves[7 + 3 * a + b, rows] = s[:, a] * q[:, b]          # exact: two float32 factors
        leaves[16, rows] = d2.astype(np.float64)
    return tree_sum(leaves)


def horn_matrix(sums):
    m = float(sums[0])
    ss, sq = [float(v) for v in sums[1:4]], [float(v) for v in sums[4:7]]
    M = [[float(sums[7 + 3 * a + b]) - (ss[a] * sq[b]) / m for b in range(3)] for a in range(3)]
    (xx, xy, xz), (yx, yy, yz), (zx, zy, zz) = M
    N = [[0.0] * 4 for _ in range(4)]
    N[0][0] = (xx + yy) + zz
    N[1][1] = (xx - yy) - zz
    N[2][2] = (yy - xx) - zz
    N[3][3] = (zz - xx) - yy
    N[0][1] = N[1][0] = yz - zy
    N[0][2] = N[2][0] = zx - xz
    N[0][3] = N[3][0] = xy - yx
    N[1][2] = N[2][1] = xy + yx
    N[1][3] = N[3][1] = zx + xz
    N[2][3] = N[3][2] = yz + zy
    return N


def jacobi_sweep(A, V):
    """One sweep over the six pairs, in place."""
    for p, q in PAIRS:
        apq = A[p][q]
        if apq == 0.0:
            continue
        theta = (A[q][q] - A[p][p]) / (2.0 * apq)
        t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
        c = 1.0 / math.sqrt(t * t + 1.0)
        s = t * c
        h = t * apq
        A[p][p] -= h
        A[q][q] += h
        A[p][q] = A[q][p] = 0.0
        for r in range(4):
            if r != p and r != q:
                g, f = A[r][p], A[r][q]
                A[r][p] = A[p][r] = c * g - s * f
                A[r][q] = A[q][r] = s * g + c * f
        for r in range(4):
            g, f = V[r][p], V[r][q]
            V[r][p] = c * g - s * f
            V[r][q] = s * g + c * f


def jacobi(N, sweeps=SWEEPS):
    """Cyclic Jacobi on a symmetric 4x4 (lists of Python floats) -> (A, V): the diagonal of A holds the eigenvalues, the columns of V
    the eigenvectors."""
    A = [[float(v) for v in row] for row in N]
    V = [[1.0 if r == c else 0.0 for c in range(4)] for r in range(4)]
    for _ in range(sweeps):
        jacobi_sweep(A, V)
    return A, V


def rotation_of(quat):
    """[R] (9 floats, row-major) from the UNNORMALISED quaternion (w, x, y, z), as include/epcnet_stamps.h builds it."""
    w, x, y, z = quat
    nn = ((w * w + x * x) + y * y) + z * z
    u = 2.0 / nn if nn != 0.0 else math.nan
    return [1.0 - u * (y * y + z * z), u * (x * y - w * z), u * (x * z + w * y),
            u * (x * y + w * z), 1.0 - u * (x * x + z * z), u * (y * z - w * x),
            u * (x * z - w * y), u * (y * z + w * x), 1.0 - u * (x * x + y * y)]


def dominant(A, V):
    k = 0
    for c in range(1, 4):
        if A[c][c] > A[k][k]:
            k = c
    return [V[r][k] for r in range(4)]


def solve(sums, sweeps=SWEEPS):
    """The pose [R | t] (12 float64) of the 17 sums, or None where it holds a non-finite word."""
    try:
        A, V = jacobi(horn_matrix(sums), sweeps)
        R = rotation_of(dominant(A, V))
        m = float(sums[0])
        sm, qm = [float(v) / m for v in sums[1:4]], [float(v) / m for v in sums[4:7]]
        pose = []
        for c in range(3):
            pose += R[3 * c:3 * c + 3] + [qm[c] - ((R[3 * c] * sm[0] + R[3 * c + 1] * sm[1]) + R[3 * c + 2] * sm[2])]
    except (OverflowError, ZeroDivisionError, ValueError):     # Python raises where IEEE arithmetic gives Inf or NaN
        return None
    pose = np.array(pose, np.float64)
    return pose if np.isfinite(pose).all() else None


def register_pair(source, target, seeds, gate2, iterations, min_pairs, sums_of=None):
    """One valid pair -> (pose (12,), fit (2,), info [4], status).  ``sums_of(m)``: the pass under pose m (default pass_sums)."""
    sums_of = sums_of or (lambda m: pass_sums(m, source, target, gate2))
    ns, nt = int(present(source).sum()), int(present(target).sum())
    nan = np.full(12, np.nan), np.full(2, np.nan)

    def flagged(bit):
        return nan[0], nan[1], [-1, 0, ns, nt], bit

    best, best_sums = -1, None
    for h, seed in enumerate(seeds):
        if not np.isfinite(seed).all():
            continue
        s = sums_of(seed)
        if best < 0 or s[0] > best_sums[0] or (s[0] == best_sums[0] and s[16] < best_sums[16]):
            best, best_sums = h, s
    if best < 0:
        return flagged(NO_PAIR)
    pose, sums = np.array(seeds[best], np.float64), best_sums
    for it in range(iterations):
        if it:
            sums = sums_of(pose)
        if sums[0] < min_pairs:
            return flagged(NO_FIT)
        pose = solve(sums)
        if pose is None:
            return flagged(NO_FIT)
    if iterations:
        sums = sums_of(pose)
    if sums[0] < min_pairs:
        return flagged(NO_FIT)
    m = float(sums[0])
    return pose, np.array([float(sums[16]) / m, m / ns]), [best, int(m), ns, nt], 0


def register_reference(clouds, pairs, seeds, max_dist, iterations, min_pairs, memo=None):
    """The whole entry: clouds (C, n, 3) float32, pairs (P, 2), seeds (P, H, 12) float64 or None -> pose (P, 12), fit (P, 2) float64, info
    (P, 4), status (P,) int32.  ``memo`` (a dict) keeps passes by (source, target, pose, gate): calls on the same clouds share them."""
    clouds = np.asarray(clouds, np.float32)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    P, C = len(pairs), len(clouds)
    gate2 = gate2_of(max_dist)
    pose, fit = np.full((P, 12), np.nan), np.full((P, 2), np.nan)
    info, status = np.zeros((P, 4), np.int32), np.zeros(P, np.int32)
    for i, (s, t) in enumerate(pairs):
        if not (0 <= s < C and 0 <= t < C):
            info[i], status[i] = [-1, 0, 0, 0], NO_PAIR
            continue
        hyp = IDENTITY[None] if seeds is None else np.asarray(seeds[i], np.float64).reshape(-1, 12)

        def sums_of(m, s=int(s), t=int(t)):
            if memo is None:
                return pass_sums(m, clouds[s], clouds[t], gate2)
            key = (s, t, np.asarray(m, np.float64).tobytes(), float(gate2))
            if key not in memo:
                memo[key] = pass_sums(m, clouds[s], clouds[t], gate2)
            return memo[key]

        pose[i], fit[i], info[i], status[i] = register_pair(clouds[s], clouds[t], hyp, gate2, iterations, min_pairs, sums_of)
    return pose, fit, info, status


# ---- scenes and poses for the tests -------------------------------------------------------------------------------------------------
def pose_of(yaw_deg=0.0, pitch_deg=0.0, roll_deg=0.0, t=(0.0, 0.0, 0.0)):
    """[R | t] (12,) float64, R = Rz(yaw) Ry(pitch) Rx(roll)."""
    a, b, c = (math.radians(v) for v in (yaw_deg, pitch_deg, roll_deg))
    Rz = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
    Ry = np.array([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]])
    Rx = np.array([[1, 0, 0], [0, math.cos(c), -math.sin(c)], [0, math.sin(c), math.cos(c)]])
    return np.concatenate([Rz @ Ry @ Rx, np.asarray(t, np.float64)[:, None]], 1).reshape(12)


def apply_pose(m, rows):
    m = np.asarray(m, np.float64).reshape(3, 4)
    return np.asarray(rows, np.float64) @ m[:, :3].T + m[:, 3]


def invert_pose(m):
    m = np.asarray(m, np.float64).reshape(3, 4)
    return np.concatenate([m[:, :3].T, -(m[:, :3].T @ m[:, 3])[:, None]], 1).reshape(12)


def pose_error(got, want):
    """(rotation angle in radians, translation distance) between two [R | t].  The angle from the chord |Rg - Rw|_F = 2 sqrt(2) sin(a / 2):
    acos of the trace loses everything below 1e-8."""
    g, w = np.asarray(got, np.float64).reshape(3, 4), np.asarray(want, np.float64).reshape(3, 4)
    chord = float(np.linalg.norm(g[:, :3] - w[:, :3])) / (2.0 * math.sqrt(2.0))
    return 2.0 * math.asin(min(1.0, chord)), float(np.linalg.norm(g[:, 3] - w[:, 3]))


def structured_scene(seed, n):
    """n float64 points of a street-like scene with no symmetry: a ground plane, two walls at different distances and angles, three boxes
    of different sizes -- planes and boxes, not a uniform blob.  About 40 m x 30 m x 6 m."""
    rng = np.random.default_rng([seed, n])
    parts = []
    k = n // 8
    g = rng.uniform([-20, -15, 0], [20, 15, 0], size=(n - 7 * k, 3))
    g[:, 2] = 0.02 * g[:, 0]                                            # a slightly tilted ground
    parts.append(g)
    w = rng.uniform([-20, 0, 0], [20, 0, 6], size=(2 * k, 3))
    w[:, 1] = 12.0 + 0.1 * w[:, 0]                                      # a long wall, slightly skew
    parts.append(w)
    w = rng.uniform([0, -15, 0], [0, 5, 4], size=(k, 3))
    w[:, 0] = -17.0                                                     # a shorter wall across
    parts.append(w)
    for centre, size in (((5.0, -6.0, 1.0), (4.0, 2.0, 2.0)), ((-8.0, 3.0, 1.5), (2.0, 5.0, 3.0)), ((12.0, 6.0, 0.5), (1.5, 1.5, 1.0))):
        b = rng.uniform(-0.5, 0.5, size=(k, 3))
        face = rng.integers(0, 3, size=k)
        b[np.arange(k), face] = rng.choice([-0.5, 0.5], size=k)         # on the surface of the box
        parts.append(b * size + centre)
    b = rng.uniform([-3, -12, 0], [3, -9, 5], size=(k, 3))              # a slanted slab
    b[:, 1] += 0.5 * b[:, 2]
    parts.append(b)
    pts = np.concatenate(parts)
    return pts[rng.permutation(len(pts))]
