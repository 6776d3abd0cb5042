"""The definition of include/epcnet_trajectory.h in numpy, written from the header's text: elementwise float64 in the stated association
(numpy rounds every operator once and never fuses a multiply with an add; ``numpy.sqrt`` is correctly rounded), the scans by the eight
Kogge-Stone steps over blocks of 256 nodes, the sums by adjacent pairing over 65 536 (dot products, the chain's cost) or 2^20 (the loops'
cost) leaves.  Nothing here calls the library.  ``relax_reference`` is the whole entry; the pieces are public for
tests/test_relax_cpu.py."""
import numpy as np

NO_EDGE = 1024
BLOCK = 256
NODE_LEAVES = 65536
LOOP_LEAVES = 1 << 20
NAN = np.float64(np.nan)


def tree_sum(v, leaves):
    """Adjacent pairing over `leaves` leaves, +0.0 behind the end of v."""
    w = np.zeros(leaves, np.float64)
    w[:len(v)] = v
    while len(w) > 1:
        w = w[0::2] + w[1::2]
    return w[0]


def _kogge_stone(s):
    """s (blocks, 256, k): the eight steps, each reading the previous step's values."""
    off = 1
    while off < BLOCK:
        t = s.copy()
        t[:, off:] = s[:, off:] + s[:, :-off]
        s = t
        off <<= 1
    return s


def scan6(v):
    """The inclusive scan of v (n, k) down the rows in the normative order."""
    n, k = v.shape
    nb = (n + BLOCK - 1) // BLOCK
    s = np.zeros((nb * BLOCK, k), np.float64)
    s[:n] = v
    s = _kogge_stone(s.reshape(nb, BLOCK, k))
    tot = np.zeros((1, BLOCK, k), np.float64)
    tot[0, :nb] = s[:, BLOCK - 1]
    inc = _kogge_stone(tot)[0]
    before = np.zeros((nb, k), np.float64)
    before[1:] = inc[:nb - 1]
    return (before[:, None, :] + s).reshape(nb * BLOCK, k)[:n]


def dot(x, y):
    """x . y of (n, 6) vectors: the leaf of a node, then the tree over 65 536 leaves."""
    leaf = ((((x[:, 0] * y[:, 0] + x[:, 1] * y[:, 1]) + x[:, 2] * y[:, 2]) + x[:, 3] * y[:, 3]) + x[:, 4] * y[:, 4]) + x[:, 5] * y[:, 5]
    return tree_sum(leaf, NODE_LEAVES)


def _d3(a0, a1, a2, b0, b1, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def tmul(X, Y):
    """X^T Y of (m, 3, 3) stacks: out[i][j] = (X[0][i] Y[0][j] + X[1][i] Y[1][j]) + X[2][i] Y[2][j]."""
    out = np.empty_like(X)
    for i in range(3):
        for j in range(3):
            out[:, i, j] = _d3(X[:, 0, i], X[:, 1, i], X[:, 2, i], Y[:, 0, j], Y[:, 1, j], Y[:, 2, j])
    return out


def residual(Ra, Rb, ca, cb, ZR, zt):
    """(r_t (m, 3), r_R (m, 3), E (m, 3, 3)) of edges (a, b, Z)."""
    dc = cb - ca
    rt = np.stack([_d3(Ra[:, 0, i], Ra[:, 1, i], Ra[:, 2, i], dc[:, 0], dc[:, 1], dc[:, 2]) - zt[:, i] for i in range(3)], 1)
    E = tmul(ZR, tmul(Ra, Rb))
    rR = np.stack([0.5 * (E[:, 2, 1] - E[:, 1, 2]), 0.5 * (E[:, 0, 2] - E[:, 2, 0]), 0.5 * (E[:, 1, 0] - E[:, 0, 1])], 1)
    return rt, rR, E


def edge_cost(rt, rR, wt, wr):
    return wt * ((rt[:, 0] * rt[:, 0] + rt[:, 1] * rt[:, 1]) + rt[:, 2] * rt[:, 2]) + wr * ((rR[:, 0] * rR[:, 0] + rR[:, 1] * rR[:, 1]) + rR[:, 2] * rR[:, 2])


def linearise(Ra, Rb, ca, cb, ZR, zt, wt, wr):
    """-> A, B, C (m, 3, 3): J = [[A, B], [0, C]]; b (m, 6) = J^T W r; cost (m)."""
    m = len(Ra)
    rt, rR, E = residual(Ra, Rb, ca, cb, ZR, zt)
    A = np.ascontiguousarray(Ra.transpose(0, 2, 1))
    x, y, z = cb[:, 0], cb[:, 1], cb[:, 2]
    B = np.empty((m, 3, 3))
    for i in range(3):
        B[:, i, 0] = A[:, i, 2] * y - A[:, i, 1] * z
        B[:, i, 1] = A[:, i, 0] * z - A[:, i, 2] * x
        B[:, i, 2] = A[:, i, 1] * x - A[:, i, 0] * y
    tr = (E[:, 0, 0] + E[:, 1, 1]) + E[:, 2, 2]
    G = np.empty((m, 3, 3))
    for i in range(3):
        for j in range(3):
            G[:, i, j] = tr - E[:, i, i] if i == j else -E[:, j, i]
    C = np.empty((m, 3, 3))
    for i in range(3):
        for j in range(3):
            C[:, i, j] = 0.5 * _d3(G[:, i, 0], G[:, i, 1], G[:, i, 2], Rb[:, j, 0], Rb[:, j, 1], Rb[:, j, 2])
    wrt, wrR = wt[:, None] * rt, wr[:, None] * rR
    b = np.empty((m, 6))
    for j in range(3):
        b[:, j] = _d3(A[:, 0, j], A[:, 1, j], A[:, 2, j], wrt[:, 0], wrt[:, 1], wrt[:, 2])
        b[:, 3 + j] = _d3(B[:, 0, j], B[:, 1, j], B[:, 2, j], wrt[:, 0], wrt[:, 1], wrt[:, 2]) + _d3(C[:, 0, j], C[:, 1, j], C[:, 2, j], wrR[:, 0], wrR[:, 1], wrR[:, 2])
    return A, B, C, b, edge_cost(rt, rR, wt, wr)


def apply_edge(A, B, C, wt, wr, d):
    """J^T W J d of (m, 6) differences d."""
    yt = [wt * (_d3(A[:, i, 0], A[:, i, 1], A[:, i, 2], d[:, 0], d[:, 1], d[:, 2]) + _d3(B[:, i, 0], B[:, i, 1], B[:, i, 2], d[:, 3], d[:, 4], d[:, 5]))
          for i in range(3)]
    yr = [wr * _d3(C[:, i, 0], C[:, i, 1], C[:, i, 2], d[:, 3], d[:, 4], d[:, 5]) for i in range(3)]
    u = np.empty_like(d)
    for j in range(3):
        u[:, j] = _d3(A[:, 0, j], A[:, 1, j], A[:, 2, j], yt[0], yt[1], yt[2])
        u[:, 3 + j] = _d3(B[:, 0, j], B[:, 1, j], B[:, 2, j], yt[0], yt[1], yt[2]) + _d3(C[:, 0, j], C[:, 1, j], C[:, 2, j], yr[0], yr[1], yr[2])
    return u


def block_matrix(A, B, C, wt, wr):
    """D = J^T W J (m, 6, 6): the upper triangle computed, the lower its mirror."""
    m = len(A)
    D = np.zeros((m, 6, 6))
    col = lambda M, j: (M[:, 0, j], M[:, 1, j], M[:, 2, j])
    for i in range(6):
        for j in range(i, 6):
            if i < 3:
                D[:, i, j] = wt * _d3(*col(A, i), *(col(A, j) if j < 3 else col(B, j - 3)))
            else:
                D[:, i, j] = wt * _d3(*col(B, i - 3), *col(B, j - 3)) + wr * _d3(*col(C, i - 3), *col(C, j - 3))
            D[:, j, i] = D[:, i, j]
    return D


def cholesky(D):
    """Unpivoted, in the header's order -> (Lc (m, 6, 6) lower, ok (m): every pivot > 0)."""
    m = len(D)
    Lc = np.zeros((m, 6, 6))
    ok = np.ones(m, bool)
    with np.errstate(all="ignore"):
        for j in range(6):
            s = D[:, j, j].copy()
            for k in range(j):
                s = s - Lc[:, j, k] * Lc[:, j, k]
            ok &= s > 0
            Lc[:, j, j] = np.sqrt(s)
            for i in range(j + 1, 6):
                s = D[:, i, j].copy()
                for k in range(j):
                    s = s - Lc[:, i, k] * Lc[:, j, k]
                Lc[:, i, j] = s / Lc[:, j, j]
    return Lc, ok


def cholesky_solve(Lc, r):
    y = np.empty_like(r)
    z = np.empty_like(r)
    with np.errstate(all="ignore"):
        for i in range(6):
            s = r[:, i].copy()
            for k in range(i):
                s = s - Lc[:, i, k] * y[:, k]
            y[:, i] = s / Lc[:, i, i]
        for i in range(5, -1, -1):
            s = y[:, i].copy()
            for k in range(i + 1, 6):
                s = s - Lc[:, k, i] * z[:, k]
            z[:, i] = s / Lc[:, i, i]
    return z


def rotation_of(w):
    """C(w) (m, 3, 3): the rotation of the unnormalised quaternion (1, w / 2), by the formula of include/epcnet_stamps.h."""
    qw = np.ones(len(w))
    x, y, z = 0.5 * w[:, 0], 0.5 * w[:, 1], 0.5 * w[:, 2]
    nn = ((qw * qw + x * x) + y * y) + z * z
    u = 2.0 / nn
    C = np.empty((len(w), 3, 3))
    C[:, 0, 0] = 1.0 - u * (y * y + z * z)
    C[:, 0, 1] = u * (x * y - qw * z)
    C[:, 0, 2] = u * (x * z + qw * y)
    C[:, 1, 0] = u * (x * y + qw * z)
    C[:, 1, 1] = 1.0 - u * (x * x + z * z)
    C[:, 1, 2] = u * (y * z - qw * x)
    C[:, 2, 0] = u * (x * z - qw * y)
    C[:, 2, 1] = u * (y * z + qw * x)
    C[:, 2, 2] = 1.0 - u * (x * x + y * y)
    return C


def retract(R, c, eta):
    """R <- C(w) R, c <- C(w) c + rho, of every node."""
    C = rotation_of(eta[:, 3:])
    Rn = np.empty_like(R)
    for i in range(3):
        for j in range(3):
            Rn[:, i, j] = _d3(C[:, i, 0], C[:, i, 1], C[:, i, 2], R[:, 0, j], R[:, 1, j], R[:, 2, j])
    cn = np.stack([_d3(C[:, i, 0], C[:, i, 1], C[:, i, 2], c[:, 0], c[:, 1], c[:, 2]) + eta[:, i] for i in range(3)], 1)
    return Rn, cn


def check_loops(pairs, rel, weights, te):
    """status (L) int32 of the loops: 0 = used."""
    L = len(pairs)
    status = np.zeros(L, np.int32)
    for e in range(L):
        s, t = int(pairs[e, 0]), int(pairs[e, 1])
        wt, wr = weights[e]
        ok = 0 <= s < te and 0 <= t < te and s != t and np.isfinite(rel[e]).all() and np.isfinite(wt) and np.isfinite(wr) \
            and wt >= 0 and wr >= 0 and (wt > 0 or wr > 0)
        status[e] = 0 if ok else NO_EDGE
    return status


class Problem:
    """The state of one call: nodes 0 .. te - 1 (R, c), the chain edges 1 .. te - 1 and the used loops."""

    def __init__(self, poses, pairs, rel, weights, odo_w_t, odo_w_r):
        poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
        self.poses, self.T = poses, len(poses)
        fin = np.isfinite(poses).all(1)
        self.te = te = self.T if fin.all() else int(np.argmin(fin))
        self.pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
        self.rel = np.asarray(rel, np.float64).reshape(-1, 12)
        self.weights = np.asarray(weights, np.float64).reshape(-1, 2)
        self.L = len(self.pairs)
        self.status = check_loops(self.pairs, self.rel, self.weights, te)
        self.used = np.nonzero(self.status == 0)[0]
        self.active = len(self.used) > 0 and te >= 2
        m = poses[:te].reshape(te, 3, 4)
        self.R = m[:, :, :3].copy()
        self.t0 = m[0, :, 3].copy() if te else np.zeros(3)
        self.c = m[:, :, 3] - self.t0[None, :]
        # the chain's measurements from the input: Z_n = X_{n-1}^-1 X_n
        self.ZR = tmul(self.R[:-1], self.R[1:]) if te >= 2 else np.zeros((0, 3, 3))
        dc = self.c[1:] - self.c[:-1]
        Ra = self.R[:-1]
        self.zt = np.stack([_d3(Ra[:, 0, i], Ra[:, 1, i], Ra[:, 2, i], dc[:, 0], dc[:, 1], dc[:, 2]) for i in range(3)], 1) if te >= 2 else np.zeros((0, 3))
        self.wt = np.full(max(te - 1, 0), float(odo_w_t))
        self.wr = np.full(max(te - 1, 0), float(odo_w_r))
        u = self.used
        self.la, self.lb = self.pairs[u, 1].astype(np.int64), self.pairs[u, 0].astype(np.int64)      # a = target, b = source
        lm = self.rel[u].reshape(-1, 3, 4)
        self.lZR, self.lzt = lm[:, :, :3].copy(), lm[:, :, 3].copy()
        self.lwt, self.lwr = self.weights[u, 0].copy(), self.weights[u, 1].copy()
        self.failed = False

    def linearise(self):
        """Linearises every edge at (R, c) -> the cost; keeps J, the gradient pieces and the chain's Cholesky factors."""
        R, c = self.R, self.c
        with np.errstate(all="ignore"):
            self.cJ = linearise(R[:-1], R[1:], c[:-1], c[1:], self.ZR, self.zt, self.wt, self.wr)
            self.lJ = linearise(R[self.la], R[self.lb], c[self.la], c[self.lb], self.lZR, self.lzt, self.lwt, self.lwr)
            self.Lc, ok = cholesky(block_matrix(*self.cJ[:3], self.wt, self.wr))
        if not ok.all():
            self.failed = True
        leaf = np.zeros(self.te)
        leaf[1:] = self.cJ[4]
        lleaf = np.zeros(self.L)
        lleaf[self.used] = self.lJ[4]
        self.chi2 = np.full(self.L, NAN)
        self.chi2[self.used] = self.lJ[4]
        with np.errstate(all="ignore"):
            return tree_sum(leaf, NODE_LEAVES) + tree_sum(lleaf, LOOP_LEAVES)

    def _assemble(self, v, u):
        """out[n] = v[n] + scan(g)[n], g from the loops' u in ascending loop index; out[0] = 0."""
        g = np.zeros((self.te + 1, 6))
        for k in range(len(self.used)):
            g[self.la[k] + 1] = g[self.la[k] + 1] + u[k]
            g[self.lb[k] + 1] = g[self.lb[k] + 1] - u[k]
        out = v + scan6(g[:self.te])
        out[0] = 0.0
        return out

    def gradient(self):
        v = np.zeros((self.te, 6))
        v[1:] = self.cJ[3]
        with np.errstate(all="ignore"):
            return self._assemble(v, self.lJ[3])

    def product(self, p):
        with np.errstate(all="ignore"):
            eta = scan6(p)
            v = np.zeros((self.te, 6))
            v[1:] = apply_edge(*self.cJ[:3], self.wt, self.wr, p[1:])
            u = apply_edge(*self.lJ[:3], self.lwt, self.lwr, eta[self.lb] - eta[self.la])
            return self._assemble(v, u)

    def precondition(self, r):
        z = np.zeros_like(r)
        z[1:] = cholesky_solve(self.Lc, r[1:])
        return z

    def solve(self, cg_iterations):
        """cg_iterations of preconditioned CG on H x = -gradient from x = 0."""
        with np.errstate(all="ignore"):
            r = -self.gradient()
            r[0] = 0.0
            x = np.zeros_like(r)
            z = self.precondition(r)
            p = z.copy()
            rz = dot(r, z)
            for _ in range(cg_iterations):
                hp = self.product(p)
                php = dot(p, hp)
                if not (np.isfinite(php) and php > 0):
                    break
                alpha = rz / php
                x = x + alpha * p
                r = r - alpha * hp
                z = self.precondition(r)
                rz_new = dot(r, z)
                beta = rz_new / rz
                p = z + beta * p
                rz = rz_new
        return x

    def step(self, x):
        with np.errstate(all="ignore"):
            eta = scan6(x)
            R, c = retract(self.R[1:], self.c[1:], eta[1:])
        self.R[1:], self.c[1:] = R, c


def relax_reference(poses, pairs, rel, weights, odo_w_t=1.0, odo_w_r=100.0, iterations=4, cg_iterations=64):
    """The entry: -> (poses_out (T, 12) f64, cost (iterations + 1) f64, loop_chi2 (L) f64, loop_status (L) i32, num_out (2) i32)."""
    P = Problem(poses, pairs, rel, weights, odo_w_t, odo_w_r)
    T, te = P.T, P.te
    out = np.full((T, 12), NAN)
    cost = np.zeros(iterations + 1)
    out[:te] = P.poses[:te]
    num = np.array([te, len(P.used)], np.int32)
    if not P.active:
        return out, cost, np.full(P.L, NAN), P.status, num
    for it in range(iterations):
        cost[it] = P.linearise()
        P.step(P.solve(cg_iterations))
    cost[iterations] = P.linearise()
    if P.failed:
        num[1] = -1
        return out, np.zeros(iterations + 1), np.full(P.L, NAN), P.status, num
    m = np.empty((te, 3, 4))
    m[:, :, :3] = P.R
    m[:, :, 3] = P.c + P.t0[None, :]
    out[1:te] = m.reshape(te, 12)[1:]
    return out, cost, P.chi2, P.status, num


# ---- scenes for the tests -------------------------------------------------------------------------------------------------------------
def pose_of(t, rotvec):
    """[R | t] (12) of a translation and a rotation vector (Rodrigues; not part of the definition)."""
    rv = np.asarray(rotvec, np.float64)
    th = np.linalg.norm(rv)
    K = np.array([[0, -rv[2], rv[1]], [rv[2], 0, -rv[0]], [-rv[1], rv[0], 0]])
    R = np.eye(3) if th == 0 else np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)
    return np.concatenate([R, np.asarray(t, np.float64).reshape(3, 1)], 1).reshape(12)


def mat4(p):
    return np.vstack([np.asarray(p, np.float64).reshape(3, 4), [0, 0, 0, 1]])


def compose(a, b):
    return (mat4(a) @ mat4(b))[:3].reshape(12)


def inverse(a):
    m = np.asarray(a, np.float64).reshape(3, 4)
    return np.concatenate([m[:, :3].T, -(m[:, :3].T @ m[:, 3:])], 1).reshape(12)


def circle_scene(T=64, laps=2, step=10.0, seed=0, noise_t=0.05, noise_r=0.004, loops=3, origin=(0.0, 0.0, 0.0)):
    """`laps` laps of a circle in T nodes with `step` metres between them: -> (truth (T, 12), the integrated noisy odometry (T, 12), pairs
    (loops, 2) int32 joining lap 2 to lap 1, rel (loops, 12) exact from the truth, weights (loops, 2))."""
    rng = np.random.default_rng(seed)
    per = T // laps
    dth = 2 * np.pi / per
    inc = pose_of([step, 0.0, 0.0], [0.0, 0.0, dth])
    truth = [pose_of(origin, [0.0, 0.0, 0.3])]
    odo = [truth[0].copy()]
    for n in range(1, T):
        truth.append(compose(truth[-1], inc))
        noisy = compose(inc, pose_of(noise_t * rng.normal(size=3), noise_r * rng.normal(size=3)))
        odo.append(compose(odo[-1], noisy))
    truth, odo = np.stack(truth), np.stack(odo)
    src = np.linspace(per + 2, T - 3, loops).astype(np.int32)
    pairs = np.stack([src, src - per], 1).astype(np.int32)
    rel = np.stack([compose(inverse(truth[t]), truth[s]) for s, t in pairs])
    weights = np.tile(np.array([[1.0, 100.0]]), (loops, 1))
    return truth, odo, pairs, rel, weights


def walk_scene(T, L, seed=0, step=5.0, noise_t=0.05, noise_r=0.003):
    """A wandering trajectory of T nodes and L loops between random distinct nodes, either direction, measured from the truth with a
    little noise, each with its own weights: -> (odo (T, 12), pairs (L, 2) int32, rel (L, 12), weights (L, 2))."""
    rng = np.random.default_rng([seed, T, L])
    truth = [pose_of(rng.normal(size=3) * 100.0, rng.normal(size=3) * 0.5)]
    odo = [truth[0].copy()]
    for n in range(1, T):
        inc = pose_of([step, 0.3 * rng.normal(), 0.1 * rng.normal()], [0.02 * rng.normal(), 0.02 * rng.normal(), 0.2 * rng.normal()])
        truth.append(compose(truth[-1], inc))
        odo.append(compose(odo[-1], compose(inc, pose_of(noise_t * rng.normal(size=3), noise_r * rng.normal(size=3)))))
    pairs = np.zeros((L, 2), np.int32)
    for e in range(L):
        s = int(rng.integers(0, T))
        t = int((s + 1 + rng.integers(0, T - 1)) % T)
        pairs[e] = (s, t)
    rel = np.stack([compose(compose(inverse(truth[t]), truth[s]), pose_of(0.02 * rng.normal(size=3), 0.002 * rng.normal(size=3)))
                    for s, t in pairs]) if L else np.zeros((0, 12))
    weights = np.stack([rng.uniform(0.5, 2.0, size=L), rng.uniform(50.0, 200.0, size=L)], 1) if L else np.zeros((0, 2))
    return np.stack(odo), pairs, rel, weights
