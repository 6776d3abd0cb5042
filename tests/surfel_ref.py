"""numpy restatement of include/epcnet_surfels.h (epcnet_map_surfels), operation for operation, written from the header's text: the rows,
cells, keys and numbering are ``map_ref``'s; the own moments are ``np.add.at`` on int64; the pool walks the (2 ring + 1)^3 offsets, each a
``searchsorted`` into the sorted keys; the solve is elementwise float64 in the stated association over all voxels at once (numpy fuses
nothing, ``np.sqrt`` is correctly rounded) and ONE ``astype(float32)`` per output.  The device's outputs are compared with these on bit
patterns."""
import numpy as np

import map_ref as M

NAN_WORD = M.NAN_WORD
MAX_RING = 2
SWEEPS = 5                       # EPC_SURFEL_SWEEPS
PAIRS = ((0, 1, 2), (0, 2, 1), (1, 2, 0))          # (p, q, the third index r)
_AB = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


# ---- the solve: covariance, Jacobi, order, normal -------------------------------------------------------------------------------------------
def covariance(N, S1, S2):
    """``(mu (V, 3), C (V, 6))`` float64 from the pooled integer sums; C in the order 00 01 02 11 12 22."""
    with np.errstate(all="ignore"):
        n = N.astype(np.float64)
        mu = S1.astype(np.float64) / n[:, None]
        C = np.stack([S2[:, i].astype(np.float64) / n - mu[:, a] * mu[:, b] for i, (a, b) in enumerate(_AB)], 1)
    return mu, C


def jacobi(C, sweeps=SWEEPS):
    """Cyclic Jacobi on (V, 6) symmetric 3 x 3 matrices -> ``(diag (V, 3), Vec (V, 3, 3))``: Vec[:, i, k] is component i of column k."""
    V = len(C)
    a = {(0, 0): C[:, 0].copy(), (0, 1): C[:, 1].copy(), (0, 2): C[:, 2].copy(), (1, 1): C[:, 3].copy(), (1, 2): C[:, 4].copy(),
         (2, 2): C[:, 5].copy()}
    at = lambda i, j: (i, j) if i <= j else (j, i)
    v = np.zeros((V, 3, 3))
    v[:, 0, 0] = v[:, 1, 1] = v[:, 2, 2] = 1.0
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p, q, r in PAIRS:
                apq = a[at(p, q)]
                go = apq != 0.0
                theta = (a[(q, q)] - a[(p, p)]) / (2.0 * apq)
                t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                h = t * apq
                a[(p, p)] = np.where(go, a[(p, p)] - h, a[(p, p)])
                a[(q, q)] = np.where(go, a[(q, q)] + h, a[(q, q)])
                a[at(p, q)] = np.where(go, 0.0, apq)
                g, f = a[at(r, p)], a[at(r, q)]
                a[at(r, p)] = np.where(go, c * g - s * f, g)
                a[at(r, q)] = np.where(go, s * g + c * f, f)
                for i in range(3):
                    g, f = v[:, i, p].copy(), v[:, i, q].copy()
                    v[:, i, p] = np.where(go, c * g - s * f, g)
                    v[:, i, q] = np.where(go, s * g + c * f, f)
    return np.stack([a[(0, 0)], a[(1, 1)], a[(2, 2)]], 1), v


def order_and_normal(diag, vec):
    """``(lam (V, 3) ascending and clamped, n (V, 3))`` float64 by the header's rules."""
    V = len(diag)
    rows = np.arange(V)
    with np.errstate(all="ignore"):
        k0 = np.zeros(V, np.int64)
        k0 = np.where(diag[:, 1] < diag[rows, k0], 1, k0)
        k0 = np.where(diag[:, 2] < diag[rows, k0], 2, k0)
        p = np.where(k0 == 0, 1, 0)                    # the other two, in index order
        q = np.where(k0 == 2, 1, 2)
        swap = diag[rows, q] < diag[rows, p]
        k1, k2 = np.where(swap, q, p), np.where(swap, p, q)
        lam = np.stack([diag[rows, k0], diag[rows, k1], diag[rows, k2]], 1)
        lam = np.where(lam < 0.0, 0.0, lam)
        col = vec[rows, :, k0]
        nn = np.sqrt((col[:, 0] * col[:, 0] + col[:, 1] * col[:, 1]) + col[:, 2] * col[:, 2])
        n = col / nn[:, None]
        k = np.zeros(V, np.int64)
        k = np.where(np.abs(n[:, 1]) > np.abs(n[rows, k]), 1, k)
        k = np.where(np.abs(n[:, 2]) > np.abs(n[rows, k]), 2, k)
        n = np.where((n[rows, k] < 0.0)[:, None], -n, n)
    return lam, n


def solve(N, S1, S2, sweeps=SWEEPS):
    """mu, lam, n (float64) of the pooled sums."""
    mu, C = covariance(N, S1, S2)
    diag, vec = jacobi(C, sweeps)
    lam, n = order_and_normal(diag, vec)
    return mu, lam, n


def finish(g, mu, lam, n, voxel):
    """The three float32 outputs of valid surfels: centroid, normal, eigen."""
    with np.errstate(all="ignore"):
        s = np.float64(voxel) / np.float64(256.0)
        centroid = (((256 * g).astype(np.float64) + mu) * s).astype(np.float32)
        eigen = ((lam * s) * s).astype(np.float32)
        return centroid, n.astype(np.float32), eigen


# ---- the voxels, their moments and the pool -----------------------------------------------------------------------------------------------
def voxels(points, offsets, poses, origin, voxel):
    """The voxels by ascending leader (valid offsets): dict with ``g`` (V, 3) int64 cells, ``n`` (V,), ``A`` (V, 3), ``B`` (V, 6) int64 own
    moments, ``keys`` (V,)."""
    kind, w = M.lattice(points, offsets, poses, origin, voxel)
    rows = np.nonzero(kind == M.KEPT)[0]
    uniq, first, inverse = np.unique(M.keys_of(w[rows]), return_index=True, return_inverse=True)
    V = len(uniq)
    order = np.argsort(first, kind="stable")
    number = np.empty(V, np.int64)
    number[order] = np.arange(V)
    j = number[inverse.reshape(-1)]
    u = (w[rows] & 4095) >> 4
    n, A, B = np.zeros(V, np.int64), np.zeros((V, 3), np.int64), np.zeros((V, 6), np.int64)
    np.add.at(n, j, 1)
    np.add.at(A, j, u)
    np.add.at(B, j, np.stack([u[:, a] * u[:, b] for a, b in _AB], 1))
    g = w[rows[first[order]]] >> 12 if V else np.zeros((0, 3), np.int64)
    return dict(g=g, n=n, A=A, B=B, keys=uniq[order])


def pool(vox, ring, min_count):
    """``(N (V,), S1 (V, 3), S2 (V, 6))`` int64: the pooled sums of every voxel in the frame of its own cell."""
    g, n, A, B, keys = vox["g"], vox["n"], vox["A"], vox["B"], vox["keys"]
    V = len(n)
    N, S1, S2 = np.zeros(V, np.int64), np.zeros((V, 3), np.int64), np.zeros((V, 6), np.int64)
    if V == 0:
        return N, S1, S2
    by_key = np.argsort(keys)
    sorted_keys = keys[by_key]
    span = range(-ring, ring + 1)
    for o2 in span:
        for o1 in span:
            for o0 in span:
                o = np.array([o0, o1, o2], np.int64)
                cell = g + o
                inside = ((cell >= -M.MAX_CELL) & (cell < M.MAX_CELL)).all(1)
                cell = np.where(inside[:, None], cell, 0)
                key = ((cell[:, 2] + M.MAX_CELL) << 42) | ((cell[:, 1] + M.MAX_CELL) << 21) | (cell[:, 0] + M.MAX_CELL)
                at = np.minimum(np.searchsorted(sorted_keys, key), V - 1)
                i = by_key[at]
                ok = inside & (sorted_keys[at] == key) & (n[i] >= min_count)
                e = 256 * o
                nn, AA, BB = n[i], A[i], B[i]
                N += np.where(ok, nn, 0)
                S1 += np.where(ok[:, None], AA + nn[:, None] * e, 0)
                add = np.stack([BB[:, k] + e[a] * AA[:, b] + e[b] * AA[:, a] + nn * (e[a] * e[b]) for k, (a, b) in enumerate(_AB)], 1)
                S2 += np.where(ok[:, None], add, 0)
    return N, S1, S2


def reference(points, offsets, poses, origin, voxel, max_voxels, min_count=1, ring=1, min_support=8, num_rows=None, sweeps=SWEEPS):
    """Every output of epcnet_map_surfels as a dict: ``map_points``, ``count``, ``num_out`` (map_ref.reference's), ``centroid``,
    ``normal``, ``eigen`` (max_voxels, 3) float32, ``support`` (max_voxels,) int32; besides ``V``, ``leader``, and for the tests ``valid``
    (V,), ``pooled`` = (N, S1, S2) and ``vox``."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    num_rows = len(points) if num_rows is None else num_rows
    out = M.reference(points, offsets, poses, origin, voxel, max_voxels, min_count, num_rows)
    for name in ("centroid", "normal", "eigen"):
        out[name] = np.zeros((max_voxels, 3), np.float32)
        out[name].view(np.uint32)[:] = NAN_WORD
    out["support"] = np.zeros(max_voxels, np.int32)
    out["valid"] = np.zeros(0, bool)
    if out["num_out"][0] < 0:
        return out
    vox = voxels(points, offsets, poses, origin, voxel)
    V = len(vox["n"])
    assert V == out["V"] and (vox["n"] == out["count"][:V]).all()
    N, S1, S2 = pool(vox, ring, min_count)
    mu, lam, n = solve(N, S1, S2, sweeps)
    centroid, normal, eigen = finish(vox["g"], mu, lam, n, voxel)
    valid = (vox["n"] >= min_count) & (N >= min_support)
    for name, value in (("centroid", centroid), ("normal", normal), ("eigen", eigen)):
        value.view(np.uint32)[~valid] = NAN_WORD
        out[name][:V] = value
    out["support"][:V] = N
    out.update(valid=valid, pooled=(N, S1, S2), vox=vox)
    return out


# ---- seeded material ----------------------------------------------------------------------------------------------------------------------
def sums_of(sets):
    """(N, S1, S2) of a list of integer point sets (n_i, 3)."""
    N = np.array([len(p) for p in sets], np.int64)
    S1 = np.array([p.sum(0) for p in sets], np.int64).reshape(-1, 3)
    S2 = np.array([[(p[:, a] * p[:, b]).sum() for a, b in _AB] for p in sets], np.int64).reshape(-1, 6)
    return N, S1, S2


def lattice_sets(seed, count):
    """``count`` pooled sums of lattice point sets in [-512, 767]^3, a quarter each: random, near-planar (a random plane, thickness up
    to 2 lattice steps), linear, coincident.  Built from moments directly: (N, S1, S2)."""
    rng = np.random.default_rng(seed)
    N, S1, S2 = [], [], []
    for i in range(count // 1000 + (count % 1000 > 0)):
        m = min(1000, count - i * 1000)
        size = int(rng.integers(3, 40))
        kind = i % 4
        if kind == 0:
            p = rng.integers(-512, 768, size=(m, size, 3))
        elif kind == 1:
            c = rng.integers(-200, 400, size=(m, 1, 3))
            basis = rng.normal(size=(m, 2, 3))
            uv = rng.uniform(-150, 150, size=(m, size, 2))
            p = np.floor(c + np.einsum("msk,mkc->msc", uv, basis / np.linalg.norm(basis, axis=2, keepdims=True))
                         + rng.uniform(0, 2, size=(m, size, 3))).astype(np.int64)
        elif kind == 2:
            c = rng.integers(-100, 300, size=(m, 1, 3))
            d = rng.integers(-6, 7, size=(m, 1, 3))
            p = c + d * rng.integers(-30, 31, size=(m, size, 1))
        else:
            p = np.repeat(rng.integers(-512, 768, size=(m, 1, 3)), size, 1)
        p = np.clip(p, -512, 767).astype(np.int64)
        N.append(np.full(m, size, np.int64))
        S1.append(p.sum(1))
        S2.append(np.stack([(p[:, :, a] * p[:, :, b]).sum(1) for a, b in _AB], 1))
    return np.concatenate(N), np.concatenate(S1), np.concatenate(S2)


def settled_sweeps(N, S1, S2, voxel=0.2, top=9):
    """The smallest sweep count k at which k + 1 sweeps move no bit of the float32 outputs (normal, eigen) of any of the given sums, and
    the number of sets that still moved at k - 1."""
    mu, C = covariance(N, S1, S2)
    g = np.zeros((len(N), 3), np.int64)
    outs = []
    for k in range(top + 1):
        diag, vec = jacobi(C, k)
        lam, n = order_and_normal(diag, vec)
        _, normal, eigen = finish(g, mu, lam, n, voxel)
        outs.append(np.concatenate([normal.view(np.uint32), eigen.view(np.uint32)], 1))
    moved = [int((outs[k] != outs[k + 1]).any(1).sum()) for k in range(top)]
    k = top
    while k > 0 and moved[k - 1] == 0:
        k -= 1
    return k, moved
