"""The definition of include/epcnet_surfels.h as tests/surfel_ref.py restates it, without a device: the pooled sums against a second
formulation that gathers the rows of the neighbour cells and sums them in Python integers, the covariance against exact fractions, the
eigenvalues and normals against numpy.linalg.eigh, a tilted plane, the sweep count, the eleventh header's binding, and the entry's
refusals, which launch nothing."""
import ctypes
import os
from fractions import Fraction as F

import numpy as np
import pytest

import helpers as H
import map_ref as M
import surfel_ref as S


def _block_scene(seed=3, rows=700, half=1.5):
    """Rows uniform in [-half, half]^3 around an integer translation: at voxel 0.5 a block of 6 x 6 x 6 cells with three rows each on
    average, cells on both sides of the origin."""
    rng = np.random.default_rng(seed)
    points = rng.uniform(-half, half, size=(rows, 3)).astype(np.float32)
    return points, np.array([0, rows // 2, rows], np.int32), M.identity_poses(2, (3.0, -2.0, 1.0)), np.array([3.0, -2.0, 1.0])


@pytest.mark.parametrize("ring,min_count", [(0, 1), (1, 1), (1, 2), (2, 1), (2, 3)])
def test_pool_agrees_with_rows_gathered_and_summed_in_python_integers(ring, min_count):
    """Second formulation: per voxel, the kept rows of every qualifying cell around it, their 8-bit lattice coordinates taken relative to
    the voxel's own cell and summed directly -- no own-cell sums are shifted.  N, S1, S2 are equal as integers; the float64 covariance
    lies within the rounding bound of its four operations of the exact rational one."""
    points, offsets, poses, origin = _block_scene()
    voxel = 0.5
    ref = S.reference(points, offsets, poses, origin, voxel, len(points), min_count, ring, 3)
    kind, w = M.lattice(points, offsets, poses, origin, voxel)
    assert (kind == M.KEPT).all()
    cells = {}
    for r in range(len(points)):
        cells.setdefault(tuple(int(v) for v in w[r] >> 12), []).append([int(v) >> 4 for v in w[r]])     # the global voxel / 256 lattice
    N, S1, S2 = ref["pooled"]
    g = ref["vox"]["g"]
    mu, C = S.covariance(N, S1, S2)
    u = F(1, 2 ** 53)
    assert ref["V"] == len(cells) > 150 and (N > 0).sum() > 100
    for j in range(ref["V"]):
        own = tuple(int(v) for v in g[j])
        n, s1, s2 = 0, [0, 0, 0], [0] * 6
        for o0 in range(-ring, ring + 1):
            for o1 in range(-ring, ring + 1):
                for o2 in range(-ring, ring + 1):
                    rows = cells.get((own[0] + o0, own[1] + o1, own[2] + o2), [])
                    if len(rows) < min_count:
                        continue
                    for p in rows:
                        q = [p[a] - 256 * own[a] for a in range(3)]
                        assert all(-256 * ring <= v < 256 * (ring + 1) for v in q)
                        n += 1
                        for a in range(3):
                            s1[a] += q[a]
                        for k, (a, b) in enumerate(S._AB):
                            s2[k] += q[a] * q[b]
        assert (int(N[j]), S1[j].tolist(), S2[j].tolist()) == (n, s1, s2), j
        if n == 0:
            continue
        for k, (a, b) in enumerate(S._AB):
            exact = F(s2[k], n) - F(s1[a], n) * F(s1[b], n)
            # fl(S2 / N) and each mu carry one rounding, the product one more (three on mu_a mu_b), the difference one: relative 2^-53 each
            bound = u * (abs(F(s2[k], n)) + 3 * abs(F(s1[a], n) * F(s1[b], n)) + abs(exact)) * F(1001, 1000)
            assert abs(F(float(C[j, k])) - exact) <= bound, (j, k)


def _eigh(N, S1, S2):
    """numpy.linalg.eigh on the exact covariance rounded once: eigenvalues ascending, the first eigenvector signed by the header's rule."""
    lam, normal = [], []
    for n, s1, s2 in zip(N.tolist(), S1.tolist(), S2.tolist()):
        c = {ab: float(F(s2[k], n) - F(s1[ab[0]], n) * F(s1[ab[1]], n)) for k, ab in enumerate(S._AB)}
        m = np.array([[c[(min(a, b), max(a, b))] for b in range(3)] for a in range(3)])
        values, vectors = np.linalg.eigh(m)
        v = vectors[:, 0]
        k = 0
        for a in (1, 2):
            if abs(v[a]) > abs(v[k]):
                k = a
        lam.append(values)
        normal.append(-v if v[k] < 0 else v)
    return np.array(lam), np.array(normal)


def test_eigenvalues_and_normals_against_eigh_on_well_separated_cases():
    """Random lattice sets of 12 to 40 points in an ellipsoid with axes 1 : 3 : 9 under a random rotation: neighbouring eigenvalues
    differ by a factor between 2 and 40 (asserted).  Jacobi's float64 error is 1e-16 of the largest eigenvalue, against a float32 spacing
    of 6e-8 of the smallest (at most 1600 times smaller): what separates the two results is the ONE rounding to float32, half a spacing,
    and the other side's float64 noise.  Tolerance: one float32 spacing at the value's size; for the unit normal one spacing at 1
    (2^-23 = 1.2e-7) per component -- the eigenvector's float64 error, 1e-16 times largest / gap, is far below it."""
    rng = np.random.default_rng(7)
    sets = []
    while len(sets) < 400:
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        p = (rng.normal(size=(int(rng.integers(12, 41)), 3)) * np.array([9.0, 27.0, 81.0])) @ q.T + rng.integers(-100, 300, size=3)
        sets.append(np.clip(np.floor(p), -512, 767).astype(np.int64))
    N, S1, S2 = S.sums_of(sets)
    want_lam, want_n = _eigh(N, S1, S2)
    keep = (want_lam[:, 1] > 2 * want_lam[:, 0]) & (want_lam[:, 2] > 2 * want_lam[:, 1]) & (want_lam[:, 2] < 1600 * want_lam[:, 0]) \
        & (np.sort(np.abs(want_n), 1)[:, 2] > 1.01 * np.sort(np.abs(want_n), 1)[:, 1])        # (the sign rule has a clear winner)
    assert keep.sum() > 250
    mu, lam, n = S.solve(N, S1, S2)
    centroid, normal, eigen = S.finish(np.zeros((len(N), 3), np.int64), mu, lam, n, 256.0)      # s = 1: lattice units
    want_eigen = want_lam.astype(np.float32)
    tol = np.spacing(np.abs(want_eigen))
    assert (np.abs(eigen.astype(np.float64) - want_eigen.astype(np.float64)) <= tol)[keep].all()
    assert (np.abs(normal.astype(np.float64) - want_n)[keep] <= 2.0 ** -23).all()
    assert (np.abs(np.linalg.norm(normal.astype(np.float64), axis=1) - 1.0) < 3e-7).all()
    assert (eigen[:, 0] <= eigen[:, 1]).all() and (eigen[:, 1] <= eigen[:, 2]).all()
    assert (np.abs(centroid.astype(np.float64) - np.array([p.mean(0) for p in sets])) <= 768 * 2.0 ** -23).all()


def test_a_tilted_plane_of_lattice_points_gives_its_normal():
    """Lattice points a (2, -1, 0) + b (0, 1, -1) + c: the plane x + 2 y + 2 z = const, normal (1, 2, 2) / 3.  The smallest eigenvalue is
    0 up to the covariance's cancellation error (a few 1e-10 lattice units squared: epcnet_surfels.h), negative ones clamped."""
    rng = np.random.default_rng(8)
    sets, raw = [], 0
    for i in range(200):
        ab = rng.integers(-40, 41, size=(int(rng.integers(6, 30)), 2))
        p = ab[:, :1] * np.array([2, -1, 0]) + ab[:, 1:] * np.array([0, 1, -1]) + rng.integers(-100, 200, size=3)
        if np.linalg.matrix_rank(ab - ab[0]) == 2:
            sets.append(p.astype(np.int64))
    N, S1, S2 = S.sums_of(sets)
    assert np.abs(np.concatenate(sets)).max() <= 512 and len(sets) > 150
    mu, C = S.covariance(N, S1, S2)
    diag, vec = S.jacobi(C)
    raw = int((diag.min(1) < 0).sum())
    mu, lam, n = S.solve(N, S1, S2)
    assert 0 < raw < len(sets) and (lam >= 0).all() and (lam[:, 0] < 1e-8).all() and (lam[:, 1] > 1.0).all()
    want = np.array([1.0, 2.0, 2.0]) / 3.0
    assert np.abs(n.astype(np.float32) - want.astype(np.float32)).max() <= 2.0 ** -23
    # degenerate statistics: coincident points -> C == 0, nothing rotates, V stays I: eigen 0 0 0, normal +x; a line along x: normal +y
    N, S1, S2 = S.sums_of([np.repeat(np.array([[5, -7, 300]]), 9, 0), np.stack([np.arange(10), np.full(10, 3), np.full(10, -4)], 1)])
    mu, lam, n = S.solve(N, S1, S2)
    assert lam[0].tolist() == [0.0, 0.0, 0.0] and n[0].tolist() == [1.0, 0.0, 0.0]
    assert lam[1].tolist() == [0.0, 0.0, 8.25] and n[1].tolist() == [0.0, 1.0, 0.0]


def test_sweep_count():
    """EPC_SURFEL_SWEEPS is one more than the smallest count at which a further sweep moves no bit of the float32 normals and
    eigenvalues: on 320,000 covariances of lattice point sets (random, near-planar, linear, coincident) and on the pooled sums of two
    scenes."""
    L = H.pkg("lib")
    assert L.EPC_SURFEL_SWEEPS == S.SWEEPS
    settled, moved = S.settled_sweeps(*S.lattice_sets(1, 320000), top=7)
    print("sets that one more sweep still moves, after 0..6 sweeps:", moved)
    assert settled == S.SWEEPS - 1 and moved[settled - 1] > 0
    for scene, voxel in ((M.drive(1, (5000,) * 4), 0.5), (_block_scene(rows=3000, half=4.0), 0.5)):
        ref = S.reference(*scene, voxel, 20000, 1, 1, 3)
        N, S1, S2 = (v[ref["valid"]] for v in ref["pooled"])
        assert len(N) > 2000
        settled, moved = S.settled_sweeps(N, S1, S2, top=7)
        print("scene:", moved)
        assert settled <= S.SWEEPS - 1


def test_reference_rules():
    """support is written whatever min_count and min_support; the surfel is NaN below either; a voxel below min_count is in no pool."""
    points, offsets, poses, origin = _block_scene()
    base = S.reference(points, offsets, poses, origin, 0.5, 800, 1, 1, 3)
    V = base["V"]
    assert (base["support"][:V] >= base["count"][:V]).all() and not base["support"][V:].any() and base["valid"].all()
    assert (base["centroid"][V:].view(np.uint32) == S.NAN_WORD).all()
    two = S.reference(points, offsets, poses, origin, 0.5, 800, 3, 1, 40)
    low = two["count"][:V] < 3
    assert 0 < low.sum() < V and (two["support"][:V] <= base["support"][:V]).all() and (two["support"][:V][low] > 0).any()
    gone = np.isnan(two["normal"][:V]).all(1)
    assert (gone == (low | (two["support"][:V] < 40))).all() and (two["support"][:V][~low] < 40).any() and not gone.all()
    assert (two["map_points"].view(np.uint32) == M.reference(points, offsets, poses, origin, 0.5, 800, 3)["map_points"].view(np.uint32)).all()
    # the centroid of ring 0 is the mean of the voxel's own rows on the coarser lattice: within voxel / 256 below map_points' mean
    own = S.reference(points, offsets, poses, origin, 0.5, 800, 1, 0, 3)
    ok = own["valid"]
    d = own["map_points"][:V][ok].astype(np.float64) - own["centroid"][:V][ok]
    assert ok.sum() > 50 and (d > -1e-6).all() and (d < 0.5 / 256 + 0.5 / 4096 + 1e-6).all()
    over = S.reference(points, offsets, poses, origin, 0.5, V - 1)
    assert over["num_out"][0] == -1 and not over["support"].any() and (over["eigen"].view(np.uint32) == S.NAN_WORD).all()


def test_eleventh_header_is_bound_like_the_others():
    L = H.pkg("lib")
    text = open(os.path.join(H.ROOT, "include", "epcnet_surfels.h")).read()
    assert L.SURFELS_HEADER_PATH == os.path.join(H.ROOT, "include", "epcnet_surfels.h")
    assert ("surfels", "SURFEL", False, False) in L._HEADERS
    assert [row[0] for row in L._HEADERS].index("surfels") == [row[0] for row in L._HEADERS].index("maps") + 1
    functions, constants, status = L.parse_header(text, need_status=False)     # no `double` by value: the plain scalars read it
    assert list(functions) == L.SURFEL_EXPORTS == ["epcnet_map_surfels_workspace_bytes", "epcnet_map_surfels"]
    assert status == {} and constants == {"EPC_SURFEL_PARAMS": 8, "EPC_SURFEL_MAX_RING": 2, "EPC_SURFEL_SWEEPS": S.SWEEPS}
    assert L.EPC_SURFEL_PARAMS == 8 and L.EPC_SURFEL_MAX_RING == S.MAX_RING == 2
    for other in (L.EXPORTS, L.POSE_EXPORTS, L.SCAN_EXPORTS, L.SUBMAP_EXPORTS, L.STAMP_EXPORTS, L.REVISIT_EXPORTS, L.PAIR_EXPORTS,
                  L.TRAJECTORY_EXPORTS, L.MAP_EXPORTS, L.FORM_EXPORTS, L.LAUNCHING):
        assert not set(L.SURFEL_EXPORTS) & set(other)
    for name in L.SURFEL_EXPORTS:
        assert hasattr(L.lib(), name)
    size, entry = L.lib().epcnet_map_surfels_workspace_bytes, L.lib().epcnet_map_surfels
    assert size.restype is ctypes.c_size_t and size.argtypes == [ctypes.c_longlong, ctypes.c_int, ctypes.c_longlong]
    ret, types, names = functions["epcnet_map_surfels"]
    assert names == ["points", "offsets", "num_rows", "num_clouds", "poses", "origin", "params", "max_voxels", "map_points", "count",
                     "centroid", "normal", "eigen", "support", "num_out", "workspace", "workspace_bytes", "stream"]
    assert ret == "int" and (types[-1], names[-1]) == ("void*", "stream") and entry.restype is ctypes.c_int
    for n, t in (("points", "float*"), ("map_points", "float*"), ("centroid", "float*"), ("normal", "float*"), ("eigen", "float*"),
                 ("poses", "double*"), ("origin", "double*"), ("params", "double*"), ("offsets", "int32_t*"), ("count", "int32_t*"),
                 ("support", "int32_t*"), ("num_out", "int32_t*"), ("num_rows", "long long"), ("max_voxels", "long long")):
        assert types[names.index(n)] == t, n
    P, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    assert entry.argtypes == [P, P, ll, i, P, P, P, ll, P, P, P, P, P, P, P, P, ctypes.c_size_t, P]
    assert hasattr(L.run, "epcnet_map_surfels") and not hasattr(L.run, "epcnet_map_surfels_workspace_bytes")
    with pytest.raises(ValueError):                                           # a second declaration of a name is refused like everywhere
        L.parse_header(text + "\nint epcnet_map_surfels(int n);\n", need_status=False)
    ops, scans = H.pkg("ops"), H.pkg("scans")
    assert ops.fuse_surfels is scans.fuse_surfels


def test_entry_refusals_launch_nothing():
    """EPC_EINVAL / EPC_ENOMEM from addresses that are never followed: nothing is launched, so no device is needed."""
    L = H.pkg("lib")
    size = L.lib().epcnet_map_surfels_workspace_bytes
    assert size(1000, 4, 1000) > 0 and size(1000, 4, 1000) % 16 == 0 and size(1001, 4, 1000) >= size(1000, 4, 1000) + 4 - 16
    assert size(1 << 20, 4, 1000) > size(1000, 4, 1000) and size(1000, 4, 1025) > size(1000, 4, 1000)
    assert size(1000, 4, 1000) == size(1000, 4, 1023) == size(1000, 999, 600)          # the table: the power of two >= 2 max_voxels + 1
    assert size(1000, 4, 1025) - size(1000, 4, 1000) == 2048 * 128                      # ... of 128-byte slots
    assert size(0, 0, 1) > 0 and size((1 << 31) - 1, 1 << 24, 1 << 28) > 0
    for rows, clouds, voxels in ((-1, 4, 10), (1 << 31, 4, 10), (10, -1, 10), (10, (1 << 24) + 1, 10), (10, 4, 0), (10, 4, (1 << 28) + 1)):
        assert size(rows, clouds, voxels) == 0
    a = 0x10000

    def call(rows=1000, clouds=4, voxels=1000, points=a, offsets=a, poses=a, origin=a, voxel=0.2, min_count=1.0, ring=1.0, min_support=8.0,
             reserved=(0.0,) * 4, params=True, out=a, count=a, centroid=a, normal=a, eigen=a, support=a, num=a, ws=a, ws_bytes=None):
        need = size(1000, 4, 1000) if ws_bytes is None else ws_bytes
        p = (ctypes.c_double * 8)(voxel, min_count, ring, min_support, *reserved) if params else None
        return L.lib().epcnet_map_surfels(points, offsets, rows, clouds, poses, origin, p, voxels, out, count, centroid, normal, eigen,
                                          support, num, ws, need, None)

    nan, inf = float("nan"), float("inf")
    bad = [dict(rows=-1), dict(rows=1 << 31), dict(clouds=-1), dict(clouds=(1 << 24) + 1), dict(voxels=0), dict(voxels=(1 << 28) + 1),
           dict(voxel=0.0), dict(voxel=-0.2), dict(voxel=nan), dict(voxel=inf), dict(voxel=2.0 ** -21), dict(voxel=2.0 ** 20 + 1.0),
           dict(min_count=0.0), dict(min_count=1.5), dict(min_count=nan), dict(min_count=2.0 ** 31), dict(min_count=-1.0),
           dict(ring=-1.0), dict(ring=3.0), dict(ring=0.5), dict(ring=nan), dict(ring=inf),
           dict(min_support=2.0), dict(min_support=2.0 ** 31), dict(min_support=8.5), dict(min_support=nan), dict(min_support=-8.0),
           dict(ws=a + 8), dict(points=None), dict(offsets=None), dict(poses=None), dict(origin=None), dict(params=False), dict(out=None),
           dict(count=None), dict(centroid=None), dict(normal=None), dict(eigen=None), dict(support=None), dict(num=None), dict(ws=None)]
    bad += [dict(reserved=tuple(1.0 if i == k else 0.0 for i in range(4))) for k in range(4)]
    bad += [dict(reserved=(0.0, nan, 0.0, 0.0))]
    for kw in bad:
        assert call(**kw) == L.EPC_EINVAL, kw
        assert b"epcnet_map_surfels" in L.lib().epc_last_error()
    assert call(ws_bytes=size(1000, 4, 1000) - 1) == L.EPC_ENOMEM and call(ws_bytes=0) == L.EPC_ENOMEM
    assert call(voxels=1025) == L.EPC_ENOMEM                                   # a workspace sized for a smaller table
