"""epcnet_map_surfels on the device against its numpy restatement (tests/surfel_ref.py): every output goes into a poisoned buffer with
slack behind it, the workspace has exactly the size asked for, and everything is compared on BIT PATTERNS -- integer moments, then a fixed
sequence of float64 operations, so there is no tolerance anywhere.  map_points, count and num_out are compared with map_ref.reference as
well: they are epcnet_map_fuse's.

What a contracted multiply-add would do: the planar scene of ``_planar_scene`` holds voxels whose float32 outputs change when
C_ab = fl(fl(S2 / N) - fl(mu_a mu_b)) is contracted to one fused operation (emulated with exact fractions, ``_contracted``), and voxels
whose smallest eigenvalue is negative before the clamp; test_planar_lattice_scene re-counts both before it runs the device."""
import ctypes
import functools
from fractions import Fraction as F

import numpy as np
import pytest
import torch

import helpers as H
import map_ref as M
import stage_ref as SG
import submap_ref as SR
import surfel_ref as S

pytestmark = pytest.mark.gpu

MP_TILE = 256            # MP_TILE of csrc/map_common.h: the rows of one insert / count / emit tile
MP_LEVEL = 256 * 256     # MP_TILE * MP_GROUP: the rows behind which the leaders' scan takes its second level
FLOATS = ("map_points", "centroid", "normal", "eigen")
INTS = ("count", "support", "num_out")


def _up(a, dtype, dev):
    a = np.ascontiguousarray(a, dtype)
    if a.size == 0:
        return torch.zeros(12, dtype=torch.float64, device=dev).view(torch.from_numpy(a).dtype)      # a pointer that is never followed
    return torch.from_numpy(a).to(dev)


def _raw(points, offsets, poses, origin, voxel, max_voxels, min_count=1, ring=1, min_support=8, num_rows=None):
    """The entry itself on poisoned outputs and a workspace of exactly the size asked for -> the outputs as host arrays after the checks
    that nothing was written behind any of them."""
    L = H.pkg("lib")
    dev = torch.device("cuda")
    num_rows = len(points) if num_rows is None else num_rows
    C = len(offsets) - 1
    pts, off = _up(points, np.float32, dev), _up(offsets, np.int32, dev)
    pos, org = _up(np.asarray(poses).reshape(-1, 12), np.float64, dev), _up(origin, np.float64, dev)
    need = L.lib().epcnet_map_surfels_workspace_bytes(num_rows, C, max_voxels)
    assert need > 0
    out = {name: SG.Poisoned((max_voxels, 3), torch.float32, dev) for name in FLOATS}
    out.update(count=SG.Poisoned((max_voxels,), torch.int32, dev), support=SG.Poisoned((max_voxels,), torch.int32, dev),
               num_out=SG.Poisoned((4,), torch.int32, dev))
    ws = SG.Poisoned((need,), torch.uint8, dev)
    params = (ctypes.c_double * 8)(voxel, float(min_count), float(ring), float(min_support))
    L.run.epcnet_map_surfels(pts, off, num_rows, C, pos, org, params, max_voxels, out["map_points"].t, out["count"].t, out["centroid"].t,
                             out["normal"].t, out["eigen"].t, out["support"].t, out["num_out"].t, ws.t, need)
    torch.cuda.synchronize()
    for p in list(out.values()) + [ws]:
        assert p.untouched()
    return {name: p.t.cpu().numpy() for name, p in out.items()}


def _check(got, want, what):
    assert got["num_out"].tolist() == want["num_out"].tolist(), (what, got["num_out"].tolist(), want["num_out"].tolist())
    for name in ("count", "support"):
        assert (got[name] == want[name]).all(), (what, name, int((got[name] != want[name]).sum()))
    for name in FLOATS:
        differ = (got[name].view(np.uint32) != want[name].view(np.uint32)).any(1).nonzero()[0]
        assert differ.size == 0, (what, name, "%d rows differ, the first is row %d" % (differ.size, int(differ[0])))


def _both(points, offsets, poses, origin, voxel, max_voxels, what, min_count=1, ring=1, min_support=8, num_rows=None):
    want = S.reference(points, offsets, poses, origin, voxel, max_voxels, min_count, ring, min_support, num_rows)
    fused = M.reference(points, offsets, poses, origin, voxel, max_voxels, min_count, num_rows)
    got = _raw(points, offsets, poses, origin, voxel, max_voxels, min_count, ring, min_support, num_rows)
    _check(got, want, what)
    for name in ("map_points", "count", "num_out"):
        assert (got[name].view(np.uint32) == fused[name].view(np.uint32)).all(), (what, name, "against map_ref")
    return got, want


@functools.lru_cache(maxsize=None)
def _drive(seed, sizes, extent=12.0):
    return M.drive(seed, sizes, extent=extent)


def _split(rows):
    """``rows`` rows over three clouds, the middle one empty, the last one a quarter."""
    return (rows - rows // 4, 0, rows // 4)


SIZES = [0, 1, 63, 64, 65, MP_TILE - 1, MP_TILE, MP_TILE + 1, 3 * MP_TILE + 5]


@pytest.mark.parametrize("rows,ring", [(r, 1) for r in SIZES + [MP_LEVEL + MP_TILE + 37]] + [(r, 0) for r in SIZES] + [(r, 2) for r in SIZES])
def test_row_counts(rows, ring):
    """Around the wave, the tile and the scan's first level; the small scenes are 3 m wide so that their voxels have neighbours."""
    points, offsets, poses, origin = _drive(3, _split(rows), 12.0 if rows > 1000 else 1.5)
    got, want = _both(points, offsets, poses, origin, 0.5, max(rows, 1), "%d rows, ring %d" % (rows, ring), ring=ring, min_support=3)
    assert want["num_out"].tolist()[1:] == [rows, 0, 0]
    if rows >= 63 and ring > 0:
        assert want["valid"].any()
    if rows > MP_LEVEL:                                # leaders on both sides of the level
        assert (want["leader"] >= MP_LEVEL + MP_TILE).any() and 1000 < want["valid"].sum() < want["V"]


def _cells(cells, voxel=1.0, at=0.5):
    """One row inside each of the given integer cells (n, 3), at the fraction ``at`` of the cell."""
    return ((np.asarray(cells, np.float64) + at) * voxel).astype(np.float32)


@pytest.mark.parametrize("ring", [0, 1, 2])
def test_dense_block_of_cells(ring):
    """5 x 5 x 5 cells around the origin with four rows each: the centre sees 1, 27 or 125 cells, a corner 1, 8 or 27."""
    axis = np.arange(-2, 3)
    cells = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(31)
    points = np.concatenate([_cells(cells, 0.5, rng.uniform(0.02, 0.98, size=(125, 3))) for _ in range(4)])
    got, want = _both(points, [0, 200, 500], M.identity_poses(2), np.zeros(3), 0.5, 500, "block, ring %d" % ring, ring=ring, min_support=4)
    assert want["V"] == 125 and (want["count"][:125] == 4).all()
    g = want["vox"]["g"]
    centre, corner = int(np.nonzero((g == 0).all(1))[0][0]), int(np.nonzero((g == -2).all(1))[0][0])
    assert got["support"][centre] == 4 * (2 * ring + 1) ** 3 and got["support"][corner] == 4 * (ring + 1) ** 3
    assert want["valid"].all() and np.isfinite(got["normal"][:125]).all()


def test_neighbours_across_the_origin_and_past_the_range_edges():
    """At voxel 1: voxels in the last cells of the range on x (2^20 - 1, 2^20 - 2) and in the first on y (-2^20).  A neighbour outside
    the range is skipped: a key formed from it would carry into the next axis' field and name the cell (-2^20, y + 1, z) -- which holds
    rows here, as do the cells a borrow would name."""
    top = float(2 ** 20)
    rows = []
    for x in (top - 0.25, top - 0.5, top - 0.75, top - 1.5, top - 1.25):
        rows += [[x, 0.5, 0.5], [x, 0.25, -0.5]]
    for y in (-top, -top + 0.5, -top + 1.25):
        rows += [[0.5, y, 0.5], [-0.5, y, 0.25], [-0.25, y, -0.75]]
    rows += [[-top + 0.5, 1.5, 0.5], [-top + 0.25, 1.25, 0.5], [-top + 0.5, 0.5, 0.5], [top - 0.5, -1.5, 0.5], [top - 0.5, 1.5, 1.5]]
    rows += [[0.25, -0.25, 0.25], [-0.25, 0.25, -0.25], [-0.75, -0.5, 0.5], [0.5, 0.5, -0.5], [0.75, 0.25, 0.5]]     # around the origin
    points = np.array(rows, np.float32)
    assert (points.astype(np.float64) == np.array(rows)).all()
    for ring in (1, 2):
        got, want = _both(points, [0, len(points)], M.identity_poses(1), np.zeros(3), 1.0, 64, "range edges, ring %d" % ring, ring=ring,
                          min_support=3)
        g = want["vox"]["g"]
        assert g[:, 0].max() == 2 ** 20 - 1 and g[:, 1].min() == -2 ** 20 and g[:, 0].min() == -2 ** 20 and want["num_out"][3] == 0
        edge = int(np.nonzero((g == [2 ** 20 - 1, 0, 0]).all(1))[0][0])
        assert got["support"][edge] == (11 if ring == 1 else 12) and want["valid"].sum() > 8      # never the rows at x = -2^20


def _block_scene(seed=3, rows=700, half=1.5):
    rng = np.random.default_rng(seed)
    points = rng.uniform(-half, half, size=(rows, 3)).astype(np.float32)
    return points, np.array([0, rows // 2, rows], np.int32), M.identity_poses(2, (3.0, -2.0, 1.0)), np.array([3.0, -2.0, 1.0])


def test_min_count_rule_and_min_support_edge():
    points, offsets, poses, origin = _block_scene()
    base = S.reference(points, offsets, poses, origin, 0.5, 700, 1, 1, 3)
    V = base["V"]
    for min_count in (2, 3, 5, int(base["count"].max()) + 1):
        got, want = _both(points, offsets, poses, origin, 0.5, 700, "min_count %d" % min_count, min_count=min_count, min_support=3)
        low = got["count"][:V] < min_count
        assert low.any() and np.isnan(got["normal"][:V][low]).all() and (got["support"][:V] <= base["support"][:V]).all()
        if min_count <= 5:
            assert (got["support"][:V][low] > 0).any() and not low.all()      # written although the voxel's own surfel is NaN
        else:
            assert low.all() and not got["support"].any()
    supports = set(base["support"][:V].tolist())
    edges = [s for s in sorted(supports) if s - 1 in supports and s >= 8]
    assert len(edges) >= 3
    for s in (edges[0], edges[len(edges) // 2], edges[-1]):
        got, want = _both(points, offsets, poses, origin, 0.5, 700, "min_support %d" % s, min_support=s)
        at, below = got["support"][:V] == s, got["support"][:V] == s - 1
        assert at.any() and below.any() and np.isfinite(got["eigen"][:V][at]).all() and np.isnan(got["eigen"][:V][below]).all()
    _both(points, offsets, poses, origin, 0.5, 700, "min_support 2^31 - 1", min_support=2 ** 31 - 1)


def test_every_row_in_one_voxel():
    """4096 rows in ONE voxel of 1 m: the highest contention and the largest second-moment sums of one slot."""
    rng = np.random.default_rng(11)
    points = (rng.uniform(0.0, 1.0, size=(4096, 3)) * np.array([0.999, 0.999, 0.999])).astype(np.float32)
    poses = M.identity_poses(2, (7.0, -3.0, 2.0))
    for max_voxels in (1, 8):
        got, want = _both(points, [0, 1000, 4096], poses, np.zeros(3), 1.0, max_voxels, "one voxel, max_voxels %d" % max_voxels)
        assert want["num_out"].tolist() == [1, 4096, 0, 0] and got["support"][0] == 4096 and np.isfinite(got["normal"][0]).all()
        assert int(want["vox"]["B"].max()) > 4096 * 255 * 255 // 4
    got, want = _both(points * np.float32(2.5), [0, 1000, 4096], poses, np.zeros(3), 1.0, 1, "27 voxels, max_voxels = 1")
    assert want["num_out"].tolist() == [-1, 4096, 0, 0] and not got["support"].any()


def test_every_row_its_own_voxel_and_overflow_by_one():
    """max_voxels == V: the fullest table the contract allows, and most neighbour lookups end at an empty slot."""
    rng = np.random.default_rng(12)
    cells = np.unique(rng.integers(-8, 8, size=(3000, 3)), axis=0)
    rng.shuffle(cells)
    V = len(cells)
    points = _cells(cells, 1.0, rng.uniform(0.05, 0.95, size=(V, 3)))
    poses = M.identity_poses(1)
    got, want = _both(points, [0, V], poses, np.zeros(3), 1.0, V, "max_voxels == V", min_support=6)
    assert want["num_out"].tolist() == [V, V, 0, 0] and (want["count"] == 1).all() and 100 < want["valid"].sum() < V
    got, want = _both(points, [0, V], poses, np.zeros(3), 1.0, V - 1, "max_voxels == V - 1")
    assert want["num_out"].tolist() == [-1, V, 0, 0]
    for name in FLOATS:
        assert (got[name].view(np.uint32) == M.NAN_WORD).all()
    assert not got["count"].any() and not got["support"].any()
    for max_voxels in (1, 2, V // 2):
        _both(points, [0, V], poses, np.zeros(3), 1.0, max_voxels, "overflow at max_voxels = %d" % max_voxels)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_cells_on_a_line_and_at_strides_of_powers_of_two(axis):
    line = np.zeros((1500, 3), np.int64)
    line[:, axis] = np.arange(-750, 750)
    strides = np.zeros((21 * 40, 3), np.int64)
    strides[:, axis] = (np.arange(40)[None, :] * (1 << np.arange(21))[:, None]).reshape(-1) % (1 << 20)
    strides[:, (axis + 1) % 3] = np.repeat(np.arange(21), 40) % 2
    both = (1 << np.arange(20))
    corner = np.stack([np.roll(np.array([s, -s, s - 1]), axis) for s in both])
    for name, cells in (("line", line), ("strides", strides), ("corner", corner)):
        points = np.concatenate([_cells(cells, 1.0, 0.25), _cells(cells[::-1], 1.0, [0.75, 0.5, 0.625])])     # every voxel twice
        got, want = _both(points, [0, len(points)], M.identity_poses(1), np.zeros(3), 1.0, len(points), "%s along axis %d" % (name, axis),
                          min_support=3)
        V = len(np.unique(cells, axis=0))
        assert want["num_out"].tolist() == [V, len(points), 0, 0] and (want["leader"] < len(cells)).all()
        assert name != "line" or (want["valid"].all() and (got["support"][:V] >= 4).all())


def test_degenerate_statistics():
    """Coincident rows: C == 0, every rotation is skipped, V stays the identity.  The eight corners of a cube: three equal eigenvalues.
    A line: the two smallest are tied at 0.  Each in a voxel of its own (voxel 1, values on the lattice of 1 / 256), ring 0 and ring 1."""
    q = 1.0 / 256
    same = np.repeat(np.array([[0.5, 0.25, 0.125]]), 9, 0)
    cube = np.array([[10 + (20 + 40 * i) * q, (20 + 40 * j) * q, (20 + 40 * k) * q] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    line = np.stack([20 + np.arange(3, 13) * 8 * q, np.full(10, 3 * q), np.full(10, 100 * q)], 1)
    skew = np.stack([30 + np.arange(8) * 9 * q, 5 * q + np.arange(8) * 18 * q, 7 * q + np.arange(8) * 18 * q], 1)     # along (1, 2, 2)
    points = np.concatenate([same, cube, line, skew]).astype(np.float32)
    for ring in (0, 1):
        got, want = _both(points, [0, 9, len(points)], M.identity_poses(2), np.zeros(3), 1.0, 16, "degenerate, ring %d" % ring, ring=ring)
        assert want["V"] == 4 and got["support"][:4].tolist() == [9, 8, 10, 8]
        assert got["eigen"][0].tolist() == [0.0, 0.0, 0.0] and got["normal"][0].tolist() == [1.0, 0.0, 0.0]
        assert got["centroid"][0].tolist() == [0.5, 0.25, 0.125]
        assert got["eigen"][1].tolist() == [(20 * q) ** 2] * 3 and got["normal"][1].tolist() == [1.0, 0.0, 0.0]
        assert got["eigen"][2][:2].tolist() == [0.0, 0.0] and got["eigen"][2][2] > 0 and got["normal"][2].tolist() == [0.0, 1.0, 0.0]
        assert got["eigen"][3][1] < 1e-12 * got["eigen"][3][2] and abs(float(got["normal"][3] @ np.array([1.0, 2.0, 2.0]))) < 1e-6


def _planar_scene():
    """Rows exactly on the plane x + 2 y + 2 z = 0 and on the lattice of voxel / 256 (voxel 1): a (2, -1, 0) + b (0, 1, -1), in 1 / 256."""
    rng = np.random.default_rng(41)
    ab = rng.integers(-380, 381, size=(3000, 2))
    p = (ab[:, :1] * np.array([2, -1, 0]) + ab[:, 1:] * np.array([0, 1, -1])) / 256.0
    return p.astype(np.float32), np.array([0, 1000, 3000], np.int32), M.identity_poses(2, (4.0, -2.0, 8.0)), np.array([4.0, -2.0, 8.0])


def _contracted(N, S1, S2):
    """C with fl(fl(S2 / N) - fl(mu_a mu_b)) contracted to ONE fused operation, fma(-mu_a, mu_b, fl(S2 / N)), rounded once."""
    mu, C = S.covariance(N, S1, S2)
    out = C.copy()
    for j in range(len(N)):
        for k, (a, b) in enumerate(S._AB):
            out[j, k] = float(F(float(np.float64(S2[j, k]) / np.float64(N[j]))) - F(float(mu[j, a])) * F(float(mu[j, b])))
    return mu, out


def test_planar_lattice_scene():
    points, offsets, poses, origin = _planar_scene()
    want = S.reference(points, offsets, poses, origin, 1.0, 3000, 1, 1, 6)
    ok = want["valid"]
    N, S1, S2 = (v[ok] for v in want["pooled"])
    mu, C = S.covariance(N, S1, S2)
    diag, vec = S.jacobi(C)
    negative = int((diag.min(1) < 0).sum())
    mu2, C2 = _contracted(N, S1, S2)
    lam2, n2 = S.order_and_normal(*S.jacobi(C2))
    fused = S.finish(want["vox"]["g"][ok], mu2, lam2, n2, 1.0)
    V = want["V"]
    mine = [want[name][:V][ok] for name in ("centroid", "normal", "eigen")]
    changed = int(np.any([(a.view(np.uint32) != b.view(np.uint32)).any(1) for a, b in zip(mine, fused)], 0).sum())
    print("planar scene: %d valid voxels, %d with a negative eigenvalue before the clamp, %d that a contracted C_ab changes"
          % (ok.sum(), negative, changed))
    assert ok.sum() > 30 and negative > ok.sum() // 10 and changed > ok.sum() // 3
    got, want = _both(points, offsets, poses, origin, 1.0, 3000, "planar", min_support=6)
    n = got["normal"][:V][ok].astype(np.float64)
    assert (np.abs(n - np.array([1.0, 2.0, 2.0]) / 3.0) < 1e-6).all() and (got["eigen"][:V][ok][:, 0] < 1e-12).all()


@pytest.mark.parametrize("voxel", [0.2, 0.5])
def test_utm_sized_poses_with_general_rotations(voxel):
    points, offsets, poses, origin = _drive(1, (5000,) * 4)
    points = points.copy()
    points[::97, 0] = np.nan
    got, want = _both(points, offsets, poses, origin, voxel, len(points), "UTM, voxel %g" % voxel, min_support=3)
    assert want["num_out"].tolist()[1:] == [19793, 207, 0] and np.abs(poses.reshape(-1, 3, 4)[:, 0, 3]).min() > 5e6
    assert want["valid"].sum() > (5000 if voxel == 0.5 else 200)
    got, want = _both(points, offsets, poses, np.zeros(3), voxel, len(points), "origin 0")
    assert want["num_out"].tolist() == [0, 0, 207, 19793]


def test_nan_and_structural_inputs():
    points, offsets, poses, origin = _drive(4, (300, 0, 0, 500, 0, 200), 2.0)
    kw = dict(min_support=3)
    got, want = _both(points, offsets, poses, origin, 0.5, 1000, "empty clouds between full ones", **kw)
    assert want["num_out"].tolist()[1:] == [1000, 0, 0] and want["valid"].sum() > 100
    broken = poses.copy()
    broken[3, 5] = np.nan                              # every row of cloud 3 is absent
    got, want = _both(points, offsets, broken, origin, 0.5, 1000, "a NaN pose", **kw)
    assert want["num_out"].tolist()[1:] == [500, 500, 0]
    rows = points.copy()
    rows[7, 1], rows[299, 2], rows[300, 0], rows[999] = np.nan, np.inf, -np.inf, np.nan
    got, want = _both(rows, offsets, poses, origin, 0.5, 1000, "non-finite rows", **kw)
    assert want["num_out"].tolist()[1:] == [996, 4, 0]
    got, want = _both(points, offsets, poses, np.array([0.0, np.nan, 0.0]), 0.5, 1000, "a NaN origin", **kw)
    assert want["num_out"].tolist() == [0, 0, 1000, 0]
    got, want = _both(points[:0], offsets[:1], poses[:0], origin, 0.5, 5, "no cloud, no row", **kw)
    assert want["num_out"].tolist() == [0, 0, 0, 0]
    got, want = _both(points, offsets[:1], poses[:0], origin, 0.5, 5, "no cloud, 1000 rows", **kw)
    assert want["num_out"].tolist() == [0, 0, 0, 0]
    inner = np.array([10, 310, 700], np.int32)
    got, want = _both(points, inner, poses[:2], origin, 0.5, 1000, "rows outside the clouds", **kw)
    assert want["num_out"].tolist()[1:] == [690, 0, 0] and want["leader"][0] == 10
    for at, value in ((0, -1), (2, 299), (6, 1001)):
        bad = offsets.copy()
        bad[at] = value
        got, want = _both(points, bad, poses, origin, 0.5, 1000, "invalid offsets", **kw)
        assert want["num_out"].tolist() == [-1, 0, 0, 0] and not got["support"].any()
    _both(points[:900], offsets, poses, origin, 0.5, 1000, "offsets[-1] behind num_rows", **kw)      # invalid: 1000 > 900


def test_position_independence_and_two_runs():
    """The same clouds behind 333 rows that belong to no cloud and in front of 77 more give the same bits; so do two runs."""
    points, offsets, poses, origin = _drive(7, (700, 0, 900), 2.0)
    got, want = _both(points, offsets, poses, origin, 0.5, 1600, "as it is", min_support=3)
    again = _raw(points, offsets, poses, origin, 0.5, 1600, min_support=3)
    for name in got:
        assert (got[name].view(np.uint32) == again[name].view(np.uint32)).all(), name
    wide = np.concatenate([SR.scan(999, 333), points, SR.scan(998, 77)])
    moved, _ = _both(wide, offsets + 333, poses, origin, 0.5, 1600, "inside a larger buffer", min_support=3)
    for name in got:
        assert (got[name].view(np.uint32) == moved[name].view(np.uint32)).all(), name


def _dev(points, offsets, poses, origin):
    dev = torch.device("cuda")
    return (torch.from_numpy(np.ascontiguousarray(points, np.float32)).to(dev), torch.from_numpy(np.asarray(offsets, np.int32)).to(dev),
            torch.from_numpy(np.ascontiguousarray(poses, np.float64)).to(dev), torch.from_numpy(np.ascontiguousarray(origin, np.float64)).to(dev))


NAMES = ("map_points", "count", "centroid", "normal", "eigen", "support", "num_out")


def _host(result):
    return {name: t.cpu().numpy() for name, t in zip(NAMES, result)}


def test_wrapper_against_the_entry_its_defaults_and_refusals():
    ops, L = H.pkg("ops"), H.pkg("lib")
    dev = torch.device("cuda")
    points, offsets, poses, origin = _drive(8, (1200, 800), 2.0)
    pts, off, pos, org = _dev(points, offsets, poses, origin)
    raw = _raw(points, offsets, poses, origin, 0.2, 2000)
    res = ops.fuse_surfels(pts, off, pos, origin=org)                         # voxel 0.2, max_voxels = rows, min_count 1, ring 1, min_support 8
    assert len(res) == 8 and all(t.is_cuda for t in res) and res[7] is org
    assert [tuple(t.shape) for t in res[:7]] == [(2000, 3), (2000,), (2000, 3), (2000, 3), (2000, 3), (2000,), (4,)]
    _check(_host(res), raw, "wrapper against the entry")
    assert np.isfinite(raw["normal"]).all(1).sum() > 30
    fused = ops.fuse_map(pts, off, pos, origin=org)                           # the three shared outputs: epcnet_map_fuse's bits
    for mine, theirs in ((res[0], fused[0]), (res[1], fused[1]), (res[6], fused[2])):
        assert torch.equal(mine.view(torch.int32), theirs.view(torch.int32))
    own = ops.fuse_surfels(pts, off, pos.reshape(2, 3, 4))                    # origin=None: the first translation, a device copy
    assert own[7].is_cuda and own[7].dtype == torch.float64 and own[7].tolist() == poses[0, 3::4].tolist()
    assert own[7].data_ptr() != pos.data_ptr() + 24
    _check(_host(own), raw, "origin=None")
    need = L.lib().epcnet_map_surfels_workspace_bytes(2000, 2, 1200)
    ref = S.reference(points, offsets, poses, origin, 0.5, 1200, 2, 2, 20)
    assert ref["num_out"][0] > 0
    for size in (need, need + 4096):
        ws = torch.full((size,), 0xAB, dtype=torch.uint8, device=dev)
        res = ops.fuse_surfels(pts, off, pos, voxel=0.5, origin=org, max_voxels=1200, min_count=2, ring=2, min_support=20, workspace=ws)
        _check(_host(res), ref, "a caller's workspace")
    with pytest.raises(L.EpcNetError) as e:
        ops.fuse_surfels(pts, off, pos, voxel=0.5, origin=org, max_voxels=1200, workspace=torch.empty(need - 1, dtype=torch.uint8, device=dev))
    assert e.value.status == L.EPC_ENOMEM
    for change in (dict(points=pts.cpu()), dict(offsets=off.cpu()), dict(offsets=off.long()), dict(poses=pos.float()), dict(poses=pos.cpu()),
                   dict(poses=pos[:1]), dict(origin=org.cpu()), dict(origin=org.float()), dict(origin=pos[0, :4].contiguous()),
                   dict(voxel=0.0), dict(voxel=float("nan")), dict(voxel=2.0 ** 21), dict(min_count=0), dict(max_voxels=0),
                   dict(max_voxels=2 ** 28 + 1), dict(ring=-1), dict(ring=3), dict(ring=0.5), dict(min_support=2), dict(min_support=2 ** 31),
                   dict(min_support=8.5), dict(workspace=torch.empty(1 << 20, dtype=torch.float32, device=dev)),
                   dict(workspace=torch.empty(1 << 20, dtype=torch.uint8))):
        with pytest.raises(L.EpcNetError):
            ops.fuse_surfels(**dict(dict(points=pts, offsets=off, poses=pos, origin=org), **change))
    with pytest.raises(L.EpcNetError) as e:
        ops.fuse_surfels(pts, off, pos.float())
    assert "float64" in str(e.value) and "never converted" in str(e.value)


def test_one_graph_replayed_on_other_data():
    """Captured once, replayed (twice each) after points, offsets, poses and origin were overwritten: another V, then the overflow, then
    the first scene again; the outputs hold junk before every replay."""
    ops, L = H.pkg("ops"), H.pkg("lib")
    dev = torch.device("cuda")
    scenes = [M.drive(21, (900, 600, 500), extent=3.0), M.drive(22, (100, 1500, 400), extent=2.0), M.drive(23, (700, 700, 600), extent=60.0)]
    refs = [M.reference(*s, 0.5, 2000) for s in scenes]
    cap = max(refs[0]["V"], refs[1]["V"])
    assert refs[0]["V"] != refs[1]["V"] and refs[2]["V"] > cap
    refs = [S.reference(*s, 0.5, cap, 2, 1, 5) for s in scenes]
    assert refs[2]["num_out"][0] == -1 and refs[0]["valid"].sum() > 50 and refs[1]["valid"].sum() > 50
    pts, off, pos, org = _dev(*scenes[0])
    ws = torch.empty(L.lib().epcnet_map_surfels_workspace_bytes(2000, 3, cap), dtype=torch.uint8, device=dev)
    kw = dict(voxel=0.5, origin=org, max_voxels=cap, min_count=2, ring=1, min_support=5, workspace=ws)
    ops.fuse_surfels(pts, off, pos, **kw)                                      # (warm-up)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.fuse_surfels(pts, off, pos, **kw)
    for scene, ref in ((scenes[1], refs[1]), (scenes[2], refs[2]), (scenes[0], refs[0])):
        for dst, src in zip((pts, off, pos, org), _dev(*scene)):
            dst.copy_(src)
        for replay in range(2):
            for t in out[:7]:
                t.fill_(7)                                                     # (a replay that wrote nothing would show)
            g.replay()
            torch.cuda.synchronize()
            _check(_host(out), ref, "replay %d" % replay)


def test_pipeline_submaps_into_surfels():
    """build_submaps -> fuse_surfels with sub_pose: equal to the restatement on what the device handed over."""
    ops = H.pkg("ops")
    dev = torch.device("cuda")
    poses, along = SR.trajectory(5, 24, step=1.0, wobble=0.01, general=False)
    points, offsets = SR.pack([SR.scan(300 + i, 400) for i in range(24)])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    sub_points, sub_offsets, status, sub_pose, info, num_out = ops.build_submaps(
        up(points), up(offsets), up(poses), along=up(along), length=6.0, spacing=3.0, max_submaps=8, out_rows=24 * 400 * 3,
        out=torch.zeros((24 * 400 * 3, 3), dtype=torch.float32, device=dev))
    assert 5 <= int(num_out[0]) < 8
    res = ops.fuse_surfels(sub_points, sub_offsets, sub_pose, voxel=0.5, min_count=2)
    want = S.reference(sub_points.cpu().numpy(), sub_offsets.cpu().numpy(), sub_pose.cpu().numpy(), res[7].cpu().numpy(), 0.5,
                       int(sub_points.shape[0]), 2, 1, 8)
    _check(_host(res), want, "sub_pose")
    assert 0 < want["num_out"][0] < want["num_out"][1] and want["valid"].any()
