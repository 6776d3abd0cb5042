"""epcnet_map_fuse on the device against its numpy restatement (tests/map_ref.py): every output goes into a poisoned buffer with slack
behind it, the workspace has exactly the size asked for, and everything is compared on BIT PATTERNS -- the definition is float64 with one
rounding per operation up to an integer lattice and integers from there on, so there is no tolerance anywhere.  Row counts around the
wave, the tile and the scan's first level; voxel structures that load the table (one voxel, every row its own, overflow by one, lines and
strides of 2^k); the arithmetic (rows exactly on cell faces, the range edges, UTM-sized poses, rows whose cell sits in float64's last
bit); and the plumbing (the wrapper, a graph replayed on other data, the pipeline end to end).

What a contracted multiply-add would do: the scene of ``map_ref.face_scene`` holds 48 rows (of 768; one per cloud and axis) whose cell
changes when fl(fl(fl(R0 x) + fl(R1 y)) + fl(R2 z)) is contracted to two fused operations -- found on the CPU with the restatement and
exact fractions (``map_ref.contracted``); test_rows_whose_cell_sits_in_the_last_bit re-counts them before it runs the device."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import helpers as H
import map_ref as M
import stage_ref as S
import submap_ref as SR

pytestmark = pytest.mark.gpu

MP_TILE = 256            # MP_TILE of csrc/map.hip: the rows of one insert / count / emit tile
MP_LEVEL = 256 * 256     # MP_TILE * MP_GROUP: the rows behind which the leaders' scan takes its second level


def _up(a, dtype, dev):
    a = np.ascontiguousarray(a, dtype)
    if a.size == 0:
        return torch.zeros(12, dtype=torch.float64, device=dev).view(torch.from_numpy(a).dtype)      # a pointer that is never followed
    return torch.from_numpy(a).to(dev)


def _raw(points, offsets, poses, origin, voxel, max_voxels, min_count=1, num_rows=None):
    """The entry itself on poisoned outputs and a workspace of exactly the size asked for -> the outputs as host arrays after the checks
    that nothing was written behind any of them."""
    L = H.pkg("lib")
    dev = torch.device("cuda")
    num_rows = len(points) if num_rows is None else num_rows
    C = len(offsets) - 1
    pts, off = _up(points, np.float32, dev), _up(offsets, np.int32, dev)
    pos, org = _up(np.asarray(poses).reshape(-1, 12), np.float64, dev), _up(origin, np.float64, dev)
    need = L.lib().epcnet_map_fuse_workspace_bytes(num_rows, C, max_voxels)
    assert need > 0
    out, count = S.Poisoned((max_voxels, 3), torch.float32, dev), S.Poisoned((max_voxels,), torch.int32, dev)
    num_out, ws = S.Poisoned((4,), torch.int32, dev), S.Poisoned((need,), torch.uint8, dev)
    params = (ctypes.c_double * 8)(voxel, float(min_count))
    L.run.epcnet_map_fuse(pts, off, num_rows, C, pos, org, params, max_voxels, out.t, count.t, num_out.t, ws.t, need)
    torch.cuda.synchronize()
    for p in (out, count, num_out, ws):
        assert p.untouched()
    return dict(map_points=out.t.cpu().numpy(), count=count.t.cpu().numpy(), num_out=num_out.t.cpu().numpy())


def _check(got, want, what):
    assert got["num_out"].tolist() == want["num_out"].tolist(), (what, got["num_out"].tolist(), want["num_out"].tolist())
    assert (got["count"] == want["count"]).all(), (what, "count", int((got["count"] != want["count"]).sum()))
    differ = (got["map_points"].view(np.uint32) != want["map_points"].view(np.uint32)).any(1).nonzero()[0]
    assert differ.size == 0, (what, "%d rows differ, the first is row %d" % (differ.size, int(differ[0])))


def _both(points, offsets, poses, origin, voxel, max_voxels, what, min_count=1, num_rows=None):
    want = M.reference(points, offsets, poses, origin, voxel, max_voxels, min_count, num_rows)
    got = _raw(points, offsets, poses, origin, voxel, max_voxels, min_count, num_rows)
    _check(got, want, what)
    return got, want


@functools.lru_cache(maxsize=None)
def _drive(seed, sizes):
    return M.drive(seed, sizes)


def _split(rows):
    """``rows`` rows over three clouds, the middle one empty, the last one a quarter."""
    return (rows - rows // 4, 0, rows // 4)


@pytest.mark.parametrize("rows", [0, 1, 63, 64, 65, MP_TILE - 1, MP_TILE, MP_TILE + 1, 3 * MP_TILE + 5, MP_LEVEL + 1, MP_LEVEL + MP_TILE + 37])
def test_row_counts(rows):
    points, offsets, poses, origin = _drive(3, _split(rows))
    got, want = _both(points, offsets, poses, origin, 0.5, max(rows, 1), "%d rows" % rows)
    assert want["num_out"].tolist()[1:] == [rows, 0, 0] and (rows < 1000 or 0 < want["V"] < rows)
    if rows > MP_LEVEL + 1:                            # leaders on both sides of the level, and voxels that span it
        assert (want["leader"] >= MP_LEVEL + MP_TILE).any() and want["count"].max() > 4


def test_no_cloud_empty_clouds_and_a_nan_pose():
    points, offsets, poses, origin = _drive(4, (300, 0, 0, 500, 0, 200))
    got, want = _both(points, offsets, poses, origin, 0.5, 1000, "empty clouds between full ones")
    assert want["num_out"].tolist()[1:] == [1000, 0, 0]
    broken = poses.copy()
    broken[3, 5] = np.nan                              # every row of cloud 3 is absent
    got, want = _both(points, offsets, broken, origin, 0.5, 1000, "a NaN pose")
    assert want["num_out"].tolist()[1:] == [500, 500, 0]
    rows = points.copy()
    rows[7, 1], rows[299, 2], rows[300, 0], rows[999] = np.nan, np.inf, -np.inf, np.nan
    got, want = _both(rows, offsets, poses, origin, 0.5, 1000, "non-finite rows")
    assert want["num_out"].tolist()[1:] == [996, 4, 0]
    got, want = _both(points, offsets, poses, np.array([0.0, np.nan, 0.0]), 0.5, 1000, "a NaN origin")
    assert want["num_out"].tolist() == [0, 0, 1000, 0]
    # no cloud at all, with and without rows; rows in front of offsets[0] and behind offsets[-1] belong to no cloud
    got, want = _both(points[:0], offsets[:1], poses[:0], origin, 0.5, 5, "no cloud, no row")
    assert want["num_out"].tolist() == [0, 0, 0, 0]
    got, want = _both(points, offsets[:1], poses[:0], origin, 0.5, 5, "no cloud, 1000 rows")
    assert want["num_out"].tolist() == [0, 0, 0, 0]
    inner = np.array([10, 310, 700], np.int32)
    got, want = _both(points, inner, poses[:2], origin, 0.5, 1000, "rows outside the clouds")
    assert want["num_out"].tolist()[1:] == [690, 0, 0] and want["leader"][0] == 10
    # invalid offsets: the whole call fails
    for at, value in ((0, -1), (2, 299), (6, 1001)):
        bad = offsets.copy()
        bad[at] = value
        got, want = _both(points, bad, poses, origin, 0.5, 1000, "invalid offsets")
        assert want["num_out"].tolist() == [-1, 0, 0, 0]
    _both(points[:900], offsets, poses, origin, 0.5, 1000, "offsets[-1] behind num_rows")      # invalid: 1000 > 900


def test_every_row_in_one_voxel():
    """4096 rows in ONE voxel of 1 m: the highest contention; three sums of 4096 terms decide the bits."""
    rng = np.random.default_rng(11)
    points = (rng.uniform(0.0, 1.0, size=(4096, 3)) * np.array([0.999, 0.999, 0.999])).astype(np.float32)
    poses = M.identity_poses(2, (7.0, -3.0, 2.0))
    got, want = _both(points, [0, 1000, 4096], poses, np.zeros(3), 1.0, 8, "one voxel")
    assert want["num_out"].tolist() == [1, 4096, 0, 0] and want["count"][0] == 4096
    got, want = _both(points, [0, 1000, 4096], poses, np.zeros(3), 1.0, 1, "one voxel, max_voxels = 1")
    assert want["num_out"].tolist() == [1, 4096, 0, 0]
    got, want = _both(points * np.float32(2.5), [0, 1000, 4096], poses, np.zeros(3), 1.0, 1, "27 voxels, max_voxels = 1")
    assert want["num_out"].tolist() == [-1, 4096, 0, 0] and want["V"] == 27


def _cells(cells, voxel=1.0):
    """One row in the middle of each of the given integer cells (n, 3)."""
    return ((np.asarray(cells, np.float64) + 0.5) * voxel).astype(np.float32)


def test_every_row_its_own_voxel_and_overflow_by_one():
    rng = np.random.default_rng(12)
    cells = np.unique(rng.integers(-40, 40, size=(3000, 3)), axis=0)
    rng.shuffle(cells)
    V = len(cells)
    points = _cells(cells)
    poses = M.identity_poses(1)
    got, want = _both(points, [0, V], poses, np.zeros(3), 1.0, V, "max_voxels == V")       # the fullest table the contract allows
    assert want["num_out"].tolist() == [V, V, 0, 0] and (want["count"] == 1).all() and (want["leader"] == np.arange(V)).all()
    got, want = _both(points, [0, V], poses, np.zeros(3), 1.0, V - 1, "max_voxels == V - 1")
    assert want["num_out"].tolist() == [-1, V, 0, 0]
    assert (got["map_points"].view(np.uint32) == M.NAN_WORD).all() and not got["count"].any()
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
        points = np.concatenate([_cells(cells), _cells(cells[::-1])])          # every voxel twice: the leader is in the first half
        got, want = _both(points, [0, len(points)], M.identity_poses(1), np.zeros(3), 1.0, len(points), "%s along axis %d" % (name, axis))
        V = len(np.unique(cells, axis=0))
        assert want["num_out"].tolist() == [V, len(points), 0, 0] and (want["leader"] < len(cells)).all()


def test_two_clouds_in_the_same_voxels_and_a_shuffled_order():
    """Cloud 1 is cloud 0's world points expressed in another frame (a quarter turn about z and an integer shift: exact), so both land in
    the same voxels: every leader comes from cloud 0.  Then the rows shuffled: the same voxel set under another numbering."""
    rng = np.random.default_rng(13)
    a = (rng.integers(-64, 64, size=(2000, 3)) / 4.0 + 0.125).astype(np.float32)
    turn = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    t = np.array([5.0, -7.0, 2.0])
    b = ((a.astype(np.float64) - t) @ turn).astype(np.float32)                # R b + t == a
    poses = np.concatenate([M.identity_poses(1), np.concatenate([turn, t[:, None]], 1).reshape(1, 12)])
    points = np.concatenate([a, b])
    got, want = _both(points, [0, 2000, 4000], poses, np.zeros(3), 0.5, 4000, "two clouds")
    V = want["V"]
    assert (want["leader"] < 2000).all() and (want["count"][:V] % 2 == 0).all() and V < 2000
    perm = rng.permutation(2000)
    moved = np.concatenate([a[perm], b])
    got2, want2 = _both(moved, [0, 2000, 4000], poses, np.zeros(3), 0.5, 4000, "shuffled")
    assert want2["V"] == V and not (got2["map_points"].view(np.uint32) == got["map_points"].view(np.uint32)).all()
    as_set = lambda g: sorted(map(tuple, np.concatenate([g["map_points"][:V].view(np.uint32), g["count"][:V, None].astype(np.uint32)], 1).tolist()))
    assert as_set(got) == as_set(got2)


def test_lattice_scene_with_rows_on_cell_faces():
    points, offsets, poses, origin = M.lattice_scene()
    _both(points, offsets, poses, origin, 0.75, len(points), "lattice, voxel 0.75")
    got, want = _both(points, offsets, poses, origin, 0.5, len(points), "lattice, voxel 0.5")
    voxels, _ = M.exact_map(points, offsets, poses.reshape(-1, 3, 4), origin, 0.5)
    assert want["V"] == len(voxels) and got["count"][:len(voxels)].tolist() == [n for _, n, _ in voxels]
    # the rows at x = -0.5, -0.25 (cell -1), -0.0, 0.25 (cell 0) and 0.5 (cell 1): a face belongs to the cell above it
    kind, w = M.lattice(points, offsets, poses, origin, 0.5)
    n = int(offsets[1])                                # (cloud 0: its translation is the origin)
    x, w = points[:n, 0], w[:n]
    assert set((w[x == -0.5, 0] >> 12).tolist()) == {-1} and set((w[x == 0.0, 0] >> 12).tolist()) == {0}
    assert set((w[x == 0.5, 0] >> 12).tolist()) == {1} and set((w[x == -0.25, 0] >> 12).tolist()) == {-1}


def test_range_edges():
    """At voxel 1: w = 2^32 - 1 and -2^32 are kept, 2^32 and -2^32 - 1 are out of range (float32 1048575.75 is exact)."""
    top, e = 1048575.75, 1.0 / 4096
    points = np.array([[top, 0, 0], [0, -1048576.0, 0], [0, 0, top], [top, -1048576.0, top], [1.0, 1.0, 1.0]], np.float32)
    offsets = [0, 5]
    got, want = _both(points, offsets, M.identity_poses(1, (0.25 - e, 0.0, 0.25 - e)), np.zeros(3), 1.0, 8, "the last lattice points")
    assert want["num_out"].tolist() == [5, 5, 0, 0]
    assert want["map_points"][3].tolist() == [float(np.float32(1048576.0 - e)), -1048576.0, float(np.float32(1048576.0 - e))]
    got, want = _both(points, offsets, M.identity_poses(1, (0.25, 0.0, 0.0)), np.zeros(3), 1.0, 8, "x one lattice step beyond")
    assert want["num_out"].tolist() == [3, 3, 0, 2]
    got, want = _both(points, offsets, M.identity_poses(1, (0.0, -e, 0.0)), np.zeros(3), 1.0, 8, "y one lattice step below")
    assert want["num_out"].tolist() == [3, 3, 0, 2]
    got, want = _both(points, offsets, M.identity_poses(1), np.array([0.0, 2.0 ** -20, 0.0]), 1.0, 8, "y below -2^32 after the floor")
    assert want["num_out"].tolist() == [3, 3, 0, 2]
    for voxel in (2.0 ** -20, 2.0 ** 20):                                    # the smallest and the largest voxel
        got, want = _both(points, offsets, M.identity_poses(1), np.zeros(3), voxel, 8, "voxel %g" % voxel)
        assert want["num_out"][3] == (5 if voxel < 1 else 0)


@pytest.mark.parametrize("voxel", [0.2, 0.5, 3.0])
def test_utm_sized_poses_with_general_rotations(voxel):
    points, offsets, poses, origin = _drive(1, (5000,) * 4)
    points = points.copy()
    points[::97, 0] = np.nan
    got, want = _both(points, offsets, poses, origin, voxel, len(points), "UTM, voxel %g" % voxel)
    assert want["num_out"].tolist()[1:] == [19793, 207, 0] and np.abs(poses.reshape(-1, 3, 4)[:, 0, 3]).min() > 5e6
    if voxel == 0.5:
        assert want["num_out"][0] == 16166
    # an origin 5.7e6 m from the drive: more than 2^20 voxels away, every finite row is out of range
    got, want = _both(points, offsets, poses, np.zeros(3), voxel, len(points), "origin 0")
    assert want["num_out"].tolist() == [0, 0, 207, 19793]


def test_rows_whose_cell_sits_in_the_last_bit():
    points, offsets, poses, origin, voxel, tuned = M.face_scene()
    P = poses.reshape(-1, 3, 4)
    kind, w = M.lattice(points, offsets, poses, origin, voxel)
    moved = 0
    for r in tuned:                                    # re-count: the contracted q_a lands in another cell
        c = r // 48
        q = [np.float64(M.contracted(P[c, a, :3], points[r])) + np.float64(P[c, a, 3]) for a in range(3)]
        moved += int(any(int(np.floor(q[a])) != int(w[r, a] >> 12) for a in range(3)))
    assert moved == len(tuned) == 48 and len(points) == 768
    got, want = _both(points, offsets, poses, origin, voxel, len(points), "cells in the last bit")
    assert want["num_out"].tolist()[1:] == [768, 0, 0]


def test_min_count():
    points, offsets, poses, origin = _drive(6, (3000, 3000))
    base = M.reference(points, offsets, poses, origin, 0.5, 6000)
    top = int(base["count"].max())
    assert top >= 3
    for min_count in (1, 2, top, top + 1, 2 ** 31 - 1):
        got, want = _both(points, offsets, poses, origin, 0.5, 6000, "min_count %d" % min_count, min_count=min_count)
        assert (want["count"] == base["count"]).all()
        gone = int(np.isnan(want["map_points"][:base["V"]]).all(1).sum())
        assert gone == int((base["count"][:base["V"]] < min_count).sum()) and (gone == base["V"]) == (min_count > top)


def test_position_independence_and_two_runs():
    """The same clouds behind 333 rows that belong to no cloud and in front of 77 more give the same bits; so do two runs."""
    points, offsets, poses, origin = _drive(7, (700, 0, 900))
    got, want = _both(points, offsets, poses, origin, 0.5, 1600, "as it is")
    again = _raw(points, offsets, poses, origin, 0.5, 1600)
    for name in got:
        assert (got[name].view(np.uint32) == again[name].view(np.uint32)).all(), name
    wide = np.concatenate([SR.scan(999, 333), points, SR.scan(998, 77)])
    moved, _ = _both(wide, offsets + 333, poses, origin, 0.5, 1600, "inside a larger buffer")
    for name in got:
        assert (got[name].view(np.uint32) == moved[name].view(np.uint32)).all(), name


def _dev(points, offsets, poses, origin):
    dev = torch.device("cuda")
    return (torch.from_numpy(np.ascontiguousarray(points, np.float32)).to(dev), torch.from_numpy(np.asarray(offsets, np.int32)).to(dev),
            torch.from_numpy(np.ascontiguousarray(poses, np.float64)).to(dev), torch.from_numpy(np.ascontiguousarray(origin, np.float64)).to(dev))


def _host(result):
    return dict(map_points=result[0].cpu().numpy(), count=result[1].cpu().numpy(), num_out=result[2].cpu().numpy())


def test_wrapper_against_the_entry_its_defaults_and_refusals():
    ops, L = H.pkg("ops"), H.pkg("lib")
    dev = torch.device("cuda")
    points, offsets, poses, origin = _drive(8, (1200, 800))
    pts, off, pos, org = _dev(points, offsets, poses, origin)
    raw = _raw(points, offsets, poses, origin, 0.2, 2000)
    res = ops.fuse_map(pts, off, pos, origin=org)                             # voxel 0.2, max_voxels = rows, min_count 1
    assert len(res) == 4 and all(t.is_cuda for t in res) and res[3] is org
    assert tuple(res[0].shape) == (2000, 3) and tuple(res[1].shape) == (2000,) and tuple(res[2].shape) == (4,)
    _check(_host(res), raw, "wrapper against the entry")
    own = ops.fuse_map(pts, off, pos.reshape(2, 3, 4))                        # origin=None: the first translation, a device copy
    assert own[3].is_cuda and own[3].dtype == torch.float64 and own[3].tolist() == poses[0, 3::4].tolist()
    assert own[3].data_ptr() != pos.data_ptr() + 24
    _check(_host(own), raw, "origin=None")
    # a caller's workspace, larger than needed and exactly as needed; one byte short is the library's refusal
    need = L.lib().epcnet_map_fuse_workspace_bytes(2000, 2, 500)
    for size in (need, need + 4096):
        ws = torch.full((size,), 0xAB, dtype=torch.uint8, device=dev)
        res = ops.fuse_map(pts, off, pos, voxel=0.5, origin=org, max_voxels=500, min_count=2, workspace=ws)
        _check(_host(res), M.reference(points, offsets, poses, origin, 0.5, 500, 2), "a caller's workspace")
    with pytest.raises(L.EpcNetError) as e:
        ops.fuse_map(pts, off, pos, voxel=0.5, origin=org, max_voxels=500, workspace=torch.empty(need - 1, dtype=torch.uint8, device=dev))
    assert e.value.status == L.EPC_ENOMEM
    for change in (dict(points=pts.cpu()), dict(offsets=off.cpu()), dict(offsets=off.long()), dict(poses=pos.float()), dict(poses=pos.cpu()),
                   dict(poses=pos[:1]), dict(origin=org.cpu()), dict(origin=org.float()), dict(origin=pos[0, :4].contiguous()),
                   dict(voxel=0.0), dict(voxel=float("nan")), dict(voxel=2.0 ** 21), dict(min_count=0), dict(max_voxels=0),
                   dict(max_voxels=2 ** 28 + 1), dict(workspace=torch.empty(1 << 20, dtype=torch.float32, device=dev)),
                   dict(workspace=torch.empty(1 << 20, dtype=torch.uint8))):
        with pytest.raises(L.EpcNetError):
            ops.fuse_map(**dict(dict(points=pts, offsets=off, poses=pos, origin=org), **change))
    with pytest.raises(L.EpcNetError) as e:
        ops.fuse_map(pts, off, pos.float())
    assert "float64" in str(e.value) and "never converted" in str(e.value)


def test_one_graph_replayed_on_other_data():
    """Captured once, replayed (twice each) after points, offsets, poses and origin were overwritten: another V, then the overflow."""
    ops, L = H.pkg("ops"), H.pkg("lib")
    dev = torch.device("cuda")
    scenes = [M.drive(21, (900, 600, 500)), M.drive(22, (100, 1500, 400)), M.drive(23, (700, 700, 600), extent=60.0)]
    refs = [M.reference(*s, 0.5, 2000) for s in scenes]
    cap = max(refs[0]["V"], refs[1]["V"])
    assert refs[0]["V"] != refs[1]["V"] and refs[2]["V"] > cap
    refs = [M.reference(*s, 0.5, cap, 2) for s in scenes]
    assert refs[2]["num_out"][0] == -1 and refs[0]["num_out"][0] > 0 and refs[1]["num_out"][0] > 0
    pts, off, pos, org = _dev(*scenes[0])
    ws = torch.empty(L.lib().epcnet_map_fuse_workspace_bytes(2000, 3, cap), dtype=torch.uint8, device=dev)
    kw = dict(voxel=0.5, origin=org, max_voxels=cap, min_count=2, workspace=ws)
    ops.fuse_map(pts, off, pos, **kw)                                          # (warm-up)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.fuse_map(pts, off, pos, **kw)
    for scene, ref in ((scenes[1], refs[1]), (scenes[2], refs[2]), (scenes[0], refs[0])):
        for dst, src in zip((pts, off, pos, org), _dev(*scene)):
            dst.copy_(src)
        for replay in range(2):
            out[0].fill_(7.0), out[1].fill_(-7), out[2].fill_(-7)             # (a replay that wrote nothing would show)
            g.replay()
            torch.cuda.synchronize()
            _check(_host(out), ref, "replay %d" % replay)


def test_pipeline_submaps_into_one_map():
    """build_submaps -> fuse_map with sub_pose, then with poses perturbed as close_loops would return them: each equals the restatement
    on what the device handed over."""
    ops = H.pkg("ops")
    dev = torch.device("cuda")
    poses, along = SR.trajectory(5, 24, step=1.0, wobble=0.01, general=False)
    points, offsets = SR.pack([SR.scan(300 + i, 400) for i in range(24)])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    sub_points, sub_offsets, status, sub_pose, info, num_out = ops.build_submaps(
        up(points), up(offsets), up(poses), along=up(along), length=6.0, spacing=3.0, max_submaps=8, out_rows=24 * 400 * 3,
        out=torch.zeros((24 * 400 * 3, 3), dtype=torch.float32, device=dev))
    assert 5 <= int(num_out[0]) < 8                                            # (the slots behind them: no rows, NaN poses)
    rng = np.random.default_rng(9)
    corrected = sub_pose.clone()
    corrected[:, 3::4] += torch.from_numpy(rng.normal(size=(8, 3)) * 0.05).to(dev)
    for name, pose in (("sub_pose", sub_pose), ("corrected", corrected)):
        res = ops.fuse_map(sub_points, sub_offsets, pose, voxel=0.5, min_count=2)
        want = M.reference(sub_points.cpu().numpy(), sub_offsets.cpu().numpy(), pose.cpu().numpy(), res[3].cpu().numpy(), 0.5,
                           int(sub_points.shape[0]), 2)
        _check(_host(res), want, name)
        V = int(want["num_out"][0])
        assert 0 < V < want["num_out"][1] and want["num_out"][2] == 0 and want["count"].max() > 4
    # the map goes on as it is: NaN rows are absent for the down-sampler
    xyz, st, info = ops.grid_downsample(res[0], torch.tensor([0, res[0].shape[0]], dtype=torch.int32, device=dev), 256, normalize=False)
    finite = int(torch.isfinite(res[0]).all(1).sum())
    assert int(info[0, 0]) == finite == int((want["count"] >= 2).sum()) and int(st[0]) == 0 and bool(torch.isfinite(xyz).all())
