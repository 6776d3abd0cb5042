"""epcnet_surfel_map_move on the device (include/epcnet_remap.h), in the manner of tests/test_gpu_growmap.py, whose poisoned buffers and
uploads it reuses: state, workspace and outputs of exactly the size asked for with slack behind them, everything compared on BIT
PATTERNS.  After every call the seven outputs and ``num_call`` are pinned to the restatement (tests/remap_ref.py) -- row for row, the
rows it leaves alone included --, and the voxels that hold rows to ``surfel_ref.reference`` over the rows currently in the map at their
current poses, matched by cell: the one-shot definition, never the code under test."""
import ctypes

import numpy as np
import pytest
import torch

import growmap_ref as G
import helpers as H
import localize_ref as Z
import map_ref as M
import register_ref as RR
import remap_ref as R
import stage_ref as SG
import submap_ref as SR
import surfel_ref as S
import test_gpu_growmap as TG

pytestmark = pytest.mark.gpu

MP_TILE, MP_LEVEL = TG.MP_TILE, TG.MP_LEVEL
FLOATS, NAMES, SENTINEL = TG.FLOATS, TG.NAMES, TG.SENTINEL


class _Dev(TG._Dev):
    """The grow tests' device map with the move entry: per call a poisoned workspace of exactly epcnet_surfel_map_move_workspace_bytes."""

    def move(self, points, offsets, old_poses, new_poses=None, params=None, max_voxels=None, state=None):
        points = np.asarray(points, np.float32).reshape(-1, 3)
        rows, C = len(points), len(offsets) - 1
        need = self.L.lib().epcnet_surfel_map_move_workspace_bytes(rows, C, self.ring)
        assert need > 0
        ws, call = SG.Poisoned((need,), torch.uint8, self.dev), SG.Poisoned((4,), torch.int32, self.dev)
        up = lambda p: TG._up(np.asarray(p).reshape(-1, 12), np.float64, self.dev)
        state = self.state if state is None else state
        self.L.run.epcnet_surfel_map_move(TG._up(points, np.float32, self.dev), TG._up(offsets, np.int32, self.dev), rows, C, up(old_poses),
                                          None if new_poses is None else up(new_poses), self.params if params is None else params,
                                          self.max_voxels if max_voxels is None else max_voxels, state.t, self.need, *self._arrays(), call.t,
                                          ws.t, need)
        torch.cuda.synchronize()
        for p in list(self.out.values()) + [ws, call, state]:
            assert p.untouched()
        return call.t.cpu().tolist()


class _Pair:
    """One map on the device and in the restatement: every call goes through both, ``num_call`` and all seven outputs are pinned."""

    def __init__(self, origin, voxel, max_voxels, what, **kw):
        self.args, self.kw, self.what = (origin, voxel, max_voxels), kw, what
        self.dev, self.ref = _Dev(origin, voxel, max_voxels, **kw), R.Map(origin, voxel, max_voxels, **kw)

    def _same(self, got, report, step):
        assert got == report["num_call"].tolist(), (self.what, step, "num_call", got, report["num_call"].tolist())
        TG._check(self.dev.host(), self.ref.out, "%s: %s" % (self.what, step))
        return report

    def add(self, call, step="add"):
        return self._same(self.dev.add(*call), self.ref.add(*call), step)

    def move(self, points, offsets, old_poses, new_poses=None, step="move"):
        return self._same(self.dev.move(points, offsets, old_poses, new_poses), self.ref.move(points, offsets, old_poses, new_poses), step)

    def by_cell(self, current, step):
        """The device's arrays against the one-shot reference over ``current`` = [(points, offsets, poses), ...], matched by cell."""
        origin, voxel, max_voxels = self.args
        want = S.reference(*G.concatenation(current), origin, voxel, max_voxels, self.kw.get("min_count", 1), self.kw.get("ring", 1),
                           self.kw.get("min_support", 8))
        assert want["num_out"][0] >= 0
        assert R.by_cell(self.dev.host(), self.ref.numbers_by_key(), want) is None, (self.what, step, R.by_cell(self.dev.host(), self.ref.numbers_by_key(), want))
        return want


def _three(rows, seed=3):
    """Three calls of ``rows`` rows (three clouds each, the middle one empty) along a drive, and the middle call's poses re-posed."""
    points, offsets, poses, origin = M.drive(seed, TG._split(rows) * 3, extent=1.5)
    calls = [TG._clouds(points, offsets, poses, 3 * k, 3 * k + 3) for k in range(3)]
    return calls, R.nudged(poses, (3, 4, 5))[3:6], origin


SIZES = [1, 63, 64, 65, MP_TILE - 1, MP_TILE, MP_TILE + 1, 3 * MP_TILE + 5]


@pytest.mark.parametrize("rows,ring", [(r, ring) for ring in (1, 0, 2) for r in SIZES])
def test_three_adds_then_the_middle_call_reposed(rows, ring):
    calls, moved, origin = _three(rows)
    p = _Pair(origin, 0.5, 4 * rows, "3 x %d rows, ring %d" % (rows, ring), ring=ring, min_support=3)
    for call in calls:
        p.add(call)
    report = p.move(calls[1][0], calls[1][1], calls[1][2], moved)
    want = p.by_cell([calls[0], (calls[1][0], calls[1][1], moved), calls[2]], "after the re-pose")
    assert want["num_out"].tolist()[1:] == [3 * rows, 0, 0] and report["num_call"][3] == 0
    if rows >= 63:
        assert report["num_call"][0] > 0 and len(report["emptied"]) > 0 and 0 < report["num_call"][1] <= rows
        assert 0 < report["num_call"][2] < p.dev.host()["num_out"][0]        # some solved again, never all


def test_clean_rows_are_not_written():
    """Before the move the rows of the voxels the restatement calls clean are overwritten with a sentinel: behind the call they still hold
    it, and the voxels that hold rows are the one-shot's."""
    points, offsets, poses, origin = TG._spread_scene()
    calls = [TG._clouds(points, offsets, poses, 0, 3), TG._clouds(points, offsets, poses, 3, 6)]
    moved = R.nudged(poses, (3, 4, 5))[3:]
    for ring in (0, 1, 2):
        p = _Pair(origin, 0.5, 640, "sentinel, ring %d" % ring, ring=ring, min_support=3)
        for call in calls:
            p.add(call)
        probe = R.Map(origin, 0.5, 640, ring=ring, min_support=3)
        for call in calls:
            probe.add(*call)
        clean = probe.move(calls[1][0], calls[1][1], calls[1][2], moved)["clean"]
        assert len(clean) > 20
        at = torch.from_numpy(clean).to(p.dev.dev)
        for name in NAMES[:6]:
            p.dev.out[name].t.view(torch.int32)[at] = SENTINEL
            p.ref.out[name].view(np.uint32)[clean] = SENTINEL
        report = p.move(calls[1][0], calls[1][1], calls[1][2], moved)       # (pins every row to the restatement, the sentinels included)
        assert (report["clean"] == clean).all() and len(report["dirty"]) > 10 and (len(report["dirty"]) > len(report["touched"])) == (ring > 0)
        got = p.dev.host()
        for name in NAMES[:6]:
            assert (got[name].view(np.uint32)[clean] == SENTINEL).all(), (ring, name, "a clean row was written")


def test_round_trip_then_everything_removed_and_added_again():
    calls, moved, origin = _three(300)
    p = _Pair(origin, 0.5, 1200, "round trip", min_support=3)
    for call in calls:
        p.add(call)
    first = p.dev.host()
    V = int(first["num_out"][0])
    there = p.move(calls[1][0], calls[1][1], calls[1][2], moved, "there")
    back = p.move(calls[1][0], calls[1][1], moved, calls[1][2], "back")
    again = p.dev.host()
    opened = int(there["num_call"][0])
    assert opened > 20 and back["num_call"][0] == 0 and again["num_out"].tolist() == [V + opened, 900, 0, 0]
    for name in NAMES[:6]:
        assert (again[name].view(np.uint32)[:V] == first[name].view(np.uint32)[:V]).all(), name
    assert not again["count"][V:].any()
    p.by_cell(calls, "back")
    for k, call in enumerate(calls):
        p.move(call[0], call[1], call[2], None, "remove %d" % k)
    empty = p.dev.host()
    assert empty["num_out"].tolist() == [V + opened, 0, 0, 0] and not empty["count"].any() and not empty["support"].any()
    for name in FLOATS:
        assert (empty[name].view(np.uint32) == M.NAN_WORD).all(), name
    for call in calls[::-1]:
        assert p.add(call, "add again")["num_call"][0] == 0
    last = p.dev.host()
    for name in NAMES[:6]:
        assert (last[name].view(np.uint32) == again[name].view(np.uint32)).all(), name
    p.by_cell(calls, "added again")


def test_contention_one_voxel_into_another_and_inside_itself():
    """1024 rows of ONE voxel of 1 m move into one other voxel; then 1024 rows move inside their voxel: the same slot takes the take-outs
    and the put-ins of one call."""
    rng = np.random.default_rng(11)
    points = (rng.uniform(0.0, 0.5, size=(1024, 3))).astype(np.float32)
    offsets = np.array([0, 300, 1024], np.int32)
    here, there, inside = M.identity_poses(2, (7.0, -3.0, 2.0)), M.identity_poses(2, (8.0, -3.0, 2.0)), M.identity_poses(2, (8.25, -2.75, 2.0))
    p = _Pair(np.zeros(3), 1.0, 8, "contention")
    assert p.add((points, offsets, here))["num_call"].tolist() == [1, 1024, 1, 0]
    assert p.move(points, offsets, here, there)["num_call"].tolist() == [1, 1024, 2, 0]
    got = p.dev.host()
    assert got["count"][:2].tolist() == [0, 1024] and got["support"][:2].tolist() == [1024, 1024] and got["num_out"].tolist() == [2, 1024, 0, 0]
    p.by_cell([(points, offsets, there)], "into another voxel")
    assert p.move(points, offsets, there, inside)["num_call"].tolist() == [0, 1024, 2, 0]
    assert p.dev.host()["count"][:2].tolist() == [0, 1024]
    p.by_cell([(points, offsets, inside)], "inside one voxel")
    one = _Pair(np.zeros(3), 1.0, 1, "contention, max_voxels 1", ring=0)
    one.add((points, offsets, there))
    assert one.move(points, offsets, there, inside)["num_call"].tolist() == [0, 1024, 1, 0]
    one.by_cell([(points, offsets, inside)], "max_voxels 1")


def test_identical_poses_write_nothing():
    calls, moved, origin = _three(300)
    p = _Pair(origin, 0.5, 1200, "identical poses", min_support=3)
    for call in calls:
        p.add(call)
    before = p.dev.host()
    for name in NAMES[:6]:
        p.dev.out[name].t.view(torch.int32)[:] = SENTINEL
    assert p.dev.move(*calls[1], calls[1][2].copy()) == [0, 0, 0, 0] == p.ref.move(*calls[1], calls[1][2].copy())["num_call"].tolist()
    got = p.dev.host()
    for name in NAMES[:6]:
        assert (got[name].view(np.uint32) == SENTINEL).all(), name
    assert got["num_out"].tolist() == before["num_out"].tolist()


def test_a_cloud_that_was_never_added_is_unmatched():
    calls, moved, origin = _three(300)
    p = _Pair(origin, 0.5, 1200, "never added", min_support=3)
    p.add(calls[0])
    p.add(calls[2])
    before = p.dev.host()
    far = calls[1][2].copy()
    far[:, 3::4] += 500.0
    for new in (R.nudged(far, (0, 1, 2)), None):
        assert p.move(calls[1][0], calls[1][1], far, new)["num_call"].tolist() == [0, 0, 0, 300]
        after = p.dev.host()
        for name in NAMES:
            assert (after[name].view(np.uint32) == before[name].view(np.uint32)).all(), name
    p.by_cell([calls[0], calls[2]], "unmatched")


def test_nan_poses_and_the_range_edge():
    calls, moved, origin = _three(300)
    p = _Pair(origin, 0.5, 1200, "kinds", min_support=3)
    for call in calls:
        p.add(call)
    first = p.dev.host()
    V = int(first["num_out"][0])
    pts, off, pose = calls[1]
    broken = pose.copy()
    broken[:, 5] = np.nan
    assert p.move(pts, off, pose, broken, "to NaN")["num_call"][:2].tolist() == [0, 0]
    assert p.dev.host()["num_out"].tolist() == [V, 600, 300, 0]
    p.by_cell([calls[0], (pts, off, broken), calls[2]], "a NaN new pose")
    assert p.move(pts, off, broken, pose, "from NaN")["num_call"][:2].tolist() == [0, 300]      # nothing leaves; the rows are put in
    back = p.dev.host()
    for name in NAMES:
        assert (back[name].view(np.uint32) == first[name].view(np.uint32)).all(), name
    away = pose.copy()
    away[:, 3] += 0.5 * 2.0 ** 21                       # 2^20 cells further on x: past the range, never wrapped
    assert p.move(pts, off, pose, away, "out of range")["num_call"][:2].tolist() == [0, 0]
    assert p.dev.host()["num_out"].tolist() == [V, 600, 0, 300]
    p.by_cell([calls[0], (pts, off, away), calls[2]], "out of range")
    edge = pose.copy()
    edge[:, 3] += 0.5 * (2.0 ** 20 - 64)                # back inside, within 64 cells of the end of the range on x: kept again
    report = p.move(pts, off, away, edge, "to the edge")
    assert report["num_call"][1] == 300 and p.dev.host()["num_out"].tolist()[1:] == [900, 0, 0]
    p.by_cell([calls[0], (pts, off, edge), calls[2]], "at the edge")


def test_overflow_through_voxels_a_repose_opens():
    calls, moved, origin = _three(300)
    probe = R.Map(origin, 0.5, 1200, min_support=3)
    for call in calls:
        probe.add(*call)
    V = int(probe.out["num_out"][0])
    opened = int(probe.move(calls[1][0], calls[1][1], calls[1][2], moved)["num_call"][0])
    assert opened > 20
    p = _Pair(origin, 0.5, V + opened, "max_voxels == claimed", min_support=3)
    for call in calls:
        p.add(call)
    assert p.move(calls[1][0], calls[1][1], calls[1][2], moved)["num_call"][0] == opened
    p.by_cell([calls[0], (calls[1][0], calls[1][1], moved), calls[2]], "the fullest table")
    p = _Pair(origin, 0.5, V + opened - 1, "max_voxels == claimed - 1", min_support=3)
    for call in calls:
        p.add(call)
    assert p.move(calls[1][0], calls[1][1], calls[1][2], moved)["num_call"][0] == -1
    got = p.dev.host()
    assert got["num_out"].tolist() == [-1, 900, 0, 0] and not got["count"].any() and not got["support"].any()
    for name in FLOATS:
        assert (got[name].view(np.uint32) == M.NAN_WORD).all()
    assert p.move(calls[1][0], calls[1][1], moved, calls[1][2], "back")["num_call"][0] == -1
    assert p.move(*calls[2], None, "remove")["num_call"][0] == -1
    assert p.add(calls[0], "add")["num_call"].tolist() == [-1, 300, 0, 0]
    assert p.dev.host()["num_out"].tolist() == [-1, 900, 0, 0]


def test_a_refused_call_changes_nothing():
    """Invalid offsets, params or max_voxels that differ from init's, a state init never wrote: -1, 0, 0, 0, and the seven outputs AND the
    state are what they were, bit for bit; the next valid call is the restatement's."""
    calls, moved, origin = _three(300)
    p = _Pair(origin, 0.5, 1200, "refusals", min_support=3)
    for call in calls:
        p.add(call)
    before, state = p.dev.host(), p.dev.state.t.clone()
    pts, off, pose = calls[1]
    refusals = []
    for at, value in ((1, 250), (0, -1), (3, 301)):
        bad = off.copy()
        bad[at] = value
        assert not M.valid(bad, len(pts))
        refusals.append(dict(offsets=bad))
    other = lambda **c: (ctypes.c_double * 8)(*[c.get(k, v) for k, v in (("voxel", 0.5), ("min_count", 1.0), ("ring", 1.0), ("min_support", 3.0))])
    refusals += [dict(params=other(voxel=0.5000000000000001)), dict(params=other(min_count=2.0)), dict(params=other(min_support=4.0)),
                 dict(max_voxels=1199), dict(state=SG.Poisoned((p.dev.need,), torch.uint8, p.dev.dev))]
    for change in refusals:
        for new in (moved, None):
            foreign = change.get("state")
            mine = foreign.t.clone() if foreign is not None else None
            got = p.dev.move(pts, change.get("offsets", off), pose, new, params=change.get("params"), max_voxels=change.get("max_voxels"), state=foreign)
            assert got == [-1, 0, 0, 0], (change, got)
            after = p.dev.host()
            for name in NAMES:
                assert (after[name].view(np.uint32) == before[name].view(np.uint32)).all(), (change, name)
            assert torch.equal(p.dev.state.t, state), (change, "the state")
            assert foreign is None or torch.equal(foreign.t, mine), "the foreign state"
    assert p.ref.move(pts, refusals[0]["offsets"], pose, moved)["num_call"].tolist() == [-1, 0, 0, 0]
    p.move(pts, off, pose, moved, "behind the refused calls")
    p.by_cell([calls[0], (pts, off, moved), calls[2]], "behind the refused calls")


def test_second_level_of_the_scan():
    """One move of 256 * 256 + 256 + 37 rows: its second cloud goes 50 m away, so leaders sit in front of the scan's first level and --
    the last 37 rows each open a voxel -- behind it."""
    rng = np.random.default_rng(17)
    big = MP_LEVEL + MP_TILE + 37
    dense = rng.uniform(-1.5, 1.5, size=(big - 37, 3))
    lone = np.stack([100.0 + 1.5 * np.arange(37), np.zeros(37), np.zeros(37)], 1) + 0.25
    points, offsets = np.concatenate([dense, lone]).astype(np.float32), np.array([0, 40000, big], np.int32)
    poses = M.identity_poses(2, (3.0, -2.0, 1.0))
    moved = poses.copy()
    moved[1, 7] += 50.0
    p = _Pair(np.array([3.0, -2.0, 1.0]), 0.5, 4096, "the scan's second level", min_support=3)
    added = p.add((points, offsets, poses))
    report = p.move(points, offsets, poses, moved)
    assert report["num_call"][0] > 37 + 200 and report["num_call"][1] == big - 40000 and report["num_call"][3] == 0
    assert len(report["emptied"]) == 37 and report["num_call"][2] <= p.dev.host()["num_out"][0] == added["num_call"][0] + report["num_call"][0]
    want = p.by_cell([(points, offsets, moved)], "moved")
    assert (want["leader"] >= MP_LEVEL + MP_TILE).sum() >= 37 and ((want["leader"] >= 40000) & (want["leader"] < MP_LEVEL)).sum() > 200


def test_one_captured_repose_replayed_three_times_on_other_poses():
    ops, L = H.pkg("ops"), H.pkg("lib")
    dev = torch.device("cuda")
    calls, moved, origin = _three(600, seed=21)
    pts, off, pose = calls[1]
    stops = [pose, moved, R.nudged(pose, (0, 2), seed=5), pose]              # three moves: there, further, back
    kw = dict(max_voxels=4500, voxel=0.5, origin=torch.from_numpy(origin).to(dev), min_count=1, ring=1, min_support=4)
    ws = torch.empty(L.lib().epcnet_surfel_map_move_workspace_bytes(600, 3, 1), dtype=torch.uint8, device=dev)
    d_pts, d_off, d_old = TG._dev(pts, off, stops[0])
    d_new = d_old.clone()
    warm = ops.SurfelMap(**kw)                                               # (warm-up, on a map of its own)
    warm.add(d_pts, d_off, d_old)
    warm.repose(d_pts, d_off, d_old, d_new, workspace=ws)
    m, ref = ops.SurfelMap(**kw), R.Map(origin, 0.5, 4500, 1, 1, 4)
    for call in calls:
        m.add(*TG._dev(*call))
        ref.add(*call)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        num_call = m.repose(d_pts, d_off, d_old, d_new, workspace=ws)
    for k in range(3):
        d_old.copy_(torch.from_numpy(np.ascontiguousarray(stops[k])).to(dev))
        d_new.copy_(torch.from_numpy(np.ascontiguousarray(stops[k + 1])).to(dev))
        g.replay()
        torch.cuda.synchronize()
        report = ref.move(pts, off, stops[k], stops[k + 1])
        assert num_call.tolist() == report["num_call"].tolist(), k
        TG._check(TG._host(m), ref.out, "replay %d" % k)
        want = S.reference(*G.concatenation([calls[0], (pts, off, stops[k + 1]), calls[2]]), origin, 0.5, 4500, 1, 1, 4)
        assert R.by_cell(TG._host(m), ref.numbers_by_key(), want) is None, k
        assert report["num_call"][1] > 0 and report["num_call"][2] > 0


def test_wrapper_remove_repose_and_their_refusals():
    ops, L = H.pkg("ops"), H.pkg("lib")
    dev = torch.device("cuda")
    calls, moved, origin = _three(300)
    a, b = TG._dev(*calls[0]), TG._dev(*calls[1])
    new = torch.from_numpy(np.ascontiguousarray(moved)).to(dev)
    m = ops.SurfelMap(1200, voxel=0.5, origin=torch.from_numpy(origin).to(dev), min_support=3)
    ref = R.Map(origin, 0.5, 1200, 1, 1, 3)
    tensors = [getattr(m, n) for n in NAMES]
    m.add(*a), m.add(*b), ref.add(*calls[0]), ref.add(*calls[1])
    got = m.repose(b[0], b[1], b[2].reshape(3, 3, 4), new.reshape(3, 3, 4))
    assert got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == (4,)
    assert got.tolist() == ref.move(*calls[1], moved)["num_call"].tolist() and got[0] > 0
    TG._check(TG._host(m), ref.out, "repose")
    assert all(getattr(m, n) is t for n, t in zip(NAMES, tensors))
    need = L.lib().epcnet_surfel_map_move_workspace_bytes(300, 3, 1)
    got = m.remove(a[0], a[1], a[2], workspace=torch.full((need,), 0xAB, dtype=torch.uint8, device=dev))
    assert got.tolist() == ref.move(*calls[0])["num_call"].tolist() and got.tolist()[:2] == [0, 0] and got[2] > 0
    TG._check(TG._host(m), ref.out, "remove")
    want = S.reference(calls[1][0], calls[1][1], moved, origin, 0.5, 1200, 1, 1, 3)
    assert R.by_cell(TG._host(m), ref.numbers_by_key(), want) is None
    kept = TG._host(m)
    args = dict(points=b[0], offsets=b[1], old_poses=new, new_poses=b[2])
    with pytest.raises(L.EpcNetError) as e:
        m.repose(**dict(args, workspace=torch.empty(need - 1, dtype=torch.uint8, device=dev)))
    assert e.value.status == L.EPC_ENOMEM
    for change in (dict(old_poses=new.float()), dict(new_poses=b[2].float())):
        with pytest.raises(L.EpcNetError) as e:
            m.repose(**dict(args, **change))
        assert "float64" in str(e.value) and "never converted" in str(e.value)
    with pytest.raises(L.EpcNetError) as e:
        m.remove(b[0], b[1], new.float())
    assert "float64" in str(e.value)
    for change in (dict(new_poses=b[2].reshape(3, 3, 4)), dict(new_poses=b[2][:2]), dict(old_poses=new[:0], new_poses=b[2][:0]),
                   dict(points=b[0].cpu()), dict(offsets=b[1].cpu()), dict(offsets=b[1].long()), dict(old_poses=new.cpu()),
                   dict(new_poses=b[2].cpu()), dict(workspace=torch.empty(1 << 20, dtype=torch.float32, device=dev)),
                   dict(workspace=torch.empty(1 << 20, dtype=torch.uint8))):
        with pytest.raises(L.EpcNetError):
            m.repose(**dict(args, **change))
    TG._check(TG._host(m), kept, "refusals change nothing")
    bare = ops.SurfelMap(1200, voxel=0.5)                                    # origin=None and no add: there is no map to move rows in
    for call in (lambda: bare.remove(*a), lambda: bare.repose(b[0], b[1], b[2], new)):
        with pytest.raises(L.EpcNetError) as e:
            call()
        assert "origin" in str(e.value)
    assert bare.origin is None


def test_the_loop_with_a_submap_that_drifted():
    """Three submaps in the map, the middle one at a drifted pose; ``repose`` takes it to its true pose; index_surfels and localize_scans
    of one 1024-row cloud then find the truth within the bound of the grow tests' loop, and the voxels that hold rows are fuse_surfels'
    over the three submaps at their true poses."""
    ops = H.pkg("ops")
    dev = torch.device("cuda")
    patches = [q.astype(np.float32) for q in Z.plane_patches(5, *Z.THREE_PLANES, 3000)]
    sub_points, sub_offsets = SR.pack(patches)
    fixed = M.identity_poses(3)
    drifted = fixed.copy()
    drifted[1] = RR.pose_of(2.0, -1.0, 1.5, (0.25, -0.2, 0.15))
    truth = RR.pose_of(3.0, -2.0, 1.5, (0.05, -0.04, 0.03))
    cloud = Z.plane_scan(77, *Z.THREE_PLANES, 1024, truth)
    origin = torch.zeros(3, dtype=torch.float64, device=dev)
    m = ops.SurfelMap(max_voxels=16384, voxel=0.2, origin=origin)
    pts, off, before = TG._dev(sub_points, sub_offsets, drifted)
    after = torch.from_numpy(fixed).to(dev)
    m.add(pts, off, before)
    num_call = m.repose(pts, off, before, after)
    index, num = ops.index_surfels(m.map_points, m.centroid, m.normal, 0.2)
    seeds = torch.from_numpy(np.asarray(RR.IDENTITY, np.float64).reshape(1, 1, 12)).to(dev)
    scan = torch.from_numpy(cloud).to(dev)
    pose, fit, hessian, info, status = ops.localize_scans(scan[None], index, m.centroid, m.normal, seeds)
    assert status.tolist() == [0] and torch.isfinite(pose).all() and int(num[0]) > 500
    assert float((pose.cpu().reshape(3, 4)[:, 3] - torch.from_numpy(np.asarray(truth).reshape(3, 4)[:, 3])).abs().max()) < 0.05
    call = num_call.tolist()
    assert call[0] > 0 and 0 < call[1] <= 3000 and call[2] > 0 and call[3] == 0
    fused = ops.fuse_surfels(pts, off, after, voxel=0.2, origin=origin, max_voxels=16384)
    assert m.num_out.tolist()[1:] == fused[6].tolist()[1:] and int(m.num_out[0]) > int(fused[6][0]) > 0

    def rows_of(arrays):
        """The voxels that hold rows as sorted rows of bit patterns: the numbers differ, the cells' contents do not."""
        cols = [t.cpu().numpy().view(np.int32).reshape(len(t), -1) for t in arrays]
        table = np.concatenate(cols, 1)[cols[1][:, 0] > 0]
        return table[np.lexsort(table.T[::-1])]

    mine, theirs = rows_of([getattr(m, n) for n in NAMES[:6]]), rows_of(fused[:6])
    assert mine.shape == theirs.shape and (mine == theirs).all()
