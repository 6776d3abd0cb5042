"""epcnet_scan_deskew and epcnet_pose_interp on the device against their numpy restatement (tests/stamps_ref.py): every output goes into a
poisoned buffer with guard bytes IN FRONT of it and behind it and is compared on BIT PATTERNS -- the definition is integer times, float64
with one rounding per operation, one correctly rounded division per pose and one rounding to float32, so there is no tolerance anywhere.
Scans around the row kernel's tile, one scan across three tiles, more scans in a tile than one batch of pairs lists, empty scans, rows in
front of the first scan, brackets reached from near and far in both directions, times on knots and on both ends of the odometry and one
nanosecond outside, a drop-out of exactly the gap and one above, the longer arc, non-finite poses and rows, the call without point_dt, the
whole-call failures, the interpolation alone, two runs, one captured graph replayed on other data, and the engine's entry.

Outside the bit contract: ops.travel_along (torch, float64) against a numpy loop, within 1e-9 m."""
import functools

import numpy as np
import pytest
import torch

import helpers as H
import stamps_ref as R
import submap_ref as SR
from helpers import GUARD, Guarded, O

pytestmark = pytest.mark.gpu

T = 1024        # ST_TILE of csrc/stamps.hip: the rows of one tile of the row kernel
PAIRS = 32      # ST_PAIRS: the (scan, row range) pairs a tile lists at a time
GAP = 500_000_000
MS = 1_000_000


def _poison(t):
    return bool((t.contiguous().view(torch.uint8) == 0xFF).all())


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _raw(points, offsets, scan_time, pose_time, pose, point_dt, gap=GAP, num_rows=None):
    """The entry itself on guarded, poisoned outputs and a workspace of exactly the size asked for -> the outputs as host tensors
    (points_out whole, poison included) after the checks that nothing was written in front of or behind any of them."""
    L = H.pkg("lib")
    dev = torch.device("cuda")
    num_rows = len(points) if num_rows is None else num_rows
    S = len(offsets) - 1
    pts = _up(np.asarray(points, np.float32).reshape(-1, 3), dev) if len(points) else torch.zeros((1, 3), dtype=torch.float32, device=dev)
    off, st = _up(np.asarray(offsets, np.int32), dev), _up(np.asarray(scan_time, np.int64), dev)
    pt, po = _up(np.asarray(pose_time, np.int64), dev), _up(np.asarray(pose, np.float64), dev)
    dt = None if point_dt is None else (_up(np.asarray(point_dt, np.int32), dev) if len(point_dt) else torch.zeros(1, dtype=torch.int32, device=dev))
    need = L.lib().epcnet_deskew_workspace_bytes(S, len(pose_time), num_rows)
    assert need > 0 and need % 16 == 0
    out = Guarded((max(num_rows, 1), 3), torch.float32, dev)
    scan_pose, status, ws = Guarded((S, 12), torch.float64, dev), Guarded((S,), torch.int32, dev), Guarded((need,), torch.uint8, dev)
    L.run.epcnet_scan_deskew(pts, off, num_rows, S, dt, st, pt, po, len(pose_time), gap, None if dt is None else out.t, scan_pose.t, status.t,
                             ws.t, need)
    torch.cuda.synchronize()
    for g in (out, scan_pose, status, ws):
        assert g.intact()
    return dict(points_out=out.t[:num_rows].cpu(), scan_pose=scan_pose.t.cpu(), status=status.t.cpu())


def _check(got, want, what, with_rows=True):
    assert _same(got["scan_pose"], torch.from_numpy(want["scan_pose"])), (what, "scan_pose")
    assert got["status"].tolist() == want["status"].tolist(), (what, "status", got["status"].tolist(), want["status"].tolist())
    if not with_rows:
        assert _poison(got["points_out"]), (what, "rows were written without point_dt")
        return
    first, n = want["first"], len(want["points_out"])
    differ = (_bits(got["points_out"][first:first + n]) != _bits(torch.from_numpy(want["points_out"]))).any(1).nonzero()
    assert differ.numel() == 0, (what, "%d rows differ, the first is row %d of the written ones" % (differ.numel(), int(differ[0])))
    assert _poison(got["points_out"][:first]) and _poison(got["points_out"][first + n:]), (what, "rows outside the scans were written")


def _both(points, offsets, scan_time, pose_time, pose, point_dt, what, gap=GAP, num_rows=None):
    want = R.deskew_reference(points, offsets, scan_time, pose_time, pose, point_dt, gap, num_rows=num_rows)
    got = _raw(points, offsets, scan_time, pose_time, pose, point_dt, gap, num_rows=num_rows)
    _check(got, want, what, with_rows=point_dt is not None)
    return got, want


@functools.lru_cache(maxsize=None)
def _odometry(seed=1, num_poses=1000):
    """10 s of odometry on a jittered 10 ms clock, general rotations, quaternions unit only up to 2 %."""
    return R.odometry(seed, num_poses, jitter_ns=300_000)


def _scans(sizes, seed, pose_time, first_knot=20, every=5, sweep_ms=55):
    """Scans of the given sizes stamped `every` knots apart (3 ms behind a knot), rows stamped up to +- sweep_ms around the scan."""
    rng = np.random.default_rng([seed, len(sizes)])
    points, offsets = SR.pack([SR.scan(seed + i, m) for i, m in enumerate(sizes)])
    scan_time = np.array([pose_time[first_knot + every * i] + 3 * MS for i in range(len(sizes))], np.int64)
    dt = rng.integers(-sweep_ms * MS, sweep_ms * MS, size=len(points)).astype(np.int32)
    return points, offsets, scan_time, dt


@pytest.mark.parametrize("rows", [T - 1, T, T + 1, 2 * T + 3])
def test_one_scan_around_the_tile(rows):
    pose_time, pose = _odometry()
    points, offsets, scan_time, dt = _scans((rows,), 10, pose_time)
    got, want = _both(points, offsets, scan_time, pose_time, pose, dt, "%d rows" % rows)
    assert want["status"].tolist() == [0] and not np.isnan(want["points_out"]).any()


def test_rows_in_front_one_scan_across_three_tiles_and_empty_scans():
    pose_time, pose = _odometry()
    # offsets[0] = 500 > 0; empty scans at the front, in the middle (two in a row) and at the end; scan 4 holds the rows
    # [T - 24, 2 T + 176): three tiles; offsets[S] lies below num_rows
    sizes = (0, 500, 0, 0, T + 200, 7, 0)
    points, offsets, scan_time, dt = _scans(sizes, 20, pose_time)
    lead, trail = SR.scan(900, 500), SR.scan(901, 300)
    points = np.concatenate([lead, points, trail])
    dt = np.concatenate([np.zeros(500, np.int32), dt, np.zeros(300, np.int32)])
    offsets = (offsets + 500).astype(np.int32)
    assert offsets[4] // T == 0 and (offsets[5] - 1) // T == 2
    got, want = _both(points, offsets, scan_time, pose_time, pose, dt, "three tiles")
    assert want["first"] == 500 and len(want["points_out"]) == sum(sizes) and want["status"].tolist() == [0] * 7
    # the same scans give the same bits wherever their rows stand
    moved, _ = _both(points[500:], offsets - 500, scan_time, pose_time, pose, dt[500:], "the same scans from row 0", num_rows=len(points) - 500)
    assert _same(moved["points_out"][:sum(sizes)], got["points_out"][500:500 + sum(sizes)]) and _same(moved["scan_pose"], got["scan_pose"])


def test_more_scans_in_a_tile_than_one_batch_of_pairs():
    pose_time, pose = _odometry()
    sizes = tuple([3] * (PAIRS + 8) + [0, 1, 2 * T, 0, 5] + [3] * (2 * PAIRS + 1))
    points, offsets, scan_time, dt = _scans(sizes, 30, pose_time, every=2)
    assert offsets[PAIRS + 8] < T and len(points) - offsets[PAIRS + 13] < T
    got, want = _both(points, offsets, scan_time, pose_time, pose, dt, "many pairs")
    assert not want["status"].any()


def _reach_scene(num_poses):
    """Rows whose own bracket lies 0, 1 and 5 brackets from their scan's in both directions, rows exactly on knots and on both ends of the
    odometry, and rows one nanosecond outside either end."""
    if num_poses == 2:
        pose_time, pose = R.odometry(7, 2)
        scan_time = np.array([pose_time[0], pose_time[0] + 4 * MS, pose_time[1]], np.int64)
        span = int(pose_time[1] - pose_time[0])
        dts = [[0, 1, span, span + 1, -1, span // 3], [0, -4 * MS, -4 * MS - 1, span - 4 * MS, span - 4 * MS + 1, 17], [0, -span, -span - 1, 1, -5, -span // 2]]
        return pose_time, pose, scan_time, dts, None
    pose_time, pose = _odometry()
    k = 500
    scan_time = np.array([pose_time[k] + 3 * MS, pose_time[5] + 2 * MS, pose_time[-6] + 1 * MS, pose_time[k]], np.int64)
    at = lambda knot, scan: int(pose_time[knot] - scan_time[scan])
    dts = [[0, 10 * MS, -10 * MS, 51 * MS, -51 * MS, 1, -1, at(k, 0), at(k + 1, 0), at(k - 4, 0), at(k + 1, 0) - 1],
           [at(0, 1), at(0, 1) - 1, at(0, 1) + 1, at(1, 1), 0, at(10, 1)],
           [at(-1, 2), at(-1, 2) + 1, at(-1, 2) - 1, at(-2, 2), 0, at(-11, 2)],
           [0, -1, 1, at(k + 5, 3), at(k - 5, 3)]]
    return pose_time, pose, scan_time, dts, k


@pytest.mark.parametrize("num_poses", [2, 1000])
def test_brackets_near_and_far_knots_and_the_ends(num_poses):
    pose_time, pose, scan_time, dts, k = _reach_scene(num_poses)
    points, offsets = SR.pack([SR.scan(40 + i, len(d)) for i, d in enumerate(dts)])
    dt = np.concatenate(dts).astype(np.int32)
    got, want = _both(points, offsets, scan_time, pose_time, pose, dt, "reach, %d poses" % num_poses)
    gone = np.isnan(want["points_out"]).any(1)
    if num_poses == 2:
        assert gone.tolist() == [False, False, False, True, True, False] + [False, False, True, False, True, False] + [False, False, True, True, False, False]
        assert want["status"].tolist() == [R.PART_POSE] * 3
        return
    j_scan = R.bracket(pose_time, scan_time, GAP)[0]
    j_row = R.bracket(pose_time, np.repeat(scan_time, [len(d) for d in dts]) + dt, GAP)[0]
    assert (j_row[:7] - j_scan[0]).tolist() == [0, 1, -1, 5, -5, 0, 0] and (j_row[7:11] - j_scan[0]).tolist() == [0, 1, -4, 0]
    assert j_row[11:17].tolist() == [0, -1, 0, 1, 5, 10] and j_row[17:23].tolist() == [998, 998, 998, 998, 994, 989]
    assert (j_row[23:] - j_scan[3]).tolist() == [0, -1, 0, 5, -5]
    assert gone.tolist() == [False] * 11 + [False, True] + [False] * 4 + [False, True] + [False] * 4 + [False] * 5
    assert want["status"].tolist() == [0, R.PART_POSE, R.PART_POSE, 0]
    # the rows ON a knot take the knot's translation exactly: with the scan on that knot too (scan 3, row 0) the row only turns there and back
    assert _same(got["points_out"][23], torch.from_numpy(points[23]))


def test_a_gap_of_exactly_max_gap_and_one_above():
    pose_time, pose = R.odometry(11, 40)
    pose_time = pose_time.copy()
    gap = 35 * MS
    pose_time[10:] += gap - 10 * MS                    # bracket 9 is exactly the gap
    pose_time[20:] += gap - 10 * MS + 1                # bracket 19 is one nanosecond longer
    assert pose_time[10] - pose_time[9] == gap and pose_time[20] - pose_time[19] == gap + 1
    scan_time = np.array([pose_time[9] + 5 * MS, pose_time[19] + 5 * MS, pose_time[18] + 1 * MS, pose_time[20]], np.int64)
    dts = [[0, 20 * MS, -6 * MS, 31 * MS], [0, 1, 2], [0, 9 * MS - 1, 9 * MS, 9 * MS + gap, 9 * MS + gap + 1], [0, -1, 3]]
    points, offsets = SR.pack([SR.scan(50 + i, len(d)) for i, d in enumerate(dts)])
    got, want = _both(points, offsets, scan_time, pose_time, pose, np.concatenate(dts).astype(np.int32), "gap", gap=gap)
    assert want["status"].tolist() == [0, R.NO_POSE, R.PART_POSE, R.PART_POSE]
    gone = np.isnan(want["points_out"]).any(1)
    assert gone.tolist() == [False] * 4 + [True] * 3 + [False, False, True, True, False] + [False, True, False]


def test_the_longer_arc_nan_poses_and_non_finite_rows():
    pose_time, pose = _odometry()
    pose = pose.copy()
    pose[101:140:2, 3:] *= -1.0                        # d < 0 in the brackets 100 .. 138
    pose[160, 5] = np.nan                              # the brackets 159 and 160 go, and nothing else
    pose[180, 1] = np.inf                              # a translation: the same
    sizes = (300, 300, 300, 40)
    points, offsets = SR.pack([SR.scan(60 + i, m) for i, m in enumerate(sizes)])
    scan_time = np.array([pose_time[120] + 3 * MS, pose_time[158] + 3 * MS, pose_time[160] + 3 * MS, pose_time[178] + 1 * MS], np.int64)
    rng = np.random.default_rng(6)
    dt = rng.integers(-25 * MS, 25 * MS, size=len(points)).astype(np.int32)
    points = points.copy()
    points[5, 0], points[17, 1], points[250, 2], points[310] = np.nan, np.inf, -np.inf, np.nan
    got, want = _both(points, offsets, scan_time, pose_time, pose, dt, "non-finite")
    assert want["status"].tolist() == [0, R.PART_POSE, R.NO_POSE, R.PART_POSE]
    gone = np.isnan(want["points_out"]).any(1)
    assert gone[:300].sum() == 3 and gone[[5, 17, 250]].all() and 0 < gone[300:600].sum() < 300 and gone[600:900].all()
    tau = np.repeat(scan_time, sizes) + dt
    inside = ((tau >= pose_time[159]) & (tau < pose_time[161])) | ((tau >= pose_time[179]) & (tau < pose_time[181]))
    assert (gone[300:600] == (inside[300:600] | (np.arange(300, 600) == 310))).all() and (gone[900:] == inside[900:]).all()
    d = (pose[100:139, 3:] * pose[101:140, 3:]).sum(1)
    assert (d < 0).all()
    assert (got["points_out"][gone].view(torch.int32) == R.NAN_WORD).all()


def test_without_point_dt_only_poses_and_status():
    pose_time, pose = _odometry()
    points, offsets, scan_time, dt = _scans((50, 0, 70, 9), 70, pose_time)
    scan_time[3] = pose_time[-1] + 1
    got, want = _both(points, offsets, scan_time, pose_time, pose, None, "no point_dt")
    assert want["status"].tolist() == [0, 0, 0, R.NO_POSE]
    with_dt, _ = _both(points, offsets, scan_time, pose_time, pose, dt, "with point_dt")
    assert _same(with_dt["scan_pose"], got["scan_pose"])
    # through the wrapper: None for the points
    ops = H.pkg("ops")
    dev = torch.device("cuda")
    moved, scan_pose, status = ops.deskew_scans(_up(points, dev), _up(offsets, dev), _up(scan_time, dev), _up(pose_time, dev), _up(pose, dev))
    assert moved is None and _same(scan_pose.cpu(), got["scan_pose"]) and status.tolist() == want["status"].tolist()


def test_whole_call_failures_write_no_row():
    pose_time, pose = _odometry(2, 60)
    points, offsets, scan_time, dt = _scans((700, 0, 800, 30), 80, pose_time, first_knot=10)
    cases = []
    down, equal = pose_time.copy(), pose_time.copy()
    down[41] = down[40] - 1
    equal[59] = equal[58]
    cases += [(offsets, down), (offsets, equal), (offsets, pose_time[::-1].copy())]
    for at, value in ((2, offsets[1] - 1), (0, -1), (4, len(points) + 1)):
        o = offsets.copy()
        o[at] = value
        cases.append((o, pose_time))
    for o, t in cases:
        got, want = _both(points, o, scan_time, t, pose, dt, "whole-call failure")
        assert want["failed"] and want["status"].tolist() == [R.NO_POSE] * 4 and _poison(got["points_out"])
        assert (got["scan_pose"].view(torch.int64) == R.NAN64_WORD).all()
    for t in (down, equal):
        L, dev = H.pkg("lib"), torch.device("cuda")
        out, status = Guarded((4, 12), torch.float64, dev), Guarded((4,), torch.int32, dev)
        L.run.epcnet_pose_interp(_up(t, dev), _up(pose, dev), 60, _up(scan_time, dev), 4, GAP, out.t, status.t)
        torch.cuda.synchronize()
        assert out.intact() and status.intact() and status.t.tolist() == [R.NO_POSE] * 4 and (out.t.view(torch.int64) == R.NAN64_WORD).all()


@pytest.mark.parametrize("num_queries", [0, 1, 2, 777])
def test_pose_interp_alone(num_queries):
    L, ops = H.pkg("lib"), H.pkg("ops")
    dev = torch.device("cuda")
    pose_time, pose = _odometry()
    rng = np.random.default_rng(num_queries)
    query = rng.integers(pose_time[0] - 50 * MS, pose_time[-1] + 50 * MS, size=num_queries).astype(np.int64)
    if num_queries > 2:
        query[:6] = [pose_time[0], pose_time[0] - 1, pose_time[-1], pose_time[-1] + 1, pose_time[400], pose_time[400] - 1]
    elif num_queries:
        query[0] = pose_time[300] + 4 * MS              # (query 0 is written behind all the others)
    want, want_status = R.interp_reference(pose_time, pose, query, GAP)
    out, status = Guarded((num_queries, 12), torch.float64, dev), Guarded((num_queries,), torch.int32, dev)
    pt, po, qt = _up(pose_time, dev), _up(pose, dev), _up(query, dev) if num_queries else torch.zeros(1, dtype=torch.int64, device=dev)
    # (an empty tensor has no address: with no query the entry gets the address between the guards)
    L.run.epcnet_pose_interp(pt, po, 1000, qt, num_queries, GAP, out.t if num_queries else out.buf.data_ptr() + GUARD,
                             status.t if num_queries else status.buf.data_ptr() + GUARD)
    torch.cuda.synchronize()
    assert out.intact() and status.intact()
    assert _same(out.t.cpu(), torch.from_numpy(want)) and status.t.tolist() == want_status.tolist()
    if num_queries > 2:
        assert want_status[:6].tolist() == [0, R.NO_POSE, 0, R.NO_POSE, 0, 0] and 0 < (want_status != 0).sum() < 40
    poses, st = ops.interpolate_poses(pt, po, qt[:num_queries])
    assert _same(poses.cpu(), torch.from_numpy(want)) and st.tolist() == want_status.tolist()
    # float stamps and float32 poses are refused, never converted
    for change in (dict(pose_time=pt.double()), dict(query_time=qt.double()), dict(pose=po.float()), dict(pose=po[:, :6].contiguous()),
                   dict(pose_time=pt.cpu()), dict(max_gap=0.0), dict(max_gap=3.0), dict(query_time=qt.int())):
        with pytest.raises(L.EpcNetError):
            ops.interpolate_poses(**dict(dict(pose_time=pt, pose=po, query_time=qt), **change))


def test_two_runs_the_wrapper_and_its_refusals():
    L, ops = H.pkg("lib"), H.pkg("ops")
    dev = torch.device("cuda")
    pose_time, pose = _odometry()
    points, offsets, scan_time, dt = _scans((T + 5, 0, 300, 2 * T), 90, pose_time)
    a, want = _both(points, offsets, scan_time, pose_time, pose, dt, "first run")
    b = _raw(points, offsets, scan_time, pose_time, pose, dt)
    assert all(_same(a[k], b[k]) for k in a)
    args = dict(points=_up(points, dev), offsets=_up(offsets, dev), scan_time=_up(scan_time, dev), pose_time=_up(pose_time, dev),
                pose=_up(pose, dev), point_dt=_up(dt, dev))
    moved, scan_pose, status = ops.deskew_scans(**args)
    assert _same(moved.cpu(), a["points_out"]) and _same(scan_pose.cpu(), a["scan_pose"]) and status.tolist() == want["status"].tolist()
    mine = torch.full_like(args["points"], 7.0)
    again = ops.deskew_scans(out=mine, **args)
    assert again[0].data_ptr() == mine.data_ptr() and _same(mine, moved)
    for change in (dict(scan_time=args["scan_time"].double()), dict(point_dt=args["point_dt"].long()), dict(point_dt=args["point_dt"].float()),
                   dict(pose_time=args["pose_time"].int()), dict(pose=args["pose"].float()), dict(out=args["points"]),
                   dict(scan_time=args["scan_time"][:3].contiguous()), dict(point_dt=args["point_dt"][:-1].contiguous()), dict(max_gap=2.2),
                   dict(points=args["points"].cpu()), dict(point_dt=None, out=mine)):
        with pytest.raises(L.EpcNetError) as e:
            ops.deskew_scans(**dict(args, **change))
        if "scan_time" in change and change["scan_time"].dtype == torch.float64:
            assert "torch.round" in str(e.value)            # the message names the conversion the caller may choose
    with pytest.raises(L.EpcNetError) as e:                 # the entry's own refusal of points_out == points
        L.run.epcnet_scan_deskew(args["points"], args["offsets"], len(points), 4, args["point_dt"], args["scan_time"], args["pose_time"],
                                 args["pose"], 1000, GAP, args["points"], scan_pose, status, torch.zeros(64, dtype=torch.uint8, device=dev), 64)
    assert e.value.status == L.EPC_EINVAL


def test_one_graph_replayed_on_other_data():
    L = H.pkg("lib")
    dev = torch.device("cuda")
    sizes = (T + 5, 0, 300, 2 * T)

    def scene(seed, first_knot):
        pose_time, pose = R.odometry(seed, 400, jitter_ns=200_000)
        points, offsets, scan_time, dt = _scans(sizes, seed, pose_time, first_knot=first_knot)
        return points, offsets, scan_time, pose_time, pose, dt

    one, two = scene(3, 20), scene(4, 33)
    two = (two[0], np.array([0, 900, 1400, 1400, sum(sizes) - 7], np.int32)) + two[2:]          # other offsets too, and rows left alone
    two[2][3] = two[3][-1] + 5                                # ... and a scan behind the odometry's end
    eager = _raw(*two)
    want = R.deskew_reference(*two, GAP)
    _check(eager, want, "eager, second scene")
    assert want["status"].tolist()[3] == R.NO_POSE
    bufs = [_up(a, dev) for a in one]
    need = L.lib().epcnet_deskew_workspace_bytes(4, 400, sum(sizes))
    out, scan_pose, status = Guarded((sum(sizes), 3), torch.float32, dev), Guarded((4, 12), torch.float64, dev), Guarded((4,), torch.int32, dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    call = lambda: L.run.epcnet_scan_deskew(bufs[0], bufs[1], sum(sizes), 4, bufs[5], bufs[2], bufs[3], bufs[4], 400, GAP, out.t, scan_pose.t,
                                            status.t, ws, need)
    call()                                                   # (warm-up: the code objects are loaded before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for replay in range(2):
        for dst, src in zip(bufs, two):
            dst.copy_(_up(src, dev))
        out.buf[GUARD:GUARD + out.nbytes] = 0xFF
        g.replay()
        torch.cuda.synchronize()
        assert out.intact() and scan_pose.intact() and status.intact()
        _check(dict(points_out=out.t.cpu(), scan_pose=scan_pose.t.cpu(), status=status.t.cpu()), want, "replay %d" % replay)
        assert _same(out.t.cpu(), eager["points_out"])


def test_travel_along_against_a_loop():
    ops, L = H.pkg("ops"), H.pkg("lib")
    dev = torch.device("cuda")
    poses, _ = SR.trajectory(12, 50, step=0.7)
    poses = poses.copy()
    status = np.zeros(50, np.int32)
    for i in (0, 1, 20, 21, 22, 35, 48, 49):                 # invalid at the front, in the middle and at the end
        poses[i] = np.nan
        status[i] = R.NO_POSE
    status[10] = R.PART_POSE                                 # (a scan that lost rows still has its pose)
    poses[30, 7] = np.inf                                    # a non-finite translation without the status word
    status[40] = R.NO_POSE                                   # the status word on a finite pose
    want, total, last = np.zeros(50), 0.0, None
    for i in range(50):
        t = poses[i].reshape(3, 4)[:, 3]
        if np.isfinite(t).all() and not status[i] & R.NO_POSE:
            if last is not None:
                total += float(np.sqrt(((t - last) ** 2).sum()))
            last = t
        want[i] = total
    got = ops.travel_along(_up(poses, dev), _up(status, dev))
    assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == (50,)
    worst = float(np.abs(got.cpu().numpy() - want).max())
    print("travel_along against the loop: %.2e m" % worst)
    assert worst <= 1e-9 and want[1] == 0.0 and want[22] == want[19] and want[49] == want[47] and want[-1] > 25.0
    # all valid, no status: the sum build_submaps(along=None) makes, and (S, 3, 4) goes too
    clean, _ = SR.trajectory(12, 50, step=0.7)
    own = ops.build_submaps(torch.zeros((50, 3), dtype=torch.float32, device=dev), torch.arange(51, dtype=torch.int32, device=dev),
                            _up(clean, dev), length=4.0, spacing=2.0, return_along=True)[-1]
    mine = ops.travel_along(_up(clean, dev).reshape(50, 3, 4))
    assert float((mine - own).abs().max()) <= 1e-9 and float(own[-1]) > 30.0
    with pytest.raises(L.EpcNetError):
        ops.travel_along(_up(clean, dev).float())


@functools.lru_cache(maxsize=None)
def _stamped_drive(on_knots):
    """60 scans of 200 rows 50 ms (0.5 m) apart over 4 s of odometry; the sweeps last 40 ms."""
    pose_time, pose = R.odometry(21, 400, jitter_ns=0 if on_knots else 200_000, wobble=0.01)
    points, offsets = SR.pack([SR.scan(300 + i, 200, extent=12.0) for i in range(60)])
    scan_time = pose_time[10:310:5].copy() + (0 if on_knots else 3 * MS)
    rng = np.random.default_rng(8)
    dt = np.zeros(len(points), np.int32) if on_knots else np.sort(rng.integers(0, 40 * MS, size=(60, 200)), axis=1).reshape(-1).astype(np.int32)
    return points, offsets, scan_time, pose_time, pose, dt


def test_engine_forward_stamped():
    ops, L = H.pkg("ops"), H.pkg("lib")
    dev = torch.device("cuda")
    arch = "epc-net-l"
    eng, _ = H.make_engine(arch, O.seeded_weights(arch, 0), dev, in_flight=1)
    sub = dict(length=3.0, spacing=1.3, max_submaps=24, out_rows=4 * 60 * 200, max_range=50.0)
    points, offsets, scan_time, pose_time, pose, dt = (_up(a, dev) for a in _stamped_drive(False))
    scan_time = scan_time.clone()
    scan_time[17] = pose_time[-1] + 1                        # one scan without a pose: it goes on as NaN rows, the trajectory stays whole
    # the four calls one by one
    moved, scan_pose, scan_status = ops.deskew_scans(points, offsets, scan_time, pose_time, pose, point_dt=dt)
    along = ops.travel_along(scan_pose, scan_status)
    built = ops.build_submaps(moved, offsets, scan_pose, along=along, **sub)
    want, want_status = eng.forward_scans(built[0], built[1], num_points=32)
    want, want_status = want.clone(), want_status | built[2]
    desc, status, sub_pose, num_out, st_scan = eng.forward_stamped(points, offsets, scan_time, pose_time, pose, point_dt=dt, num_points=32, submaps=sub)
    assert _same(desc, want) and _same(status, want_status) and _same(sub_pose, built[3]) and _same(num_out, built[5]) and _same(st_scan, scan_status)
    n = int(num_out[0])
    assert 18 <= n < 24 and scan_status.tolist() == [0] * 17 + [R.NO_POSE] + [0] * 42
    finite = torch.isfinite(desc).all(1)
    assert int(finite[:n].sum()) >= n - 1 and not bool(finite[n:].any())
    with pytest.raises(L.EpcNetError):
        eng.forward_stamped(points, offsets, scan_time, pose_time, pose, point_dt=dt, submaps=dict(along=along))
    # every row stamped with its scan, every scan on a knot: the trajectory entry on the knots' own [R | t]
    points, offsets, scan_time, pose_time, pose, dt = _stamped_drive(True)
    knots, valid = R.pose_at(pose_time, pose, scan_time, GAP)
    assert valid.all()
    up = [_up(a, dev) for a in (points, offsets, scan_time, pose_time, pose, dt)]
    ref = eng.forward_trajectory(up[0], up[1], _up(knots, dev), num_points=32, submaps=sub)
    ref = tuple(t.clone() for t in ref)
    got = eng.forward_stamped(*up[:5], point_dt=up[5], num_points=32, submaps=sub)
    assert _same(got[2], ref[2]) and _same(got[3], ref[3]) and _same(got[1], ref[1]) and _same(got[0], ref[0])
    assert int(got[3][0]) >= 18 and bool(torch.isfinite(got[0][:int(got[3][0])]).all()) and not got[4].any()
    # ... and without point_dt at all (a line scanner): the same again
    flat = eng.forward_stamped(*up[:5], num_points=32, submaps=sub)
    assert _same(flat[0], ref[0]) and _same(flat[1], ref[1])
    # one graph, replayed once on the other drive
    first = [_up(a, dev) for a in _stamped_drive(False)]
    eager = tuple(t.clone() for t in eng.forward_stamped(*first[:5], point_dt=first[5], num_points=32, submaps=sub))
    out = torch.empty((24, 256), dtype=torch.float32, device=dev)
    eng.forward_stamped(*up[:5], point_dt=up[5], num_points=32, submaps=sub, out=out)                  # (warm-up)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = eng.forward_stamped(*up[:5], point_dt=up[5], num_points=32, submaps=sub, out=out)
    for dst, src in zip(up, first):
        dst.copy_(src)
    g.replay()
    torch.cuda.synchronize()
    assert _same(out, eager[0]) and all(_same(c, e) for c, e in zip(captured[1:], eager[1:]))
