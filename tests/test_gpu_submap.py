"""epcnet_submap_build on the device against its numpy restatement (tests/submap_ref.py): every output goes into a poisoned buffer with
slack behind it and is compared on BIT PATTERNS -- the definition is float64 with one rounding per operation, one rounding to float32
and integer counts, so there is no tolerance anywhere.  Scans around the gather's tile, scans and submap boundaries that share a tile,
the capacities, the overlaps, the crop with rows exactly ON every bound, non-finite rows and poses, the whole-call failures and the
refusals, position independence, and the engine's trajectory entry eagerly and in one captured graph.

What the float32 words alone would NOT catch: checked on 1000 seeded rows, one contracted multiply-add changes 546 rows' float64 values
and none of their float32 bits.  The keep decisions sit in float64; the rows exactly on a bound (the lattice scene, where every value
is exact, for the direction of each comparison; the seeded scene whose z limits ARE two rows' float64 q_2, which a contraction would
move off the bound) are what hold that part."""
import functools

import numpy as np
import pytest
import torch

import ground_ref as G
import helpers as H
import stage_ref as S
import submap_ref as R
from helpers import O

pytestmark = pytest.mark.gpu

T = 1024        # SM_TILE of csrc/submap.hip: the output rows of one gather tile
PAIRS = 32      # SM_PAIRS: the (submap, scan) pairs a tile lists at a time
INF = float("inf")


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _raw(points, offsets, poses, along, length, spacing, max_submaps, out_rows, min_range=0.0, max_range=100.0, z_min=-INF, z_max=INF,
         with_info=True, num_rows=None):
    """The entry itself on poisoned outputs and a workspace of exactly the size asked for -> the outputs as host tensors (points_out
    whole, poison included) after the checks that nothing was written behind any of them."""
    import ctypes
    L = H.pkg("lib")
    dev = torch.device("cuda")
    num_rows = len(points) if num_rows is None else num_rows
    S_ = len(offsets) - 1
    spare = torch.zeros(12, dtype=torch.float64, device=dev)
    pts = torch.from_numpy(np.ascontiguousarray(points, np.float32)).to(dev) if len(points) else spare.view(torch.float32)
    off = torch.from_numpy(np.asarray(offsets, np.int32)).to(dev)
    pos = torch.from_numpy(np.ascontiguousarray(poses, np.float64).reshape(-1, 12)).to(dev) if S_ else spare
    alo = torch.from_numpy(np.ascontiguousarray(along, np.float64)).to(dev) if S_ else spare
    need = L.lib().epcnet_submap_workspace_bytes(S_, max_submaps, num_rows, out_rows)
    assert need > 0
    out = S.Poisoned((out_rows, 3), torch.float32, dev)
    sub_offsets, status = S.Poisoned((max_submaps + 1,), torch.int32, dev), S.Poisoned((max_submaps,), torch.int32, dev)
    num_out, sub_pose = S.Poisoned((2,), torch.int32, dev), S.Poisoned((max_submaps, 12), torch.float64, dev)
    info, ws = S.Poisoned((max_submaps, 4), torch.int32, dev), S.Poisoned((need,), torch.uint8, dev)
    params = (ctypes.c_double * 8)(length, spacing, min_range, max_range, z_min, z_max, 0.0, 0.0)
    L.run.epcnet_submap_build(pts, off, num_rows, S_, pos, alo, params, max_submaps, out_rows, out.buf.data_ptr(), sub_offsets.t, num_out.t,
                              sub_pose.t, info.t if with_info else None, status.t, ws.t, need)
    torch.cuda.synchronize()
    for p in (out, sub_offsets, status, num_out, sub_pose, info, ws):
        assert p.untouched()
    if not with_info:
        assert S.holds_poison(info.t)
    return dict(points_out=out.t.cpu(), sub_offsets=sub_offsets.t.cpu(), status=status.t.cpu(), num_out=num_out.t.cpu(),
                sub_pose=sub_pose.t.cpu(), sub_info=info.t.cpu())


def _check(got, want, what, with_info=True, poisoned=True):
    for name in ("num_out", "sub_offsets", "status") + (("sub_info",) if with_info else ()):
        w = torch.from_numpy(np.asarray(want[name], np.int32))
        assert torch.equal(got[name], w), (what, name, got[name].tolist(), w.tolist())
    assert _same(got["sub_pose"], torch.from_numpy(want["sub_pose"])), (what, "sub_pose")
    total = int(want["sub_offsets"][-1])
    ro = torch.from_numpy(want["points_out"])
    assert tuple(ro.shape) == (total, 3)
    differ = (_bits(got["points_out"][:total]) != _bits(ro)).any(1).nonzero()
    assert differ.numel() == 0, (what, "%d rows differ, the first is row %d" % (differ.numel(), int(differ[0])))
    if poisoned and total < got["points_out"].shape[0]:
        assert S.holds_poison(got["points_out"][total:]), (what, "rows behind sub_offsets[max_submaps] were written")


def _both(points, offsets, poses, along, length, spacing, max_submaps, out_rows, what, **kw):
    with_info, num_rows = kw.pop("with_info", True), kw.pop("num_rows", None)
    want = R.reference(points, offsets, poses, along, length, spacing, max_submaps=max_submaps, out_rows=out_rows, **kw)
    got = _raw(points, offsets, poses, along, length, spacing, max_submaps, out_rows, with_info=with_info, num_rows=num_rows, **kw)
    _check(got, want, what, with_info)
    return got, want


@functools.lru_cache(maxsize=None)
def _scene(name):
    """(points, offsets, poses, along) of a named scene."""
    if name in ("edges", "seven"):      # scans 1 m apart: 0, 1, T - 1, T, T + 1 rows, three rows, one scan that spans many tiles
        sizes = (0, 1, T - 1, T, T + 1, 3, 3 * T + 5, 2)[:7 if name == "seven" else 8]
        poses, along = R.trajectory(5, len(sizes), step=1.0)
    elif name == "small":    # 64 scans 0.5 m apart of 37 rows (a few of none): several scans and submap boundaries inside one tile
        sizes = tuple(0 if i in (5, 6, 40) else 37 for i in range(64))
        poses, along = R.trajectory(0, 64)
    elif name == "tiny":     # 64 scans of 0, 1, 2, 3 or 7 rows: one tile holds many times PAIRS pairs and takes them in batches
        sizes = tuple((0, 1, 2, 3, 7)[(i * 3) % 5] for i in range(64))
        poses, along = R.trajectory(8, 64)
    elif name == "two":
        sizes = (T + 1, 9)
        poses, along = R.trajectory(6, 2, step=4.0)
    elif name == "one":
        sizes = (50,)
        poses, along = R.trajectory(7, 1)
    else:
        raise KeyError(name)
    points, offsets = R.pack([R.scan(100 + i, m) for i, m in enumerate(sizes)])
    return points, offsets, poses, along


def test_scans_around_the_tile_and_one_across_many_tiles():
    points, offsets, poses, along = _scene("edges")
    # length 3 every 1 m: submap k = scans k, k + 1, k + 2 (overlap 3); five submaps, every scan size at the head, inside and at the tail,
    # the last one ends with the scan of 3 T + 5 rows
    got, want = _both(points, offsets, poses, along, 3.0, 1.0, 7, 4 * len(points), "edges")
    assert want["num_out"].tolist() == [5, 0]
    assert want["sub_info"][:5, :3].tolist() == [[0, 3, 2], [1, 4, 3], [2, 5, 4], [3, 6, 5], [4, 7, 6]]
    assert want["sub_info"][:, 3].tolist() == [T, 2 * T, 3 * T, 2 * T + 4, 4 * T + 9, 0, 0]
    assert want["status"].tolist() == [0] * 5 + [R.NO_SUBMAP] * 2
    # abutting, sub_info NULL: submaps of 1, 2 T - 1 and T + 4 rows (the long scan lies behind the last submap)
    got, want = _both(points, offsets, poses, along, 2.0, 2.0, 3, len(points), "edges, abutting", with_info=False)
    assert want["num_out"].tolist() == [3, 0] and np.diff(want["sub_offsets"]).tolist() == [1, 2 * T - 1, T + 4]


@pytest.mark.parametrize("name,length,spacing,count", [("one", 1.0, 1.0, 0), ("two", 4.0, 4.0, 1), ("seven", 3.0, 1.0, 4),
                                                       ("small", 4.0, 2.0, 14), ("tiny", 4.0, 0.8, 35)])
def test_one_two_seven_and_sixty_four_scans(name, length, spacing, count):
    points, offsets, poses, along = _scene(name)
    got, want = _both(points, offsets, poses, along, length, spacing, max(len(along), 2), 6 * len(points), name)
    assert want["num_out"].tolist() == [count, 0]
    if name == "two":        # [0, 4) holds scan 0 alone; its frame is scan 1, outside the submap
        assert want["sub_info"][0].tolist() == [0, 1, 1, T + 1]
    if name == "tiny":
        pairs = sum(int(offsets[i + 1] > offsets[i]) for lo, hi in want["sub_info"][:35, :2] for i in range(lo, hi))
        assert int(want["sub_offsets"][-1]) < T and pairs > 6 * PAIRS
    if name == "small":      # 296 rows or fewer per submap: every tile holds several submaps' boundaries and a dozen scans
        assert int(want["sub_offsets"][-1]) == 14 * 8 * 37 - (2 + 2 + 2) * 37            # (scans 5, 6 and 40 hold no row)


@pytest.mark.parametrize("max_submaps,num_out", [(1, [1, 1]), (13, [13, 1]), (14, [14, 0]), (15, [14, 0])])
def test_max_submaps_around_the_count(max_submaps, num_out):
    points, offsets, poses, along = _scene("small")
    got, want = _both(points, offsets, poses, along, 4.0, 2.0, max_submaps, 3 * len(points), "max_submaps=%d" % max_submaps)
    assert want["num_out"].tolist() == num_out


def test_out_rows_exact_one_short_and_none():
    points, offsets, poses, along = _scene("edges")
    full = int(R.reference(points, offsets, poses, along, 3.0, 1.0, max_submaps=6)["sub_offsets"][-1])
    assert full == 12 * T + 13
    got, want = _both(points, offsets, poses, along, 3.0, 1.0, 6, full, "out_rows exact")
    assert want["status"].tolist() == [0] * 5 + [R.NO_SUBMAP]
    got, want = _both(points, offsets, poses, along, 3.0, 1.0, 6, full - 1, "one row short of the last submap")
    assert want["status"].tolist() == [0] * 4 + [R.NO_ROOM, R.NO_SUBMAP] and int(want["sub_offsets"][-1]) == 8 * T + 4
    got, want = _both(points, offsets, poses, along, 3.0, 1.0, 6, 6 * T - 1, "one row short of P[3]")
    assert want["status"].tolist() == [0, 0] + [R.NO_ROOM] * 3 + [R.NO_SUBMAP] and want["sub_offsets"].tolist() == [0, T] + [3 * T] * 5
    assert want["sub_info"][:, 3].tolist() == [T, 2 * T, 3 * T, 2 * T + 4, 4 * T + 9, 0]          # (what each would have needed)
    got, want = _both(points, offsets, poses, along, 3.0, 1.0, 6, 0, "out_rows = 0")
    assert want["status"].tolist() == [R.NO_ROOM] * 5 + [R.NO_SUBMAP] and not want["sub_offsets"].any()


@pytest.mark.parametrize("overlap", [1, 2, 5])
def test_overlaps(overlap):
    points, offsets, poses, along = _scene("small")
    spacing = 4.0 / overlap                            # (0.8 is no binary fraction: c_k, s_k, e_k round, alike on both sides)
    got, want = _both(points, offsets, poses, along, 4.0, spacing, 40, (overlap + 1) * len(points), "overlap %d" % overlap)
    assert want["num_out"].tolist() == [{1: 7, 2: 14, 5: 35}[overlap], 0]


def test_crop_with_rows_on_every_bound():
    # the lattice: identity rotations, integer translations, integer rows: every value of the definition is exact
    lattice = np.stack(np.meshgrid(*[np.arange(-6, 7)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    scans = [lattice, lattice[::3], lattice[::-1]]
    points, offsets = R.pack(scans)
    poses, along = R.identity_poses(3, step=1.0), np.array([0.0, 1.0, 2.0])
    kw = dict(min_range=5.0, max_range=5.0, z_min=-2.0, z_max=3.0)
    got, want = _both(points, offsets, poses, along, 2.0, 2.0, 2, len(points), "lattice", **kw)
    assert want["sub_info"][0].tolist() == [0, 2, 1, len(lattice) + len(lattice[::3])]
    out = want["points_out"]                           # scan 0 in the frame of scan 1: q = p - (1, 0, 0)
    row = {tuple(int(v) for v in p): out[j] for j, p in enumerate(lattice)}
    on, off = lambda p: not np.isnan(row[p]).any(), lambda p: bool((row[p].view(np.uint32) == R.NAN_WORD).all())
    assert on((4, 4, 0)) and row[(4, 4, 0)].tolist() == [3.0, 4.0, 0.0]      # rr = 32; q_0^2 + q_1^2 = 25: ON max_range, kept
    assert off((5, 4, 0))                                                    # q_0^2 + q_1^2 = 32
    assert on((4, 3, 0)) and on((3, 4, 0)) and on((0, 4, 3)) and on((0, 0, -5)) is False      # rr = 25: ON min_range, kept (z = -5 is out)
    assert off((-3, 4, 0))                                                   # rr = 25, but q_0 = -4: 32 > 25
    assert off((0, 4, 2)) and off((2, 4, 1))                                 # rr = 20, 21: below min_range
    assert on((1, 5, -2)) and off((1, 5, -3)) and on((1, 5, 3)) and off((1, 5, 4))       # ON z_min and z_max, kept; one beyond, gone
    # a seeded scene where each limit alone drops a share of the rows strictly between 0 and 1
    points, offsets, poses, along = _scene("small")
    for name, kw in (("min_range", dict(min_range=20.0)), ("max_range", dict(max_range=25.0)), ("z_min", dict(z_min=0.5)),
                     ("z_max", dict(z_max=2.0))):
        got, want = _both(points, offsets, poses, along, 4.0, 2.0, 14, 3 * len(points), name, **kw)
        share = float(np.isnan(want["points_out"]).any(1).mean())
        assert 0.05 < share < 0.95, (name, share)
    # the z limits ARE the float64 q_2 of two rows of submap 3: both rows are on their bound, and kept
    base = R.reference(points, offsets, poses, along, 4.0, 2.0, max_submaps=14, out_rows=3 * len(points))
    lo, hi, ref, _ = base["sub_info"][3]
    M, u = R.pair(poses[lo + 1], poses[ref])
    q2 = R.transform64(points[offsets[lo + 1]:offsets[lo + 2]], M, u)[:, 2]
    a, b = int(np.argsort(q2)[9]), int(np.argsort(q2)[27])
    got, want = _both(points, offsets, poses, along, 4.0, 2.0, 14, 3 * len(points), "z limits from rows", z_min=float(q2[a]), z_max=float(q2[b]))
    at = int(want["sub_offsets"][3]) + int(offsets[lo + 1] - offsets[lo])
    kept = ~np.isnan(want["points_out"][at:at + 37]).any(1)
    assert kept[a] and kept[b] and int(kept.sum()) == 19


def test_non_finite_rows_and_a_nan_pose():
    points, offsets, poses, along = _scene("small")
    points, poses = points.copy(), poses.copy()
    points[3, 0], points[40, 1], points[41, 2], points[700] = np.nan, np.inf, -np.inf, np.nan
    poses[9, 5] = np.nan                               # scan 9 lies in submaps 1 and 2 and is the frame of neither
    poses[20, 3] = np.nan                              # scan 20 is the frame of submap 4: the whole submap goes
    got, want = _both(points, offsets, poses, along, 4.0, 2.0, 14, 3 * len(points), "non-finite")
    gone = np.isnan(want["points_out"]).any(1)
    so = want["sub_offsets"]
    assert gone[so[4]:so[5]].all() and want["status"][4] == 0 and np.isnan(want["sub_pose"][4][3])
    assert gone[3] and gone[40] and gone[41] and 0 < gone[so[1]:so[2]].sum() < so[2] - so[1]
    assert (want["points_out"].view(np.uint32)[gone] == R.NAN_WORD).all()


def test_whole_call_failures_write_no_row():
    points, offsets, poses, along = _scene("small")
    cases = []
    for at, value in ((7, offsets[6] - 1), (0, -1), (64, len(points) + 1)):
        o = offsets.copy()
        o[at] = value
        cases.append((o, along))
    for at, value in ((0, np.nan), (30, np.inf), (63, -np.inf), (31, along[30] - 1e-9)):
        a = along.copy()
        a[at] = value
        cases.append((offsets, a))
    for o, a in cases:
        got, want = _both(points, o, poses, a, 4.0, 2.0, 14, 3 * len(points), "whole-call failure")
        assert want["status"].tolist() == [R.NO_SUBMAP] * 14 and S.holds_poison(got["points_out"])
    # no scan at all; and a trajectory that stands still: valid, no submap
    got, want = _both(points, offsets[:1], poses[:0], along[:0], 4.0, 2.0, 3, 100, "no scan")
    assert want["status"].tolist() == [R.NO_SUBMAP] * 3
    got, want = _both(points, offsets, poses, np.full(64, 2.5), 4.0, 2.0, 3, 100, "standing still")
    assert want["num_out"].tolist() == [0, 0]
    # offsets[num_scans] may lie below num_rows, and offsets[0] above 0
    _both(points, offsets, poses, along, 4.0, 2.0, 14, 3 * len(points), "more rows than the scans hold", num_rows=len(points) + 5)


def test_refusals_write_nothing():
    import ctypes
    L, ops = H.pkg("lib"), H.pkg("ops")
    dev = torch.device("cuda")
    points, offsets, poses, along = _scene("small")
    rows, S_ = len(points), 64
    pts, off = torch.from_numpy(points).to(dev), torch.from_numpy(offsets).to(dev)
    pos, alo = torch.from_numpy(poses).to(dev), torch.from_numpy(along).to(dev)
    need = L.lib().epcnet_submap_workspace_bytes(S_, 14, rows, 3 * rows)
    good = dict(length=4.0, spacing=2.0, min_range=0.0, max_range=100.0, z_min=-INF, z_max=INF, num_rows=rows, num_scans=S_,
                max_submaps=14, out_rows=3 * rows, ws_bytes=need, reserved=0.0)
    nan = float("nan")
    bad = [dict(length=0.0), dict(length=INF), dict(length=nan), dict(spacing=0.0), dict(spacing=-1.0), dict(spacing=INF),
           dict(min_range=-1.0), dict(min_range=nan), dict(max_range=0.0), dict(max_range=INF), dict(max_range=nan), dict(z_min=nan),
           dict(z_max=nan), dict(num_rows=-1), dict(num_scans=-1), dict(max_submaps=0), dict(max_submaps=65536), dict(out_rows=-1),
           dict(out_rows=1 << 31), dict(reserved=1.0), dict(ws_bytes=need - 1)]
    out = torch.full((3 * rows, 3), 7.0, dtype=torch.float32, device=dev)
    sub_offsets, status = torch.full((15,), -7, dtype=torch.int32, device=dev), torch.full((14,), -7, dtype=torch.int32, device=dev)
    num_out, info = torch.full((2,), -7, dtype=torch.int32, device=dev), torch.full((14, 4), -7, dtype=torch.int32, device=dev)
    sub_pose = torch.full((14, 12), 7.0, dtype=torch.float64, device=dev)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    for change in bad:
        a = dict(good, **change)
        params = (ctypes.c_double * 8)(a["length"], a["spacing"], a["min_range"], a["max_range"], a["z_min"], a["z_max"], a["reserved"], 0.0)
        with pytest.raises(L.EpcNetError) as e:
            L.run.epcnet_submap_build(pts, off, a["num_rows"], a["num_scans"], pos, alo, params, a["max_submaps"], a["out_rows"], out,
                                      sub_offsets, num_out, sub_pose, info, status, ws, a["ws_bytes"])
        assert e.value.status == (L.EPC_ENOMEM if "ws_bytes" in change else L.EPC_EINVAL), change
    for null in (0, 1, 4, 5, 6, 9, 10, 11, 12, 14, 15):    # every pointer but sub_info
        args = [pts, off, rows, S_, pos, alo, (ctypes.c_double * 8)(4.0, 2.0, 0.0, 100.0, -INF, INF, 0.0, 0.0), 14, 3 * rows, out,
                sub_offsets, num_out, sub_pose, info, status, ws, need]
        args[null] = None
        with pytest.raises(L.EpcNetError) as e:
            L.run.epcnet_submap_build(*args)
        assert e.value.status == L.EPC_EINVAL, null
    with pytest.raises(L.EpcNetError):                     # a workspace that is not 16-byte aligned
        L.run.epcnet_submap_build(pts, off, rows, S_, pos, alo, (ctypes.c_double * 8)(4.0, 2.0, 0.0, 100.0, -INF, INF, 0.0, 0.0), 14,
                                  3 * rows, out, sub_offsets, num_out, sub_pose, info, status, ws.data_ptr() + 8, need - 8)
    # the wrapper's own refusals
    for change in (dict(points=pts.cpu()), dict(offsets=off.long()), dict(poses=pos.float()), dict(poses=pos.cpu()), dict(poses=pos[:63]),
                   dict(along=alo.float()), dict(along=alo[:63].contiguous()), dict(length=0.0), dict(max_submaps=0), dict(out_rows=1 << 31),
                   dict(out=torch.empty((5, 3), dtype=torch.float32, device=dev), out_rows=6)):
        with pytest.raises(L.EpcNetError):
            ops.build_submaps(**dict(dict(points=pts, offsets=off, poses=pos, along=alo, length=4.0, spacing=2.0), **change))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((sub_pose == 7.0).all())
    assert all(bool((t == -7).all()) for t in (sub_offsets, status, num_out, info))


def test_position_independence():
    """The same scans behind another prefix of rows (and of scans that lie in front of the first submap's reach) give the same submap bits."""
    points, offsets, poses, along = _scene("small")
    got, want = _both(points, offsets, poses, along, 4.0, 2.0, 14, 3 * len(points), "as it is")
    prefix = R.scan(999, 333)
    moved, _ = _both(np.concatenate([prefix, points]), np.concatenate([[333], offsets[1:] + 333]).astype(np.int32), poses, along, 4.0, 2.0,
                     14, 3 * len(points), "behind 333 rows")
    for name in got:
        assert _same(moved[name], got[name]), name


def test_wrapper_defaults_and_its_along():
    ops, L = H.pkg("ops"), H.pkg("lib")
    dev = torch.device("cuda")
    points, offsets, poses, along = _scene("small")
    pts, off = ops.pack_scans([points[offsets[i]:offsets[i + 1]] for i in range(64)])
    pos = torch.from_numpy(poses).to(dev)
    res = ops.build_submaps(pts, off, pos.reshape(64, 3, 4), length=4.0, spacing=2.0, return_along=True)
    assert len(res) == 7 and all(t.is_cuda for t in res)
    sub_points, sub_offsets, status, sub_pose, info, num_out, own = res
    assert tuple(sub_points.shape) == (3 * len(points), 3) and tuple(status.shape) == (64,) and own.dtype == torch.float64
    t = poses.reshape(64, 3, 4)[:, :, 3]
    assert np.allclose(own.cpu().numpy(), np.concatenate([[0.0], np.cumsum(np.linalg.norm(np.diff(t, axis=0), axis=1))]), rtol=0, atol=1e-6)
    want = R.reference(points, offsets, poses, own.cpu().numpy(), 4.0, 2.0)      # (the wrapper's own sum: read back, as the contract says)
    got = dict(points_out=sub_points.cpu(), sub_offsets=sub_offsets.cpu(), status=status.cpu(), sub_pose=sub_pose.cpu(), sub_info=info.cpu(),
               num_out=num_out.cpu())
    total = int(want["sub_offsets"][-1])
    _check(got, want, "defaults", poisoned=False)                               # (torch.empty behind the submaps' rows)
    assert int(num_out[0]) >= 13
    # sub_pose[:, [3, 7]] is the (T, 2) float64 array the pose entries take
    n = int(num_out[0])
    xy = sub_pose[:n][:, [3, 7]].contiguous()
    tuples = ops.PoseTuples(xy, r_pos=3.0, r_neg=8.0)
    assert len(tuples) == n and int(tuples.counts.max()) >= 1
    # with `along` given and `out` given: the same bits, in the caller's buffer
    mine = torch.full((3 * len(points), 3), 7.0, dtype=torch.float32, device=dev)
    again = ops.build_submaps(pts, off, pos, along=own, length=4.0, spacing=2.0, out=mine)
    assert again[0].data_ptr() == mine.data_ptr() and _same(again[0][:total], sub_points[:total]) and bool((mine[total:] == 7.0).all())
    assert all(_same(x, y) for x, y in zip(again[1:], res[1:6]))


@functools.lru_cache(maxsize=None)
def _drive(seed, sizes, step):
    poses, along = R.trajectory(seed, len(sizes), step=step, wobble=0.01, general=False)      # (z stays up: the ground is below)
    points, offsets = R.pack([G.family(seed + i)[:m] for i, m in enumerate(sizes)])
    return points, offsets, poses, along


def test_engine_forward_trajectory_and_its_graph():
    ops, L = H.pkg("ops"), H.pkg("lib")
    dev = torch.device("cuda")
    arch = "epc-net-l"
    eng, _ = H.make_engine(arch, O.seeded_weights(arch, 0), dev, in_flight=1)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    # six scans 1 m apart, 3 m every 1 m: three submaps of three scans (4 500 rows each) in four slots
    points, offsets, poses, along = (up(a) for a in _drive(11, (1500,) * 6, 1.0))
    sub = dict(length=3.0, spacing=1.0, max_submaps=4, out_rows=14000)
    built = ops.build_submaps(points, offsets, poses, along=along, **sub)
    want, want_status = eng.forward_scans(built[0], built[1], num_points=256, ground=True)
    want, want_status = want.clone(), want_status | built[2]
    desc, status, sub_pose, num_out = eng.forward_trajectory(points, offsets, poses, along=along, num_points=256, ground=True, submaps=sub)
    assert _same(desc, want) and _same(status, want_status) and _same(sub_pose, built[3]) and num_out.tolist() == [3, 0]
    assert status[:3].tolist() == [0, 0, 0] and int(status[3]) & L.EPC_STATUS_NO_SUBMAP and int(status[3]) & L.EPC_STATUS_NO_GRID
    assert bool(torch.isfinite(desc[:3]).all()) and bool(torch.isnan(desc[3]).all())
    assert not _same(desc[0], desc[1])
    with pytest.raises(L.EpcNetError):
        eng.forward_trajectory(points, offsets, poses, along=along, submaps=[3.0])
    # captured on one stream, replayed TWICE after the buffers were overwritten with another drive of the same rows and scans (twice: a
    # node that clears a word has been seen to write other bytes from the second replay on -- csrc/scan_common.h, scan_clear_words)
    p2, o2, q2, a2 = (up(a) for a in _drive(31, (900, 2100, 1500, 0, 3000, 1500), 1.25))
    assert p2.shape == points.shape
    eager = eng.forward_trajectory(p2, o2, q2, along=a2, num_points=256, ground=True, submaps=sub)
    eager = tuple(t.clone() for t in eager)
    assert eager[3].tolist() == [4, 0]                                       # 3 + k <= 6.25: another number of submaps than captured
    out = torch.empty((4, 256), dtype=torch.float32, device=dev)
    eng.forward_trajectory(points, offsets, poses, along=along, num_points=256, ground=True, submaps=sub, out=out)       # (warm-up)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _, st_graph, pose_graph, num_graph = eng.forward_trajectory(points, offsets, poses, along=along, num_points=256, ground=True,
                                                                    submaps=sub, out=out)
    for dst, src in ((points, p2), (offsets, o2), (poses, q2), (along, a2)):
        dst.copy_(src)
    for replay in range(2):
        out.fill_(7.0), st_graph.fill_(-1), pose_graph.fill_(7.0), num_graph.fill_(-1)       # (a replay that wrote nothing would show)
        g.replay()
        torch.cuda.synchronize()
        assert _same(out, eager[0]) and _same(st_graph, eager[1]) and _same(pose_graph, eager[2]) and _same(num_graph, eager[3]), replay
