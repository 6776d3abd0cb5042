"""include/epcnet_remap.h without a device: the restatement of a move (tests/remap_ref.py: rows subtracted from their old cells and added
to their new ones, ONLY the dirty voxels solved again, empty voxels keeping their numbers) against ``surfel_ref.reference`` over the rows
currently in the map at their current poses, matched by cell and bit for bit -- which is the proof that the dirty rule is sufficient for
removals too --, the header's row and binding, and the entry's refusals, which launch nothing."""
import ctypes
import os

import numpy as np
import pytest

import growmap_ref as G
import helpers as H
import map_ref as M
import remap_ref as R
import surfel_ref as S

VOXEL, CAP = 0.5, 640


def _scene():
    """The scene of the grow tests: six clouds of 70 rows along a drive of 2 m per cloud, 3 m wide -> one call per cloud."""
    points, offsets, poses, origin = M.drive(3, (70,) * 6, extent=1.5)
    calls = [(points[offsets[c]:offsets[c + 1]], np.array([0, 70], np.int32), poses[c:c + 1]) for c in range(6)]
    return points, offsets, poses, origin, calls


def _late(points, offsets, first=2):
    """The clouds first .. 5 as ONE call's points and offsets."""
    return points[offsets[first]:], (offsets[first:] - offsets[first]).astype(np.int32)


def _one_shot(points, offsets, poses, origin, min_count, ring):
    return S.reference(points, offsets, poses, origin, VOXEL, CAP, min_count, ring, 3)


def _built(calls, origin, min_count, ring):
    m = R.Map(origin, VOXEL, CAP, min_count, ring, 3)
    for call in calls:
        m.add(*call)
    return m


@pytest.mark.parametrize("min_count", [1, 2])
@pytest.mark.parametrize("ring", [0, 1, 2])
def test_repose_round_trip_and_remove_equal_the_reference_by_cell(ring, min_count):
    """Clouds 3 to 5 re-posed by about 0.3 m and a few degrees, cloud 2 passed with its pose unchanged: every voxel that holds rows is the
    one-shot's over all rows at their current poses.  Moving back restores the first V rows of all six arrays bit for bit with every
    voxel behind them empty.  Then two clouds are removed."""
    points, offsets, poses, origin, calls = _scene()
    m = _built(calls, origin, min_count, ring)
    first = m.outputs()
    V = int(first["num_out"][0])
    assert G.same_bits(first, _one_shot(points, offsets, poses, origin, min_count, ring)) is None and V > 300
    moved = R.nudged(poses, (3, 4, 5))
    assert (moved[:3] == poses[:3]).all() and 0.05 < np.abs(moved[3:] - poses[3:]).max() < 0.31
    late, late_offsets = _late(points, offsets)
    report = m.move(late, late_offsets, poses[2:], moved[2:])
    there = m.outputs()
    opened, emptied = int(report["num_call"][0]), len(report["emptied"])
    assert opened > 20 and emptied > 20 and len(report["clean"]) > 20 and report["num_call"][3] == 0
    assert 0 < report["num_call"][1] <= 210                                  # cloud 2's 70 rows did not move; a row or two of the others may not
    assert report["num_call"][2] == len(report["dirty"]) and set(report["touched"]) <= set(report["dirty"])
    assert (len(report["dirty"]) > len(report["touched"])) == (ring > 0)
    assert there["num_out"].tolist() == [V + opened, 420, 0, 0] and (m.empty_numbers() == report["emptied"]).all()
    assert R.by_cell(there, m.numbers_by_key(), _one_shot(points, offsets, moved, origin, min_count, ring)) is None
    assert (there["count"][report["emptied"]] == 0).all() and np.isnan(there["map_points"][report["emptied"]]).all()
    # ... and back
    back = m.move(late, late_offsets, moved[2:], poses[2:])
    again = m.outputs()
    assert back["num_call"][0] == 0 and back["num_call"][3] == 0 and len(back["emptied"]) == opened
    for name in G.FLOATS + ("count", "support"):
        assert (again[name].view(np.uint32)[:V] == first[name].view(np.uint32)[:V]).all(), name
    assert not again["count"][V:].any() and (m.empty_numbers() == np.arange(V, V + opened)).all()
    assert again["num_out"].tolist() == [V + opened, 420, 0, 0]
    assert R.by_cell(again, m.numbers_by_key(), _one_shot(points, offsets, poses, origin, min_count, ring)) is None
    # ... and two clouds out
    gone, gone_offsets = points[offsets[1]:offsets[3]], (offsets[1:4] - offsets[1]).astype(np.int32)
    report = m.move(gone, gone_offsets, poses[1:3])
    assert report["num_call"][:2].tolist() == [0, 0] and report["num_call"][3] == 0 and report["num_call"][2] > 0 and len(report["clean"]) > 0
    rest = G.concatenation([calls[0]] + calls[3:])
    after = m.outputs()
    assert after["num_out"].tolist() == [V + opened, 280, 0, 0]
    assert R.by_cell(after, m.numbers_by_key(), _one_shot(*rest, origin, min_count, ring)) is None


@pytest.mark.parametrize("min_count", [1, 2])
@pytest.mark.parametrize("ring", [0, 1, 2])
def test_everything_removed_and_added_again_keeps_the_numbers(ring, min_count):
    points, offsets, poses, origin, calls = _scene()
    m = _built(calls, origin, min_count, ring)
    first = m.outputs()
    V = int(first["num_out"][0])
    report = m.move(points, offsets, poses)
    empty = m.outputs()
    assert report["num_call"].tolist() == [0, 0, V, 0] and len(report["emptied"]) == V and empty["num_out"].tolist() == [V, 0, 0, 0]
    assert not empty["count"].any() and not empty["support"].any()
    for name in G.FLOATS:
        assert (empty[name].view(np.uint32) == M.NAN_WORD).all(), name
    assert R.by_cell(empty, m.numbers_by_key(), S.reference(*G.concatenation([]), origin, VOXEL, CAP, min_count, ring, 3)) is None
    for call in calls[::-1]:                                                 # in another order: the numbers are the first life's
        assert m.add(*call)["num_call"][0] == 0
    assert G.same_bits(m.outputs(), first) is None


def test_unmoved_unmatched_and_kinds():
    """Identical poses touch nothing; a cloud that was never added is unmatched row for row; a NaN new pose takes the rows out and counts
    them absent, a NaN old pose takes nothing out and puts the rows in; rows moved past the range are counted out of range."""
    points, offsets, poses, origin, calls = _scene()
    m = _built(calls[:4], origin, 1, 1)
    first = m.outputs()
    V = int(first["num_out"][0])
    for name in G.FLOATS:
        m.out[name].view(np.uint32)[:] = 0x12345678
    assert m.move(points[:280], offsets[:5], poses[:4], poses[:4].copy())["num_call"].tolist() == [0, 0, 0, 0]
    assert all((m.out[name].view(np.uint32) == 0x12345678).all() for name in G.FLOATS) and m.out["num_out"].tolist() == first["num_out"].tolist()
    for name in G.FLOATS:
        m.out[name][:] = first[name]
    far = M.identity_poses(1, origin + 500.0)
    report = m.move(calls[5][0], calls[5][1], far, R.nudged(far, (0,)))
    assert report["num_call"].tolist() == [0, 0, 0, 70] and G.same_bits(m.outputs(), first) is None
    broken = poses[3:4].copy()
    broken[0, 5] = np.nan
    report = m.move(*calls[3], broken)                                       # poses[3] -> NaN
    assert report["num_call"][:2].tolist() == [0, 0] and m.out["num_out"].tolist() == [V, 210, 70, 0]
    now = G.concatenation(calls[:3] + [(calls[3][0], calls[3][1], broken)])  # the rows are still the map's, absent at their current pose
    assert R.by_cell(m.outputs(), m.numbers_by_key(), S.reference(*now, origin, VOXEL, CAP, 1, 1, 3)) is None
    report = m.move(calls[3][0], calls[3][1], broken, poses[3:4])            # NaN -> poses[3]: nothing leaves, the rows come back
    assert report["num_call"][:2].tolist() == [0, 70] and G.same_bits(m.outputs(), first) is None
    away = poses[3:4].copy()
    away[0, 3] += 0.5 * 2.0 ** 21                                            # 2^20 cells further on x
    report = m.move(calls[3][0], calls[3][1], poses[3:4], away)
    assert report["num_call"][:2].tolist() == [0, 0] and m.out["num_out"].tolist() == [V, 210, 0, 70]


def test_overflow_through_a_repose_is_sticky():
    points, offsets, poses, origin, calls = _scene()
    moved = R.nudged(poses, (3, 4, 5))
    late, late_offsets = _late(points, offsets, 3)
    probe = _built(calls, origin, 1, 1)
    V = int(probe.out["num_out"][0])
    opened = int(probe.move(late, late_offsets, poses[3:], moved[3:])["num_call"][0])
    assert opened > 20
    for cap, over in ((V + opened, False), (V + opened - 1, True)):
        m = R.Map(origin, VOXEL, cap, 1, 1, 3)
        for call in calls:
            m.add(*call)
        report = m.move(late, late_offsets, poses[3:], moved[3:])
        assert (report["num_call"][0] == -1) == over and (m.out["num_out"][0] == -1) == over
        if over:
            assert not m.out["count"].any() and (m.out["normal"].view(np.uint32) == M.NAN_WORD).all()
            assert m.move(late, late_offsets, moved[3:], poses[3:])["num_call"][0] == -1 and m.out["num_out"].tolist() == [-1, 420, 0, 0]
            assert m.add(*calls[0])["num_call"].tolist() == [-1, 70, 0, 0] and m.out["num_out"].tolist() == [-1, 490, 0, 0]


# ---- the header -------------------------------------------------------------------------------------------------------------------------------
def test_fourteenth_header_is_bound_like_the_others():
    L = H.pkg("lib")
    path = os.path.join(H.ROOT, "include", "epcnet_remap.h")
    text = open(path).read()
    assert L.REMAP_HEADER_PATH == path and L._HEADERS[-1] == ("remap", "REMAP", False, False) and L._HEADERS[-2][0] == "growmap"
    functions, constants, status = L.parse_header(text, need_status=False)
    assert list(functions) == L.REMAP_EXPORTS == ["epcnet_surfel_map_move_workspace_bytes", "epcnet_surfel_map_move"]
    assert status == {} and constants == {}
    for stem, prefix, _, _ in L._HEADERS:
        if stem != "remap":
            assert not set(L.REMAP_EXPORTS) & set(getattr(L, prefix + "_EXPORTS")), stem
    assert not set(L.REMAP_EXPORTS) & set(L.EXPORTS) and not set(L.REMAP_EXPORTS) & set(L.LAUNCHING)
    assert "_kernel" not in text
    i, ll, z, P = ctypes.c_int, ctypes.c_longlong, ctypes.c_size_t, ctypes.c_void_p
    want = {"epcnet_surfel_map_move_workspace_bytes": (z, [ll, i, i]),
            "epcnet_surfel_map_move": (i, [P, P, ll, i, P, P, P, ll, P, z, P, P, P, P, P, P, P, P, P, z, P])}
    for name, (restype, argtypes) in want.items():
        fn = getattr(L.lib(), name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    ret, types, names = functions["epcnet_surfel_map_move"]
    assert names == ["points", "offsets", "num_rows", "num_clouds", "old_poses", "new_poses", "params", "max_voxels", "state", "state_bytes",
                     "map_points", "count", "centroid", "normal", "eigen", "support", "num_out", "num_call", "workspace", "workspace_bytes",
                     "stream"]
    for n, t in (("points", "float*"), ("old_poses", "double*"), ("new_poses", "double*"), ("params", "double*"), ("offsets", "int32_t*"),
                 ("num_call", "int32_t*"), ("state", "void*"), ("workspace", "void*")):
        assert types[names.index(n)] == t, n
    assert [n for n in L.REMAP_EXPORTS if hasattr(L.run, n)] == ["epcnet_surfel_map_move"]
    growmap = H.pkg("growmap")
    assert callable(growmap.SurfelMap.remove) and callable(growmap.SurfelMap.repose)


def test_size_query_and_refusals_launch_nothing():
    """EPC_EINVAL / EPC_ENOMEM from addresses that are never followed: nothing is launched, so no device is needed."""
    L = H.pkg("lib")
    lib = L.lib()
    state, need, add_need = lib.epcnet_surfel_map_state_bytes, lib.epcnet_surfel_map_move_workspace_bytes, lib.epcnet_surfel_map_add_workspace_bytes
    for bad in ((-1, 1, 1), (1 << 31, 1, 1), (10, -1, 1), (10, (1 << 24) + 1, 1), (10, 1, -1), (10, 1, 3)):
        assert need(*bad) == 0
    assert need(0, 0, 0) == 128 and need(0, 0, 2) == 128 and need(1000, 3, 1) % 16 == 0
    assert need(1000, 3, 1) == need(1000, 999, 1) == 128 + 8000 + 16 + 16 + 8000 * 27      # two slots a row, twice the dirty list
    assert need(1000, 3, 0) == 128 + 8000 + 16 + 16 + 8000 and need(1000, 3, 2) == 128 + 8000 + 16 + 16 + 8000 * 125
    assert need(1000, 3, 1) > add_need(1000, 3, 1) == 128 + 4000 + 16 + 16 + 4000 * 27
    assert need((1 << 31) - 1, 1 << 24, 2) > 8 * 126 * ((1 << 31) - 1)                      # (no 32-bit product on the way)
    a = 0x10000

    def move(rows=1000, clouds=4, points=a, offsets=a, old=a, new=a, voxel=0.2, min_count=1.0, ring=1.0, min_support=8.0, reserved=(0.0,) * 4,
             params=True, voxels=1000, st=a, st_bytes=None, out=a, count=a, centroid=a, normal=a, eigen=a, support=a, num=a, call=a, ws=a,
             ws_bytes=None):
        p = (ctypes.c_double * 8)(voxel, min_count, ring, min_support, *reserved) if params else None
        return lib.epcnet_surfel_map_move(points, offsets, rows, clouds, old, new, p, voxels, st, state(1000) if st_bytes is None else st_bytes,
                                          out, count, centroid, normal, eigen, support, num, call, ws,
                                          need(1000, 4, 1) if ws_bytes is None else ws_bytes, None)

    nan, inf = float("nan"), float("inf")
    refused = [dict(voxels=0), dict(voxels=(1 << 28) + 1), dict(voxel=0.0), dict(voxel=-0.2), dict(voxel=nan), dict(voxel=inf),
               dict(voxel=2.0 ** -21), dict(voxel=2.0 ** 20 + 1.0), dict(min_count=0.0), dict(min_count=1.5), dict(min_count=nan),
               dict(min_count=2.0 ** 31), dict(ring=-1.0), dict(ring=3.0), dict(ring=0.5), dict(ring=nan), dict(min_support=2.0),
               dict(min_support=2.0 ** 31), dict(min_support=8.5), dict(min_support=nan), dict(params=False), dict(st=None), dict(st=a + 8),
               dict(out=None), dict(count=None), dict(centroid=None), dict(normal=None), dict(eigen=None), dict(support=None), dict(num=None),
               dict(rows=-1), dict(rows=1 << 31), dict(clouds=-1), dict(clouds=(1 << 24) + 1), dict(points=None), dict(offsets=None),
               dict(old=None), dict(old=None, new=None), dict(call=None), dict(ws=None), dict(ws=a + 8)]
    refused += [dict(reserved=tuple(1.0 if i == k else 0.0 for i in range(4))) for k in range(4)] + [dict(reserved=(0.0, nan, 0.0, 0.0))]
    for kw in refused:
        assert move(**kw) == L.EPC_EINVAL, kw
        assert b"epcnet_surfel_map_move" in lib.epc_last_error()
    for new in (a, None):                                                    # new_poses == NULL is legal (remove): the size checks are reached
        assert move(new=new, st_bytes=state(1000) - 1) == L.EPC_ENOMEM and move(new=new, voxels=1025) == L.EPC_ENOMEM
        assert move(new=new, ws_bytes=need(1000, 4, 1) - 1) == L.EPC_ENOMEM and move(new=new, ws_bytes=0) == L.EPC_ENOMEM
        assert move(new=new, ws_bytes=add_need(1000, 4, 1)) == L.EPC_ENOMEM                # an add's workspace is too small
        assert move(new=new, ring=2.0) == L.EPC_ENOMEM and move(new=new, rows=1001) == L.EPC_ENOMEM
