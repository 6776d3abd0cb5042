"""The definition of include/epcnet_submaps.h as tests/submap_ref.py restates it, without a device: the segmentation against a
brute-force double loop, the M | u transform against the textbook form in float64 (and why float32 poses will not do), the spacings, the
ties on a boundary, a jump in `along`, the fit rule, the whole-call failures, and the header's binding."""
import ctypes
import os

import numpy as np

import helpers as H
import submap_ref as R


def _brute(along, length, spacing, max_submaps):
    """Slots and scans in a double loop of Python floats: membership is s_k <= along[i] < e_k, the frame the first scan at or behind c_k."""
    out = []
    h = float(length) * 0.5
    for k in range(max_submaps + 1):
        c = (float(along[0]) + h) + float(k) * float(spacing)
        s, e = c - h, c + h
        if not e <= float(along[-1]):
            out.append((False, -1, -1, -1, []))
            continue
        members = [i for i in range(len(along)) if s <= float(along[i]) < e]
        before_s = sum(1 for i in range(len(along)) if float(along[i]) < s)
        before_e = sum(1 for i in range(len(along)) if float(along[i]) < e)
        ref = min(i for i in range(len(along)) if float(along[i]) >= c)
        out.append((True, before_s, before_e, ref, members))
    return out


def _agrees_with_brute(along, length, spacing, max_submaps):
    is_submap, lo, hi, ref = R.segment(along, length, spacing, max_submaps)
    for k, (sub, blo, bhi, bref, members) in enumerate(_brute(along, length, spacing, max_submaps)):
        assert (bool(is_submap[k]), int(lo[k]), int(hi[k]), int(ref[k])) == (sub, blo, bhi, bref), k
        if sub:
            assert members == list(range(blo, bhi)), k                    # a sorted `along`: the members are one run of scans
    return is_submap, lo, hi, ref


def test_segmentation_against_the_double_loop():
    _, along = R.trajectory(0, 64)
    is_submap, lo, hi, ref = _agrees_with_brute(along, 4.0, 2.0, 20)
    assert int(is_submap.sum()) == 14 and (hi - lo)[:14].tolist() == [8] * 14     # 64 scans 0.5 m apart, 4 m every 2 m
    assert ref[:14].tolist() == [4 + 4 * k for k in range(14)]
    rng = np.random.default_rng(3)
    for trial in range(20):                                                  # uneven steps, with standing still in between
        steps = rng.uniform(0.0, 1.5, size=50) * (rng.uniform(size=50) > 0.2)
        along = np.concatenate([[rng.uniform(-5, 5)], steps]).cumsum()
        _agrees_with_brute(along, rng.uniform(0.5, 8.0), rng.uniform(0.5, 8.0), 30)


def test_overlap_abut_gap_and_standing_still():
    along = 0.5 * np.arange(64)
    for spacing, count, first in ((2.0, 14, [0, 4, 8]), (4.0, 7, [0, 8, 16]), (6.0, 5, [0, 12, 24])):
        is_submap, lo, hi, ref = _agrees_with_brute(along, 4.0, spacing, 16)
        assert int(is_submap.sum()) == count and is_submap[:count].all()
        assert lo[:3].tolist() == first and (hi - lo)[:count].tolist() == [8] * count
    # overlap: scan 9 (4.5 m) lies in submaps 1 and 2; gap: scan 9 lies in none (submap 0 ends at 4 m, submap 1 begins at 6 m)
    _, lo, hi, _ = R.segment(along, 4.0, 2.0, 16)
    assert [k for k in range(14) if lo[k] <= 9 < hi[k]] == [1, 2]
    _, lo, hi, _ = R.segment(along, 4.0, 6.0, 16)
    assert [k for k in range(5) if lo[k] <= 9 < hi[k]] == []
    # a stationary trajectory is valid and holds no submap
    still = np.full(10, 3.25)
    assert R.valid(np.arange(11) * 5, still, 50)
    assert not R.segment(still, 4.0, 2.0, 4)[0].any()
    ref = R.reference(R.scan(0, 50), np.arange(11) * 5, R.identity_poses(10), still, 4.0, 2.0, max_submaps=4)
    assert ref["status"].tolist() == [R.NO_SUBMAP] * 4 and ref["num_out"].tolist() == [0, 0] and not ref["sub_offsets"].any()


def test_ties_on_the_boundaries_and_a_jump():
    # repeated `along` values exactly AT s_1 = 2, c_1 = 4 and e_1 = 6 (length 4, spacing 2, along[0] = 0: every bound is exact)
    along = np.array([0.0, 1.0, 2.0, 2.0, 2.0, 3.0, 4.0, 4.0, 5.0, 6.0, 6.0, 7.0, 8.0])
    is_submap, lo, hi, ref = _agrees_with_brute(along, 4.0, 2.0, 4)
    assert is_submap.tolist() == [True, True, True, False, False]
    # >= at s: the first of the scans at 2.0 opens submap 1; >= at c: the first scan at 4.0 is its frame; < at e: both scans at 6.0 are out
    assert (int(lo[1]), int(ref[1]), int(hi[1])) == (2, 6, 9)
    assert (int(lo[0]), int(ref[0]), int(hi[0])) == (0, 2, 6) and (int(lo[2]), int(ref[2]), int(hi[2])) == (6, 9, 12)
    # a jump: nothing between 3 and 20.  Submap 1 = [2, 6) holds scans 2, 3 and its frame is scan 4 (at 20), outside [lo, hi); submaps
    # 2 .. 8 ([4, 8) .. [16, 20)) hold no scan at all and are submaps all the same
    along = np.array([0.0, 1.0, 2.0, 3.0, 20.0, 21.0])
    is_submap, lo, hi, ref = _agrees_with_brute(along, 4.0, 2.0, 10)
    assert int(is_submap.sum()) == 9
    assert (int(lo[1]), int(hi[1]), int(ref[1])) == (2, 4, 4) and not lo[1] <= ref[1] < hi[1]
    assert all(lo[k] == hi[k] == 4 for k in range(2, 9))
    points, offsets = R.pack([R.scan(i, 7) for i in range(6)])
    out = R.reference(points, offsets, R.trajectory(2, 6)[0], along, 4.0, 2.0, max_submaps=10)
    assert out["status"][:9].tolist() == [0] * 9 and out["status"][9] == R.NO_SUBMAP       # an empty submap: zero rows, status 0
    assert np.diff(out["sub_offsets"])[:9].tolist() == [28, 14] + [0] * 7
    assert np.isfinite(out["sub_pose"][2:9]).all()


def test_transform_against_the_textbook_form():
    """q = M p + u with M = Rr^T Ri, u = Rr^T (ti - tr) against ((p Ri^T + ti) - tr) Rr, both float64.  The difference is the
    TEXTBOOK form's rounding: p Ri^T + ti is a sum of four terms of magnitude up to |ti| + |p|, rounded four times at that magnitude,
    so each component is off by at most 4 * 2^-53 * (|ti| + |p|); the difference of the two translations is then (nearly) exact, and
    the rotation by the orthonormal Rr carries the error vector on with its length: at most sqrt(3) * 4 < 8 units.  The M | u form itself
    only rounds at the magnitude of |ti - tr| + |p| (tens of metres: 1e-14).  Bound: 8 * 2^-53 * (|ti| + |tr| + |p|) = 1.0e-8 m at
    these translations; seen: 3.8e-10 m (4.4e-10 m on the scene of the feature's proposal)."""
    poses, along = R.trajectory(0, 64)
    worst, bound = 0.0, np.inf
    for i, r in ((0, 4), (7, 4), (33, 36), (63, 60)):
        rows = R.scan(i, 250)
        M, u = R.pair(poses[i], poses[r])
        diff = np.abs(R.transform64(rows, M, u) - R.direct64(rows, poses[i], poses[r])).max()
        ti, tr = poses[i].reshape(3, 4)[:, 3], poses[r].reshape(3, 4)[:, 3]
        b = 8 * 2.0 ** -53 * (np.linalg.norm(ti) + np.linalg.norm(tr) + np.linalg.norm(rows.astype(np.float64), axis=1).max())
        worst, bound = max(worst, diff), min(bound, b)
        assert diff <= b, (i, r, diff, b)
    print("M | u against the textbook form: %.3e m (bound %.3e m)" % (worst, bound))
    assert worst > 0.0                                                       # (two associations: they do differ)


def test_float32_poses_are_not_enough():
    """The reason the poses stay float64, pinned: the same scene through float32 poses and arithmetic is off by more than 0.1 m."""
    poses, along = R.trajectory(0, 64)
    rows = R.scan(7, 250)
    want = R.direct64(rows, poses[7], poses[4])
    Ri, Rr = poses[7].astype(np.float32).reshape(3, 4), poses[4].astype(np.float32).reshape(3, 4)
    got = ((rows @ Ri[:, :3].T + Ri[:, 3]) - Rr[:, 3]) @ Rr[:, :3]
    assert got.dtype == np.float32
    off = float(np.abs(got.astype(np.float64) - want).max())
    print("float32 poses: off by %.3f m" % off)
    assert off > 0.1


def test_reference_rows_keep_their_order_and_the_crop():
    poses, along = R.trajectory(1, 12, step=1.0)
    scans = [R.scan(i, 3 + i) for i in range(12)]
    points, offsets = R.pack(scans)
    out = R.reference(points, offsets, poses, along, 2.0, 1.0, max_range=25.0, min_range=5.0, z_min=-1.0, z_max=4.0, max_submaps=12)
    info = out["sub_info"]
    assert out["num_out"].tolist() == [10, 0]
    for k in range(10):
        lo, hi, ref, rows = info[k]
        assert rows == offsets[hi] - offsets[lo] == out["sub_offsets"][k + 1] - out["sub_offsets"][k]
        at = out["sub_offsets"][k]
        for i in range(lo, hi):                                              # row j of submap k is source row offsets[lo] + j
            M, u = R.pair(poses[i], poses[ref])
            q = R.transform64(scans[i], M, u)
            got = out["points_out"][at:at + len(scans[i])]
            kept = ~np.isnan(got).any(1)
            assert (got[kept] == q[kept].astype(np.float32)).all()
            assert (got.view(np.uint32)[~kept] == R.NAN_WORD).all()
            r2 = (scans[i].astype(np.float64) ** 2).sum(1)
            inside = (r2 >= 25.0) & ((q[:, :2] ** 2).sum(1) <= 625.0) & (q[:, 2] >= -1.0) & (q[:, 2] <= 4.0)
            clear = np.abs(r2 - 25.0) > 1e-6                                 # (away from the bound the association does not matter)
            assert (kept == inside)[clear].all()
            at += len(scans[i])
    share = np.isnan(out["points_out"]).any(1).mean()
    assert 0.1 < share < 0.9


def test_fit_rule_and_the_row_limit_from_offsets_alone():
    along = 0.5 * np.arange(64)
    offsets = np.arange(65) * 100
    is_submap, lo, hi, ref = R.segment(along, 4.0, 2.0, 16)
    full, status, rows = R.layout(offsets, is_submap, lo, hi, 14 * 800)
    assert rows.tolist() == [800] * 14 + [0, 0] and full.tolist() == [800 * min(k, 14) for k in range(17)]
    assert status.tolist() == [0] * 14 + [R.NO_SUBMAP] * 2
    # one row short of P[6]: submaps 0 .. 4 fit, 5 .. 13 get no room and zero rows, the offsets stay at P[5]
    short, status, rows = R.layout(offsets, is_submap, lo, hi, 6 * 800 - 1)
    assert short.tolist() == [800 * min(k, 5) for k in range(17)]
    assert status.tolist() == [0] * 5 + [R.NO_ROOM] * 9 + [R.NO_SUBMAP] * 2 and rows.tolist() == [800] * 14 + [0, 0]
    exact, status, _ = R.layout(offsets, is_submap, lo, hi, 6 * 800)
    assert exact.tolist() == [800 * min(k, 6) for k in range(17)] and status.tolist() == [0] * 6 + [R.NO_ROOM] * 8 + [R.NO_SUBMAP] * 2
    none, status, _ = R.layout(offsets, is_submap, lo, hi, 0)
    assert not none.any() and status.tolist() == [R.NO_ROOM] * 14 + [R.NO_SUBMAP] * 2
    # a submap above 2^20 rows counts as zero rows and has no room; its neighbours are laid out as if it were empty.  Abutting submaps
    # of two scans: submap 1 = scans 2, 3 holds 2^20 + 1 rows, submap 2 exactly 2^20
    sizes = [10, 20, 1 << 19, (1 << 19) + 1, 1 << 19, 1 << 19, 30, 40, 5]
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    along = 1.0 * np.arange(9)
    is_submap, lo, hi, ref = R.segment(along, 2.0, 2.0, 5)
    assert is_submap.tolist() == [True] * 4 + [False] * 2
    sub_offsets, status, rows = R.layout(offsets, is_submap, lo, hi, 1 << 22)
    assert rows.tolist() == [30, 0, 1 << 20, 70, 0] and status.tolist() == [0, R.NO_ROOM, 0, 0, R.NO_SUBMAP]
    assert sub_offsets.tolist() == [0, 30, 30, 30 + (1 << 20), 100 + (1 << 20), 100 + (1 << 20)]


def test_whole_call_failures():
    poses, along = R.trajectory(4, 6)
    points, offsets = R.pack([R.scan(i, 5) for i in range(6)])
    assert R.valid(offsets, along, 30) and R.reference(points, offsets, poses, along, 1.0, 0.5, max_submaps=3)["num_out"].tolist() == [3, 1]
    bad_offsets = ([0, 5, 4, 15, 20, 25, 30], [-1, 5, 10, 15, 20, 25, 30], [0, 5, 10, 15, 20, 25, 31])
    bad_along = []
    for value in (np.nan, np.inf, -np.inf):
        a = along.copy()
        a[3] = value
        bad_along.append(a)
    down = along.copy()
    down[4] = down[3] - 1e-9
    bad_along.append(down)
    cases = [(o, along) for o in bad_offsets] + [(offsets, a) for a in bad_along]
    for o, a in cases:
        assert not R.valid(o, a, 30)
        out = R.reference(points, o, poses, a, 1.0, 0.5, max_submaps=3)
        assert out["status"].tolist() == [R.NO_SUBMAP] * 3 and out["num_out"].tolist() == [0, 0] and out["sub_offsets"].tolist() == [0] * 4
        assert np.isnan(out["sub_pose"]).all() and out["sub_info"].tolist() == [[-1, -1, -1, 0]] * 3 and len(out["points_out"]) == 0
    assert not R.valid([0], np.zeros(0), 30)                                 # no scan at all
    assert R.reference(points, [0], np.zeros((0, 12)), np.zeros(0), max_submaps=2)["status"].tolist() == [R.NO_SUBMAP] * 2
    equal = along.copy()
    equal[4] = equal[3]
    assert R.valid(offsets, equal, 30)                                       # standing still between two scans is no failure


def test_fourth_header_is_bound_like_the_others():
    L = H.pkg("lib")
    text = open(os.path.join(H.ROOT, "include", "epcnet_submaps.h")).read()
    assert L.SUBMAPS_HEADER_PATH == os.path.join(H.ROOT, "include", "epcnet_submaps.h")
    functions, constants, status = L.parse_header(text, need_status=False)
    assert list(functions) == L.SUBMAP_EXPORTS == ["epcnet_submap_workspace_bytes", "epcnet_submap_build"] and status == {}
    for other in (L.EXPORTS, L.POSE_EXPORTS, L.SCAN_EXPORTS, L.LAUNCHING):
        assert not set(L.SUBMAP_EXPORTS) & set(other)
    assert constants["EPC_STATUS_NO_SUBMAP"] == L.EPC_STATUS_NO_SUBMAP == R.NO_SUBMAP == 16
    assert constants["EPC_STATUS_NO_ROOM"] == L.EPC_STATUS_NO_ROOM == R.NO_ROOM == 32
    assert constants["EPC_SUBMAP_MAX_ROWS"] == L.EPC_SUBMAP_MAX_ROWS == R.MAX_ROWS == L.EPC_GROUND_MAX_ROWS
    taken = L.EPC_STATUS_NONFINITE_INPUT | L.EPC_STATUS_FP16_RANGE | L.EPC_STATUS_NO_GRID | L.EPC_STATUS_NO_GROUND
    assert taken == 15 and (L.EPC_STATUS_NO_SUBMAP | L.EPC_STATUS_NO_ROOM) & taken == 0
    size, build = L.lib().epcnet_submap_workspace_bytes, L.lib().epcnet_submap_build            # the library exports both
    assert size.restype is ctypes.c_size_t and size.argtypes == [ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong]
    assert build.restype is ctypes.c_int and len(build.argtypes) == 18
    assert not hasattr(L.run, "epcnet_submap_workspace_bytes") and hasattr(L.run, "epcnet_submap_build")
    ret, types, names = functions["epcnet_submap_build"]
    assert ret == "int" and (types[-1], names[-1]) == ("void*", "stream") and names[-3:-1] == ["workspace", "workspace_bytes"]
    assert types[names.index("poses")] == types[names.index("along")] == types[names.index("params")] == "double*"
    assert types[names.index("sub_pose")] == "double*" and types[names.index("num_rows")] == types[names.index("out_rows")] == "long long"
    # the size query launches nothing and answers 0 for what the entry refuses
    assert size(64, 14, 1000, 1000) > 0 and size(0, 1, 0, 0) > 0
    for bad in ((-1, 14, 0, 0), ((1 << 24) + 1, 14, 0, 0), (64, 0, 0, 0), (64, 65536, 0, 0), (64, 14, -1, 0), (64, 14, 0, -1), (64, 14, 0, 1 << 31)):
        assert size(*bad) == 0, bad
