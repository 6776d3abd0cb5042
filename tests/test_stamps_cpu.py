"""The definition of include/epcnet_stamps.h as tests/stamps_ref.py restates it, without a device: the integer fraction against Python
ints, the pose at a knot, the orthonormality of a rotation built from an unnormalised quaternion, the shorter arc, nlerp against slerp, a
physical scene that de-skewing puts right and leaving it out does not, the header's binding and the entries' refusals."""
import ctypes
import os

import numpy as np
import pytest

import helpers as H
import stamps_ref as R
import submap_ref as SR

GAP = 500_000_000


def test_fraction_against_python_ints():
    big = 2 ** 31 - 1
    cases = [(0, 1), (1, 1), (0, big), (big, big), (big - 1, big), (1, big), (0, 7), (7, 7), (3, 7), (1, 2), (1, 3), (12345, 10_000_000)]
    rng = np.random.default_rng(1)
    den = rng.integers(1, 2 ** 31, size=2000)
    num = (rng.uniform(size=2000) * (den + 1)).astype(np.int64).clip(0, den)
    cases += list(zip(num.tolist(), den.tolist()))
    got = R.fraction([c[0] for c in cases], [c[1] for c in cases])
    assert got.dtype == np.uint64
    for (n, d), fi in zip(cases, got.tolist()):
        assert fi == (n * 2 ** 32) // d, (n, d)
    assert int(R.fraction([5], [5])[0]) == 2 ** 32 and int(R.fraction([0], [5])[0]) == 0
    # f and g are exact: fi has at most 33 bits
    f = got.astype(np.float64) * 2.0 ** -32
    assert (f * 2.0 ** 32 == got.astype(np.float64)).all() and ((1.0 - f) + f == 1.0).all()


def test_bracket_index_and_its_validity():
    pt = np.array([100, 200, 300, 1000], np.int64)
    j, num, den, valid = R.bracket(pt, [99, 100, 150, 200, 299, 300, 650, 1000, 1001], 500)
    assert j.tolist() == [-1, 0, 0, 1, 1, 2, 2, 2, 2]
    assert valid.tolist() == [False, True, True, True, True, False, False, False, False]      # the last bracket is 700 long: a drop-out
    j, num, den, valid = R.bracket(pt, [300, 1000, 1001], 700)
    assert valid.tolist() == [True, True, False] and num.tolist() == [0, 700, 701] and den.tolist() == [700] * 3


def test_pose_at_a_knot_is_the_knots_pose():
    pose_time, pose = R.odometry(3, 50)
    m, valid = R.pose_at(pose_time, pose, pose_time, GAP)
    assert valid.all()
    assert (m[:, 3::4].view(np.uint64) == pose[:, :3].view(np.uint64)).all()          # f = 0 (f = 1 at the last knot): exact
    for k in (0, 7, 48, 49):
        q = pose[k, 3:]
        want = SR.quat_matrix(q)
        assert np.abs(m[k].reshape(3, 4)[:, :3] - want).max() <= 4e-16 * 4, k
    # the last knot is reached as the END of the last bracket, and gives the same bits as a blend at f = 1
    end, _ = R.blend(pose[48:49], pose[49:50], np.array([1.0]))
    assert (end.view(np.uint64) == m[49].view(np.uint64)).all()
    # one ns outside either end: invalid, twelve NaN words
    m, valid = R.pose_at(pose_time, pose, [pose_time[0] - 1, pose_time[-1] + 1], GAP)
    assert not valid.any() and (m.view(np.uint64) == R.NAN64_WORD).all()


def test_rotation_of_an_unnormalised_quaternion_is_orthonormal():
    rng = np.random.default_rng(5)
    n = 20000
    q0 = rng.normal(size=(n, 4))
    q0 *= (rng.uniform(0.7, 1.0, size=n) / np.linalg.norm(q0, axis=1))[:, None]
    q1 = q0 + 0.3 * rng.normal(size=(n, 4))
    q1 *= (rng.uniform(0.7, 1.0, size=n) / np.linalg.norm(q1, axis=1))[:, None]
    p0, p1 = np.concatenate([np.zeros((n, 3)), q0], 1), np.concatenate([np.ones((n, 3)), q1], 1)
    f = R.fraction(rng.integers(0, 1000, size=n), np.full(n, 1000)).astype(np.float64) * 2.0 ** -32
    m, ok = R.blend(p0, p1, f)
    assert ok.all()
    rot = m.reshape(n, 3, 4)[:, :, :3]
    worst = np.abs(rot @ rot.transpose(0, 2, 1) - np.eye(3)).max()
    print("|R R^T - I| <= %.2e" % worst)
    assert worst <= 1e-14
    assert (np.linalg.det(rot) > 0.99).all()


def test_both_signs_of_the_second_quaternion_give_the_same_rotation():
    pose_time, pose = R.odometry(9, 40)
    flipped = pose.copy()
    flipped[1::2, 3:] *= -1.0                                # every bracket now has d < 0
    tau = pose_time[0] + np.arange(0, 390_000_000, 1_234_567, dtype=np.int64)
    a, va = R.pose_at(pose_time, pose, tau, GAP)
    b, vb = R.pose_at(pose_time, flipped, tau, GAP)
    assert va.all() and vb.all()
    assert (a.view(np.uint64) == b.view(np.uint64)).all()
    # without the sign the blend would pass near the origin of the quaternions: the rule is what keeps n away from 0
    d = (flipped[:-1, 3:] * flipped[1:, 3:]).sum(1)
    assert (d < 0).all()


def _slerp(q0, q1, f):
    d = float(q0 @ q1)
    if d < 0:
        q1, d = -q1, -d
    omega = np.arccos(min(d, 1.0))
    return (np.sin((1 - f) * omega) * q0 + np.sin(f * omega) * q1) / np.sin(omega)


def _angle_between(Ra, Rb):
    """The rotation angle of Ra Rb^T from |Ra Rb^T - I|_F = 2 sqrt(2) sin(angle / 2): accurate near 0, where arccos of a trace is not."""
    return 2.0 * np.arcsin(min(np.linalg.norm(Ra @ Rb.T - np.eye(3)) / (2.0 * np.sqrt(2.0)), 1.0))


@pytest.mark.parametrize("omega", [0.02, 0.1, 0.5, 1.0])
def test_nlerp_against_slerp(omega):
    rng = np.random.default_rng(int(omega * 1000))
    worst = 0.0
    for trial in range(8):
        q0 = rng.normal(size=4)
        q0 /= np.linalg.norm(q0)
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        dq = np.concatenate([[np.cos(omega / 2)], np.sin(omega / 2) * axis])          # a rotation by omega about the axis
        w0, x0, y0, z0 = q0
        w1, x1, y1, z1 = dq
        q1 = np.array([w0 * w1 - x0 * x1 - y0 * y1 - z0 * z1, w0 * x1 + x0 * w1 + y0 * z1 - z0 * y1,
                       w0 * y1 - x0 * z1 + y0 * w1 + z0 * x1, w0 * z1 + x0 * y1 - y0 * x1 + z0 * w1])
        if trial % 2:
            q1 = -q1
        steps = 64
        fi = R.fraction(np.arange(steps + 1), np.full(steps + 1, steps))
        f = fi.astype(np.float64) * 2.0 ** -32
        p0, p1 = np.concatenate([np.zeros(3), q0])[None].repeat(steps + 1, 0), np.concatenate([np.zeros(3), q1])[None].repeat(steps + 1, 0)
        m, ok = R.blend(p0, p1, f)
        assert ok.all()
        for k in range(steps + 1):
            got = m[k].reshape(3, 4)[:, :3]
            want = SR.quat_matrix(_slerp(q0, q1, float(f[k])))
            worst = max(worst, _angle_between(got, want))
    print("omega %.2f: nlerp is at most %.3e rad from slerp (bound %.3e)" % (omega, worst, 0.0041 * omega ** 3 + 1e-12))
    assert worst <= 0.0041 * omega ** 3 + 1e-12


@pytest.mark.parametrize("yaw", [0.005, 0.05])
def test_physical_scene_is_put_right_by_deskewing_and_not_without(yaw):
    sc = R.physical_scene(2, 4000, yaw)
    out = R.deskew_reference(sc["points"], sc["offsets"], sc["scan_time"], sc["pose_time"], sc["pose"], sc["point_dt"], GAP)
    assert out["status"].tolist() == [0] and not np.isnan(out["points_out"]).any()
    tol = sc["ranges"] * 0.0041 * yaw ** 3 + sc["ranges"] * 2.0 ** -22 + 1e-9
    err = np.linalg.norm(out["points_out"].astype(np.float64) - sc["truth"], axis=1)
    print("yaw %.3f per interval: de-skewed within %.3e m (worst share of its bound %.3f)" % (yaw, err.max(), (err / tol).max()))
    assert (err <= tol).all()
    assert int(sc["point_dt"].max()) > 90_000_000 and (np.diff(sc["point_dt"]) >= 0).all()
    # the same scene WITHOUT point_dt: every row is taken at the scan's own time.  It misses the bound by orders of magnitude
    flat = R.deskew_reference(sc["points"], sc["offsets"], sc["scan_time"], sc["pose_time"], sc["pose"], np.zeros_like(sc["point_dt"]), GAP)
    err0 = np.linalg.norm(flat["points_out"].astype(np.float64) - sc["truth"], axis=1)
    print("            left skewed: off by up to %.3f m" % err0.max())
    assert err0.max() > 100 * tol.max() and err0.max() > 0.5
    # ... and with point_dt = 0 the rows come back as they went in (R_s^T R_s p rounds to p)
    assert (flat["points_out"].view(np.uint32) == sc["points"].view(np.uint32)).all()
    none = R.deskew_reference(sc["points"], sc["offsets"], sc["scan_time"], sc["pose_time"], sc["pose"], None, GAP)
    assert "points_out" not in none and (none["scan_pose"].view(np.uint64) == out["scan_pose"].view(np.uint64)).all()


def test_reference_statuses():
    pose_time, pose = R.odometry(4, 30)
    scans = [SR.scan(i, 6) for i in range(4)]
    points, offsets = SR.pack(scans)
    scan_time = np.array([pose_time[0] - 5, pose_time[3] + 77, pose_time[-1] - 10, pose_time[10]], np.int64)
    dt = np.zeros(24, np.int32)
    dt[6:12] = [-1000, 0, 5, 10_000_000, 60_000_000, -30_000_000]
    dt[12:18] = [0, 10, 11, -5, 9, 10]                      # 11 ns behind the scan lies 1 ns outside the odometry
    points[20, 1] = np.inf
    out = R.deskew_reference(points, offsets, scan_time, pose_time, pose, dt, GAP)
    assert out["status"].tolist() == [R.NO_POSE, 0, R.PART_POSE, 0]
    gone = (out["points_out"].view(np.uint32) == R.NAN_WORD).all(1)
    assert gone.tolist() == [True] * 6 + [False] * 6 + [False, False, True, False, False, False] + [False, False, True] + [False] * 3
    # whole-call failures
    for bad_time in (pose_time[::-1].copy(), np.concatenate([pose_time[:5], pose_time[4:-1]])):
        bad = R.deskew_reference(points, offsets, scan_time, bad_time, pose, dt, GAP)
        assert bad["failed"] and bad["status"].tolist() == [R.NO_POSE] * 4 and len(bad["points_out"]) == 0
        assert (bad["scan_pose"].view(np.uint64) == R.NAN64_WORD).all()
        assert R.interp_reference(bad_time, pose, scan_time, GAP)[1].tolist() == [R.NO_POSE] * 4
    for bad_offsets in ([0, 6, 5, 18, 24], [-1, 6, 12, 18, 24], [0, 6, 12, 18, 25]):
        assert R.deskew_reference(points, bad_offsets, scan_time, pose_time, pose, dt, GAP)["failed"]
    # a NaN in one pose row: only the times inside its two brackets go
    hurt = pose.copy()
    hurt[12, 5] = np.nan
    tau = pose_time[10] + np.arange(0, 40_000_001, 2_500_000, dtype=np.int64)
    m, valid = R.pose_at(pose_time, hurt, tau, GAP)
    inside = (tau >= pose_time[11]) & (tau < pose_time[13])          # (knot 11 blends with 0 * NaN; knot 13 opens the next bracket)
    assert (valid == ~inside).all() and inside.sum() == 8


def test_fifth_header_is_bound_like_the_others():
    L = H.pkg("lib")
    text = open(os.path.join(H.ROOT, "include", "epcnet_stamps.h")).read()
    assert L.STAMPS_HEADER_PATH == os.path.join(H.ROOT, "include", "epcnet_stamps.h")
    functions, constants, status = L.parse_header(text, need_status=False)
    assert list(functions) == L.STAMP_EXPORTS == ["epcnet_deskew_workspace_bytes", "epcnet_pose_interp", "epcnet_scan_deskew"]
    assert status == {}
    for other in (L.EXPORTS, L.POSE_EXPORTS, L.SCAN_EXPORTS, L.SUBMAP_EXPORTS, L.LAUNCHING):
        assert not set(L.STAMP_EXPORTS) & set(other)
    assert constants == {"EPC_STATUS_NO_POSE": 64, "EPC_STATUS_PART_POSE": 128}
    assert L.EPC_STATUS_NO_POSE == R.NO_POSE == 64 and L.EPC_STATUS_PART_POSE == R.PART_POSE == 128
    taken = (L.EPC_STATUS_NONFINITE_INPUT | L.EPC_STATUS_FP16_RANGE | L.EPC_STATUS_NO_GRID | L.EPC_STATUS_NO_GROUND | L.EPC_STATUS_NO_SUBMAP
             | L.EPC_STATUS_NO_ROOM)
    assert taken == 63 and (L.EPC_STATUS_NO_POSE | L.EPC_STATUS_PART_POSE) & taken == 0
    size, interp, deskew = L.lib().epcnet_deskew_workspace_bytes, L.lib().epcnet_pose_interp, L.lib().epcnet_scan_deskew
    assert size.restype is ctypes.c_size_t and size.argtypes == [ctypes.c_int, ctypes.c_int, ctypes.c_longlong]
    assert interp.restype is ctypes.c_int and len(interp.argtypes) == 9 and deskew.restype is ctypes.c_int and len(deskew.argtypes) == 16
    assert not hasattr(L.run, "epcnet_deskew_workspace_bytes") and hasattr(L.run, "epcnet_pose_interp") and hasattr(L.run, "epcnet_scan_deskew")
    # the `long long` parameters: times by pointer (a void* to ctypes: ops checks the int64 dtype), counts and the gap by value
    ret, types, names = functions["epcnet_scan_deskew"]
    assert ret == "int" and (types[-1], names[-1]) == ("void*", "stream") and names[-3:-1] == ["workspace", "workspace_bytes"]
    assert types[names.index("scan_time")] == types[names.index("pose_time")] == "long long*"
    assert types[names.index("num_rows")] == types[names.index("max_gap_ns")] == "long long"
    assert types[names.index("point_dt")] == "int32_t*" and types[names.index("pose")] == types[names.index("scan_pose")] == "double*"
    assert deskew.argtypes[names.index("max_gap_ns")] is ctypes.c_longlong and deskew.argtypes[names.index("scan_time")] is ctypes.c_void_p
    ret, types, names = functions["epcnet_pose_interp"]
    assert names == ["pose_time", "pose", "num_poses", "query_time", "num_queries", "max_gap_ns", "pose_out", "status", "stream"]
    assert types[0] == types[3] == "long long*" and types[5] == "long long" and interp.argtypes[5] is ctypes.c_longlong
    assert "long long*" not in L._POINTEES
    # the size query launches nothing and answers 0 for what the entries refuse
    assert size(64, 1000, 100000) >= 16 + 4 * 64 and size(0, 2, 0) > 0 and size(64, 1000, 100000) % 16 == 0
    for bad in ((-1, 2, 0), ((1 << 24) + 1, 2, 0), (4, 1, 0), (4, 0, 0), (4, (1 << 24) + 1, 0), (4, 2, -1), (4, 2, 1 << 31)):
        assert size(*bad) == 0, bad


def test_refusals_launch_nothing():
    """Every EPC_EINVAL and the EPC_ENOMEM are decided on the host before anything touches a device: the pointers here are made-up
    addresses that are never followed."""
    L = H.pkg("lib")
    lib = L.lib()
    A = 0x10000                                              # 16-byte aligned
    need = lib.epcnet_deskew_workspace_bytes(8, 50, 400)
    good = dict(points=A, offsets=2 * A, num_rows=400, num_scans=8, point_dt=3 * A, scan_time=4 * A, pose_time=5 * A, pose=6 * A,
                num_poses=50, max_gap_ns=GAP, points_out=7 * A, scan_pose=8 * A, status=9 * A, workspace=10 * A, workspace_bytes=need)
    order = list(good)
    bad = [dict(points=None), dict(offsets=None), dict(scan_time=None), dict(pose_time=None), dict(pose=None), dict(scan_pose=None),
           dict(status=None), dict(workspace=None), dict(points_out=None), dict(points_out=A), dict(num_rows=-1), dict(num_rows=1 << 31),
           dict(num_scans=-1), dict(num_scans=(1 << 24) + 1), dict(num_poses=1), dict(num_poses=0), dict(num_poses=(1 << 24) + 1),
           dict(max_gap_ns=0), dict(max_gap_ns=-5), dict(max_gap_ns=1 << 31), dict(workspace=10 * A + 8)]
    for change in bad:
        a = dict(good, **change)
        assert lib.epcnet_scan_deskew(*[a[k] for k in order], None) == L.EPC_EINVAL, change
        assert b"epcnet_scan_deskew" in lib.epc_last_error()
    assert lib.epcnet_scan_deskew(*[dict(good, workspace_bytes=need - 1)[k] for k in order], None) == L.EPC_ENOMEM
    good = dict(pose_time=A, pose=2 * A, num_poses=50, query_time=3 * A, num_queries=8, max_gap_ns=GAP, pose_out=4 * A, status=5 * A)
    order = list(good)
    bad = [dict(pose_time=None), dict(pose=None), dict(query_time=None), dict(pose_out=None), dict(status=None), dict(num_poses=1),
           dict(num_poses=(1 << 24) + 1), dict(num_queries=-1), dict(num_queries=(1 << 24) + 1), dict(max_gap_ns=0), dict(max_gap_ns=1 << 31)]
    for change in bad:
        a = dict(good, **change)
        assert lib.epcnet_pose_interp(*[a[k] for k in order], None) == L.EPC_EINVAL, change
        assert b"epcnet_pose_interp" in lib.epc_last_error()
    assert lib.epcnet_pose_interp(*[dict(good, num_queries=0)[k] for k in order], None) == L.EPC_OK       # no query: nothing to launch
