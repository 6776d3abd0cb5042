"""The numpy restatement of epcnet_ground_remove (tests/ground_ref.py) against the formulas of include/epcnet_scans.h written a second way
(float64 geometry, Python-integer hashing), what it recovers on the seeded scenes, its degenerate inputs, and the binding of the third
header.  No GPU: tests/test_gpu_ground.py holds the kernels to this restatement bit for bit."""
import ctypes
import os

import numpy as np
import pytest

import downsample_ref as D
import ground_ref as G
import helpers as H

U = 2.0 ** -24          # float32 unit roundoff


def _mix_int(x):
    x &= 0xffffffff
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    x ^= x >> 16
    return x


@pytest.mark.parametrize("seed", [0, 1, -1, 0x123456789abcdef, -(1 << 63)])
def test_candidate_rows_by_python_integers(seed):
    H_, K, M = 128, 8, 54321
    rows = G.candidate_rows(M, H_, K, seed)
    assert rows.shape == (H_, 3, K) and rows.min() >= 0 and rows.max() < M
    s64 = seed & 0xffffffffffffffff
    s = _mix_int(_mix_int(s64 & 0xffffffff) ^ (s64 >> 32))
    for h in (0, 1, 63, 64, 127):
        sh = _mix_int(s ^ h)
        for j in range(3):
            for k in range(K):
                assert rows[h, j, k] == (_mix_int(sh ^ (K * j + k)) * M) >> 32
    assert len(np.unique(rows)) > 0.9 * rows.size * (1 - rows.size / (2.0 * M))          # a spread draw, not a stuck one
    assert G.candidate_rows(1, 64, 16, seed).max() == 0 and G.candidate_rows(1 << 20, 64, 1, seed).max() < (1 << 20)


def test_vertices_are_the_lowest_finite_candidates():
    p = G.family(3)
    K = 8
    rows = G.candidate_rows(len(p), 64, K, 5)
    n, d0, thr, valid = G.planes(p, 64, K, 0.2, G.cos2_of(15.0), np.inf, 5)
    for h in range(64):
        vs = []
        for j in range(3):
            best = None
            for k in range(K):
                q = p[rows[h, j, k]]
                if np.isfinite(q).all() and (best is None or q[2] < best[2]):
                    best = q
            vs.append(best)
        if any(v is None for v in vs):
            assert not valid[h]
            continue
        v = np.array(vs, np.float64)
        n64 = np.cross(v[1] - v[0], v[2] - v[0])
        if n64[2] < 0:
            n64 = -n64
        scale = np.abs(v[1] - v[0]).max() * np.abs(v[2] - v[0]).max()
        assert np.abs(n[h] - n64).max() <= 8 * U * scale                                 # (two products and a difference per component)
        if n64 @ n64 > 1e-6 and abs(n64[2] ** 2 - float(G.cos2_of(15.0)) * (n64 @ n64)) > 1e-4 * (n64 @ n64):
            assert valid[h] == (n64[2] ** 2 >= float(G.cos2_of(15.0)) * (n64 @ n64))
            if valid[h]:
                assert abs(thr[h] - 0.04 * (n64 @ n64)) <= 1e-5 * 0.04 * (n64 @ n64)


@pytest.mark.parametrize("seed", [0, 7])
def test_removal_against_float64_geometry(seed):
    """Row by row: float64 ``pts @ n - d0`` decides as the restatement wherever its margin to the threshold exceeds the float32
    rounding bound of the sum (three products, two sums, a difference, the square, and the threshold's own three roundings)."""
    p = G.family(seed)
    out, status, plane, info = G.remove_ground_ref(p)
    assert status == 0
    n, d0 = plane[:3].astype(np.float64), float(plane[3])
    fin = np.isfinite(p).all(1)
    p64 = np.where(fin[:, None], p, 0).astype(np.float64)
    e = p64 @ n - d0
    bound = 0.2 * np.sqrt(n @ n)
    slack = 8 * U * (np.abs(p64 * n).sum(1) + abs(d0) + bound)
    gone = np.isnan(out).all(1) & fin
    sure_gone, sure_kept = fin & (e < bound - slack), fin & (e > bound + slack)
    assert (sure_gone | sure_kept)[fin].mean() > 0.999
    assert gone[sure_gone].all() and not gone[sure_kept].any()
    kept = ~gone
    assert (out.view(np.uint32)[kept] == p.view(np.uint32)[kept]).all()                  # every other row keeps its bits, NaN rows too
    assert (out.view(np.uint32)[gone] == G.NAN_WORD).all()
    # the score is the count of finite rows inside the slab
    inside = fin & (np.abs(e) <= bound - slack)
    maybe = fin & (np.abs(e) <= bound + slack)
    assert inside.sum() <= info[3] <= maybe.sum() and info[0] == fin.sum()


def _recovered(p, n, d):
    out, status, plane, info = G.remove_ground_ref(p)
    fin = np.isfinite(p).all(1)
    dist = np.where(fin[:, None], p, 0).astype(np.float64) @ n - d
    gone = np.isnan(out).all(1) & fin
    near, above = fin & (np.abs(dist) <= 0.1), fin & (dist >= 0.5)
    return status, float(gone[near].mean()), int(gone[above].sum())


@pytest.mark.parametrize("block", range(6))
def test_recovery_on_the_scene_family(block):
    """At the defaults, 60 scans of the family (ten per case): a plane is found, at least 0.999 of the finite rows within 0.1 m of the
    true plane go, and NO finite row 0.5 m or more above it goes."""
    for seed in range(10 * block, 10 * block + 10):
        p, n, d = G.family(seed, with_truth=True)
        status, recall, wrong = _recovered(p, n, d)
        assert status == 0 and recall >= 0.999 and wrong == 0, (seed, status, recall, wrong)


@pytest.mark.parametrize("M", [40, 41, 100, 200, 1000, 3000, 9000, 20000, 32768, 70000])
def test_recovery_on_the_downsampler_scenes(M):
    status, recall, wrong = _recovered(D.scene(M, M), np.array([0.0, 0.0, 1.0]), 0.0)
    assert status == 0 and recall >= 0.999 and wrong == 0, (M, status, recall, wrong)


def _unchanged(p, res):
    return res[0].shape == p.shape and (res[0].view(np.uint32) == p.view(np.uint32)).all() and np.isnan(res[2]).all()


def test_degenerate_inputs_report_no_ground_and_change_nothing():
    wall = G.wall_only(5000, 1)
    res = G.remove_ground_ref(wall)
    assert res[1] == G.NO_GROUND and res[3] == [5000, 0, -1, 0] and _unchanged(wall, res)       # no valid hypothesis at all
    cube = G.cube(5000, 2)
    res = G.remove_ground_ref(cube)
    assert res[1] == G.NO_GROUND and res[3][1] > 0 and 3 <= res[3][3] < 0.05 * 5000 and _unchanged(cube, res)   # the share is too small
    scene = D.scene(40, 3)
    for M in (0, 1, 2, 3):
        res = G.remove_ground_ref(scene[:M])
        assert res[1] == G.NO_GROUND and res[3][0] == M and _unchanged(scene[:M], res)
    nans = np.full((500, 3), np.nan, np.float32)
    nans[::3, 1] = 1.0
    nans[1::3, 0] = np.inf
    res = G.remove_ground_ref(nans)
    assert res[1] == G.NO_GROUND and res[3] == [0, 0, -1, 0] and _unchanged(nans, res)
    out, status, plane, info = G.reference_batch([wall, scene, cube])
    assert status.tolist() == [8, 0, 8] and out.shape == (10040, 3) and plane.shape == (3, 4) and info.shape == (3, 4)


def test_max_z_chooses_the_plane_below_the_sensor():
    roofed = G.roofed(0)
    top, low = G.remove_ground_ref(roofed), G.remove_ground_ref(roofed, max_z=0.0)
    assert top[1] == 0 and abs(top[2][3] / top[2][2] - 3.0) < 0.1 and top[3][3] >= 29000
    assert low[1] == 0 and abs(low[2][3] / low[2][2] + 1.8) < 0.1 and 2400 <= low[3][3] <= 2600


def test_third_header_is_bound_like_the_others():
    L = H.pkg("lib")
    text = open(os.path.join(H.ROOT, "include", "epcnet_scans.h")).read()
    functions, constants, status = L.parse_header(text, need_status=False)
    assert list(functions) == L.SCAN_EXPORTS == ["epcnet_ground_workspace_bytes", "epcnet_ground_remove"] and status == {}
    for other in (L.EXPORTS, L.POSE_EXPORTS, L.LAUNCHING):
        assert not set(L.SCAN_EXPORTS) & set(other)
    assert constants["EPC_STATUS_NO_GROUND"] == L.EPC_STATUS_NO_GROUND == G.NO_GROUND == 8
    assert L.EPC_STATUS_NO_GROUND & (L.EPC_STATUS_NONFINITE_INPUT | L.EPC_STATUS_FP16_RANGE | L.EPC_STATUS_NO_GRID) == 0
    size, remove = L.lib().epcnet_ground_workspace_bytes, L.lib().epcnet_ground_remove
    assert size.restype is ctypes.c_size_t and size.argtypes == [ctypes.c_int, ctypes.c_int, ctypes.c_longlong]
    assert not hasattr(L.run, "epcnet_ground_workspace_bytes") and hasattr(L.run, "epcnet_ground_remove")
    ret, types, names = functions["epcnet_ground_remove"]
    assert remove.restype is ctypes.c_int and len(remove.argtypes) == len(types) == 18 and names[-1] == "stream"
    assert remove.argtypes[names.index("seed")] is ctypes.c_longlong and remove.argtypes[names.index("workspace_bytes")] is ctypes.c_size_t
    assert [remove.argtypes[names.index(n)] for n in ("threshold", "cos2_tilt", "max_z", "min_share")] == [ctypes.c_float] * 4
    # the size query launches nothing: 0 for what the call refuses
    assert size(64, 256, 1 << 21) > 0 and size(0, 64, 0) > 0 and size(64, 1024, 0) > size(64, 64, 0)
    assert size(64, 100, 10) == 0 and size(64, 32, 10) == 0 and size(64, 1088, 10) == 0 and size(-1, 64, 10) == 0 and size(1, 64, -1) == 0
    assert size(1, 64, 1 << 31) == 0
    # a refusal reaches the caller before anything is launched: no device is needed for it (the pointers are never followed)
    good = dict(hypotheses=256, draws=8, threshold=0.2, cos2_tilt=0.9, max_z=float("inf"), min_share=0.05)
    for bad in (dict(hypotheses=100), dict(hypotheses=0), dict(hypotheses=2048), dict(draws=0), dict(draws=17), dict(threshold=0.0),
                dict(threshold=float("inf")), dict(threshold=float("nan")), dict(cos2_tilt=0.0), dict(cos2_tilt=1.5), dict(cos2_tilt=float("nan")),
                dict(max_z=float("nan")), dict(min_share=-0.1), dict(min_share=1.5), dict(min_share=float("nan"))):
        a = dict(good, **bad)
        with pytest.raises(L.EpcNetError) as e:
            L.run.epcnet_ground_remove(4096, 4096, 10, 1, a["hypotheses"], a["draws"], a["threshold"], a["cos2_tilt"], a["max_z"], a["min_share"],
                                       0, 4096, 4096, None, 4096, 4096, 1 << 20, stream=0)
        assert e.value.status == L.EPC_EINVAL and "epcnet_ground_remove" in str(e.value), bad
    with pytest.raises(L.EpcNetError) as e:                                             # a short workspace
        L.run.epcnet_ground_remove(4096, 4096, 10, 1, 256, 8, 0.2, 0.9, float("inf"), 0.05, 0, 4096, 4096, None, 4096, 4096,
                                   size(1, 256, 10) - 1, stream=0)
    assert e.value.status == L.EPC_ENOMEM
