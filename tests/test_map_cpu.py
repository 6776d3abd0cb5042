"""The definition of include/epcnet_maps.h as tests/map_ref.py restates it, without a device: the restatement against a second
formulation in Python integers and fractions, why float32 poses are refused, the tenth header's binding, and the entry's refusals, which
launch nothing."""
import ctypes
import math
import os
from fractions import Fraction as F

import numpy as np
import pytest
import torch

import helpers as H
import map_ref as M


def _one(row, voxel=1.0, t=(0.0, 0.0, 0.0), origin=(0.0, 0.0, 0.0)):
    """kind and w of ONE row under the identity rotation, from the restatement."""
    kind, w = M.lattice(np.asarray([row], np.float32), [0, 1], M.identity_poses(1, t), np.asarray(origin, np.float64), voxel)
    return int(kind[0]), [int(v) for v in w[0]]


def test_restatement_agrees_with_integers_and_fractions():
    """The lattice scene (every value exact) voxel by voxel against dictionaries of Python integers: cells, leaders' order, counts and
    means; then single rows: negative coordinates, cell faces, -0.0, the four range edges at voxel 1, exact float32 inputs."""
    points, offsets, poses, origin = M.lattice_scene()
    for voxel in (0.5, 0.75):
        ref = M.reference(points, offsets, poses, origin, voxel, len(points))
        voxels, kinds = M.exact_map(points, offsets, poses.reshape(-1, 3, 4), origin, voxel)
        assert ref["num_out"].tolist() == [len(voxels), len(points), 0, 0] and set(kinds) == {M.KEPT}
        step = F(voxel) / 4096
        want = np.array([[float(np.float32(float((c * 4096 + m) * step))) for c, m in zip(cell, mean)] for cell, _, mean in voxels], np.float32)
        assert (ref["map_points"][:len(voxels)].view(np.uint32) == want.view(np.uint32)).all()
        assert ref["count"][:len(voxels)].tolist() == [n for _, n, _ in voxels]
        assert (ref["map_points"][len(voxels):].view(np.uint32) == M.NAN_WORD).all() and not ref["count"][len(voxels):].any()
    # w >> 12 == floor(q / voxel) at negative coordinates, for voxels that are no power of two as well
    rng = np.random.default_rng(0)
    for voxel in (0.2, 0.5, 1.0, 3.0):
        rows = rng.uniform(-50, 50, size=(200, 3)).astype(np.float32)
        kind, w = M.lattice(rows, [0, 200], M.identity_poses(1), np.zeros(3), voxel)
        q = rows.astype(np.float64)
        assert (kind == M.KEPT).all() and ((w >> 12) == np.floor(q / np.float64(voxel)).astype(np.int64)).all()
        assert (w >> 12).min() < -10 and ((w & 4095) >= 0).all()
        for r in range(0, 200, 17):                                          # ... and the rational floor of the rounded quotient
            for a in range(3):
                assert int(w[r, a]) == math.floor(F(float(np.float64(q[r, a]) / np.float64(voxel))) * 4096)
    # exactly on a cell face, on both sides of the origin; -0.0 is cell 0, the double below it cell -1
    assert _one((1.0, -1.0, 0.0)) == (M.KEPT, [4096, -4096, 0])
    assert _one((-0.0, 0.5, -0.5), voxel=0.5) == (M.KEPT, [0, 4096, -4096])
    assert _one((-1e-30, 0.0, 0.0))[1][0] == -1 and (-1 >> 12) == -1 and (-1 & 4095) == 4095
    assert _one((2.0, 2.0, 2.0), voxel=0.5, t=(-1.0, -2.0, -3.0)) == (M.KEPT, [2 * 4096, 0, -2 * 4096])
    # the four range edges at voxel 1: w = 2^32 - 1 and -2^32 are kept (cells 2^20 - 1 and -2^20), 2^32 and -2^32 - 1 are out of range
    top = 1048575.75                                                         # exact in float32; with t = 1/4 - 1/4096 the lattice's last point
    assert float(np.float32(top)) == top
    assert _one((top, 0.0, 0.0), t=(0.25 - 1.0 / 4096, 0.0, 0.0)) == (M.KEPT, [(1 << 32) - 1, 0, 0])
    assert _one((top, 0.0, 0.0), t=(0.25, 0.0, 0.0))[0] == M.OUT_OF_RANGE
    assert _one((0.0, -1048576.0, 0.0)) == (M.KEPT, [0, -(1 << 32), 0])
    assert _one((0.0, -1048576.0, 0.0), t=(0.0, -1.0 / 4096, 0.0))[0] == M.OUT_OF_RANGE
    assert _one((0.0, 0.0, -1048576.0), origin=(0.0, 0.0, 2.0 ** -20))[0] == M.OUT_OF_RANGE     # w = -2^32 - 1 after the floor
    keys = M.keys_of(np.array([[(1 << 32) - 1, -(1 << 32), 0]], np.int64))
    assert int(keys[0]) == ((1 << 20) << 42) | (0 << 21) | ((1 << 21) - 1) and int(keys[0]) < (1 << 63)
    # absent: a NaN or infinite row, a NaN pose, a NaN origin; an overflowing quotient
    assert _one((np.nan, 0.0, 0.0))[0] == M.ABSENT and _one((0.0, np.inf, 0.0))[0] == M.ABSENT
    assert _one((0.0, 0.0, 0.0), t=(0.0, np.nan, 0.0))[0] == M.ABSENT and _one((0.0, 0.0, 0.0), origin=(np.nan, 0.0, 0.0))[0] == M.ABSENT
    assert _one((3e38, 0.0, 0.0), voxel=2.0 ** -20)[0] == M.OUT_OF_RANGE and _one((1.0, 0.0, 0.0), t=(1e308, 0.0, 0.0), voxel=2.0 ** -20)[0] == M.ABSENT


def test_reference_rules():
    points, offsets, poses, origin = M.drive(1, (5000,) * 4)
    points = points.copy()
    points[::97, 0] = np.nan
    ref = M.reference(points, offsets, poses, origin, 0.5, len(points))
    V = ref["V"]
    assert ref["num_out"].tolist() == [V, 19793, 207, 0] and 10000 < V < 19793 and int(ref["count"].sum()) == 19793
    assert (np.diff(ref["leader"]) > 0).all() and ref["leader"][0] == 1                      # row 0 is a NaN row
    assert np.isfinite(ref["map_points"][:V]).all() and np.abs(ref["map_points"][:V]).max() < 100.0
    # a voxel's point lies inside its voxel
    kind, w = M.lattice(points, offsets, poses, origin, 0.5)
    g = (w[ref["leader"]] >> 12).astype(np.float64)
    assert (ref["map_points"][:V] >= (g * 0.5).astype(np.float32)).all() and (ref["map_points"][:V] <= ((g + 1) * 0.5).astype(np.float32)).all()
    # min_count: the same numbering and counts, NaN rows where the count is smaller
    two = M.reference(points, offsets, poses, origin, 0.5, len(points), min_count=2)
    assert (two["count"] == ref["count"]).all() and two["num_out"].tolist() == ref["num_out"].tolist()
    gone = np.isnan(two["map_points"][:V]).all(1)
    assert (gone == (ref["count"][:V] < 2)).all() and 0 < gone.sum() < V
    # overflow by one voxel, and invalid offsets
    over = M.reference(points, offsets, poses, origin, 0.5, V - 1)
    assert over["num_out"].tolist() == [-1, 19793, 207, 0] and not over["count"].any() and (over["map_points"].view(np.uint32) == M.NAN_WORD).all()
    exact = M.reference(points, offsets, poses, origin, 0.5, V)
    assert exact["num_out"][0] == V and (exact["map_points"].view(np.uint32) == ref["map_points"][:V].view(np.uint32)).all()
    bad = offsets.copy()
    bad[2] = bad[1] - 1
    assert M.reference(points, bad, poses, origin, 0.5, 100)["num_out"].tolist() == [-1, 0, 0, 0]


def test_float32_poses_would_move_rows_across_voxel_faces():
    """Why float32 poses are refused: at UTM size a float32 translation is up to 0.25 m off (the spacing is 0.5 m at 5.7e6), more than a
    0.2 m voxel: of 2000 rows most change their voxel, and the map's voxel set changes."""
    points, offsets, poses, origin = M.drive(2, (500,) * 4)
    rounded = poses.astype(np.float32).astype(np.float64)
    assert np.abs(rounded - poses).max() > 0.05
    _, w64 = M.lattice(points, offsets, poses, origin, 0.2)
    _, w32 = M.lattice(points, offsets, rounded, origin, 0.2)
    moved = ((w64 >> 12) != (w32 >> 12)).any(1)
    print("rows whose voxel a float32 pose changes: %d of %d" % (moved.sum(), len(points)))
    assert moved.mean() > 0.5
    L = H.pkg("lib")

    class Fake:
        def __init__(self, dtype):
            self.dtype, self.is_cuda = dtype, True

        def data_ptr(self):
            return 0x10000

    f32, f64, i32 = Fake(torch.float32), Fake(torch.float64), Fake(torch.int32)
    params = (ctypes.c_double * 8)(0.2, 1.0)
    with pytest.raises(L.EpcNetError) as e:                                   # refused before the library is reached
        L.run.epcnet_map_fuse(f32, i32, 8, 1, f32, f64, params, 8, f32, i32, i32, f64, 1 << 20, stream=0)
    assert "argument 5" in str(e.value) and "poses" in str(e.value) and "torch.float64" in str(e.value)


def test_tenth_header_is_bound_like_the_others():
    L = H.pkg("lib")
    text = open(os.path.join(H.ROOT, "include", "epcnet_maps.h")).read()
    assert L.MAPS_HEADER_PATH == os.path.join(H.ROOT, "include", "epcnet_maps.h")
    assert ("maps", "MAP", False, False) in L._HEADERS
    functions, constants, status = L.parse_header(text, need_status=False)     # no `double` by value: the plain scalars read it
    assert list(functions) == L.MAP_EXPORTS == ["epcnet_map_fuse_workspace_bytes", "epcnet_map_fuse"]
    assert status == {} and constants == {"EPC_MAP_PARAMS": 8, "EPC_MAP_MAX_CELL": 1048576}
    assert L.EPC_MAP_PARAMS == 8 and L.EPC_MAP_MAX_CELL == M.MAX_CELL == 1 << 20
    for other in (L.EXPORTS, L.POSE_EXPORTS, L.SCAN_EXPORTS, L.SUBMAP_EXPORTS, L.STAMP_EXPORTS, L.REVISIT_EXPORTS, L.PAIR_EXPORTS,
                  L.TRAJECTORY_EXPORTS, L.FORM_EXPORTS, L.LAUNCHING):
        assert not set(L.MAP_EXPORTS) & set(other)
    for name in L.MAP_EXPORTS:
        assert hasattr(L.lib(), name)
    size, entry = L.lib().epcnet_map_fuse_workspace_bytes, L.lib().epcnet_map_fuse
    assert size.restype is ctypes.c_size_t and size.argtypes == [ctypes.c_longlong, ctypes.c_int, ctypes.c_longlong]
    ret, types, names = functions["epcnet_map_fuse"]
    assert names == ["points", "offsets", "num_rows", "num_clouds", "poses", "origin", "params", "max_voxels", "map_points", "count",
                     "num_out", "workspace", "workspace_bytes", "stream"]
    assert ret == "int" and (types[-1], names[-1]) == ("void*", "stream") and entry.restype is ctypes.c_int
    for n, t in (("points", "float*"), ("map_points", "float*"), ("poses", "double*"), ("origin", "double*"), ("params", "double*"),
                 ("offsets", "int32_t*"), ("count", "int32_t*"), ("num_out", "int32_t*"), ("num_rows", "long long"), ("max_voxels", "long long")):
        assert types[names.index(n)] == t, n
    P, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    assert entry.argtypes == [P, P, ll, i, P, P, P, ll, P, P, P, P, ctypes.c_size_t, P]
    assert hasattr(L.run, "epcnet_map_fuse") and not hasattr(L.run, "epcnet_map_fuse_workspace_bytes")
    with pytest.raises(ValueError):                                           # a second declaration of a name is refused like everywhere
        L.parse_header(text + "\nint epcnet_map_fuse(int n);\n", need_status=False)
    ops, scans = H.pkg("ops"), H.pkg("scans")
    assert ops.fuse_map is scans.fuse_map


def test_entry_refusals_launch_nothing():
    """EPC_EINVAL / EPC_ENOMEM from addresses that are never followed: nothing is launched, so no device is needed."""
    L = H.pkg("lib")
    size = L.lib().epcnet_map_fuse_workspace_bytes
    assert size(1000, 4, 1000) > 0 and size(1000, 4, 1000) % 16 == 0 and size(1001, 4, 1000) >= size(1000, 4, 1000) + 4 - 16
    assert size(1 << 20, 4, 1000) > size(1000, 4, 1000) and size(1000, 4, 1025) > size(1000, 4, 1000)
    assert size(1000, 4, 1000) == size(1000, 4, 1023) == size(1000, 999, 600)          # the table: the power of two >= 2 max_voxels + 1
    assert size(0, 0, 1) > 0 and size((1 << 31) - 1, 1 << 24, 1 << 28) > 0
    for rows, clouds, voxels in ((-1, 4, 10), (1 << 31, 4, 10), (10, -1, 10), (10, (1 << 24) + 1, 10), (10, 4, 0), (10, 4, (1 << 28) + 1)):
        assert size(rows, clouds, voxels) == 0
    a = 0x10000

    def call(rows=1000, clouds=4, voxels=1000, points=a, offsets=a, poses=a, origin=a, voxel=0.2, min_count=1.0, reserved=(0.0,) * 6,
             params=True, out=a, count=a, num=a, ws=a, ws_bytes=None):
        need = size(1000, 4, 1000) if ws_bytes is None else ws_bytes
        p = (ctypes.c_double * 8)(voxel, min_count, *reserved) if params else None
        return L.lib().epcnet_map_fuse(points, offsets, rows, clouds, poses, origin, p, voxels, out, count, num, ws, need, None)

    nan, inf = float("nan"), float("inf")
    bad = [dict(rows=-1), dict(rows=1 << 31), dict(clouds=-1), dict(clouds=(1 << 24) + 1), dict(voxels=0), dict(voxels=(1 << 28) + 1),
           dict(voxel=0.0), dict(voxel=-0.2), dict(voxel=nan), dict(voxel=inf), dict(voxel=2.0 ** -21), dict(voxel=2.0 ** 20 + 1.0),
           dict(min_count=0.0), dict(min_count=1.5), dict(min_count=nan), dict(min_count=2.0 ** 31), dict(min_count=-1.0),
           dict(ws=a + 8), dict(points=None), dict(offsets=None), dict(poses=None), dict(origin=None), dict(params=False), dict(out=None),
           dict(count=None), dict(num=None), dict(ws=None)]
    bad += [dict(reserved=tuple(1.0 if i == k else 0.0 for i in range(6))) for k in range(6)]
    for kw in bad:
        assert call(**kw) == L.EPC_EINVAL, kw
        assert b"epcnet_map_fuse" in L.lib().epc_last_error()
    assert call(ws_bytes=size(1000, 4, 1000) - 1) == L.EPC_ENOMEM and call(ws_bytes=0) == L.EPC_ENOMEM
    assert call(voxels=1025) == L.EPC_ENOMEM                                   # a workspace sized for a smaller table
