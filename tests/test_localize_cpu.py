"""include/epcnet_localize.h without a device: the header's row and binding, the restatement (tests/localize_ref.py) against an
independent brute force, the index's counts on constructed anchors, and what the iteration converges to on scenes of exact planes."""
import ctypes
import functools
import os

import numpy as np
import pytest

import helpers as H
import localize_ref as Z
import register_ref as RR

VOXEL = 0.2


def test_twelfth_header_is_bound_like_the_others():
    L = H.pkg("lib")
    text = open(os.path.join(H.ROOT, "include", "epcnet_localize.h")).read()
    assert L.LOCALIZE_HEADER_PATH == os.path.join(H.ROOT, "include", "epcnet_localize.h")
    stems = [row[0] for row in L._HEADERS]
    assert ("localize", "LOCALIZE", False, False) in L._HEADERS
    assert stems.index("localize") == stems.index("surfels") + 1 == stems.index("forms") - 1
    functions, constants, status = L.parse_header(text, need_status=False)     # no `double` by value: the plain scalars read it
    assert list(functions) == L.LOCALIZE_EXPORTS == ["epcnet_surfel_index_bytes", "epcnet_surfel_index", "epcnet_scan_localize_workspace_bytes",
                                                     "epcnet_scan_localize"]
    assert status == {} and constants == {"EPC_LOCALIZE_INDEX_PARAMS": 4, "EPC_LOCALIZE_PARAMS": 8}
    assert L.EPC_STATUS_NO_PAIR == Z.NO_PAIR and L.EPC_STATUS_NO_FIT == Z.NO_FIT and L.EPC_MAP_MAX_CELL == Z.MAX_CELL
    for other in (L.EXPORTS, L.POSE_EXPORTS, L.SCAN_EXPORTS, L.SUBMAP_EXPORTS, L.STAMP_EXPORTS, L.REVISIT_EXPORTS, L.PAIR_EXPORTS,
                  L.TRAJECTORY_EXPORTS, L.MAP_EXPORTS, L.SURFEL_EXPORTS, L.FORM_EXPORTS, L.LAUNCHING):
        assert not set(L.LOCALIZE_EXPORTS) & set(other)
    assert "_kernel" not in text and "lz_" not in text                          # no kernel, no form of one, is named in the public header
    i, ll, z, P = ctypes.c_int, ctypes.c_longlong, ctypes.c_size_t, ctypes.c_void_p
    want = {"epcnet_surfel_index_bytes": (z, [ll]),
            "epcnet_surfel_index": (i, [P, P, P, ll, P, P, z, P, P]),
            "epcnet_scan_localize_workspace_bytes": (z, [i, i, i]),
            "epcnet_scan_localize": (i, [P, i, i, P, i, P, z, P, P, ll, P, P, P, P, P, P, P, z, P])}
    for name, (restype, argtypes) in want.items():
        fn = getattr(L.lib(), name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert hasattr(L.run, "epcnet_surfel_index") and hasattr(L.run, "epcnet_scan_localize") and not hasattr(L.run, "epcnet_surfel_index_bytes")
    ops = H.pkg("ops")
    for name in ("index_surfels", "localize_scans", "map_seeds"):
        assert getattr(ops, name) is getattr(H.pkg("localize"), name)


def test_size_queries_refuse_and_grow():
    lib = H.pkg("lib").lib()
    assert [lib.epcnet_surfel_index_bytes(m) for m in (0, -1, 2 ** 28 + 1)] == [0, 0, 0]
    assert lib.epcnet_surfel_index_bytes(1) == 128 + 4 * 36 and lib.epcnet_surfel_index_bytes(2 ** 28) == 128 + 2 ** 30 * 36
    for m in (1, 2, 3, 1000, 4096):                                     # an empty slot always exists
        cap = (lib.epcnet_surfel_index_bytes(m) - 128) // 36
        assert cap & (cap - 1) == 0 and 2 * m + 1 <= cap < 2 * (2 * m + 1)
    for bad in ((-1, 1, 32), (2 ** 20 + 1, 1, 32), (1, 0, 32), (1, 65, 32), (1, 1, 0), (1, 1, 48), (1, 1, 4128)):
        assert lib.epcnet_scan_localize_workspace_bytes(*bad) == 0
    assert lib.epcnet_scan_localize_workspace_bytes(0, 1, 32) == 0      # nothing to hold
    assert lib.epcnet_scan_localize_workspace_bytes(1, 1, 32) == 240 + 96 + 16 + 16 + 16        # 29 sums are 232 bytes, every region rounded up to 16
    assert lib.epcnet_scan_localize_workspace_bytes(3, 2, 4096) == 3 * 2 * 16 * 29 * 8 + 3 * 96 + 48 + 32 + 16


# ---- the index -------------------------------------------------------------------------------------------------------------------------------
def test_index_counts_on_constructed_anchors():
    """Voxel 0.2.  fl32(0.6) = 0.60000002384 lies above 3 * 0.2 = 0.6000000000000001 (double): a mean just below the face x = 0.6 of cell
    2 that float32 rounds ONTO 0.6f names cell 3 -- the duplicate the header describes."""
    f32 = np.float32
    face = f32(0.6)
    assert np.floor(np.float64(face) / 0.2) == 3.0 and np.floor(0.599999999 / 0.2) == 2.0 and f32(0.599999999) == face
    anchor = np.array([[0.1, 0.1, 0.1],          # 0 indexed, cell (0, 0, 0)
                       [0.7, 0.1, 0.1],          # 1 indexed, cell (3, 0, 0)
                       [face, 0.1, 0.1],         # 2 duplicate of 1: rounded onto the face
                       [0.15, 0.05, 0.19],       # 3 duplicate of 0
                       [np.nan, 0.1, 0.1],       # 4 not present (anchor)
                       [0.3, 0.3, 0.3],          # 5 not present (centroid)
                       [0.5, 0.5, 0.5],          # 6 not present (normal)
                       [0.2 * 2 ** 20, 0.0, 0.0],            # 7 out of range: cell 2^20
                       [-0.2 * 2 ** 20 - 0.1, 0.0, 0.0],     # 8 out of range: cell -2^20 - 1
                       [-0.2 * 2 ** 20 + 0.05, 0.0, 0.0],    # 9 indexed: the first cell of the range
                       [0.2 * 2 ** 20 - 0.1, 0.0, 0.0],      # 10 indexed: the last cell of the range
                       [-0.05, -0.05, -0.05],    # 11 indexed, cell (-1, -1, -1)
                       [0.0, 0.0, 0.0]], f32)    # 12 duplicate of 0: exactly on the faces at the origin, cell (0, 0, 0)
    centroid = anchor.copy()
    centroid[4] = 0.1
    centroid[5, 1] = np.inf
    normal = np.tile(np.array([0, 0, 1], f32), (len(anchor), 1))
    normal[6, 2] = np.nan
    idx = Z.index_reference(anchor, centroid, normal, VOXEL)
    assert idx["kind"].tolist() == [0, 0, 2, 2, 1, 1, 1, 3, 3, 0, 0, 0, 2] and idx["num"] == [5, 3, 3, 2]
    assert sorted(idx["j"].tolist()) == [0, 1, 9, 10, 11]
    rev = Z.index_reference(anchor[::-1], centroid[::-1], normal[::-1], VOXEL)     # the lowest j wins, whatever it holds
    # in the reversed order surfel 12 (cell 0) comes first among {0, 3, 12} and surfel 2 first among {1, 2}
    assert rev["num"] == [5, 3, 3, 2] and sorted((12 - rev["j"]).tolist()) == [2, 9, 10, 11, 12]


# ---- correspondences against a brute force ---------------------------------------------------------------------------------------------------
def _brute(p, anchor, centroid, normal, voxel):
    """Independent of the restatement's lookups: per row a Python loop over ALL surfels: the indexed ones (the first of every cell)
    whose cell is within one of the row's on every axis, smallest float32 d2, ties by candidate order."""
    present = np.isfinite(anchor).all(1) & np.isfinite(centroid).all(1) & np.isfinite(normal).all(1)
    cell = np.floor(anchor.astype(np.float64) / voxel)
    ok = present & ((cell >= -Z.MAX_CELL) & (cell < Z.MAX_CELL)).all(1)
    seen, indexed = set(), []
    for j in np.nonzero(ok)[0]:
        if tuple(cell[j]) not in seen:
            seen.add(tuple(cell[j]))
            indexed.append(j)
    indexed = np.array(indexed, np.int64)
    out_j, out_d = [], []
    for row in p:
        k = np.floor(row.astype(np.float64) / voxel)
        o = cell[indexed] - k
        near = (np.abs(o) <= 1).all(1)
        cand = indexed[near]
        order = (9 * (o[near][:, 2] + 1) + 3 * (o[near][:, 1] + 1) + (o[near][:, 0] + 1)).astype(np.int64)
        d = row - centroid[cand]
        d2 = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(np.float32)
        if not len(cand):
            out_j.append(-1), out_d.append(np.float32(np.inf))
            continue
        pick = np.lexsort((order, d2))[0]
        out_j.append(int(cand[pick])), out_d.append(d2[pick])
    return np.array(out_j), np.array(out_d, np.float32)


def test_correspondences_against_brute_force():
    rng = np.random.default_rng(3)
    cells = np.unique(rng.integers(-4, 4, size=(260, 3)), axis=0)
    anchor = ((cells + rng.uniform(0.05, 0.95, size=cells.shape)) * VOXEL).astype(np.float32)
    centroid = (anchor + rng.uniform(-0.15, 0.15, size=anchor.shape)).astype(np.float32)     # may lie in a neighbouring cell
    normal = rng.normal(size=anchor.shape).astype(np.float32)
    normal[::17, 1] = np.nan
    anchor = np.concatenate([anchor, anchor[:20] + np.float32(0.001)])                            # duplicates
    centroid = np.concatenate([centroid, centroid[:20] + np.float32(0.05)])
    normal = np.concatenate([normal, normal[:20]])
    idx = Z.index_reference(anchor, centroid, normal, VOXEL)
    assert idx["num"][1] > 10 and idx["num"][2] >= 15
    p = rng.uniform(-1.1, 1.1, size=(700, 3)).astype(np.float32)
    lattice = (rng.integers(-5, 6, size=(300, 3)) * 0.2).astype(np.float32)                      # rows on cell faces, both sides of 0
    p = np.concatenate([p, lattice])
    j, d2 = Z.correspond(p, idx)
    bj, bd = _brute(p, anchor, centroid, normal, VOXEL)
    assert (j == bj).all() and (d2.view(np.uint32) == bd.view(np.uint32)).all() and (j >= 0).sum() > 600 and (j < 0).sum() > 5


def test_ties_go_to_the_lower_candidate_order():
    """Centroids on a lattice of 0.2 at the cells' centres; a row at a cell's corner is equidistant from eight of them."""
    axis = np.arange(-3, 3)
    cells = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), -1).reshape(-1, 3)
    anchor = ((cells + 0.5) * 0.25).astype(np.float32)                   # voxel 0.25: every value exact
    idx = Z.index_reference(anchor, anchor, np.tile(np.float32([0, 0, 1]), (len(anchor), 1)), 0.25)
    p = (np.array([[0, 0, 0], [1, -1, 1], [-2, 2, 0]]) * 0.25).astype(np.float32)
    j, d2 = Z.correspond(p, idx)
    bj, bd = _brute(p, anchor, anchor, idx["normal"], 0.25)
    assert (j == bj).all() and (d2 == np.float32(3 * 0.125 ** 2)).all()
    assert (cells[j] == np.array([[-1, -1, -1], [0, -2, 0], [-3, 1, -1]])).all()              # the lowest o_2, then o_1, then o_0


# ---- what the iteration converges to -----------------------------------------------------------------------------------------------------------
TRUTH = RR.pose_of(3.0, -2.0, 1.5, (0.05, -0.04, 0.03))


@functools.lru_cache(maxsize=None)
def _three_planes():
    normals, offsets = Z.THREE_PLANES
    idx = Z.index_reference(*Z.plane_map(5, normals, offsets), VOXEL)
    return idx, Z.plane_scan(77, normals, offsets, 1024, TRUTH)


@functools.lru_cache(maxsize=None)
def _solved(iterations):
    idx, scan = _three_planes()
    return Z.localize_scan(scan, [RR.IDENTITY], idx, RR.gate2_of(1.0), iterations, 32)


def _translation_bound():
    """3 voxel / 256 * |N^-1|_2 of the header, N the three unit normals by rows."""
    N = np.array([np.asarray(n, np.float64) / np.linalg.norm(n) for n in Z.THREE_PLANES[0]])
    return 3.0 * VOXEL / 256.0 * float(np.linalg.norm(np.linalg.inv(N), 2))


def test_converges_on_three_planes_within_the_derived_bound():
    """Noise-free rows on three mutually non-parallel planes, the map built through surfel_ref, the scan other samples of the planes
    seen from TRUTH (3 / -2 / 1.5 degrees, 5 / 4 / 3 cm off the identity seed).  The translation is held to the header's DERIVED bound,
    3 voxel / 256 |N^-1|_2 = 2.90 mm here; the restatement leaves 0.646 mm (a floor's mean bias is half a step per axis:
    sqrt(3) voxel / 512 = 0.68 mm is what to expect).  The rotation has no derived bound: the restatement leaves 7.74e-5 rad on this
    scene, measured here on the CPU, and twice that, 1.55e-4 rad, is allowed."""
    pose, fit, hessian, info, status = _solved(16)
    angle, dist = RR.pose_error(pose, TRUTH)
    print("three planes: %.3e rad, %.3e m (bound %.3e m), fit %s, info %s" % (angle, dist, _translation_bound(), fit, info))
    assert status == 0 and info == [0, 1024, 1024, 0] and fit[1] == 1.0
    assert abs(_translation_bound() - 2.903e-3) < 1e-5 and dist < _translation_bound() and angle < 1.55e-4
    assert fit[0] < (np.sqrt(3.0) * VOXEL / 256.0) ** 2                    # the mean squared residual is under the bias bound squared
    assert np.linalg.eigvalsh(Z.hessian_matrix(hessian)).min() > 1.0       # every direction constrained
    start = RR.pose_error(RR.IDENTITY, TRUTH)
    assert start[0] > 0.05 and start[1] > 0.05                             # it did move: 3.8 degrees and 7 cm


def test_three_iterations_settle_and_one_more_moves_less_than_the_bound():
    angle3, dist3 = RR.pose_error(_solved(3)[0], TRUTH)
    assert dist3 < _translation_bound() and angle3 < 1.55e-4               # (the float64 prototype of the issue settled in three too)
    moved = RR.pose_error(_solved(17)[0], _solved(16)[0])
    print("one more iteration than the default moves the pose by %.3e rad, %.3e m" % moved)
    assert moved[1] < _translation_bound() and moved[0] < 1.55e-4 and moved[1] < 1e-5


def test_single_plane_is_no_fit_or_a_visible_null_space():
    """What the definition yields, both ways.  A plane along the axes (z = -1): every normal is (0, 0, 1) to the bit, J has three
    zero columns, the FIRST pivot that meets one is not > 0: EPC_STATUS_NO_FIT with iterations >= 1; with iterations == 0 nothing is
    solved and hessian shows three exact zero eigenvalues.  A tilted plane: the surfels' normals differ in their last bits, the
    pivots stay positive, the scan is NOT flagged, and hessian shows the three unconstrained directions as eigenvalues more than 1e7
    times below the others."""
    for normals, flat in ((((0.0, 0.0, 1.0),), True), (((0.1, 0.2, 1.0),), False)):
        idx = Z.index_reference(*Z.plane_map(5, normals, (-1.0,)), VOXEL)
        scan = Z.plane_scan(77, normals, (-1.0,), 1024, RR.IDENTITY)
        seed = [RR.pose_of(0.5, 0.2, 0.1, (0.01, 0.02, 0.03))]
        pose, fit, hessian, info, status = Z.localize_scan(scan, seed, idx, RR.gate2_of(1.0), 0, 32)
        values = np.linalg.eigvalsh(Z.hessian_matrix(hessian))
        assert status == 0 and info[1] == 1024 and (pose == seed[0]).all()
        assert (values[:3] < 1e-7 * values[3]).all() and values[3] > 100.0
        pose, fit, hessian, info, status = Z.localize_scan(scan, seed, idx, RR.gate2_of(1.0), 4, 32)
        if flat:
            assert (np.abs(values[:3]) < 1e-9).all()                       # zero up to eigvalsh's own rounding
            assert status == Z.NO_FIT and info == [-1, 0, 1024, 0] and np.isnan(pose).all() and np.isnan(hessian).all()
        else:
            values = np.linalg.eigvalsh(Z.hessian_matrix(hessian))
            assert status == 0 and (values[:3] < 1e-7 * values[3]).all()


def test_flags_and_stage_a():
    idx, scan = _three_planes()
    gate2 = RR.gate2_of(1.0)
    nan_seed = RR.IDENTITY.copy()
    nan_seed[7] = np.nan
    far = RR.pose_of(t=(50.0, 0.0, 0.0))
    assert Z.localize_scan(scan, [nan_seed], idx, gate2, 4, 32)[4] == Z.NO_PAIR
    assert Z.localize_scan(scan, [far], idx, gate2, 4, 32)[4] == Z.NO_FIT
    res = Z.localize_scan(scan, [far, nan_seed, RR.IDENTITY, RR.IDENTITY], idx, gate2, 4, 32)
    assert res[4] == 0 and res[3][0] == 2                                   # the lower index of two equal seeds
    gone = scan.copy()
    gone[:] = np.nan
    assert Z.localize_scan(gone, [RR.IDENTITY], idx, gate2, 4, 32)[3:] == ([-1, 0, 0, 0], Z.NO_FIT)
    few = scan.copy()
    few[31:] = np.nan
    assert Z.localize_scan(few, [RR.IDENTITY], idx, gate2, 2, 32)[4] == Z.NO_FIT and Z.localize_scan(few, [RR.IDENTITY], idx, gate2, 2, 31)[4] == 0
