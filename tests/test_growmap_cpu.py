"""include/epcnet_growmap.h without a device: the incremental restatement (tests/growmap_ref.py: moments carried in a dict, ONLY the dirty
voxels solved again) against ``surfel_ref.reference`` on the concatenation of the calls -- bit for bit, which is the proof that the dirty
rule is sufficient --, the header's row and binding, and the entries' refusals, which launch nothing."""
import ctypes
import os

import numpy as np
import pytest

import growmap_ref as G
import helpers as H
import map_ref as M
import surfel_ref as S


def _scene(rows=420):
    """Six clouds along a drive of 2 m per cloud, 3 m wide, at voxel 0.5: later clouds reach new ground and leave the first clouds'
    alone, at ring 2 (1 m) too."""
    sixth = rows // 6
    return M.drive(3, (sixth,) * 5 + (rows - 5 * sixth,), extent=1.5)


def _cuts(rows, parts):
    return [rows * i // parts for i in range(1, parts)]


def _agree(calls, origin, voxel, max_voxels, min_count, ring, min_support, what):
    m, reports, outs = G.run(calls, origin, voxel, max_voxels, min_count, ring, min_support)
    kept = []
    for call, report, out in zip(calls, reports, outs):
        if M.valid(call[1], len(call[0])):                                   # a call with invalid offsets adds nothing
            kept.append(call)
        want = S.reference(*G.concatenation(kept), origin, voxel, max_voxels, min_count, ring, min_support)
        assert G.same_bits(out, want) is None, (what, "after call %d" % len(kept), G.same_bits(out, want))
    return m, reports, outs


@pytest.mark.parametrize("min_count", [1, 2])
@pytest.mark.parametrize("ring", [0, 1, 2])
@pytest.mark.parametrize("parts", [1, 2, 5, 0])
def test_incremental_equals_the_reference_on_the_concatenation(parts, ring, min_count):
    """A scene split into 1, 2, 5 and (parts 0) one-row-per-call pieces: after EVERY call the seven outputs equal the reference on the
    rows so far, although only the dirty voxels were solved again."""
    rows = 420 if parts else 150
    points, offsets, poses, origin = _scene(rows)
    cuts = _cuts(rows, parts) if parts else list(range(1, rows))
    calls = G.pieces(points, offsets, poses, cuts)
    assert len(calls) == (parts or rows)
    m, reports, outs = _agree(calls, origin, 0.5, rows, min_count, ring, 3, "%d parts, ring %d, min_count %d" % (parts, ring, min_count))
    whole = S.reference(points, offsets, poses, origin, 0.5, rows, min_count, ring, 3)
    assert G.same_bits(outs[-1], whole) is None                              # the pieces' poses repeat: the same rows, the same map
    assert sum(int(r["num_call"][0]) for r in reports) == whole["V"] and sum(int(r["num_call"][1]) for r in reports) == rows
    if ring > 0 and min_count == 1:
        assert whole["valid"].sum() > 20
    for i, r in enumerate(reports):
        assert r["num_call"][2] == len(r["dirty"]) and set(r["touched"]) <= set(r["dirty"])
        assert len(r["dirty"]) + len(r["clean"]) == outs[i]["num_out"][0]
        if i > 0 and parts in (2, 5):                                        # never vacuous: some voxels are solved again, some are left
            assert len(r["clean"]) > 0, (i, "no clean voxel")
            if ring > 0:
                assert len(set(r["dirty"]) - set(r["touched"])) > 0, (i, "no dirty voxel that received no row")
            else:
                assert set(r["dirty"]) == set(r["touched"])
            assert len(r["dirty"]) < outs[i]["num_out"][0]


def test_clean_rows_are_kept_not_recomputed():
    """The restatement solves the dirty voxels only: a sentinel written into the clean rows before a call is still there behind it, and
    the dirty rows are the reference's."""
    points, offsets, poses, origin = _scene()
    calls = G.pieces(points, offsets, poses, _cuts(420, 3))
    m = G.Map(origin, 0.5, 420, 1, 1, 3)
    m.add(*calls[0])
    probe = G.Map(origin, 0.5, 420, 1, 1, 3)
    probe.add(*calls[0])
    clean = probe.add(*calls[1])["clean"]
    assert len(clean) > 10
    for name in G.FLOATS:
        m.out[name].view(np.uint32)[clean] = 0x12345678
    m.out["support"][clean] = -77
    report = m.add(*calls[1])
    want = S.reference(*G.concatenation(calls[:2]), origin, 0.5, 420, 1, 1, 3)
    assert (report["clean"] == clean).all()
    for name in G.FLOATS:
        assert (m.out[name].view(np.uint32)[clean] == 0x12345678).all()
        assert (m.out[name].view(np.uint32)[report["dirty"]] == want[name].view(np.uint32)[report["dirty"]]).all()
    assert (m.out["support"][clean] == -77).all() and (m.out["support"][report["dirty"]] == want["support"][report["dirty"]]).all()


def test_a_neighbour_crossing_min_count_changes_an_unmoved_voxel():
    """min_count 2: voxel A holds four rows, its neighbour B one -- B is in no pool.  The second call adds ONE row to B: B crosses
    min_count, and A, which received nothing, is dirty: its support, centroid and eigenvalues change."""
    a = np.array([[0.1, 0.1, 0.1], [0.3, 0.2, 0.1], [0.2, 0.4, 0.3], [0.4, 0.3, 0.2]], np.float32)
    b1, b2 = np.array([[0.7, 0.2, 0.2]], np.float32), np.array([[0.8, 0.4, 0.1]], np.float32)
    far = np.array([[5.2, 5.2, 5.2], [5.3, 5.1, 5.4], [5.1, 5.3, 5.2]], np.float32)              # a voxel that stays clean
    poses = M.identity_poses(1)
    calls = [(np.concatenate([a, b1, far]), np.array([0, 8], np.int32), poses), (b2, np.array([0, 1], np.int32), poses)]
    m, reports, outs = _agree(calls, np.zeros(3), 0.5, 8, 2, 1, 3, "crossing min_count")
    assert reports[0]["num_call"].tolist() == [3, 8, 3, 0] and reports[1]["num_call"].tolist() == [0, 1, 2, 0]
    assert reports[1]["touched"].tolist() == [1] and reports[1]["dirty"].tolist() == [0, 1] and reports[1]["clean"].tolist() == [2]
    assert outs[0]["support"][:3].tolist() == [4, 4, 3] and outs[1]["support"][:3].tolist() == [6, 6, 3]
    assert outs[0]["count"][:3].tolist() == [4, 1, 3] and outs[1]["count"][:3].tolist() == [4, 2, 3]
    for name in ("centroid", "eigen"):
        assert (outs[0][name][0].view(np.uint32) != outs[1][name][0].view(np.uint32)).any(), name
    assert np.isnan(outs[0]["centroid"][1]).all() and np.isfinite(outs[1]["centroid"][1]).all()


def test_overflow_is_sticky_and_invalid_offsets_add_nothing():
    points, offsets, poses, origin = _scene()
    calls = G.pieces(points, offsets, poses, _cuts(420, 4))
    V = [S.reference(*G.concatenation(calls[:k]), origin, 0.5, 420, 1, 1, 3)["V"] for k in (1, 2, 3, 4)]
    assert V[0] < V[1] < V[2] < V[3]
    m, reports, outs = _agree(calls, origin, 0.5, V[2], 1, 1, 3, "overflow in the last call")
    assert [int(r["num_call"][0]) for r in reports] == [V[0], V[1] - V[0], V[2] - V[1], -1] and outs[3]["num_out"].tolist() == [-1, 420, 0, 0]
    assert (outs[3]["normal"].view(np.uint32) == M.NAN_WORD).all() and not outs[3]["support"].any()
    m, reports, outs = _agree(calls, origin, 0.5, V[1], 1, 1, 3, "overflow in the third call, one more behind it")
    assert outs[2]["num_out"].tolist() == [-1, 315, 0, 0] and outs[3]["num_out"].tolist() == [-1, 420, 0, 0]
    assert reports[3]["num_call"].tolist() == [-1, 105, 0, 0]
    bad = (calls[1][0], np.array([0, 60, 50, 105], np.int32), calls[1][2])
    m, reports, outs = G.run([calls[0], bad, calls[1]], origin, 0.5, 420, 1, 1, 3)
    assert reports[1]["num_call"].tolist() == [-1, 0, 0, 0] and G.same_bits(outs[1], outs[0]) is None
    assert G.same_bits(outs[2], S.reference(*G.concatenation(calls[:2]), origin, 0.5, 420, 1, 1, 3)) is None


# ---- the header -------------------------------------------------------------------------------------------------------------------------------
def test_thirteenth_header_is_bound_like_the_others():
    L = H.pkg("lib")
    path = os.path.join(H.ROOT, "include", "epcnet_growmap.h")
    text = open(path).read()
    assert L.GROWMAP_HEADER_PATH == path
    stems = [row[0] for row in L._HEADERS]
    assert ("growmap", "GROWMAP", False, False) in L._HEADERS
    at = stems.index("growmap")                        # other tests pin maps, surfels, localize, forms as consecutive rows
    assert at < stems.index("maps") or at > stems.index("forms")
    functions, constants, status = L.parse_header(text, need_status=False)     # no `double` by value: the plain scalars read it
    assert list(functions) == L.GROWMAP_EXPORTS == ["epcnet_surfel_map_state_bytes", "epcnet_surfel_map_init",
                                                    "epcnet_surfel_map_add_workspace_bytes", "epcnet_surfel_map_add"]
    assert status == {} and constants == {"EPC_GROWMAP_HEAD_BYTES": 256} and L.EPC_GROWMAP_HEAD_BYTES == 256
    for stem, prefix, _, _ in L._HEADERS:
        if stem != "growmap":
            assert not set(L.GROWMAP_EXPORTS) & set(getattr(L, prefix + "_EXPORTS")), stem
    assert not set(L.GROWMAP_EXPORTS) & set(L.EXPORTS) and not set(L.GROWMAP_EXPORTS) & set(L.LAUNCHING)
    assert L.SURFEL_EXPORTS == ["epcnet_map_surfels_workspace_bytes", "epcnet_map_surfels"]
    assert "_kernel" not in text and "growmap_" not in text.replace("epcnet_growmap", "").replace("tests/growmap_ref", "").replace("csrc/growmap.hip", "")
    i, ll, z, P = ctypes.c_int, ctypes.c_longlong, ctypes.c_size_t, ctypes.c_void_p
    want = {"epcnet_surfel_map_state_bytes": (z, [ll]),
            "epcnet_surfel_map_init": (i, [P, P, ll, P, z, P, P, P, P, P, P, P, P]),
            "epcnet_surfel_map_add_workspace_bytes": (z, [ll, i, i]),
            "epcnet_surfel_map_add": (i, [P, P, ll, i, P, P, ll, P, z, P, P, P, P, P, P, P, P, P, z, P])}
    for name, (restype, argtypes) in want.items():
        fn = getattr(L.lib(), name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert functions["epcnet_surfel_map_add"][2] == ["points", "offsets", "num_rows", "num_clouds", "poses", "params", "max_voxels", "state",
                                                     "state_bytes", "map_points", "count", "centroid", "normal", "eigen", "support", "num_out",
                                                     "num_call", "workspace", "workspace_bytes", "stream"]
    assert functions["epcnet_surfel_map_init"][2] == ["origin", "params", "max_voxels", "state", "state_bytes", "map_points", "count", "centroid",
                                                      "normal", "eigen", "support", "num_out", "stream"]
    ret, types, names = functions["epcnet_surfel_map_add"]
    for n, t in (("points", "float*"), ("poses", "double*"), ("params", "double*"), ("offsets", "int32_t*"), ("num_out", "int32_t*"),
                 ("num_call", "int32_t*"), ("support", "int32_t*"), ("eigen", "float*"), ("state", "void*"), ("workspace", "void*")):
        assert types[names.index(n)] == t, n
    on_run = [n for n in L.GROWMAP_EXPORTS if hasattr(L.run, n)]
    assert on_run == ["epcnet_surfel_map_init", "epcnet_surfel_map_add"]       # exactly the two launching entries
    ops = H.pkg("ops")
    assert ops.SurfelMap is H.pkg("growmap").SurfelMap


def test_size_queries_and_refusals_launch_nothing():
    """EPC_EINVAL / EPC_ENOMEM from addresses that are never followed: nothing is launched, so no device is needed."""
    L = H.pkg("lib")
    lib = L.lib()
    state, need = lib.epcnet_surfel_map_state_bytes, lib.epcnet_surfel_map_add_workspace_bytes
    surfels = lib.epcnet_map_surfels_workspace_bytes
    assert [state(v) for v in (0, -1, (1 << 28) + 1)] == [0, 0, 0]
    for v in (1, 2, 1000, 1023, 1025, 1 << 20):          # a head and the one-shot entry's table: the power of two >= 2 v + 1, 128-byte slots
        cap = (state(v) - 256) // 128
        assert state(v) == 256 + cap * 128 and cap & (cap - 1) == 0 and 2 * v + 1 <= cap < 2 * (2 * v + 1)
        assert state(v) - 256 == surfels(0, 0, v) - 128
    assert state(1 << 28) == 256 + (1 << 30) * 128
    for bad in ((-1, 1, 1), (1 << 31, 1, 1), (10, -1, 1), (10, (1 << 24) + 1, 1), (10, 1, -1), (10, 1, 3)):
        assert need(*bad) == 0
    assert need(0, 0, 0) == 128 and need(0, 0, 2) == 128 and need(1000, 3, 1) % 16 == 0
    assert need(1000, 3, 1) == need(1000, 999, 1) == 128 + 4000 + 16 + 16 + 4000 * 27          # sized from the call alone
    assert need(1000, 3, 0) == 128 + 4000 + 16 + 16 + 4000 and need(1000, 3, 2) == 128 + 4000 + 16 + 16 + 4000 * 125
    assert need((1 << 31) - 1, 1 << 24, 2) > 4 * 126 * ((1 << 31) - 1)                                # (no 32-bit product on the way)
    a = 0x10000

    def init(origin=a, voxel=0.2, min_count=1.0, ring=1.0, min_support=8.0, reserved=(0.0,) * 4, params=True, voxels=1000, st=a, st_bytes=None,
             out=a, count=a, centroid=a, normal=a, eigen=a, support=a, num=a):
        p = (ctypes.c_double * 8)(voxel, min_count, ring, min_support, *reserved) if params else None
        return lib.epcnet_surfel_map_init(origin, p, voxels, st, state(1000) if st_bytes is None else st_bytes, out, count, centroid, normal,
                                          eigen, support, num, None)

    def add(rows=1000, clouds=4, points=a, offsets=a, poses=a, voxel=0.2, min_count=1.0, ring=1.0, min_support=8.0, reserved=(0.0,) * 4,
            params=True, voxels=1000, st=a, st_bytes=None, out=a, count=a, centroid=a, normal=a, eigen=a, support=a, num=a, call=a, ws=a,
            ws_bytes=None):
        p = (ctypes.c_double * 8)(voxel, min_count, ring, min_support, *reserved) if params else None
        return lib.epcnet_surfel_map_add(points, offsets, rows, clouds, poses, p, voxels, st, state(1000) if st_bytes is None else st_bytes,
                                         out, count, centroid, normal, eigen, support, num, call, ws, need(1000, 4, 1) if ws_bytes is None else ws_bytes,
                                         None)

    nan, inf = float("nan"), float("inf")
    shared = [dict(voxels=0), dict(voxels=(1 << 28) + 1), dict(voxel=0.0), dict(voxel=-0.2), dict(voxel=nan), dict(voxel=inf),
              dict(voxel=2.0 ** -21), dict(voxel=2.0 ** 20 + 1.0), dict(min_count=0.0), dict(min_count=1.5), dict(min_count=nan),
              dict(min_count=2.0 ** 31), dict(ring=-1.0), dict(ring=3.0), dict(ring=0.5), dict(ring=nan), dict(min_support=2.0),
              dict(min_support=2.0 ** 31), dict(min_support=8.5), dict(min_support=nan), dict(params=False), dict(st=None), dict(st=a + 8),
              dict(out=None), dict(count=None), dict(centroid=None), dict(normal=None), dict(eigen=None), dict(support=None), dict(num=None)]
    shared += [dict(reserved=tuple(1.0 if i == k else 0.0 for i in range(4))) for k in range(4)] + [dict(reserved=(0.0, nan, 0.0, 0.0))]
    for kw in shared + [dict(origin=None)]:
        assert init(**kw) == L.EPC_EINVAL, kw
        assert b"epcnet_surfel_map_init" in lib.epc_last_error()
    assert init(st_bytes=state(1000) - 1) == L.EPC_ENOMEM and init(st_bytes=0) == L.EPC_ENOMEM and init(voxels=1025) == L.EPC_ENOMEM
    own = [dict(rows=-1), dict(rows=1 << 31), dict(clouds=-1), dict(clouds=(1 << 24) + 1), dict(points=None), dict(offsets=None),
           dict(poses=None), dict(call=None), dict(ws=None), dict(ws=a + 8)]
    for kw in shared + own:
        assert add(**kw) == L.EPC_EINVAL, kw
        assert b"epcnet_surfel_map_add" in lib.epc_last_error()
    assert add(st_bytes=state(1000) - 1) == L.EPC_ENOMEM and add(voxels=1025) == L.EPC_ENOMEM          # a state sized for a smaller table
    assert add(ws_bytes=need(1000, 4, 1) - 1) == L.EPC_ENOMEM and add(ws_bytes=0) == L.EPC_ENOMEM
    assert add(ring=2.0) == L.EPC_ENOMEM and add(rows=1001) == L.EPC_ENOMEM                            # a workspace sized for a smaller call
