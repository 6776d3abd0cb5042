"""epcnet_surfel_index and epcnet_scan_localize on the device against their numpy restatement (tests/localize_ref.py): the index, every
output and the workspace are poisoned buffers of exactly the size asked for with slack behind them, and everything is compared on BIT
PATTERNS -- float32 distances in one candidate order, float64 sums in one order, a fixed sequence of float64 operations behind them, so
there is no tolerance anywhere.

What a contracted multiply-add would do: test_a_contracted_multiply_add_would_show re-counts with exact fractions how many rows' e or
r x n change when the header's rounded products are fused, before it runs the device."""
import ctypes
import functools
from fractions import Fraction as F

import numpy as np
import pytest
import torch

import helpers as H
import localize_ref as Z
import register_ref as RR
import stage_ref as SG

pytestmark = pytest.mark.gpu

VOXEL = 0.2
LZ_TILE = 256            # LZ_THREADS of csrc/localize.hip: the surfels of one insert / fill workgroup, the rows of one chunk
NAMES = ("pose", "fit", "hessian", "info", "status")


def _up(a, dtype, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev)


def _index_raw(anchor, centroid, normal, voxel=VOXEL):
    """The index entry on a poisoned buffer of exactly the size asked for -> (the buffer, num as a list, the device arrays)."""
    L = H.pkg("lib")
    dev = torch.device("cuda")
    M = len(anchor)
    need = L.lib().epcnet_surfel_index_bytes(M)
    assert need > 0
    index, num = SG.Poisoned((need,), torch.uint8, dev), SG.Poisoned((4,), torch.int32, dev)
    arrays = [_up(a, np.float32, dev) for a in (anchor, centroid, normal)]
    params = (ctypes.c_double * 4)(voxel)
    L.run.epcnet_surfel_index(arrays[0], arrays[1], arrays[2], M, params, index.t, need, num.t)
    torch.cuda.synchronize()
    assert index.untouched() and num.untouched() and not SG.holds_poison(index.t[:128])
    return index, num.t.tolist(), arrays


def _localize_raw(scans, seeds, index, arrays, voxel=VOXEL, max_dist=1.0, iterations=16, min_pairs=32):
    """The entry itself on poisoned outputs and a workspace of exactly the size asked for -> the outputs as host arrays after the checks
    that nothing was written behind any of them."""
    L = H.pkg("lib")
    dev = torch.device("cuda")
    scans = np.asarray(scans, np.float32)
    Q, n = scans.shape[:2]
    Hs = 1 if seeds is None else np.asarray(seeds).shape[1]
    M = int(arrays[1].shape[0])
    need = L.lib().epcnet_scan_localize_workspace_bytes(Q, Hs, n)
    assert need > 0
    out = dict(pose=SG.Poisoned((Q, 12), torch.float64, dev), fit=SG.Poisoned((Q, 2), torch.float64, dev),
               hessian=SG.Poisoned((Q, 21), torch.float64, dev), info=SG.Poisoned((Q, 4), torch.int32, dev),
               status=SG.Poisoned((Q,), torch.int32, dev))
    ws = SG.Poisoned((need,), torch.uint8, dev)
    params = (ctypes.c_double * 8)(voxel, max_dist, float(iterations), float(min_pairs))
    L.run.epcnet_scan_localize(_up(scans, np.float32, dev), Q, n, None if seeds is None else _up(seeds, np.float64, dev), Hs, index.t,
                               index.nbytes, arrays[1], arrays[2], M, params, out["pose"].t, out["fit"].t, out["hessian"].t, out["info"].t,
                               out["status"].t, ws.t, need)
    torch.cuda.synchronize()
    for p in list(out.values()) + [ws, index]:
        assert p.untouched()
    return {name: p.t.cpu().numpy() for name, p in out.items()}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _check(got, want, what):
    for name, w in zip(NAMES, want):
        g = got[name]
        w = np.asarray(w, g.dtype).reshape(g.shape)
        if g.dtype == np.float64:                     # a NaN the device writes is 0x7ff8000000000000, numpy's nan too
            assert (np.isnan(g) == np.isnan(w)).all(), (what, name)
            assert (_bits(g)[np.isnan(g)] == 0x7ff8000000000000).all(), (what, name, "another NaN")
            differ = (_bits(g) != _bits(w)) & ~np.isnan(g)
        else:
            differ = g != w
        assert not differ.any(), (what, name, "%d words differ, the first in row %d: %r against %r" % (
            differ.sum(), int(np.nonzero(differ.reshape(len(g), -1).any(1))[0][0]), g[differ][:3], w[differ][:3]))


def _both(scans, seeds, maps, what, **kw):
    """maps: (anchor, centroid, normal).  Index and localisation on the device against the restatement -> (got, want, ref index)."""
    ref = Z.index_reference(*maps, kw.get("voxel", VOXEL))
    index, num, arrays = _index_raw(*maps, kw.get("voxel", VOXEL))
    assert num == ref["num"], (what, num, ref["num"])
    want = Z.localize_reference(scans, seeds, ref, kw.get("max_dist", 1.0), kw.get("iterations", 16), kw.get("min_pairs", 32))
    got = _localize_raw(scans, seeds, index, arrays, **kw)
    _check(got, want, what)
    return got, want, ref


@functools.lru_cache(maxsize=None)
def _planes():
    return Z.plane_map(5, *Z.THREE_PLANES)


def _truths(Q):
    return [RR.pose_of(3.0 - 2 * q, -2.0 + q, 1.5, (0.05 - 0.03 * q, -0.04, 0.03 + 0.02 * q)) for q in range(Q)]


def _scans(n, Q, seed=77):
    return np.stack([Z.plane_scan(seed + q, *Z.THREE_PLANES, n, t) for q, t in enumerate(_truths(Q))])


def _seeds(Q, Hs):
    """Seed 0 far off (it accepts nothing), the others near the identity: stage A has something to choose."""
    hyp = [RR.pose_of(t=(40.0, 0.0, 0.0)), RR.IDENTITY, RR.pose_of(1.0, 0.0, 0.5, (0.01, 0.0, -0.01))]
    return np.stack([np.stack([hyp[(h + q) % 3] if Hs > 1 else RR.IDENTITY for h in range(Hs)]) for q in range(Q)])


@pytest.mark.parametrize("n,Q,Hs", [(32, 1, 1), (64, 3, 1), (96, 1, 3), (256, 3, 3), (288, 1, 1), (288, 3, 3), (4096, 1, 3), (4096, 3, 1)])
def test_shapes_where_the_kernels_change_form(n, Q, Hs):
    """Below a wave, one wave, a wave and a half, one chunk, a chunk and a part, sixteen chunks; one scan and several, one seed and
    several (NULL seeds where H == 1 and Q == 1)."""
    seeds = None if (Hs == 1 and Q == 1) else _seeds(Q, Hs)
    iterations = 16 if n <= 288 else 4
    got, want, _ = _both(_scans(n, Q), seeds, _planes(), "n %d, Q %d, H %d" % (n, Q, Hs), iterations=iterations, min_pairs=min(32, n))
    assert (got["status"] == 0).all() and (got["info"][:, 1] == n).all()
    if Hs == 3:
        assert all((got["info"][q, 0] + q) % 3 != 0 for q in range(Q))     # never the seed that is 40 m off
    for q, truth in enumerate(_truths(Q)):
        angle, dist = RR.pose_error(got["pose"][q], truth)
        assert dist < 0.01 and angle < 0.005


@pytest.mark.parametrize("M", [1, 2, LZ_TILE - 1, LZ_TILE, LZ_TILE + 1])
def test_map_sizes_around_one_and_the_tile(M):
    anchor, centroid, normal = (a[:M] for a in _planes())
    scans = np.stack([centroid[:M][np.arange(64) % M] + np.float32(0.01) * np.arange(64, dtype=np.float32)[:, None] / 64])
    for iterations in (0, 2):
        got, want, ref = _both(scans, None, (anchor, centroid, normal), "M %d, %d iterations" % (M, iterations), iterations=iterations,
                               min_pairs=6)
        assert ref["num"][0] == M and (iterations or got["info"][0].tolist() == [0, 64, 64, 0])


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_cells_at_strides_of_powers_of_two_and_duplicates(axis):
    """Cells at multiples of 2^s along one axis (long probe runs under a weak hash), every surfel twice: the second is a duplicate."""
    rng = np.random.default_rng(axis)
    cells = np.zeros((21 * 24, 3), np.int64)
    cells[:, axis] = (np.arange(24)[None, :] * (1 << np.arange(21))[:, None]).reshape(-1) % (1 << 20) - (1 << 19)
    cells[:, (axis + 1) % 3] = np.repeat(np.arange(21), 24) % 2
    cells = np.unique(cells, axis=0)
    rng.shuffle(cells)
    anchor = ((cells + rng.uniform(0.2, 0.8, size=cells.shape)) * 1.0).astype(np.float32)
    normal = rng.normal(size=cells.shape)
    normal = (normal / np.linalg.norm(normal, axis=1, keepdims=True)).astype(np.float32)
    both = lambda a: np.concatenate([a, a[::-1]])
    maps = (both(anchor), both(anchor), np.concatenate([normal, -normal[::-1]]))
    rows = anchor[np.arange(96) * 3] + rng.uniform(-0.3, 0.3, size=(96, 3)).astype(np.float32)      # (float32 keeps 0.03 m at 2^19 m)
    got, want, ref = _both(rows[None], None, maps, "strides along axis %d" % axis, voxel=1.0, iterations=0, min_pairs=6)
    assert ref["num"] == [len(cells), 0, len(cells), 0] and (ref["j"] < len(cells)).all() and got["info"][0].tolist() == [0, 96, 96, 0]
    _both(rows[None], None, maps, "strides along axis %d, two iterations" % axis, voxel=1.0, iterations=2, min_pairs=6)


def test_absent_rows_scans_seeds_and_maps():
    maps = _planes()
    scans = _scans(288, 3)
    scans[0, ::7, 1] = np.nan
    scans[0, 5, 0] = np.inf
    scans[1] = np.nan                                                      # an all-absent scan
    seeds = _seeds(3, 3)
    seeds[0, 2, 4] = np.nan                                                # one seed with a NaN word
    seeds[2] = np.nan                                                      # all seeds NaN
    seeds[2, :, 0] = 1.0
    got, want, _ = _both(scans, seeds, maps, "absent rows, scans and seeds", iterations=3)
    assert got["status"].tolist() == [0, Z.NO_FIT, Z.NO_PAIR] and got["info"][:, 2].tolist() == [288 - 43, 0, 288]
    assert got["info"][0, 0] in (0, 1) and got["info"][1:, 0].tolist() == [-1, -1] and np.isnan(got["hessian"][1:]).all()
    gone = tuple(np.full_like(a, np.nan) if i == 2 else a for i, a in enumerate(maps))              # an all-NaN map: nothing is indexed
    got, want, ref = _both(scans, seeds, gone, "an all-NaN map", iterations=3)
    assert ref["num"] == [0, len(maps[0]), 0, 0] and got["status"].tolist() == [Z.NO_FIT, Z.NO_FIT, Z.NO_PAIR]
    part = tuple(a.copy() for a in maps)
    part[2][::3, 0] = np.nan                                               # the caller's planarity filter
    got, want, ref = _both(scans, seeds, part, "a filtered map", iterations=3)
    assert ref["num"][1] == len(range(0, len(maps[0]), 3)) and got["status"][0] == 0


def test_rows_on_cell_faces_range_edges_and_ties():
    """Voxel 0.25, every value exact.  Centroids on the lattice of cell centres: a row on a cell's corner is equidistant from eight of
    them.  Rows exactly on faces on both sides of the origin.  Surfels in the first and the last cell of the range on every axis, rows
    beside them whose neighbour cells lie outside: skipped, never wrapped onto the other edge (which holds surfels here)."""
    axis = np.arange(-3, 3)
    cells = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), -1).reshape(-1, 3)
    top = 1 << 20
    edge = []
    for a in range(3):
        for c in (-top, top - 1):
            e = np.zeros(3, np.int64)
            e[a] = c
            edge.append(e)
    cells = np.concatenate([cells, np.array(edge)])
    anchor = ((cells + 0.5) * 0.25).astype(np.float32)
    assert (anchor.astype(np.float64) == (cells + 0.5) * 0.25).all()
    rng = np.random.default_rng(2)
    normal = rng.normal(size=anchor.shape)
    normal = (normal / np.linalg.norm(normal, axis=1, keepdims=True)).astype(np.float32)
    rows = [np.array(v) * 0.25 for v in ([0, 0, 0], [1, -1, 1], [-2, 2, 0], [-1, -1, -1], [0.5, 0, 0], [-0.5, 0, 0], [0, -2, 0.25])]
    for a in range(3):
        for c, d in ((-top, 0.0), (-top, 0.5), (top - 1, 0.5), (top - 1, 0.99), (top, 0.0), (-top - 1, 0.5)):
            r = np.full(3, 0.125)
            r[a] = (c + d) * 0.25
            rows.append(r)
    rows = np.array(rows + [rows[i % 7] + 0.01 * i for i in range(64 - len(rows))], np.float32)
    maps = (anchor, anchor, normal)
    for iterations in (0, 1):
        got, want, ref = _both(rows[None], None, maps, "faces, edges, ties", voxel=0.25, max_dist=0.3, iterations=iterations, min_pairs=6)
        assert ref["num"] == [len(cells), 0, 0, 0] and got["status"][0] == 0
    j, d2 = Z.correspond(rows, ref)
    assert (cells[j[:3]] == np.array([[-1, -1, -1], [0, -2, 0], [-3, 1, -1]])).all() and (d2[:4] == np.float32(3 * 0.125 ** 2)).all()
    edges = j[7:7 + 18].reshape(3, 6)
    assert (edges[:, :4] >= 216).all() and (edges[:, 4] >= 216).all() and (edges[:, 5] >= 216).all()     # each finds ITS edge's surfel
    assert (np.abs(cells[edges[:, 0]]).max(1) == top).all() and (cells[edges[:, 4]].max(1) == top - 1).all()


def test_iterations_zero_min_pairs_and_the_single_plane():
    maps = _planes()
    scans = _scans(256, 3)
    seeds = _seeds(3, 3)
    got, want, _ = _both(scans, seeds, maps, "iterations 0", iterations=0)
    for q in range(3):
        assert (got["pose"][q] == seeds[q, got["info"][q, 0]]).all()       # the best seed's own words
    scans[1, 40:] = np.nan
    got, want, _ = _both(scans, seeds, maps, "min_pairs not met", iterations=2, min_pairs=41)
    assert got["status"].tolist() == [0, Z.NO_FIT, 0] and got["info"][1].tolist() == [-1, 0, 40, 0]
    got, want, _ = _both(scans, seeds, maps, "min_pairs met", iterations=2, min_pairs=40)
    assert got["status"].tolist() == [0, 0, 0]
    for normals, flagged in ((((0.0, 0.0, 1.0),), True), (((0.1, 0.2, 1.0),), False)):
        plane = Z.plane_map(5, normals, (-1.0,))
        scan = Z.plane_scan(77, normals, (-1.0,), 256, RR.IDENTITY)[None]
        seed = RR.pose_of(0.5, 0.2, 0.1, (0.01, 0.02, 0.03))[None, None]
        got, want, _ = _both(scan, seed, plane, "a single plane", iterations=4)
        assert (got["status"][0] == Z.NO_FIT) == flagged
        got, want, _ = _both(scan, seed, plane, "a single plane, nothing solved", iterations=0)
        values = np.linalg.eigvalsh(Z.hessian_matrix(got["hessian"][0]))
        assert got["status"][0] == 0 and (values[:3] < 1e-7 * values[3]).all()


def _fused(a, b, c):
    """fma(a, b, c): one rounding of the exact a * b + c."""
    return float(F(float(a)) * F(float(b)) + F(float(c)))


def test_a_contracted_multiply_add_would_show():
    """J_0 = r_1 n_2 - r_2 n_1 (and J_1, J_2) as a compiler that contracts would form them -- fma(r_1, n_2, -fl(r_2 n_1)) -- against the
    header's, counted over the accepted rows of the first pass with exact fractions; under a seed that rotates, so that r carries a
    full float64 significand.  e = (n_0 d_0 + n_1 d_1) + n_2 d_2 is counted too and does NOT change: n is a float32 and d = p - c the
    exact difference of two nearby float32 words, so every product is exact in float64 and a fused form rounds the same sum."""
    maps = _planes()
    ref = Z.index_reference(*maps, VOXEL)
    scan = _scans(256, 1)[0]
    seed = RR.pose_of(1.0, 0.0, 0.5, (0.01, 0.0, -0.01))
    sums, rows, j, e, J, r, p = Z.pass_sums(seed, scan, ref, RR.gate2_of(1.0), detail=True)
    c, nrm, q = ref["centroid"][j].astype(np.float64), ref["normal"][j].astype(np.float64), p.astype(np.float64)
    d = q - c
    changed_e = changed_j = 0
    for i in range(len(rows)):
        fe = _fused(nrm[i, 2], d[i, 2], _fused(nrm[i, 0], d[i, 0], nrm[i, 1] * d[i, 1]))
        fj = [_fused(r[i, (a + 1) % 3], nrm[i, (a + 2) % 3], -(r[i, (a + 2) % 3] * nrm[i, (a + 1) % 3])) for a in range(3)]
        changed_e += fe != e[i]
        changed_j += fj != J[i, :3].tolist()
    print("%d accepted rows: a contracted multiply-add changes e in %d and r x n in %d" % (len(rows), changed_e, changed_j))
    assert len(rows) == 256 and changed_j > 64 and changed_e == 0
    _both(scan[None], seed[None, None], maps, "the scene of the contraction count", iterations=2)


def test_two_runs_are_bit_identical():
    maps = _planes()
    scans, seeds = _scans(288, 3), _seeds(3, 3)
    first, _, _ = _both(scans, seeds, maps, "first run", iterations=5)
    again, _, _ = _both(scans, seeds, maps, "second run", iterations=5)
    for name in NAMES:
        assert (_bits(first[name]) == _bits(again[name])).all(), name


def _refused(L, status, call):
    with pytest.raises(L.EpcNetError) as e:
        call()
    assert e.value.status == status, (e.value.status, str(e.value))


def test_every_refusal_leaves_the_buffers_untouched():
    L = H.pkg("lib")
    dev = torch.device("cuda")
    maps = _planes()
    M = len(maps[0])
    arrays = [_up(a, np.float32, dev) for a in maps]
    need = L.lib().epcnet_surfel_index_bytes(M)
    index, num = SG.Poisoned((need,), torch.uint8, dev), SG.Poisoned((4,), torch.int32, dev)

    def build(anchor=arrays[0], centroid=arrays[1], normal=arrays[2], M=M, params=(VOXEL,), index=index.t, size=need, num=num.t):
        L.run.epcnet_surfel_index(anchor, centroid, normal, M, (ctypes.c_double * 4)(*params), index, size, num)

    for change in (dict(anchor=None), dict(centroid=None), dict(normal=None), dict(index=None), dict(num=None), dict(M=0), dict(M=2 ** 28 + 1),
                   dict(params=(0.0,)), dict(params=(float("nan"),)), dict(params=(2.0 ** 21,)), dict(params=(2.0 ** -21,)),
                   dict(params=(VOXEL, 1.0)), dict(params=(VOXEL, 0.0, 0.0, 1.0)), dict(index=index.buf[8:])):
        _refused(L, L.EPC_EINVAL, lambda: build(**change))
    _refused(L, L.EPC_ENOMEM, lambda: build(size=need - 1))
    torch.cuda.synchronize()
    assert SG.holds_poison(index.t) and SG.holds_poison(num.t)
    build()

    Q, n, Hs = 2, 64, 2
    scans, seeds = _up(_scans(n, Q), np.float32, dev), _up(_seeds(Q, Hs), np.float64, dev)
    ws_need = L.lib().epcnet_scan_localize_workspace_bytes(Q, Hs, n)
    out = [SG.Poisoned(s, t, dev) for s, t in (((Q, 12), torch.float64), ((Q, 2), torch.float64), ((Q, 21), torch.float64),
                                                ((Q, 4), torch.int32), ((Q,), torch.int32))]
    ws = SG.Poisoned((ws_need,), torch.uint8, dev)
    base = dict(scans=scans, Q=Q, n=n, seeds=seeds, H=Hs, index=index.t, index_bytes=need, centroid=arrays[1], normal=arrays[2], M=M,
                params=(VOXEL, 1.0, 4.0, 32.0), pose=out[0].t, fit=out[1].t, hessian=out[2].t, info=out[3].t, status=out[4].t, ws=ws.t,
                ws_bytes=ws_need)

    def run(**change):
        a = dict(base, **change)
        L.run.epcnet_scan_localize(a["scans"], a["Q"], a["n"], a["seeds"], a["H"], a["index"], a["index_bytes"], a["centroid"], a["normal"],
                                   a["M"], (ctypes.c_double * 8)(*a["params"]), a["pose"], a["fit"], a["hessian"], a["info"], a["status"],
                                   a["ws"], a["ws_bytes"])

    changes = [dict(((name, None),)) for name in ("scans", "index", "centroid", "normal", "pose", "fit", "hessian", "info", "status", "ws")]
    changes += [dict(n=48), dict(n=0), dict(n=4128), dict(Q=-1), dict(Q=2 ** 20 + 1), dict(H=0), dict(H=65), dict(seeds=None), dict(M=0),
                dict(M=2 ** 28 + 1), dict(scans=scans.reshape(-1)[1:]), dict(index=index.buf[8:]), dict(ws=ws.buf[4:])]
    for params in ((0.0, 1.0, 4.0, 32.0), (2.0 ** 21, 1.0, 4.0, 32.0), (VOXEL, 0.0, 4.0, 32.0), (VOXEL, float("inf"), 4.0, 32.0),
                   (VOXEL, float("nan"), 4.0, 32.0), (VOXEL, 1.0, -1.0, 32.0), (VOXEL, 1.0, 65.0, 32.0), (VOXEL, 1.0, 1.5, 32.0),
                   (VOXEL, 1.0, 4.0, 5.0), (VOXEL, 1.0, 4.0, 65.0), (VOXEL, 1.0, 4.0, 32.5), (VOXEL, 1.0, 4.0, 32.0, 1.0),
                   (VOXEL, 1.0, 4.0, 32.0, 0.0, 0.0, 0.0, 2.0)):
        changes.append(dict(params=params))
    for change in changes:
        _refused(L, L.EPC_EINVAL, lambda: run(**change))
    _refused(L, L.EPC_ENOMEM, lambda: run(ws_bytes=ws_need - 1))
    _refused(L, L.EPC_ENOMEM, lambda: run(index_bytes=need - 1))
    run(Q=0)                                                               # EPC_OK, nothing launched
    torch.cuda.synchronize()
    for p in out + [ws]:
        assert SG.holds_poison(p.t) and p.untouched()
    # an index that records another voxel, or another M, is not followed: every scan is flagged
    run(params=(0.25, 1.0, 4.0, 32.0))
    torch.cuda.synchronize()
    assert out[4].t.tolist() == [Z.NO_PAIR] * Q and out[3].t[:, 0].tolist() == [-1] * Q and bool(torch.isnan(out[0].t).all())
    run(M=M - 1, index_bytes=L.lib().epcnet_surfel_index_bytes(M - 1))
    torch.cuda.synchronize()
    assert out[4].t.tolist() == [Z.NO_PAIR] * Q
    run()
    torch.cuda.synchronize()
    assert out[4].t.tolist() == [0] * Q


def _host(result):
    return {name: t.cpu().numpy() for name, t in zip(NAMES, result)}


def test_wrappers_against_the_entries_their_defaults_and_refusals():
    ops, L = H.pkg("ops"), H.pkg("lib")
    dev = torch.device("cuda")
    maps = _planes()
    M = len(maps[0])
    anchor, centroid, normal = (_up(a, np.float32, dev) for a in maps)
    scans_h, seeds_h = _scans(256, 2), _seeds(2, 3)
    scans, seeds = _up(scans_h, np.float32, dev), _up(seeds_h, np.float64, dev)
    ref = Z.index_reference(*maps, VOXEL)
    index, num = ops.index_surfels(anchor, centroid, normal, VOXEL)
    assert index.dtype == torch.uint8 and index.numel() == L.lib().epcnet_surfel_index_bytes(M) and num.tolist() == ref["num"]
    res = ops.localize_scans(scans, index, centroid, normal, seeds)       # voxel 0.2, max_dist 1, 16 iterations, min_pairs 32
    assert [tuple(t.shape) for t in res] == [(2, 12), (2, 2), (2, 21), (2, 4), (2,)] and all(t.is_cuda for t in res)
    _check(_host(res), Z.localize_reference(scans_h, seeds_h, ref, 1.0, 16, 32), "defaults")
    res = ops.localize_scans(scans, index, centroid, normal)              # seeds=None: the identity
    _check(_host(res), Z.localize_reference(scans_h, None, ref, 1.0, 16, 32), "no seeds")
    need = L.lib().epcnet_scan_localize_workspace_bytes(2, 3, 256)
    mine = torch.full((L.lib().epcnet_surfel_index_bytes(M) + 64,), 0xAB, dtype=torch.uint8, device=dev)
    index2, _ = ops.index_surfels(anchor, centroid, normal, VOXEL, index=mine)
    assert index2 is mine
    for size in (need, need + 4096):
        ws = torch.full((size,), 0xAB, dtype=torch.uint8, device=dev)
        res = ops.localize_scans(scans, mine, centroid, normal, seeds, max_dist=0.5, iterations=3, min_pairs=100, workspace=ws)
        _check(_host(res), Z.localize_reference(scans_h, seeds_h, ref, 0.5, 3, 100), "a caller's workspace")
    with pytest.raises(L.EpcNetError) as e:
        ops.localize_scans(scans, index, centroid, normal, seeds, workspace=torch.empty(need - 1, dtype=torch.uint8, device=dev))
    assert e.value.status == L.EPC_ENOMEM
    with pytest.raises(L.EpcNetError) as e:
        ops.index_surfels(anchor, centroid, normal, VOXEL, index=torch.empty(index.numel() - 1, dtype=torch.uint8, device=dev))
    assert e.value.status == L.EPC_ENOMEM
    with pytest.raises(L.EpcNetError) as e:
        ops.localize_scans(scans, index, centroid, normal, seeds.float())
    assert "float64" in str(e.value) and "never converted" in str(e.value)
    base = dict(scans=scans, index=index, centroid=centroid, normal=normal, seeds=seeds)
    for change in (dict(scans=scans.cpu()), dict(scans=scans.double()), dict(scans=scans[:, :, :2]), dict(scans=scans[:, :48].contiguous()),
                   dict(index=index.cpu()), dict(index=index.view(torch.int32)), dict(centroid=centroid.cpu()), dict(normal=normal[:-1]),
                   dict(normal=normal.double()), dict(seeds=seeds.cpu()), dict(seeds=seeds[:1]), dict(seeds=seeds[:, :, :9].contiguous()),
                   dict(voxel=0.0), dict(voxel=float("nan")), dict(max_dist=0.0), dict(iterations=65), dict(iterations=-1), dict(min_pairs=5),
                   dict(min_pairs=257), dict(workspace=torch.empty(1 << 20, dtype=torch.float32, device=dev)),
                   dict(workspace=torch.empty(1 << 20, dtype=torch.uint8))):
        with pytest.raises(L.EpcNetError):
            ops.localize_scans(**dict(base, **change))
    for change in (dict(map_points=anchor.cpu()), dict(map_points=anchor.double()), dict(centroid=centroid[:-1]), dict(normal=normal.half()),
                   dict(voxel=0.0), dict(voxel=2.0 ** 21), dict(index=torch.empty(1 << 20, dtype=torch.float32, device=dev))):
        with pytest.raises(L.EpcNetError):
            ops.index_surfels(**dict(dict(map_points=anchor, centroid=centroid, normal=normal, voxel=VOXEL), **change))
    origin = torch.tensor([5.7e6, 6.2e5, 1e2], dtype=torch.float64, device=dev)
    world = seeds[:, 1].clone()
    world[:, 3::4] += origin
    made = ops.map_seeds(world, origin, yaw=4)
    assert tuple(made.shape) == (2, 4, 12) and made.dtype == torch.float64 and torch.allclose(made[:, 0], seeds[:, 1], rtol=0, atol=1e-8)
    assert torch.allclose(made[:, 2, 0], -seeds[:, 1, 0]) and torch.equal(made[:, 2, 3::4], made[:, 0, 3::4])      # half a turn about z
    for bad in ((world.float(), origin), (world, origin.float()), (world[:, :9], origin), (world, origin[:2])):
        with pytest.raises(L.EpcNetError):
            ops.map_seeds(*bad)


def test_one_graph_replayed_on_other_scans_seeds_and_map():
    """Index and localisation captured once; replayed (twice each) after scans, seeds and the map's three arrays were overwritten by
    another scene of the same shapes, then by the first again; the outputs hold junk before every replay."""
    ops, L = H.pkg("ops"), H.pkg("lib")
    dev = torch.device("cuda")
    first = _planes()
    M = len(first[0])
    other = Z.plane_map(6, ((0.3, -0.1, 1.0), (1.0, -0.2, 0.05), (-0.1, 1.0, 0.2)), (-0.8, 1.7, -2.2))
    other = tuple(np.concatenate([a, np.full((max(M - len(a), 0), 3), np.nan, np.float32)])[:M] for a in other)      # the same M
    other[2][::50, 1] = np.nan                                             # ... and another number of surfels indexed
    scenes = [(first, _scans(288, 2), _seeds(2, 3)),
              (other, np.stack([Z.plane_scan(90 + q, ((0.3, -0.1, 1.0), (1.0, -0.2, 0.05), (-0.1, 1.0, 0.2)), (-0.8, 1.7, -2.2), 288, t)
                                for q, t in enumerate(_truths(2))]), _seeds(2, 3)[::-1].copy())]
    refs = []
    for maps, scans, seeds in scenes:
        ref = Z.index_reference(*maps, VOXEL)
        refs.append((ref["num"], Z.localize_reference(scans, seeds, ref, 1.0, 4, 32)))
    assert refs[0][0] != refs[1][0] and (refs[1][1][4] == 0).all()
    dev_maps = [_up(a, np.float32, dev) for a in first]
    scans, seeds = _up(scenes[0][1], np.float32, dev), _up(scenes[0][2], np.float64, dev)
    index = torch.empty(L.lib().epcnet_surfel_index_bytes(M), dtype=torch.uint8, device=dev)
    ws = torch.empty(L.lib().epcnet_scan_localize_workspace_bytes(2, 3, 288), dtype=torch.uint8, device=dev)

    def call():
        _, num = ops.index_surfels(*dev_maps, VOXEL, index=index)
        return ops.localize_scans(scans, index, dev_maps[1], dev_maps[2], seeds, iterations=4, workspace=ws) + (num,)

    call()                                                                 # (warm-up)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call()
    for k in (1, 0, 1):
        maps, sc, sd = scenes[k]
        for dst, src in zip(dev_maps + [scans, seeds], [_up(a, np.float32, dev) for a in maps] + [_up(sc, np.float32, dev), _up(sd, np.float64, dev)]):
            dst.copy_(src)
        for replay in range(2):
            for t in out:
                t.fill_(7)                                                 # (a replay that wrote nothing would show)
            g.replay()
            torch.cuda.synchronize()
            assert out[5].tolist() == refs[k][0]
            _check(_host(out[:5]), refs[k][1], "scene %d, replay %d" % (k, replay))
