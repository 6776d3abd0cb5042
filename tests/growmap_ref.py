"""numpy restatement of include/epcnet_growmap.h (epcnet_surfel_map_init, epcnet_surfel_map_add): the INCREMENTAL procedure, written from
the header's text.  A dict of cells holds the integer moments and each voxel's number, carried across calls; an ``add`` takes its rows
through ``map_ref.lattice``, adds their moments, numbers the new cells by first row behind the V it found, forms the dirty set -- the
voxels within ``ring`` of a cell that received a row, a cell out of range skipped, never wrapped -- and applies ``surfel_ref.solve`` to
THE DIRTY VOXELS ONLY: every other output row is kept from the call before.  What it is compared with is ``surfel_ref.reference`` on the
concatenation of the calls (``concatenation``): that the two agree on every bit shows the dirty rule is sufficient, without a device
(tests/test_growmap_cpu.py).  The device's ``num_call`` is pinned to this file's."""
import itertools

import numpy as np

import map_ref as M
import surfel_ref as S

FLOATS = ("map_points", "centroid", "normal", "eigen")
INTS = ("count", "support", "num_out")


def _nan_rows(rows):
    a = np.zeros((rows, 3), np.float32)
    a.view(np.uint32)[:] = M.NAN_WORD
    return a


class Map:
    """The state and the seven outputs.  ``cells``: key -> [number, g (3,), n, S (3,) of w & 4095, A (3,), B (6,)], Python ints and int64
    arrays; insertion order is the order of the numbers."""

    def __init__(self, origin, voxel, max_voxels, min_count=1, ring=1, min_support=8):
        self.origin, self.voxel, self.max_voxels = np.asarray(origin, np.float64), float(voxel), int(max_voxels)
        self.min_count, self.ring, self.min_support = int(min_count), int(ring), int(min_support)
        self.reset()

    def reset(self):
        self.cells, self.over, self.kept = {}, False, [0, 0, 0]
        self.out = {name: _nan_rows(self.max_voxels) for name in FLOATS}
        self.out.update(count=np.zeros(self.max_voxels, np.int32), support=np.zeros(self.max_voxels, np.int32), num_out=np.zeros(4, np.int32))

    def outputs(self):
        return {name: a.copy() for name, a in self.out.items()}

    def _fill(self):
        for name in FLOATS:
            self.out[name].view(np.uint32)[:] = M.NAN_WORD
        self.out["count"][:] = 0
        self.out["support"][:] = 0

    def _around(self, g):
        """For the cells g (D, 3): every offset o of [-ring, ring]^3 with, per cell, the dict's entry of cell g + o -- None where the
        cell lies outside the range (skipped, never wrapped) or is no voxel."""
        span = range(-self.ring, self.ring + 1)
        for o2, o1, o0 in itertools.product(span, span, span):
            o = np.array([o0, o1, o2], np.int64)
            c = g + o
            inside = ((c >= -M.MAX_CELL) & (c < M.MAX_CELL)).all(1)
            keys = ((c[:, 2] + M.MAX_CELL) << 42) | ((c[:, 1] + M.MAX_CELL) << 21) | (c[:, 0] + M.MAX_CELL)
            yield o, [self.cells.get(int(k)) if ok else None for k, ok in zip(keys, inside)]

    def add(self, points, offsets, poses, num_rows=None):
        """One call -> dict: ``num_call`` (4,) int32, and for the tests the voxel numbers ``touched`` (received a row), ``dirty`` (solved
        again: within ``ring`` of a touched cell) and ``clean`` (every other voxel of the map), each sorted."""
        points = np.asarray(points, np.float32).reshape(-1, 3)
        num_rows = len(points) if num_rows is None else num_rows
        none = np.zeros(0, np.int64)
        if not M.valid(offsets, num_rows):              # adds nothing: the state and the outputs stay as they were
            return dict(num_call=np.int32([-1, 0, 0, 0]), touched=none, dirty=none, clean=np.arange(len(self.cells)))
        kind, w = M.lattice(points[:num_rows], offsets, poses, self.origin, self.voxel)
        tally = [int((kind == k).sum()) for k in (M.KEPT, M.ABSENT, M.OUT_OF_RANGE)]
        self.kept = [a + b for a, b in zip(self.kept, tally)]
        self.out["num_out"][1:] = self.kept
        if self.over:
            return dict(num_call=np.int32([-1, tally[0], 0, 0]), touched=none, dirty=none, clean=none)
        rows = np.nonzero(kind == M.KEPT)[0]            # ascending: the first occurrence of a key is its first row
        uniq, first, inverse = np.unique(M.keys_of(w[rows]), return_index=True, return_inverse=True)
        inverse = inverse.reshape(-1)
        K = len(uniq)
        wl = w[rows] & 4095
        u = wl >> 4
        n, Ssum, A, B = np.zeros(K, np.int64), np.zeros((K, 3), np.int64), np.zeros((K, 3), np.int64), np.zeros((K, 6), np.int64)
        np.add.at(n, inverse, 1)
        np.add.at(Ssum, inverse, wl)
        np.add.at(A, inverse, u)
        np.add.at(B, inverse, np.stack([u[:, a] * u[:, b] for a, b in S._AB], 1))
        before = len(self.cells)
        for k in np.argsort(first, kind="stable"):      # by first row: new cells take the next numbers in this order
            key = int(uniq[k])
            cell = self.cells.get(key)
            if cell is None:
                cell = self.cells[key] = [len(self.cells), tuple(int(v) for v in (w[rows[first[k]]] >> 12)), 0, np.zeros(3, np.int64),
                                          np.zeros(3, np.int64), np.zeros(6, np.int64)]
            cell[2] += int(n[k])
            cell[3] += Ssum[k]
            cell[4] += A[k]
            cell[5] += B[k]
        if len(self.cells) > self.max_voxels:           # sticky: everything NaN / 0 from here on
            self.over = True
            self._fill()
            self.out["num_out"][0] = -1
            return dict(num_call=np.int32([-1, tally[0], 0, 0]), touched=none, dirty=none, clean=none)
        self.out["num_out"][0] = len(self.cells)
        touched = sorted(self.cells[int(key)][0] for key in uniq)
        dirty = {}
        g = np.array([self.cells[int(key)][1] for key in uniq], np.int64).reshape(K, 3)
        for _, found in self._around(g):
            dirty.update((cell[0], cell) for cell in found if cell is not None)
        numbers = np.array(sorted(dirty), np.int64)
        self._solve([dirty[j] for j in numbers], numbers)
        clean = np.setdiff1d(np.arange(len(self.cells)), numbers)
        return dict(num_call=np.int32([len(self.cells) - before, tally[0], len(numbers), 0]), touched=np.array(touched, np.int64),
                    dirty=numbers, clean=clean)

    def _solve(self, cells, numbers):
        """The output rows of the given voxels from the dict as it stands."""
        D = len(cells)
        if D == 0:
            return
        g = np.array([c[1] for c in cells], np.int64).reshape(D, 3)
        cnt = np.array([c[2] for c in cells], np.int64)
        m = np.stack([c[3] for c in cells]) // cnt[:, None]
        step = np.float64(self.voxel) / np.float64(4096.0)
        value = ((g * 4096 + m).astype(np.float64) * step).astype(np.float32)
        value.view(np.uint32)[cnt < self.min_count] = M.NAN_WORD
        self.out["map_points"][numbers] = value
        self.out["count"][numbers] = cnt
        N, S1, S2 = np.zeros(D, np.int64), np.zeros((D, 3), np.int64), np.zeros((D, 6), np.int64)
        for o, found in self._around(g):
            ok = np.array([q is not None and q[2] >= self.min_count for q in found], bool)
            nn = np.array([q[2] if k else 0 for q, k in zip(found, ok)], np.int64)
            AA = np.array([q[4] if k else (0, 0, 0) for q, k in zip(found, ok)], np.int64).reshape(D, 3)
            BB = np.array([q[5] if k else (0,) * 6 for q, k in zip(found, ok)], np.int64).reshape(D, 6)
            e = 256 * o
            N += nn
            S1 += np.where(ok[:, None], AA + nn[:, None] * e, 0)
            S2 += np.where(ok[:, None], np.stack([BB[:, k] + e[a] * AA[:, b] + e[b] * AA[:, a] + nn * (e[a] * e[b]) for k, (a, b) in enumerate(S._AB)], 1), 0)
        mu, lam, nrm = S.solve(N, S1, S2)
        centroid, normal, eigen = S.finish(g, mu, lam, nrm, self.voxel)
        valid = (cnt >= self.min_count) & (N >= self.min_support)
        for name, v in (("centroid", centroid), ("normal", normal), ("eigen", eigen)):
            v.view(np.uint32)[~valid] = M.NAN_WORD
            self.out[name][numbers] = v
        self.out["support"][numbers] = N


def concatenation(calls):
    """``(points, offsets, poses)`` of the concatenation of ``calls`` = [(points, offsets, poses), ...]: each call's rows in
    [offsets[0], offsets[C]) in call order, the poses appended.  Calls with invalid offsets are the caller's to leave out."""
    pts, offs, poses, at = [], [0], [], 0
    for p, o, q in calls:
        p, o = np.asarray(p, np.float32).reshape(-1, 3), np.asarray(o, np.int64)
        pts.append(p[o[0]:o[-1]])
        offs += (o[1:] - o[0] + at).tolist()
        at += int(o[-1] - o[0])
        poses.append(np.asarray(q, np.float64).reshape(-1, 12))
    return np.concatenate(pts) if pts else np.zeros((0, 3), np.float32), np.array(offs, np.int32), np.concatenate(poses) if poses else np.zeros((0, 12))


def pieces(points, offsets, poses, cuts):
    """The scene cut at the rows ``cuts`` (ascending, inside [0, rows]) into calls: every piece keeps all the poses and the offsets
    clipped to its rows (clouds outside it are empty)."""
    points, offsets = np.asarray(points, np.float32).reshape(-1, 3), np.asarray(offsets, np.int64)
    edges = [0] + list(cuts) + [len(points)]
    return [(points[a:b], (np.clip(offsets, a, b) - a).astype(np.int32), poses) for a, b in zip(edges[:-1], edges[1:])]


def run(calls, origin, voxel, max_voxels, min_count=1, ring=1, min_support=8):
    """Every call through one Map -> ``(map, [what add returned], [the outputs after each call])``."""
    m = Map(origin, voxel, max_voxels, min_count, ring, min_support)
    reports, outs = [], []
    for p, o, q in calls:
        reports.append(m.add(p, o, q))
        outs.append(m.outputs())
    return m, reports, outs


def same_bits(got, want):
    """The first output whose bit patterns differ, or None."""
    for name in INTS + FLOATS:
        if not (np.asarray(got[name]).view(np.uint32) == np.asarray(want[name]).view(np.uint32)).all():
            return name
    return None
