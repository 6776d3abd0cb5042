"""numpy restatement of include/epcnet_remap.h (epcnet_surfel_map_move), written from the header's text, on the state of
tests/growmap_ref.py: ``Map`` is that file's dict of cells with a ``move`` beside its ``add``.  A move takes every row through
``map_ref.lattice`` under BOTH poses, drops the unmoved rows first, then the unmatched ones (old cell no voxel BEFORE the call), subtracts
the moments of the rows taken out, adds those of the rows put in, numbers the cells the call opened by their lowest row put in, and solves
the voxels within ``ring`` of a cell that lost or received a row -- no other output row is written.  A voxel that lost every row stays in
the dict with its number and n == 0.  What it is compared with is ``surfel_ref.reference`` over the rows currently in the map at their
current poses, MATCHED BY CELL (``by_cell``): the numbers differ.  The device's outputs and ``num_call`` are pinned to this file's."""
import numpy as np

import growmap_ref as G
import map_ref as M
import surfel_ref as S

NONE = 4        # the new kind of a row that is removed: it has none


def _moments(w):
    wl = w & 4095
    u = wl >> 4
    return wl, u, np.stack([u[:, a] * u[:, b] for a, b in S._AB], 1).reshape(-1, 6)


class Map(G.Map):
    """growmap_ref.Map with ``move``.  An add that overflows leaves the dict as the call found it: the voxels "numbered before the
    overflow" are what later moves match rows against (the header's rule for the row counters after an overflow)."""

    def add(self, points, offsets, poses, num_rows=None):
        before, was_over = set(self.cells), self.over
        report = super().add(points, offsets, poses, num_rows)
        if self.over and not was_over:
            for key in set(self.cells) - before:
                del self.cells[key]
        return report

    def _solve(self, cells, numbers):
        with np.errstate(all="ignore"):                 # an empty voxel: 0 // 0, then NaN through cnt < min_count
            super()._solve(cells, numbers)

    def move(self, points, offsets, old_poses, new_poses=None, num_rows=None):
        """One call -> dict: ``num_call`` (4,) int32 and, for the tests, the voxel numbers ``touched`` (lost or received a row), ``dirty``
        (solved again), ``clean`` (every other numbered voxel) and ``emptied`` (count 0 after the call, among the touched), each sorted;
        ``new_poses=None``: remove."""
        points = np.asarray(points, np.float32).reshape(-1, 3)
        num_rows = len(points) if num_rows is None else num_rows
        none = np.zeros(0, np.int64)
        if not M.valid(offsets, num_rows):              # refused: nothing changes
            return dict(num_call=np.int32([-1, 0, 0, 0]), touched=none, dirty=none, clean=np.arange(len(self.cells)), emptied=none)
        ko, wo = M.lattice(points[:num_rows], offsets, old_poses, self.origin, self.voxel)
        if new_poses is None:
            kn, wn = np.where(ko == M.NO_CLOUD, M.NO_CLOUD, NONE), np.zeros_like(wo)
        else:
            kn, wn = M.lattice(points[:num_rows], offsets, new_poses, self.origin, self.voxel)
        # 1. unmoved rows leave first; 2. then the rows whose old cell is no voxel before this call
        unmoved = (ko == M.KEPT) & (kn == M.KEPT) & (wo == wn).all(1)
        active = (ko != M.NO_CLOUD) & ~unmoved
        keys_o, keys_n = M.keys_of(wo), M.keys_of(wn)
        known = np.array([int(k) in self.cells for k in keys_o], bool).reshape(-1)
        matched = active & ((ko != M.KEPT) | known)
        unmatched = int((active & ~matched).sum())
        take, put = matched & (ko == M.KEPT), matched & (kn == M.KEPT)
        for k in (M.KEPT, M.ABSENT, M.OUT_OF_RANGE):    # 3. and 4.: the row counters of the old kind fall, of the new kind rise
            self.kept[k] += int((matched & (kn == k)).sum()) - int((matched & (ko == k)).sum())
        self.out["num_out"][1:] = self.kept
        if self.over:
            return dict(num_call=np.int32([-1, int(put.sum()), 0, unmatched]), touched=none, dirty=none, clean=none, emptied=none)
        touched_keys = set()
        for r, (wl, u, uu) in zip(np.nonzero(take)[0], zip(*_moments(wo[take]))):
            cell = self.cells[int(keys_o[r])]
            cell[2] -= 1
            cell[3], cell[4], cell[5] = cell[3] - wl, cell[4] - u, cell[5] - uu
            touched_keys.add(int(keys_o[r]))
        before = len(self.cells)
        opened = []
        for r, (wl, u, uu) in zip(np.nonzero(put)[0], zip(*_moments(wn[put]))):          # ascending rows: a new cell's first row leads it
            key = int(keys_n[r])
            cell = self.cells.get(key)
            if cell is None:
                cell = self.cells[key] = [len(self.cells), tuple(int(v) for v in (wn[r] >> 12)), 0, np.zeros(3, np.int64),
                                          np.zeros(3, np.int64), np.zeros(6, np.int64)]
                opened.append(key)
            cell[2] += 1
            cell[3], cell[4], cell[5] = cell[3] + wl, cell[4] + u, cell[5] + uu
            touched_keys.add(key)
        if len(self.cells) > self.max_voxels:           # sticky: everything NaN / 0 from here on; the dict as the call found it
            for key in opened:
                del self.cells[key]
            self.over = True
            self._fill()
            self.out["num_out"][0] = -1
            return dict(num_call=np.int32([-1, int(put.sum()), 0, unmatched]), touched=none, dirty=none, clean=none, emptied=none)
        self.out["num_out"][0] = len(self.cells)
        touched = sorted(self.cells[key][0] for key in touched_keys)
        emptied = sorted(self.cells[key][0] for key in touched_keys if self.cells[key][2] == 0)
        dirty = {}
        if touched_keys:
            g = np.array([self.cells[key][1] for key in touched_keys], np.int64).reshape(-1, 3)
            for _, found in self._around(g):
                dirty.update((cell[0], cell) for cell in found if cell is not None)
        numbers = np.array(sorted(dirty), np.int64)
        self._solve([dirty[j] for j in numbers], numbers)
        clean = np.setdiff1d(np.arange(len(self.cells)), numbers)
        return dict(num_call=np.int32([len(self.cells) - before, int(put.sum()), len(numbers), unmatched]), touched=np.array(touched, np.int64),
                    dirty=numbers, clean=clean, emptied=np.array(emptied, np.int64))

    def numbers_by_key(self):
        return {key: cell[0] for key, cell in self.cells.items()}

    def empty_numbers(self):
        return np.array(sorted(cell[0] for cell in self.cells.values() if cell[2] == 0), np.int64)


def by_cell(got, numbers_by_key, want):
    """``got``: the seven arrays of a map; ``numbers_by_key``: cell key -> voxel number in them; ``want``: ``surfel_ref.reference`` over
    the rows currently in the map at their current poses.  None if every voxel of ``want`` is, bit for bit in all six arrays, the row of
    ``got`` that holds its cell, every other numbered voxel of ``got`` is empty (count 0, NaN in the four float arrays), the rows behind
    the numbered ones are untouched NaN / 0, and the three row counts agree; else a description of the first difference."""
    if got["num_out"].tolist()[1:] != want["num_out"].tolist()[1:]:
        return "row counts", got["num_out"].tolist(), want["num_out"].tolist()
    if int(got["num_out"][0]) != len(numbers_by_key):
        return "num_out[0]", int(got["num_out"][0]), len(numbers_by_key)
    V = want["V"]
    keys = want["vox"]["keys"] if V else np.zeros(0, np.int64)
    missing = [int(k) for k in keys if int(k) not in numbers_by_key]
    if missing:
        return "cells of the reference that are no voxel of the map", missing[:4]
    at = np.array([numbers_by_key[int(k)] for k in keys], np.int64)
    for name in G.FLOATS + ("count", "support"):
        a, b = np.asarray(got[name]).view(np.uint32)[at], np.asarray(want[name]).view(np.uint32)[:V]
        if not (a == b).all():
            return name, "first differing voxel of the reference", int(np.nonzero((a != b).reshape(V, -1).any(1))[0][0])
    rest = np.setdiff1d(np.arange(len(got["count"])), at)
    if got["count"][rest].any():
        return "a voxel outside the reference holds rows", int(rest[np.nonzero(got["count"][rest])[0][0]])
    for name in G.FLOATS:
        if not (np.asarray(got[name]).view(np.uint32)[rest] == M.NAN_WORD).all():
            return name, "an empty voxel that is not NaN"
    if got["support"][len(numbers_by_key):].any():
        return "support behind the numbered voxels",
    return None


def nudged(poses, which, seed=1, shift=0.3, angle=0.05):
    """``poses`` (C, 12) with the clouds ``which`` re-posed as a loop closure re-poses them: a seeded rotation of about ``angle`` radians
    in front of the cloud's own, and about ``shift`` metres on its translation.  The other rows are the same bits."""
    import submap_ref as SR
    rng = np.random.default_rng([seed, len(poses)])
    out = np.array(poses, np.float64).reshape(-1, 3, 4).copy()
    for c in which:
        q = np.concatenate([[1.0], 0.5 * angle * rng.uniform(-1.0, 1.0, size=3)])
        out[c, :, :3] = SR.quat_matrix(q) @ out[c, :, :3]
        out[c, :, 3] += shift * rng.uniform(-1.0, 1.0, size=3)
    return out.reshape(-1, 12)
