"""The surfel map that grows across calls (include/epcnet_growmap.h), none of it with a counterpart in the reference: ``SurfelMap`` owns
the persistent state and the seven output tensors of ``fuse_surfels`` on the device, and ``add`` puts further posed clouds into them at a
cost that follows the rows added, not the size of the map; ``remove`` and ``repose`` (include/epcnet_remap.h) take clouds out or move
them to corrected poses at a cost that follows the rows moved.  Contiguous tensors of the exact dtype or a refusal, nothing read back, every
call asynchronous and capturable in a graph.  ``ops`` re-exports ``SurfelMap``."""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import lib as L
from .loops import _workspace
from .scans import _device_tensor, _map_arguments, _spare

OUTPUTS = ("map_points", "count", "centroid", "normal", "eigen", "support", "num_out")


class SurfelMap:
    """``fuse_surfels`` as a map that persists: after any sequence of ``add`` calls the attributes ``map_points``, ``count``,
    ``centroid``, ``normal``, ``eigen``, ``support`` and ``num_out`` -- device tensors that stay THE SAME tensors for the life of the map,
    shaped as ``fuse_surfels`` returns them for ``max_voxels`` -- hold bit for bit what ``fuse_surfels`` returns for the concatenation of
    those calls' clouds at this ``voxel``, ``origin``, ``min_count``, ``ring``, ``min_support`` and ``max_voxels`` (include/epcnet_growmap.h;
    numpy restatement: tests/growmap_ref.py).  An ``add`` solves again only the voxels within ``ring`` of a cell that received a row and
    writes no other row of the arrays.  Tensors and attributes are the only interface: nothing is copied, nothing is read back.

    ``max_voxels`` has no default: the state (a table of the smallest power of two >= 2 max_voxels + 1 slots of 128 bytes) and the arrays
    are allocated once.  More voxels than that is the overflow of ``fuse_surfels`` -- all-NaN arrays and ``num_out[0] == -1`` -- from
    that call on.  ``origin``: (3,) float64 device tensor, kept as the attribute ``origin``; ``None`` takes the first ``add``'s first pose
    translation (a device copy), as ``fuse_map`` does, and the state is initialised then.  ``device``: where the map lives (None: the
    current ROCm device, or ``origin``'s).

    The online loop::

        m = ops.SurfelMap(max_voxels=1 << 21, voxel=0.2, origin=origin)
        m.add(sub_points, sub_offsets, fixed)                                   # the map so far
        index, _ = ops.index_surfels(m.map_points, m.centroid, normal_of(m), 0.2, index=index)   # 0.24 ms at 1.4 M voxels: rebuilt, not patched
        pose, fit, hessian, info, st = ops.localize_scans(cloud, index, m.centroid, normal_of(m), seeds)
        m.add(scan_points, scan_offsets, pose)                                  # the localised scan goes in

    (``normal_of``: the caller's planarity filter, see ``index_surfels``.)  After a loop closure, ``repose`` moves the submaps it
    corrected and ``remove`` takes clouds out (include/epcnet_remap.h; restatement: tests/remap_ref.py): voxels left without a row keep
    their number as empty voxels, ``count`` 0.  Not covered: the index patched in place, compaction of empty voxels (``reset()`` and
    ``add``), moving the origin, ray-casting."""

    def __init__(self, max_voxels, voxel=0.2, origin=None, min_count=1, ring=1, min_support=8, device=None):
        who = "SurfelMap"
        if origin is not None:
            _device_tensor(who, "origin", origin, torch.float64, (3,))
            if device is not None and torch.device(device) != origin.device:
                raise L.EpcNetError(-1, "%s: origin lives on %s, the map was asked for on %s" % (who, origin.device, torch.device(device)))
            device = origin.device
        L.require_gpu()
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise L.EpcNetError(-1, "%s: the map lives on a ROCm device (no CPU fallback), got %s" % (who, dev))
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        max_voxels = int(max_voxels)
        need = int(L.lib().epcnet_surfel_map_state_bytes(max_voxels))
        if need == 0:
            raise L.EpcNetError(-1, "%s: need 1 <= max_voxels <= 2^28, got %d" % (who, max_voxels))
        if ring != int(ring) or not 0 <= int(ring) <= L.EPC_SURFEL_MAX_RING or min_support != int(min_support) or not 3 <= int(min_support) < 2 ** 31:
            raise L.EpcNetError(-1, "%s: need an integer ring in [0, %d] and 3 <= min_support < 2^31, got %r and %r"
                                % (who, L.EPC_SURFEL_MAX_RING, ring, min_support))
        self.max_voxels, self.voxel, self.min_count, self.ring, self.min_support = max_voxels, float(voxel), int(min_count), int(ring), int(min_support)
        self.device, self.origin = dev, origin
        self._params = (ctypes.c_double * L.EPC_SURFEL_PARAMS)(self.voxel, float(self.min_count), float(self.ring), float(self.min_support))   # (host memory)
        self.state = torch.empty(need, dtype=torch.uint8, device=dev)
        self.map_points, self.centroid, self.normal, self.eigen = (torch.empty((max_voxels, 3), dtype=torch.float32, device=dev) for _ in range(4))
        self.count, self.support = (torch.empty(max_voxels, dtype=torch.int32, device=dev) for _ in range(2))
        self.num_out = torch.empty(4, dtype=torch.int32, device=dev)
        if origin is not None:
            self.reset()

    def _arrays(self):
        return (self.map_points, self.count, self.centroid, self.normal, self.eigen, self.support, self.num_out)

    def reset(self):
        """The empty map again (epcnet_surfel_map_init): the table cleared, every word of the arrays NaN / 0, ``num_out`` 0, 0, 0, 0;
        the one call whose work scales with ``max_voxels``.  The origin stays; a map that has none yet (``origin=None`` and no ``add``)
        has nothing to reset."""
        if self.origin is not None:
            L.run.epcnet_surfel_map_init(self.origin, self._params, self.max_voxels, self.state, self.state.numel(), *self._arrays())

    def add(self, points, offsets, poses, workspace: Optional[torch.Tensor] = None):
        """Posed clouds into the map (epcnet_surfel_map_add) -> ``num_call`` (4,) int32 device tensor: voxels new in this call (-1: the
        call numbered nothing -- invalid offsets, which add nothing and leave the map as it was, or a map that has overflowed), rows
        kept, voxels solved again, 0.  ``points``, ``offsets``, ``poses``: as ``fuse_surfels`` takes them, under its checks -- (C, 12) or
        (C, 3, 4) FLOAT64 poses; float32 poses are refused, never converted.  On the current stream, no host read, capturable: a
        captured graph replays on other points, offsets and poses of the same shape against this map.  ``workspace``: a uint8 device
        tensor of at least ``epcnet_surfel_map_add_workspace_bytes(rows, C, ring)`` bytes to reuse (what a captured graph needs), else
        one is allocated."""
        who = "SurfelMap.add"
        first = self.origin is None
        C, rows, dev, poses, origin, _, _, _, _ = _map_arguments(who, points, offsets, poses, self.voxel, self.origin, self.max_voxels,
                                                                 self.min_count, "epcnet_map_surfels_workspace_bytes")
        if dev != self.device:
            raise L.EpcNetError(-1, "%s: points live on %s, the map on %s" % (who, dev, self.device))
        if first:
            self.origin = origin
            self.reset()
        need = int(L.lib().epcnet_surfel_map_add_workspace_bytes(rows, C, self.ring))
        ws, own = _workspace(who, need, workspace, dev)
        num_call = torch.empty(4, dtype=torch.int32, device=dev)
        L.run.epcnet_surfel_map_add(points if rows else _spare(dev), offsets, rows, C, poses if C else _spare(dev, torch.float64), self._params,
                                    self.max_voxels, self.state, self.state.numel(), *self._arrays(), num_call, ws, ws.numel())
        if own:
            ws.record_stream(torch.cuda.current_stream(dev))
        return num_call

    def _move(self, who, points, offsets, old_poses, new_poses, workspace):
        if self.origin is None:
            raise L.EpcNetError(-1, "%s: the map has no origin yet (origin=None and no add): it holds no row to move" % who)
        if new_poses is not None:
            for name, p in (("old_poses", old_poses), ("new_poses", new_poses)):
                _device_tensor(who, name, p, torch.float64)
            if tuple(new_poses.shape) != tuple(old_poses.shape):
                raise L.EpcNetError(-1, "%s: old_poses and new_poses must have one shape, got %s and %s"
                                    % (who, tuple(old_poses.shape), tuple(new_poses.shape)))
            if new_poses.device != old_poses.device:
                raise L.EpcNetError(-1, "%s: old_poses live on %s, new_poses on %s" % (who, old_poses.device, new_poses.device))
        C, rows, dev, old_poses, _, _, _, _, _ = _map_arguments(who, points, offsets, old_poses, self.voxel, self.origin, self.max_voxels,
                                                                self.min_count, "epcnet_map_surfels_workspace_bytes")
        if dev != self.device:
            raise L.EpcNetError(-1, "%s: points live on %s, the map on %s" % (who, dev, self.device))
        need = int(L.lib().epcnet_surfel_map_move_workspace_bytes(rows, C, self.ring))
        ws, own = _workspace(who, need, workspace, dev)
        num_call = torch.empty(4, dtype=torch.int32, device=dev)
        spare = _spare(dev, torch.float64)
        L.run.epcnet_surfel_map_move(points if rows else _spare(dev), offsets, rows, C, old_poses if C else spare,
                                     None if new_poses is None else new_poses.reshape(C, 12) if C else spare, self._params, self.max_voxels,
                                     self.state, self.state.numel(), *self._arrays(), num_call, ws, ws.numel())
        if own:
            ws.record_stream(torch.cuda.current_stream(dev))
        return num_call

    def remove(self, points, offsets, poses, workspace: Optional[torch.Tensor] = None):
        """Clouds that were added at ``poses`` OUT of the map (epcnet_surfel_map_move of include/epcnet_remap.h with no new poses) ->
        ``num_call`` (4,) int32 device tensor: -1 (refused on the device, or an overflowed map) or 0, 0, voxels solved again, rows
        unmatched.  ``points``, ``offsets``, ``poses``: exactly what ``add`` was given, under its checks (FLOAT64 poses or a refusal).  Every
        row leaves the voxel that pose puts it in -- the sums are integers, so what stays is bit for bit the map of the remaining rows --;
        a voxel left with no row keeps its number as an EMPTY voxel: ``count`` 0 and NaN rows, still counted in ``num_out[0]`` and in
        ``max_voxels`` (compaction is ``reset()`` and ``add``).  A row whose cell was no voxel before the call was never added: it is
        skipped and counted as unmatched.  Refused on a map that has no origin yet.  Same stream, capture and ``workspace`` rules as
        ``add``, sized by ``epcnet_surfel_map_move_workspace_bytes(rows, C, ring)``."""
        return self._move("SurfelMap.remove", points, offsets, poses, None, workspace)

    def repose(self, points, offsets, old_poses, new_poses, workspace: Optional[torch.Tensor] = None):
        """Clouds that are in the map at ``old_poses`` moved to ``new_poses`` (epcnet_surfel_map_move) -- what a loop closure asks
        for: ``retrieval.close_loops`` returns corrected submap poses, and the submaps go where they belong at a cost that follows THEIR
        rows, not the map's -> ``num_call`` (4,) int32 device tensor: voxels new in this call (-1: refused on the device, or an
        overflowed map), rows put in, voxels solved again, rows unmatched.  Both pose tensors: FLOAT64, of one shape, (C, 12) or
        (C, 3, 4).  A row is taken out of the cell its old pose gives and put into the cell its new pose gives; a row whose lattice
        position does not change touches nothing (pass every submap with the poses before and after: the ones the closure left alone
        cost two transforms per row).  Afterwards every voxel that holds rows equals, bit for bit and matched by cell, what
        ``fuse_surfels`` returns for all rows at their current poses; empty voxels as ``remove`` leaves them.  Only the voxels within
        ``ring`` of a cell that lost or received a row are written.  Refused on a map that has no origin yet."""
        return self._move("SurfelMap.repose", points, offsets, old_poses, new_poses, workspace)
