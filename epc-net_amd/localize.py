"""Scan-to-map localisation (include/epcnet_localize.h), none of it with a counterpart in the reference: ``index_surfels`` builds the
lookup index of a surfel map once, ``localize_scans`` aligns Q scans against it by point-to-plane ICP and returns the information of
every estimate, ``map_seeds`` forms the seeds.  Plain functions over device tensors: contiguous tensors of the exact dtype or a refusal,
nothing read back, every call asynchronous and capturable in a graph.  ``ops`` re-exports these names."""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import torch

from . import lib as L
from .loops import _workspace, yaw_seeds


def _check(who: str, name: str, t, dtype, shape, device=None):
    """A contiguous device tensor of exactly ``dtype`` -- nothing is converted -- whose shape matches ``shape`` (None: any extent), given
    ``device`` on it."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise L.EpcNetError(-1, "%s: %s must live on a ROCm device (no CPU fallback)" % (who, name))
    if t.dtype != dtype or not t.is_contiguous():
        raise L.EpcNetError(-1, "%s: %s must be a contiguous %s tensor, got %s%s" % (
            who, name, dtype, t.dtype, " (poses are float64: they are refused, never converted)" if dtype == torch.float64 else ""))
    if t.dim() != len(shape) or any(s is not None and int(d) != s for d, s in zip(t.shape, shape)) or (device is not None and t.device != device):
        raise L.EpcNetError(-1, "%s: %s must be %s on the first argument's device, got %s" % (
            who, name, "(" + ", ".join("?" if s is None else str(s) for s in shape) + ")", tuple(t.shape)))


def _voxel(who: str, voxel) -> float:
    voxel = float(voxel)
    if not (math.isfinite(voxel) and 2.0 ** -20 <= voxel <= 2.0 ** 20):
        raise L.EpcNetError(-1, "%s: need 2^-20 <= voxel <= 2^20, got %r" % (who, voxel))
    return voxel


def index_surfels(map_points: torch.Tensor, centroid: torch.Tensor, normal: torch.Tensor, voxel: float, index: Optional[torch.Tensor] = None):
    """The lookup index of a surfel map (include/epcnet_localize.h: epcnet_surfel_index; numpy restatement: tests/localize_ref.py):
    ``(index uint8 device tensor, num (4,) int32: surfels indexed, not present, duplicates, out of range)``, on the current stream, no
    host read, capturable.  ``map_points``, ``centroid``, ``normal``: (M, 3) float32, what ``fuse_surfels`` returned at this ``voxel`` --
    ``map_points`` names a surfel's cell, the other two are copied into the index.  A surfel with a non-finite word is not present:
    PLANARITY FILTERING IS THE CALLER'S, ahead of this call -- with ``eigen`` of ``fuse_surfels``, ``flat = eigen[:, 0] < 0.05 *
    eigen[:, 1]``, ``normal = torch.where(flat[:, None], normal, nan)``.  Build it ONCE per map and hand it to every ``localize_scans``
    call; a map whose arrays change is indexed again.  ``index``: a uint8 device tensor of at least ``epcnet_surfel_index_bytes(M)``
    bytes to build into (what a captured graph needs), else one is allocated."""
    who = "index_surfels"
    _check(who, "map_points", map_points, torch.float32, (None, 3))
    dev, M = map_points.device, int(map_points.shape[0])
    _check(who, "centroid", centroid, torch.float32, (M, 3), dev)
    _check(who, "normal", normal, torch.float32, (M, 3), dev)
    voxel = _voxel(who, voxel)
    L.require_gpu()
    need = int(L.lib().epcnet_surfel_index_bytes(M))
    if need == 0:
        raise L.EpcNetError(-1, "%s: need 1 <= M <= 2^28 surfels, got %d" % (who, M))
    index, _ = _workspace(who, need, index, dev)
    num = torch.empty(4, dtype=torch.int32, device=dev)
    params = (ctypes.c_double * L.EPC_LOCALIZE_INDEX_PARAMS)(voxel)         # (host memory; the three reserved doubles are 0)
    L.run.epcnet_surfel_index(map_points, centroid, normal, M, params, index, index.numel(), num)
    return index, num


def localize_scans(scans: torch.Tensor, index: torch.Tensor, centroid: torch.Tensor, normal: torch.Tensor,
                   seeds: Optional[torch.Tensor] = None, voxel: float = 0.2, max_dist: float = 1.0, iterations: int = 16,
                   min_pairs: int = 32, workspace: Optional[torch.Tensor] = None):
    """Q scans localised against one surfel map (include/epcnet_localize.h: epcnet_scan_localize; numpy restatement:
    tests/localize_ref.py) by point-to-plane ICP: ``(pose (Q, 12) float64 [R | t] scan -> map frame, fit (Q, 2) float64: mean squared
    point-to-plane residual in m^2 and accepted / present rows, hessian (Q, 21) float64: the upper triangle of sum J J^T of the final
    pass in (rad, m) about the sensor -- the information of the estimate; a corridor's free direction is its near-null direction --,
    info (Q, 4) int32: best seed, accepted rows, present rows, 0, status (Q,) int32)``, device tensors, on the current stream, no host
    read, capturable.  ``scans`` (Q, n, 3) float32 in METRES (``grid_downsample(normalize=False)``, ``forward_trajectory(clouds=True)``;
    a row with a non-finite word is absent; n a multiple of 32 in [32, 4096]); ``index``: ``index_surfels``' for ``centroid``,
    ``normal`` (M, 3) float32 at this ``voxel``; ``seeds`` (Q, H, 12) FLOAT64 ``[R | t]`` relative to the map's origin (``map_seeds``),
    None = the identity; float32 seeds are refused, never converted.  The seed with the most rows within ``max_dist`` metres of a
    surfel of the 27 cells around them is refined ``iterations`` times.  EPC_STATUS_NO_PAIR: no finite seed, or an index that is not
    this map's; EPC_STATUS_NO_FIT: fewer than ``min_pairs`` (at least 6) accepted rows, or a singular system -- a single plane --; both
    leave NaN pose, fit and hessian.  ``workspace``: a uint8 device tensor of at least ``epcnet_scan_localize_workspace_bytes`` bytes
    to reuse (what a captured graph needs), else one is allocated."""
    who = "localize_scans"
    _check(who, "scans", scans, torch.float32, (None, None, 3))
    dev, Q, n = scans.device, int(scans.shape[0]), int(scans.shape[1])
    _check(who, "centroid", centroid, torch.float32, (None, 3), dev)
    M = int(centroid.shape[0])
    _check(who, "normal", normal, torch.float32, (M, 3), dev)
    _check(who, "index", index, torch.uint8, (None,), dev)
    H = 1
    if seeds is not None:
        _check(who, "seeds", seeds, torch.float64, (Q, None, 12), dev)
        H = int(seeds.shape[1])
    voxel, max_dist, iterations, min_pairs = _voxel(who, voxel), float(max_dist), int(iterations), int(min_pairs)
    L.require_gpu()
    need = int(L.lib().epcnet_scan_localize_workspace_bytes(Q, H, n))
    if need == 0 and Q:
        raise L.EpcNetError(-1, "%s: need n a multiple of 32 in [32, 4096], Q <= 2^20 and 1 <= H <= 64, got %d, %d and %d" % (who, n, Q, H))
    ws, own = _workspace(who, need, workspace, dev)
    pose = torch.empty((Q, 12), dtype=torch.float64, device=dev)
    fit = torch.empty((Q, 2), dtype=torch.float64, device=dev)
    hessian = torch.empty((Q, 21), dtype=torch.float64, device=dev)
    info = torch.empty((Q, 4), dtype=torch.int32, device=dev)
    status = torch.empty((Q,), dtype=torch.int32, device=dev)
    params = (ctypes.c_double * L.EPC_LOCALIZE_PARAMS)(voxel, max_dist, float(iterations), float(min_pairs))     # (host memory)
    arg = lambda t: t if t.numel() else ws.data_ptr()          # an empty tensor has no address: the workspace's stands in
    L.run.epcnet_scan_localize(arg(scans), Q, n, None if seeds is None else arg(seeds), H, index, index.numel(), centroid, normal, M, params,
                               arg(pose), arg(fit), arg(hessian), arg(info), arg(status), ws, ws.numel())
    if own:
        ws.record_stream(torch.cuda.current_stream(dev))
    return pose, fit, hessian, info, status


def map_seeds(poses12: torch.Tensor, origin: torch.Tensor, yaw: int = 1) -> torch.Tensor:
    """Seeds for ``localize_scans`` from world poses: ``poses12`` (Q, 12) float64 ``[R | t]`` scan -> world (odometry, or the pose of a
    revisit candidate) with ``origin`` (3,) float64 -- the map's, as ``fuse_surfels`` returned it -- taken off the translation, and
    ``yaw`` > 1 hypotheses per scan that differ by a turn about the sensor's z (``yaw_seeds``): (Q, yaw, 12) float64.  Built with torch
    in float64: outside the bit contract, like ``yaw_seeds``; ``localize_scans``' contract is seeds -> result."""
    if not torch.is_tensor(poses12) or poses12.dtype != torch.float64 or poses12.dim() != 2 or int(poses12.shape[1]) != 12:
        raise L.EpcNetError(-1, "map_seeds: poses12 must be a float64 tensor (Q, 12) (poses are refused, never converted)")
    if not torch.is_tensor(origin) or origin.dtype != torch.float64 or tuple(origin.shape) != (3,) or origin.device != poses12.device:
        raise L.EpcNetError(-1, "map_seeds: origin must be a float64 tensor (3,) on the poses' device")
    rel = poses12.clone()
    rel[:, 3::4] -= origin
    return yaw_seeds(yaw, rel)
