"""The scan front end: everything between raw sensor data and the network's (B, N, 3) clouds -- the spatial sort, packing, grid
down-sampling, ground removal, travel-length submaps, de-skewing and pose interpolation --, the voxel map the corrected submaps are
fused into, and the relations and training tuples drawn from poses.  Plain functions over device tensors: no autograd, no torch arithmetic on the hot path, no CPU fallback.  Every launch goes
through ``L.run`` (lib.py).  ``ops`` re-exports these names: ``ops.pack_scans`` and the rest are this module's."""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import lib as L
from .lib import EpcNetError
from .loops import _workspace       # a caller's workspace is refused or taken by ONE rule

# why a tensor of the wrong dtype is refused and never converted, by the dtype that was asked for
_NEVER_CONVERTED = {
    torch.int64: " (stamps are integer nanoseconds and are never converted: a float64 second count near 1.7e9 is 2.4e-7 s apart; "
                 "convert it yourself, e.g. torch.round(t * 1e9).to(torch.int64), if that is good enough)",
    torch.int32: " (offsets inside a sweep are integer nanoseconds: convert yourself, e.g. torch.round(dt * 1e9).to(torch.int32))",
    torch.float64: " (float32 UTM coordinates are 0.5 m apart: poses are never converted)",
}


def _device_tensor(who, name, t, dtype, shape=None, hint=None):
    """The refusals every entry shares: a contiguous device tensor of exactly ``dtype`` -- nothing is converted -- and, given, of
    ``shape``.  ``hint``: what follows the dtype refusal (None: the reason of ``_NEVER_CONVERTED``)."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise EpcNetError(-1, "%s: %s must live on a ROCm device (no CPU fallback)" % (who, name))
    if t.dtype != dtype or not t.is_contiguous():
        hint = _NEVER_CONVERTED.get(dtype, "") if hint is None else hint
        raise EpcNetError(-1, "%s: %s must be a contiguous %s tensor, got %s%s" % (who, name, dtype, t.dtype, hint))
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise EpcNetError(-1, "%s: %s must be %s, got %s" % (who, name, tuple(shape), tuple(t.shape)))


def _packed(who, points, offsets, count_name, offsets_hint=""):
    """The packed scans of ``pack_scans``: ``points`` (total, 3) float32 and ``offsets`` (count + 1,) int32 on the device ->
    ``(count, total, device)``."""
    _device_tensor(who, "points", points, torch.float32)
    _device_tensor(who, "offsets", offsets, torch.int32, hint=offsets_hint)
    if points.dim() != 2 or int(points.shape[1]) != 3 or offsets.dim() != 1 or offsets.numel() < 1:
        raise EpcNetError(-1, "%s: expected points (total, 3) and offsets (%s + 1,), got %s and %s"
                          % (who, count_name, tuple(points.shape), tuple(offsets.shape)))
    return int(offsets.numel()) - 1, int(points.shape[0]), points.device


def _out_like(who, out, shape, dev, what, not_same_as=None):
    """``out=``: a new (shape) float32 tensor for None, else the caller's after the refusal of anything but a contiguous float32 device
    tensor of that shape (``what`` words the shape) that is not ``not_same_as``."""
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=dev)
    if (not torch.is_tensor(out) or not out.is_cuda or tuple(out.shape) != tuple(shape) or out.dtype != torch.float32
            or not out.is_contiguous() or (not_same_as is not None and out.data_ptr() == not_same_as.data_ptr())):
        raise EpcNetError(-1, "%s: `out` must be a contiguous float32 device tensor %s%s"
                          % (who, what, "" if not_same_as is None else ", and not points itself"))
    return out


def _spare(dev, dtype=torch.float32):
    """For an empty input: a pointer the library can check (96 zero bytes of its own; nothing of them is touched)."""
    return torch.zeros(12, dtype=torch.float64, device=dev).view(dtype)


def morton_sort(xyz):
    """Order every cloud of (B, N, 3) along the Hilbert curve (epc_morton_sort): a pure re-ordering, legal because the whole network is
    permutation-equivariant and the pooling invariant; it makes the kNN culling and the gathers cache-local."""
    L.require_gpu()
    xyz = xyz.contiguous().float()
    if xyz.shape[1] > 16384:
        return xyz
    out = torch.empty_like(xyz)
    L.run.epc_morton_sort(xyz, xyz.shape[0], xyz.shape[1], out, None)
    return out


def pack_scans(scans, device=None):
    """Host helper: a list of (M_i, 3) arrays (numpy or tensors; any M_i >= 0, a different one per scan) -> ``(points (total, 3)
    float32, offsets (len + 1,) int32)`` as DEVICE tensors, the ragged form ``grid_downsample`` and ``InferenceEngine.forward_scans``
    take."""
    L.require_gpu()
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise EpcNetError(-1, "pack_scans: the scans go to a ROCm device (no CPU fallback)")
    rows = [torch.as_tensor(s, dtype=torch.float32).reshape(-1, 3) for s in scans]
    offsets = [0]
    for r in rows:
        offsets.append(offsets[-1] + int(r.shape[0]))
    if offsets[-1] >= 2 ** 31:
        raise EpcNetError(-1, "pack_scans: %d points do not fit int32 offsets" % offsets[-1])
    points = torch.cat(rows, 0) if rows else torch.zeros((0, 3), dtype=torch.float32)
    return points.to(device), torch.tensor(offsets, dtype=torch.int32).to(device)


def grid_downsample(points, offsets, n, normalize=True, out=None):
    """Ragged raw scans -> exactly ``n`` points per cloud by the grid average of include/epcnet.h (epc_grid_downsample; numpy
    restatement: tests/downsample_ref.py): ``(xyz (B, n, 3) float32, status (B,) int32, info (B, 4) int32)``, all device tensors,
    one launch on the current stream, no host read.  ``points`` (total, 3) float32 and ``offsets`` (B + 1,) int32 are device tensors
    (``pack_scans``); the offsets are read when the kernel runs.  ``normalize``: zero mean inside [-1, 1] (the benchmark's
    convention, what the networks were trained on) or, False, the sensor's units.  A scan without a grid of ``n`` cells gets NaN rows and
    the status word EPC_STATUS_NO_GRID; ``info``: finite points, R*, D(R*), count of the last kept cell.  ``n``: a multiple of 32 in
    [32, 4096]."""
    B, rows, dev = _packed("grid_downsample", points, offsets, "B")
    L.require_gpu()
    n = int(n)
    need = int(L.lib().epc_grid_downsample_workspace_bytes(B, n))
    if need == 0:
        raise EpcNetError(-1, "grid_downsample: n must be a multiple of 32 in [32, 4096], got %d" % n)
    if out is None:
        out = torch.empty((B, n, 3), dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (B, n, 3) or out.dtype != torch.float32:
        raise EpcNetError(-1, "grid_downsample: `out` must be float32 (%d, %d, 3)" % (B, n))
    status = torch.empty(B, dtype=torch.int32, device=dev)
    info = torch.empty((B, 4), dtype=torch.int32, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    L.run.epc_grid_downsample(points if rows else _spare(dev), offsets, B, n, 1 if normalize else 0, L.ptr(out), status, info, ws, ws.numel())
    return out, status, info


def remove_ground(points, offsets, threshold=0.2, max_tilt_deg=15.0, hypotheses=256, draws=8, min_share=0.05, max_z=float("inf"), seed=0,
                  out=None):
    """Ragged raw scans -> the same rows without the ground (include/epcnet_scans.h: epcnet_ground_remove; numpy restatement:
    tests/ground_ref.py): ``(points_out (total, 3) float32, status (B,) int32, plane (B, 4) float32, info (B, 4) int32)``, all device
    tensors, four launches on the current stream, no host read.  Per scan a deterministic plane RANSAC (``hypotheses`` planes, each vertex
    the lowest of ``draws`` hashed rows) finds the largest plane tilted at most ``max_tilt_deg`` against z -- the frame is the sensor's,
    z up -- and below ``max_z`` at the sensor's axis; the rows within ``threshold`` metres of it AND every row below it become NaN
    rows, which ``grid_downsample`` drops: the result goes to ``grid_downsample``, ``InferenceEngine.forward_scans`` or a bank as it is.
    One plane, not a terrain model.  A scan whose best plane holds fewer than 3 or fewer than ``min_share`` of its finite rows gets the
    status word EPC_STATUS_NO_GROUND, a NaN ``plane`` and its rows back unchanged.  ``plane``: n_x, n_y, n_z, d0 (not normalised);
    ``info``: finite rows, valid hypotheses, the best one, its score.  ``out=points`` runs in place.  ``hypotheses``: a multiple of 64
    in [64, 1024]; ``draws`` in [1, 16]."""
    B, rows, dev = _packed("remove_ground", points, offsets, "B")
    L.require_gpu()
    H = int(hypotheses)
    need = int(L.lib().epcnet_ground_workspace_bytes(B, H, rows))
    if need == 0:
        raise EpcNetError(-1, "remove_ground: hypotheses must be a multiple of 64 in [64, 1024] and B <= 65535, got %d and %d" % (H, B))
    if not 0.0 <= float(max_tilt_deg) < 90.0:
        raise EpcNetError(-1, "remove_ground: max_tilt_deg must be in [0, 90), got %r" % (max_tilt_deg,))
    cos2 = math.cos(math.radians(float(max_tilt_deg))) ** 2         # in double; the call rounds it once to float32
    out = _out_like("remove_ground", out, points.shape, dev, "of points' shape")
    status = torch.empty(B, dtype=torch.int32, device=dev)
    plane = torch.empty((B, 4), dtype=torch.float32, device=dev)
    info = torch.empty((B, 4), dtype=torch.int32, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    src, dst = points, out
    if rows == 0:
        src = dst = _spare(dev)
    L.run.epcnet_ground_remove(src, offsets, rows, B, H, int(draws), float(threshold), cos2, float(max_z), float(min_share), int(seed),
                               dst, plane, info, status, ws, ws.numel())
    return out, status, plane, info


def build_submaps(points, offsets, poses, along=None, length=20.0, spacing=10.0, min_range=0.0, max_range=100.0, z_min=float("-inf"),
                  z_max=float("inf"), max_submaps=None, out_rows=None, out=None, return_along=False):
    """Posed scans -> travel-length submaps (include/epcnet_submaps.h: epcnet_submap_build; numpy restatement: tests/submap_ref.py):
    ``(sub_points (out_rows, 3) float32, sub_offsets (max_submaps + 1,) int32, status (max_submaps,) int32, sub_pose (max_submaps, 12)
    float64, info (max_submaps, 4) int32, num_out (2,) int32)``, all device tensors, on the current stream, no host read, capturable.
    ``points`` / ``offsets``: the packed scans of ``pack_scans`` in the order they were taken; ``poses``: (S, 12) or (S, 3, 4) FLOAT64
    device tensor, row-major ``[R | t]`` sensor to world -- any other dtype is refused, never converted (float32 UTM coordinates are
    0.5 m apart); ``along`` (S,) float64: the travelled distance at each scan, non-decreasing; ``None`` computes the running sum of
    ``|t_i - t_(i-1)|`` with torch in float64 on the device (outside the header's bit-for-bit contract; ``return_along=True`` appends
    it to the result).

    Submap k covers the scans whose ``along`` lies in ``[along[0] + k * spacing, along[0] + k * spacing + length)`` and is expressed in
    the frame of the first scan at or behind its middle (``sub_pose[k]``; ``sub_pose[:, [3, 7]]`` is the (T, 2) array
    ``Trainer(poses=)``, ``PoseTuples`` and ``retrieval.truth_from_poses`` take).  A row goes (three NaN words, which ``remove_ground``
    and ``grid_downsample`` treat as absent; nothing is compacted) when its range in the SENSOR frame is below ``min_range``, its x-y
    distance from the submap's origin is above ``max_range`` (default 100 m: beyond what a spinning automotive sensor returns, so that
    only non-finite and runaway rows go; must be finite) or its z in the submap's frame is outside ``[z_min, z_max]``.
    ``sub_points, sub_offsets`` go to ``remove_ground``, ``grid_downsample`` or ``InferenceEngine.forward_scans`` as they are;
    ground removal also works per scan before this call (its NaN rows pass through as NaN rows).

    ``status``: 0, EPC_STATUS_NO_SUBMAP (the slot lies behind the trajectory's end, or the whole call failed: bad offsets, a
    non-finite or decreasing ``along``, no scan) or EPC_STATUS_NO_ROOM (more than 2^20 rows, or ``out_rows`` is full: zero rows).
    ``info``: lo, hi, ref, rows per slot; ``num_out``: the submaps among the slots, and whether the trajectory holds more.  The
    capacities default to LOOSE upper bounds by design -- ``max_submaps = S`` (at most 65535) and ``out_rows = rows * (ceil(length /
    spacing) + 1)`` -- because the true numbers are device data; a long trajectory should pass its own."""
    S, rows, dev = _packed("build_submaps", points, offsets, "S")
    _device_tensor("build_submaps", "poses", poses, torch.float64)
    if along is not None:
        _device_tensor("build_submaps", "along", along, torch.float64)
    if tuple(poses.shape) not in ((S, 12), (S, 3, 4)):
        raise EpcNetError(-1, "build_submaps: poses must be (%d, 12) or (%d, 3, 4) = [R | t] per scan, got %s" % (S, S, tuple(poses.shape)))
    poses = poses.reshape(S, 12)
    L.require_gpu()
    if along is None:
        t = poses[:, 3::4]
        along = torch.zeros(S, dtype=torch.float64, device=dev)
        if S > 1:
            along[1:] = torch.cumsum((t[1:] - t[:-1]).square().sum(1).sqrt(), 0)
    elif tuple(along.shape) != (S,):
        raise EpcNetError(-1, "build_submaps: along must be (%d,), got %s" % (S, tuple(along.shape)))
    values = [float(v) for v in (length, spacing, min_range, max_range, z_min, z_max)]
    if not (math.isfinite(values[0]) and values[0] > 0 and math.isfinite(values[1]) and values[1] > 0):
        raise EpcNetError(-1, "build_submaps: length and spacing must be finite and > 0, got %r and %r" % (length, spacing))
    if max_submaps is None:
        max_submaps = min(max(S, 1), 65535)
    if out_rows is None:
        out_rows = out.shape[0] if torch.is_tensor(out) else rows * (math.ceil(values[0] / values[1]) + 1)
    max_submaps, out_rows = int(max_submaps), int(out_rows)
    need = int(L.lib().epcnet_submap_workspace_bytes(S, max_submaps, rows, out_rows))
    if need == 0:
        raise EpcNetError(-1, "build_submaps: need S <= 2^24, 1 <= max_submaps <= 65535 and 0 <= out_rows < 2^31, got %d, %d and %d "
                              "(pass max_submaps / out_rows for a long trajectory)" % (S, max_submaps, out_rows))
    out = _out_like("build_submaps", out, (out_rows, 3), dev, "of shape (%d, 3)" % out_rows)
    sub_offsets = torch.empty(max_submaps + 1, dtype=torch.int32, device=dev)
    status = torch.empty(max_submaps, dtype=torch.int32, device=dev)
    sub_pose = torch.empty((max_submaps, 12), dtype=torch.float64, device=dev)
    info = torch.empty((max_submaps, 4), dtype=torch.int32, device=dev)
    num_out = torch.empty(2, dtype=torch.int32, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    params = (ctypes.c_double * L.EPC_SUBMAP_PARAMS)(*values, 0.0, 0.0)  # (lib.run passes ctypes objects on: the header's `const double* params` in host memory)
    L.run.epcnet_submap_build(points if rows else _spare(dev), offsets, rows, S, poses if S else _spare(dev, torch.float64),
                              along if S else _spare(dev, torch.float64), params, max_submaps, out_rows, out if out_rows else _spare(dev),
                              sub_offsets, num_out, sub_pose, info, status, ws, ws.numel())
    result = (out, sub_offsets, status, sub_pose, info, num_out)
    return result + (along,) if return_along else result


def _map_arguments(who, points, offsets, poses, voxel, origin, max_voxels, min_count, size_query):
    """The checks and defaults that fuse_map and fuse_surfels share -> ``(C, rows, dev, poses (C, 12), origin, max_voxels, voxel,
    min_count, need)``; ``size_query``: a name of the library's workspace query (looked up after the GPU is required)."""
    C, rows, dev = _packed(who, points, offsets, "C")
    _device_tensor(who, "poses", poses, torch.float64)
    if tuple(poses.shape) not in ((C, 12), (C, 3, 4)):
        raise EpcNetError(-1, "%s: poses must be (%d, 12) or (%d, 3, 4) = [R | t] per cloud, got %s" % (who, C, C, tuple(poses.shape)))
    poses = poses.reshape(C, 12)
    if origin is None:
        origin = poses[0, 3::4].clone() if C else torch.zeros(3, dtype=torch.float64, device=dev)
    else:
        _device_tensor(who, "origin", origin, torch.float64, (3,))
    L.require_gpu()
    if max_voxels is None:
        max_voxels = min(max(rows, 1), 2 ** 28)
    max_voxels, voxel, min_count = int(max_voxels), float(voxel), int(min_count)
    need = int(getattr(L.lib(), size_query)(rows, C, max_voxels))
    if need == 0:
        raise EpcNetError(-1, "%s: need fewer than 2^31 rows, C <= 2^24 and 1 <= max_voxels <= 2^28, got %d, %d and %d" % (who, rows, C, max_voxels))
    if not (math.isfinite(voxel) and 2.0 ** -20 <= voxel <= 2.0 ** 20 and 1 <= min_count < 2 ** 31):
        raise EpcNetError(-1, "%s: need 2^-20 <= voxel <= 2^20 and 1 <= min_count < 2^31, got %r and %r" % (who, voxel, min_count))
    return C, rows, dev, poses, origin, max_voxels, voxel, min_count, need


def fuse_map(points, offsets, poses, voxel=0.2, origin=None, max_voxels=None, min_count=1, workspace=None):
    """Posed clouds -> ONE voxel map in one frame (include/epcnet_maps.h: epcnet_map_fuse; numpy restatement: tests/map_ref.py):
    ``(map_points (max_voxels, 3) float32, count (max_voxels,) int32, num_out (4,) int32, origin (3,) float64)``, all device tensors, on
    the current stream, no host read, capturable.  ``points`` / ``offsets``: packed ragged clouds -- the ``sub_points, sub_offsets`` of
    ``build_submaps``, with or without ``remove_ground``; NaN rows are absent --; ``poses``: (C, 12) or (C, 3, 4) FLOAT64 device tensor,
    row-major ``[R | t]`` cloud to world -- ``sub_pose``, or what ``close_loops`` returns; any other dtype is refused, never converted
    (float32 UTM coordinates are 0.5 m apart).  ``origin`` (3,) float64 device tensor: the world point the map is relative to; ``None``
    takes the first pose's translation (a device copy).

    Every row is moved by its cloud's pose in float64 and falls into a cube of ``voxel`` metres; voxel j -- numbered by the first source
    row that fell into it -- yields the mean of its rows' positions (on a lattice of ``voxel / 4096``, summed in integers: the same
    bits on every run) as ``map_points[j]`` and their number as ``count[j]``.  A voxel of fewer than ``min_count`` rows (something that
    passed by) and every row behind the last voxel are NaN rows, which ``grid_downsample`` and ``retrieval.register_pairs`` treat as
    absent: the map goes to them as it is (a new submap is registered against the map like against a submap).  Nothing is compacted.
    ``num_out``: voxels, rows kept, rows absent, rows out of range (more than 2^20 voxels from the origin); ``num_out[0] == -1`` with
    an all-NaN map: more than ``max_voxels`` voxels, or invalid offsets.  ``max_voxels=None`` is the LOOSE bound ``min(max(rows, 1),
    2^28)`` -- the true number is device data --; ``workspace``: a uint8 device tensor of at least ``epcnet_map_fuse_workspace_bytes``
    bytes to reuse (what a captured graph needs), else one is allocated."""
    who = "fuse_map"
    C, rows, dev, poses, origin, max_voxels, voxel, min_count, need = _map_arguments(
        who, points, offsets, poses, voxel, origin, max_voxels, min_count, "epcnet_map_fuse_workspace_bytes")
    ws, own = _workspace(who, need, workspace, dev)
    map_points = torch.empty((max_voxels, 3), dtype=torch.float32, device=dev)
    count = torch.empty(max_voxels, dtype=torch.int32, device=dev)
    num_out = torch.empty(4, dtype=torch.int32, device=dev)
    params = (ctypes.c_double * L.EPC_MAP_PARAMS)(voxel, float(min_count))       # (host memory; the six reserved doubles are 0)
    L.run.epcnet_map_fuse(points if rows else _spare(dev), offsets, rows, C, poses if C else _spare(dev, torch.float64), origin, params,
                          max_voxels, map_points, count, num_out, ws, ws.numel())
    if own:
        ws.record_stream(torch.cuda.current_stream(dev))
    return map_points, count, num_out, origin


def fuse_surfels(points, offsets, poses, voxel=0.2, origin=None, max_voxels=None, min_count=1, ring=1, min_support=8, workspace=None):
    """``fuse_map`` with a SURFEL per voxel (include/epcnet_surfels.h: epcnet_map_surfels; numpy restatement: tests/surfel_ref.py):
    ``(map_points, count, centroid (max_voxels, 3) float32, normal (max_voxels, 3) float32, eigen (max_voxels, 3) float32, support
    (max_voxels,) int32, num_out, origin)``, all device tensors, on the current stream, no host read, capturable.  The arguments, their
    checks and defaults, ``map_points``, ``count``, ``num_out`` and ``origin`` are ``fuse_map``'s, bit for bit.

    A voxel's own two or three rows carry no covariance: the statistics of voxel j are pooled over the ``(2 ring + 1)^3`` cells around
    it (``ring`` in 0..2), from those that hold at least ``min_count`` rows, as integer moments on a lattice of ``voxel / 256`` -- the
    same bits on every run.  ``support[j]`` is the number of rows pooled.  Where ``count[j] >= min_count`` and ``support[j] >=
    min_support`` (at least 3), ``centroid[j]`` is their mean in metres relative to ``origin``, ``eigen[j]`` the eigenvalues of their
    covariance in m^2, ascending (flat: the first is small against the others), and ``normal[j]`` the unit eigenvector of the smallest,
    in the map's axes, its largest component positive (NOT oriented towards a viewpoint); elsewhere the three are NaN rows.
    ``workspace``: a uint8 device tensor of at least ``epcnet_map_surfels_workspace_bytes`` bytes to reuse, else one is allocated."""
    who = "fuse_surfels"
    C, rows, dev, poses, origin, max_voxels, voxel, min_count, need = _map_arguments(
        who, points, offsets, poses, voxel, origin, max_voxels, min_count, "epcnet_map_surfels_workspace_bytes")
    if ring != int(ring) or not 0 <= int(ring) <= L.EPC_SURFEL_MAX_RING or min_support != int(min_support) or not 3 <= int(min_support) < 2 ** 31:
        raise EpcNetError(-1, "%s: need an integer ring in [0, %d] and 3 <= min_support < 2^31, got %r and %r"
                          % (who, L.EPC_SURFEL_MAX_RING, ring, min_support))
    ws, own = _workspace(who, need, workspace, dev)
    map_points, centroid, normal, eigen = (torch.empty((max_voxels, 3), dtype=torch.float32, device=dev) for _ in range(4))
    count, support = (torch.empty(max_voxels, dtype=torch.int32, device=dev) for _ in range(2))
    num_out = torch.empty(4, dtype=torch.int32, device=dev)
    params = (ctypes.c_double * L.EPC_SURFEL_PARAMS)(voxel, float(min_count), float(int(ring)), float(int(min_support)))   # (host memory)
    L.run.epcnet_map_surfels(points if rows else _spare(dev), offsets, rows, C, poses if C else _spare(dev, torch.float64), origin, params,
                             max_voxels, map_points, count, centroid, normal, eigen, support, num_out, ws, ws.numel())
    if own:
        ws.record_stream(torch.cuda.current_stream(dev))
    return map_points, count, centroid, normal, eigen, support, num_out, origin


def _max_gap_ns(who, max_gap):
    ns = int(round(float(max_gap) * 1e9))
    if not 1 <= ns < 2 ** 31:
        raise EpcNetError(-1, "%s: max_gap must lie in [1e-9, 2.147] seconds, got %r" % (who, max_gap))
    return ns


def _odometry(who, pose_time, pose):
    _device_tensor(who, "pose_time", pose_time, torch.int64)
    if pose_time.dim() != 1:
        raise EpcNetError(-1, "%s: pose_time must be (P,), got %s" % (who, tuple(pose_time.shape)))
    P = int(pose_time.numel())
    _device_tensor(who, "pose", pose, torch.float64, (P, 7))
    if not 2 <= P <= 2 ** 24:
        raise EpcNetError(-1, "%s: need 2 <= P <= 2^24 poses, got %d" % (who, P))
    return P


def interpolate_poses(pose_time, pose, query_time, max_gap=0.5):
    """Odometry at other stamps (include/epcnet_stamps.h: epcnet_pose_interp; numpy restatement: tests/stamps_ref.py): ``(poses (Q, 12)
    float64, status (Q,) int32)``, device tensors, on the current stream, no host read, capturable.  ``pose_time`` (P,) INT64 nanoseconds,
    strictly increasing; ``pose`` (P, 7) FLOAT64 ``tx ty tz qw qx qy qz`` sensor to world; ``query_time`` (Q,) int64 nanoseconds.  Float
    stamps are refused, never converted.  Row i is ``[R | t]`` at ``query_time[i]`` -- what ``build_submaps`` takes --: the translation
    interpolated linearly, the rotation by normalised linear interpolation on the shorter arc.  Nothing is extrapolated and no bracket
    longer than ``max_gap`` seconds is interpolated across: such a query gets a NaN pose and EPC_STATUS_NO_POSE (every query does when
    ``pose_time`` is not strictly increasing)."""
    who = "interpolate_poses"
    P = _odometry(who, pose_time, pose)
    _device_tensor(who, "query_time", query_time, torch.int64)
    if query_time.dim() != 1:
        raise EpcNetError(-1, "%s: query_time must be (Q,), got %s" % (who, tuple(query_time.shape)))
    gap = _max_gap_ns(who, max_gap)
    L.require_gpu()
    Q, dev = int(query_time.numel()), pose.device
    if Q > 2 ** 24:
        raise EpcNetError(-1, "%s: need Q <= 2^24 queries, got %d" % (who, Q))
    out = torch.empty((Q, 12), dtype=torch.float64, device=dev)
    status = torch.empty(Q, dtype=torch.int32, device=dev)
    if Q:
        L.run.epcnet_pose_interp(pose_time, pose, P, query_time, Q, gap, out, status)
    return out, status


def deskew_scans(points, offsets, scan_time, pose_time, pose, point_dt=None, max_gap=0.5, out=None):
    """Timestamped scans -> the pose of every scan and, with ``point_dt``, the rows of every sweep moved into the sensor frame of the
    sweep's own stamp (include/epcnet_stamps.h: epcnet_scan_deskew; numpy restatement: tests/stamps_ref.py): ``(points_out (total, 3)
    float32 or None, scan_pose (S, 12) float64, status (S,) int32)``, device tensors, on the current stream, no host read, capturable.
    ``points`` / ``offsets``: the packed scans of ``pack_scans``; ``scan_time`` (S,) INT64 nanoseconds: the instant each scan is
    expressed in afterwards (typically the sweep's start); ``point_dt`` (total,) INT32 nanoseconds from the scan's time, may be
    negative; ``None`` (a 2-D line scanner) only interpolates and returns ``None`` for the points; ``pose_time`` (P,) int64, strictly
    increasing, and ``pose`` (P, 7) FLOAT64 ``tx ty tz qw qx qy qz``: the odometry on its own clock.  Float stamps and float32 poses are
    refused, never converted.  ``scan_pose`` is what ``build_submaps`` takes as ``poses``, ``travel_along(scan_pose, status)`` its
    ``along``.

    ``status``: EPC_STATUS_NO_POSE -- the scan's time lies outside the odometry or inside a bracket longer than ``max_gap`` seconds (or
    the whole call failed: bad offsets, ``pose_time`` not strictly increasing): NaN pose, NaN rows --, EPC_STATUS_PART_POSE: some rows
    had no pose at their own time and became NaN rows.  Nothing is compacted: ``offsets`` goes on with ``points_out``.  ``out`` must
    not be ``points``."""
    who = "deskew_scans"
    S, rows, dev = _packed(who, points, offsets, "S", offsets_hint=None)
    _device_tensor(who, "scan_time", scan_time, torch.int64, (S,))
    P = _odometry(who, pose_time, pose)
    if point_dt is not None:
        _device_tensor(who, "point_dt", point_dt, torch.int32, (rows,))
    elif out is not None:
        raise EpcNetError(-1, "%s: `out` without point_dt: nothing is de-skewed" % who)
    gap = _max_gap_ns(who, max_gap)
    L.require_gpu()
    need = int(L.lib().epcnet_deskew_workspace_bytes(S, P, rows))
    if need == 0:
        raise EpcNetError(-1, "%s: need S <= 2^24 scans and fewer than 2^31 rows, got %d and %d" % (who, S, rows))
    if point_dt is not None:
        out = _out_like(who, out, points.shape, dev, "of points' shape", not_same_as=points)
    scan_pose = torch.empty((S, 12), dtype=torch.float64, device=dev)
    status = torch.empty(S, dtype=torch.int32, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    src, dst, dt, st_ = points, out, point_dt, scan_time
    if rows == 0:                                                    # (points_out must not be points: a spare each)
        src = _spare(dev)
        dst = None if point_dt is None else _spare(dev)
        dt = None if point_dt is None else _spare(dev, torch.int32)
    if S == 0:
        st_ = _spare(dev, torch.int64)
        scan_pose_arg, status_arg = _spare(dev, torch.float64), _spare(dev, torch.int32)
    else:
        scan_pose_arg, status_arg = scan_pose, status
    L.run.epcnet_scan_deskew(src, offsets, rows, S, dt, st_, pose_time, pose, P, gap, dst, scan_pose_arg, status_arg, ws, ws.numel())
    return out, scan_pose, status


def travel_along(poses12, status=None):
    """The travelled distance at each scan from poses that may have gaps: ``along`` (S,) float64 for ``build_submaps``, built with torch
    in float64 on the device, no host read, capturable (like ``build_submaps``' own ``along=None`` it lies outside the headers'
    bit-for-bit contracts).  ``poses12``: (S, 12) or (S, 3, 4) float64 ``[R | t]``; ``status`` (S,) int32 or None.  A scan is VALID when
    its translation is finite and its status lacks EPC_STATUS_NO_POSE.  The result is the running sum of the steps between consecutive
    valid scans' translations; an invalid scan takes the value of the last valid scan before it, 0 if there is none.
    (``build_submaps(along=None)`` turns one NaN pose into a whole-call failure: pass this instead.)"""
    who = "travel_along"
    _device_tensor(who, "poses12", poses12, torch.float64)
    S = int(poses12.shape[0]) if poses12.dim() else -1
    if tuple(poses12.shape) not in ((S, 12), (S, 3, 4)):
        raise EpcNetError(-1, "%s: poses12 must be (S, 12) or (S, 3, 4), got %s" % (who, tuple(poses12.shape)))
    t = poses12.reshape(S, 12)[:, 3::4]
    valid = torch.isfinite(t).all(1)
    if status is not None:
        _device_tensor(who, "status", status, torch.int32, (S,))
        valid = valid & ((status & L.EPC_STATUS_NO_POSE) == 0)
    along = torch.zeros(S, dtype=torch.float64, device=poses12.device)
    if S > 1:
        index = torch.arange(S, device=poses12.device)
        last = torch.cummax(torch.where(valid, index, torch.full_like(index, -1)), 0).values      # the last valid scan at or before i
        prev = last[:-1]                                                 # ... strictly before scan i, for i = 1 .. S - 1
        safe = torch.where(valid[:, None], t, torch.zeros_like(t))
        step = (safe[1:] - safe[prev.clamp(min=0)]).square().sum(1).sqrt()
        step = torch.where(valid[1:] & (prev >= 0), step, torch.zeros_like(step))
        along[1:] = torch.cumsum(step, 0)
    return along


def _device_poses(name, poses, device=None):
    """(rows, 2) float64 poses (numpy or torch, host or device) -> a contiguous device tensor.  Any other dtype is refused, not
    converted: float32 has a 0.5 m spacing at UTM northings, and a silent round trip through it would move the relations."""
    if isinstance(poses, np.ndarray):
        if poses.dtype != np.float64:
            raise EpcNetError(-1, "%s: poses must be float64, got %s (float32 UTM coordinates are 0.5 m apart)" % (name, poses.dtype))
        poses = torch.from_numpy(np.ascontiguousarray(poses))
    if not torch.is_tensor(poses) or poses.dtype != torch.float64:
        raise EpcNetError(-1, "%s: poses must be a float64 numpy array or tensor, got %s"
                          % (name, poses.dtype if torch.is_tensor(poses) else type(poses).__name__))
    if poses.dim() != 2 or int(poses.shape[1]) != 2:
        raise EpcNetError(-1, "%s: poses must be (rows, 2) = (northing, easting), got %s" % (name, tuple(poses.shape)))
    L.require_gpu()
    if device is None:
        device = poses.device if poses.is_cuda else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise EpcNetError(-1, "%s: the poses go to a ROCm device (no CPU fallback)" % name)
    return poses.to(device).contiguous()


def _radius(r):
    return ctypes.c_double(float(r))       # (lib.run passes ctypes objects on: the header's `const double* radius` in host memory)


def pose_radius_lists(query_poses, db_poses, r, width=None, device=None):
    """For each of the Q query poses the indices of the D database poses within ``r`` (inclusive, as sklearn's
    ``KDTree.query_radius``; generate_test_sets.py:95-104), ascending: ``(padded (Q, width) int32, lens (Q,) int32)`` on the device,
    rows padded with -2 -- the tables of ``retrieval.PackedTruth``.  Poses: (rows, 2) float64, numpy or torch.  ``width=None``: the
    longest row's length (at least 1), from a count pass and ONE read of its maximum; a given ``width`` costs no host read, and a row
    that does not fit raises ``EpcNetError`` (after a read of the status word) -- ``lens`` always holds the full lengths."""
    q = _device_poses("pose_radius_lists", query_poses, device)
    d = _device_poses("pose_radius_lists", db_poses, q.device)
    Q, D, rad = int(q.shape[0]), int(d.shape[0]), _radius(r)
    lens = torch.zeros(Q, dtype=torch.int32, device=q.device)
    if Q == 0 or D == 0:
        return torch.full((Q, max(int(width or 1), 1)), -2, dtype=torch.int32, device=q.device), lens
    with torch.cuda.device(q.device):
        given = width is not None
        if not given:
            L.run.epcnet_pose_radius_count(q, Q, d, D, ctypes.byref(rad), lens)
            width = max(int(lens.max().item()), 1)
        width = int(width)
        if width <= 0:
            raise EpcNetError(-1, "pose_radius_lists: width must be positive")
        padded = torch.empty((Q, width), dtype=torch.int32, device=q.device)
        status = torch.zeros(1, dtype=torch.int32, device=q.device)
        L.run.epcnet_pose_radius_fill(q, Q, d, D, ctypes.byref(rad), width, lens, padded, status)
        if given and int(status.item()) != 0:
            raise EpcNetError(-1, "pose_radius_lists: a row holds %d entries, width is %d (the lists were truncated)"
                              % (int(lens.max().item()), width))
    return padded, lens


class PoseTuples:
    """Training tuples drawn on the device from the records' poses (include/epcnet_poses.h;
    numpy restatement: tests/tuples_ref.py) -- what generate_training_tuples_baseline.py's pickles and
    ``loading_pointclouds.get_query_tuple_ids`` do with Python lists, without any list: the (T, 2) float64 poses stay on the device and
    every relation is decided from them when it is needed.  Record i's positives are the other records within ``r_pos`` (inclusive),
    its negatives those strictly beyond ``r_neg``.  ``counts`` (T,) int32: the number of positives per record, computed once.
    The draw is a fixed hash of (seed, step, key, stream, id), so it does not depend on thread order and ``tuples_ref`` draws the same
    tuples; it is NOT Python's ``random`` stream."""

    def __init__(self, poses, r_pos: float = 10.0, r_neg: float = 50.0, seed: int = 0, device=None):
        self.poses = _device_poses("PoseTuples", poses, device)
        self.device = self.poses.device
        self.T = int(self.poses.shape[0])
        if not 0 < self.T <= 1 << 24:
            raise EpcNetError(-1, "PoseTuples: between 1 and 2^24 records, got %d" % self.T)
        self.r_pos, self.r_neg, self.seed = float(r_pos), float(r_neg), int(seed)
        self._rp, self._rn = _radius(self.r_pos), _radius(self.r_neg)
        self.counts = torch.empty(self.T, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            L.run.epcnet_pose_pos_count(self.poses, self.T, ctypes.byref(self._rp), self.counts)
        self._slots = {}             # per batch size: the sticky status words and the key that set them

    def __len__(self) -> int:
        return self.T

    @staticmethod
    def _i64(v: int) -> int:
        v &= (1 << 64) - 1
        return v - (1 << 64) if v >> 63 else v

    def _keys(self, name, keys):
        if not torch.is_tensor(keys) or not keys.is_cuda or keys.dtype != torch.int32 or not keys.is_contiguous() or keys.dim() != 1:
            raise EpcNetError(-1, "PoseTuples.%s: keys must be a contiguous 1-d int32 tensor on the ROCm device" % name)
        B = int(keys.numel())
        if B not in self._slots:
            self._slots[B] = (torch.zeros(B, dtype=torch.int32, device=self.device),
                              torch.full((B,), -1, dtype=torch.int32, device=self.device))
        return B, self._slots[B]

    def candidates(self, keys, step: int, C: int = 4000, out=None):
        """Phase A (epcnet_tuple_candidates): per key the min(C, #negatives) negatives with the smallest (hash, id) of stream 1, ascending by
        id -> ``(cand (B, C) int32, cand_count (B,) int32)``, the buffers ``retrieval.mine_topk`` takes.  ``keys``: (B,) int32 on the
        device, read when the kernel runs.  ``out``: a (cand, cand_count) pair to write into.  One launch, no host read."""
        B, (status, flagged) = self._keys("candidates", keys)
        C = int(C)
        cand, count = out if out is not None else (torch.empty((B, C), dtype=torch.int32, device=self.device),
                                                   torch.empty(B, dtype=torch.int32, device=self.device))
        if tuple(cand.shape) != (B, C) or int(count.numel()) != B or not cand.is_contiguous():
            raise EpcNetError(-1, "PoseTuples.candidates: `out` must be contiguous (B, C) and (B,) int32 tensors")
        with torch.cuda.device(self.device):
            L.run.epcnet_tuple_candidates(self.poses, self.T, keys, B, ctypes.byref(self._rn), self._i64(self.seed), self._i64(int(step)), C,
                                       cand, count, status, flagged)
        return cand, count

    def sample(self, keys, step: int, P: int, Nn: int, hard=None):
        """Phase B (epcnet_tuple_sample): ``(ids (B, 1 + P + Nn + 1) int32, status (B,) int32)`` on the device -- per key {key, P positives,
        Nn negatives, other negative} in ``TrainStep.step_ids``' order.  ``hard`` (B, H <= 32) int32 on the device or None: taken first
        (entries < 0 or >= T and repeats dropped, e.g. ``mine_topk``'s ids as they are), the rest filled from the negatives.  A slot
        that cannot be filled is -1; ``status`` is the sticky word ``check`` reads.  One launch, no host read."""
        B, (status, flagged) = self._keys("sample", keys)
        H = 0
        if hard is not None:
            if not torch.is_tensor(hard) or not hard.is_cuda or hard.dtype != torch.int32 or not hard.is_contiguous() \
                    or hard.dim() != 2 or int(hard.shape[0]) != B:
                raise EpcNetError(-1, "PoseTuples.sample: hard must be a contiguous (B, H) int32 tensor on the ROCm device")
            H = int(hard.shape[1])
        ids = torch.empty((B, 1 + int(P) + int(Nn) + 1), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            L.run.epcnet_tuple_sample(self.poses, self.T, keys, B, ctypes.byref(self._rp), ctypes.byref(self._rn), self._i64(self.seed),
                                   self._i64(int(step)), int(P), int(Nn), hard if H else None, H, ids, status, flagged)
        return ids, status

    KINDS = ((L.EPC_TUPLE_FEW_POSITIVES, "fewer positives than asked for"), (L.EPC_TUPLE_FEW_NEGATIVES, "fewer negatives than asked for"),
             (L.EPC_TUPLE_NO_OTHER, "no eligible other negative"), (L.EPC_TUPLE_BAD_KEY, "key outside the records"))

    def check(self) -> None:
        """Read the status words of every ``candidates`` / ``sample`` since the last check (a device synchronisation) and clear them;
        raises EpcNetError naming, per batch slot, the last key that set a bit and the kinds seen in that slot."""
        bad = []
        for B, (status, flagged) in sorted(self._slots.items()):
            words, keys = status.cpu().tolist(), flagged.cpu().tolist()
            if any(words):
                status.zero_()
                flagged.fill_(-1)
            for b, (w, k) in enumerate(zip(words, keys)):
                if w:
                    bad.append("key %d (slot %d of %d): %s" % (k, b, B, ", ".join(t for bit, t in self.KINDS if w & bit)))
        if bad:
            raise EpcNetError(-1, "PoseTuples: " + "; ".join(bad))
