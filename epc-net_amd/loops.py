"""Loop closing along ONE trajectory of submaps, none of it with a counterpart in the reference: ``revisit_search`` finds the candidates
(``RevisitIndex`` is its streaming form), ``register_pairs`` verifies them geometrically (``verify_revisits`` runs it on the candidates,
``yaw_seeds`` builds hypotheses) and ``relax_trajectory`` relaxes the pose graph (``close_loops`` runs it on what was verified).  Plain
functions over device tensors: contiguous tensors of the exact dtype or a refusal, nothing read back, every call asynchronous and
capturable in a graph.  ``retrieval`` re-exports these names: ``retrieval.revisit_search`` and the rest are this module's."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import lib as L

# whose device every further argument of an entry must be on: the entry's first argument
_FIRST = {"revisit_search": "descriptors", "register_pairs": "clouds", "relax_trajectory": "poses"}


def _check(who: str, name: str, t, dtype, ndim: int, device=None, last=None):
    """The refusals every entry shares: a contiguous device tensor of exactly ``dtype`` -- nothing is converted --, ``ndim``-d, given
    ``last`` with that last dimension and given ``device`` on it."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise L.EpcNetError(-1, "%s: %s must live on a ROCm device (no CPU fallback)" % (who, name))
    if t.dtype != dtype or not t.is_contiguous():
        raise L.EpcNetError(-1, "%s: %s must be a contiguous %s tensor, got %s%s" % (
            who, name, dtype, t.dtype, " (poses are float64: they are refused, never converted)" if dtype == torch.float64 else ""))
    if t.dim() != ndim or (last is not None and int(t.shape[-1]) != last) or (device is not None and t.device != device):
        raise L.EpcNetError(-1, "%s: %s must be %d-d%s on the %s' device, got %s" % (
            who, name, ndim, "" if last is None else " with a last dimension of %d" % last, _FIRST[who], tuple(t.shape)))


def _workspace(who: str, need: int, workspace, dev):
    """``(ws, own)``: the caller's ``workspace`` after the refusal of anything but a contiguous uint8 device tensor, or, for None, one of
    the entry's own of ``need`` bytes (16 at least: its address stands in for empty tensors, ``_arg``).  Its own the entry hands to
    ``record_stream`` behind the launch: the allocator may give it to another stream as soon as the entry returns."""
    if workspace is None:
        return torch.empty(max(need, 16), dtype=torch.uint8, device=dev), True
    if not torch.is_tensor(workspace) or not workspace.is_cuda or workspace.dtype != torch.uint8 or not workspace.is_contiguous():
        raise L.EpcNetError(-1, "%s: workspace must be a contiguous uint8 tensor on the ROCm device" % who)
    return workspace, False


def _arg(ws):
    """What an entry passes for a tensor: an empty tensor has no address, the workspace's (aligned, not null) stands in and is never
    followed."""
    return lambda t: t if t.numel() else ws.data_ptr()


def _pairs_of(idx):
    """``idx`` (Q, k) -> the rows (i, idx[i, j]) as (Q k, 2) int32 in the row-major order of ``idx``: query i is the source."""
    Q, k = int(idx.shape[0]), int(idx.shape[1])
    src = torch.arange(Q, dtype=torch.int32, device=idx.device).unsqueeze(1).expand(Q, k)
    return torch.stack([src, idx], -1).reshape(Q * k, 2).contiguous()


def revisit_search(descriptors: torch.Tensor, along: torch.Tensor, min_travel: float, k: int = 5, *,
                   queries: Optional[torch.Tensor] = None, q_along: Optional[torch.Tensor] = None, pass_queries: int = 0,
                   workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Loop-closure candidates along a trajectory (include/epcnet_revisits.h): for every query the exact ``k`` nearest rows of
    ``descriptors`` (T, D) float32 among those at least ``min_travel`` BEHIND it -- the rows j with ``along[j] <= q_along[i] -
    min_travel`` in float64; ``along`` (T,) float64, non-decreasing (metres from ``ops.travel_along`` or ``k * spacing``, or seconds).
    ``queries`` (Q, D) / ``q_along`` (Q,), both or neither: None searches the trajectory against itself, which is causal for
    ``min_travel > 0`` -- every revisit pair is reported once, by its later member.  Returns (dist (Q, k) float32, idx (Q, k) int32,
    count (Q,) int32): row i is bit for bit ``knn_search(descriptors[:count[i]], queries[i:i + 1], min(k, count[i]))``, padded with
    (+inf, -1); ``count[i] == -1`` (and an all-padding row) for a non-finite ``q_along[i]`` or, in EVERY row, when ``along`` holds a
    non-finite entry or decreases -- decided on the device, nothing is read back, the call is asynchronous and capturable in a graph.
    ``pass_queries`` (0 or a multiple of 128): queries per pass of the distance matrix; ``workspace``: a uint8 device tensor of at least
    ``epcnet_revisit_workspace_bytes`` bytes to reuse (what a captured graph needs), else one is allocated."""
    L.require_gpu()
    who = "revisit_search"
    _check(who, "descriptors", descriptors, torch.float32, 2)
    dev = descriptors.device
    _check(who, "along", along, torch.float64, 1, dev)
    if (queries is None) != (q_along is None):
        raise L.EpcNetError(-1, "revisit_search: queries and q_along come together or not at all")
    if queries is None:
        queries, q_along = descriptors, along
    _check(who, "queries", queries, torch.float32, 2, dev)
    _check(who, "q_along", q_along, torch.float64, 1, dev)
    d, q, dim, k = int(descriptors.shape[0]), int(queries.shape[0]), int(descriptors.shape[1]), int(k)
    if int(queries.shape[1]) != dim or along.numel() != d or q_along.numel() != q:
        raise L.EpcNetError(-1, "revisit_search: expected descriptors (T, D), along (T,), queries (Q, D), q_along (Q,)")
    ws, own = _workspace(who, int(L.lib().epcnet_revisit_workspace_bytes(d, q, int(pass_queries))), workspace, dev)
    idx = torch.empty((q, max(k, 0)), dtype=torch.int32, device=dev)
    dist = torch.empty((q, max(k, 0)), dtype=torch.float32, device=dev)
    count = torch.empty((q,), dtype=torch.int32, device=dev)
    arg = _arg(ws)
    L.run.epcnet_revisit_search(arg(descriptors), arg(along), d, arg(queries), arg(q_along), q, dim, float(min_travel), k,
                                int(pass_queries), arg(idx), arg(dist), arg(count), ws, ws.numel())
    if own:
        ws.record_stream(torch.cuda.current_stream(dev))
    return dist, idx, count


class RevisitIndex:
    """The streaming form of ``revisit_search`` for a robot that adds a submap at a time: ``capacity`` rows of ``dim`` floats and their
    travelled distances, allocated once on the device.  ``add(descriptors, along)`` copies the new rows behind the stored ones and
    searches THEM against everything stored, themselves included -- the prefix rule does the exclusion --, so piecewise adds over a
    trajectory return, concatenated, the bits of the one batch call.  A failed add (``count == -1``: the stored ``along`` decreases or
    holds a non-finite entry) has stored its rows regardless: the caller who checks ``count`` drops them with ``truncate``."""

    def __init__(self, capacity: int, dim: int = 256, min_travel: float = 100.0, k: int = 5, device=None):
        L.require_gpu()
        self.capacity, self.dim, self.min_travel, self.k = int(capacity), int(dim), float(min_travel), int(k)
        if self.capacity < 0 or self.capacity > (1 << 22) or self.dim <= 0 or self.dim % 8 or not 0 < self.k <= 56 \
                or not (self.min_travel >= 0.0 and self.min_travel != float("inf")):
            raise L.EpcNetError(-1, "RevisitIndex: need 0 <= capacity <= 2^22, dim a positive multiple of 8, 0 < k <= 56 and a finite "
                                    "min_travel >= 0")
        self._desc = torch.empty((self.capacity, self.dim), dtype=torch.float32,
                                 device=torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device()))
        self.device = self._desc.device                      # with its index, as every tensor on it reports it
        self._along = torch.empty((self.capacity,), dtype=torch.float64, device=self.device)
        self._n = 0

    def __len__(self) -> int:
        return self._n

    @property
    def descriptors(self) -> torch.Tensor:
        """The stored rows (len, dim): a view of the index's buffer, to be read only."""
        return self._desc[:self._n]

    @property
    def along(self) -> torch.Tensor:
        """The stored travelled distances (len,): a view of the index's buffer, to be read only."""
        return self._along[:self._n]

    def truncate(self, n: int) -> None:
        """Keep the first ``n`` rows (what drops the rows of a failed ``add``)."""
        n = int(n)
        if n < 0 or n > self._n:
            raise L.EpcNetError(-1, "RevisitIndex.truncate: %d is outside [0, %d]" % (n, self._n))
        self._n = n

    def add(self, descriptors: torch.Tensor, along: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """New rows (m, dim) float32 with their ``along`` (m,) float64 -> (dist, idx, count) of ``revisit_search`` for them."""
        _check("revisit_search", "descriptors", descriptors, torch.float32, 2, self.device)
        _check("revisit_search", "along", along, torch.float64, 1, self.device)
        m = int(descriptors.shape[0])
        if int(descriptors.shape[1]) != self.dim or along.numel() != m:
            raise L.EpcNetError(-1, "RevisitIndex.add: expected descriptors (m, %d) and along (m,)" % self.dim)
        if self._n + m > self.capacity:
            raise L.EpcNetError(-1, "RevisitIndex.add: %d rows on top of %d exceed the capacity %d (the index never reallocates)"
                                % (m, self._n, self.capacity))
        a, b = self._n, self._n + m
        self._desc[a:b].copy_(descriptors)
        self._along[a:b].copy_(along)
        self._n = b
        return revisit_search(self._desc[:b], self._along[:b], self.min_travel, self.k, queries=self._desc[a:b], q_along=self._along[a:b])


def register_pairs(clouds: torch.Tensor, pairs: torch.Tensor, seeds: Optional[torch.Tensor] = None, max_dist: float = 1.0,
                   iterations: int = 16, min_pairs: int = 32, workspace: Optional[torch.Tensor] = None):
    """Geometric verification of candidate pairs (include/epcnet_pairs.h): for every row (source, target) of ``pairs`` (P, 2) int32 the
    rigid alignment of cloud ``source`` onto cloud ``target`` by point-to-point ICP, and how well the two fit.  ``clouds`` (C, n, 3)
    float32 in METRIC units (``ops.grid_downsample(..., normalize=False)``; a row with a non-finite word is absent; n a multiple of 32 in
    [32, 4096]); ``seeds`` (P, H, 12) float64 row-major ``[R | t]`` source -> target hypotheses, None = the identity: the seed with the
    most correspondences within ``max_dist`` metres is refined ``iterations`` times.  Returns ``(pose (P, 12) float64, fit (P, 2)
    float64: mean squared residual and overlap, info (P, 4) int32: best seed, correspondences, source rows, target rows, status (P,)
    int32)``; EPC_STATUS_NO_PAIR: an index outside [0, C) -- the -1 of ``revisit_search`` -- or no finite seed; EPC_STATUS_NO_FIT: fewer
    than ``min_pairs`` correspondences; both leave a NaN pose and fit.  Bit for bit tests/register_ref.py; only contiguous device tensors
    of the exact dtype are taken, float32 seeds are refused, never converted; nothing is read back, the call is asynchronous and
    capturable in a graph.  ``workspace``: a uint8 device tensor of at least ``epcnet_pair_register_workspace_bytes`` bytes to reuse
    (what a captured graph needs), else one is allocated."""
    L.require_gpu()
    who = "register_pairs"
    _check(who, "clouds", clouds, torch.float32, 3, None, 3)
    dev = clouds.device
    _check(who, "pairs", pairs, torch.int32, 2, dev, 2)
    C, n, P = int(clouds.shape[0]), int(clouds.shape[1]), int(pairs.shape[0])
    H = 1
    if seeds is not None:
        _check(who, "seeds", seeds, torch.float64, 3, dev, 12)
        H = int(seeds.shape[1])
        if int(seeds.shape[0]) != P:
            raise L.EpcNetError(-1, "register_pairs: seeds must be (P, H, 12) for pairs (P, 2), got %s" % (tuple(seeds.shape),))
    ws, own = _workspace(who, int(L.lib().epcnet_pair_register_workspace_bytes(P, H, n)), workspace, dev)
    pose = torch.empty((P, 12), dtype=torch.float64, device=dev)
    fit = torch.empty((P, 2), dtype=torch.float64, device=dev)
    info = torch.empty((P, 4), dtype=torch.int32, device=dev)
    status = torch.empty((P,), dtype=torch.int32, device=dev)
    arg = _arg(ws)
    L.run.epcnet_pair_register(arg(clouds), C, n, arg(pairs), P, None if seeds is None else arg(seeds), H, float(max_dist), int(iterations),
                               int(min_pairs), arg(pose), arg(fit), arg(info), arg(status), ws, ws.numel())
    if own:
        ws.record_stream(torch.cuda.current_stream(dev))
    return pose, fit, info, status


def yaw_seeds(num: int, base: Optional[torch.Tensor] = None, device=None) -> torch.Tensor:
    """``num`` hypotheses that differ by a turn about z: ``base @ Rz(2 pi m / num)``, m = 0 .. num - 1, as (..., num, 12) float64 for a
    ``base`` (..., 12) float64 (None: the identity, on ``device``) -- a revisit driven in the other direction is seed num / 2.  Built
    with torch in float64: outside the bit contract, like ``ops.travel_along``; ``register_pairs``' contract is seeds -> result."""
    num = int(num)
    if num < 1 or num > 64:
        raise L.EpcNetError(-1, "yaw_seeds: 1 <= num <= 64")
    if base is None:
        base = torch.tensor([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=torch.float64, device=device)
    if not torch.is_tensor(base) or base.dtype != torch.float64 or base.shape[-1] != 12:
        raise L.EpcNetError(-1, "yaw_seeds: base must be a float64 tensor (..., 12)")
    a = torch.arange(num, dtype=torch.float64, device=base.device) * (2.0 * np.pi / num)
    c, s, o, l = torch.cos(a), torch.sin(a), torch.zeros_like(a), torch.ones_like(a)
    c[0], s[0] = 1.0, 0.0                                                    # m = 0 is the base itself, to the bit
    rz = torch.stack([c, -s, o, o, s, c, o, o, o, o, l, o, o, o, o, l], -1).reshape(num, 4, 4)
    m = base.reshape(base.shape[:-1] + (3, 4))
    return (m.unsqueeze(-3) @ rz).reshape(base.shape[:-1] + (num, 12)).contiguous()


def verify_revisits(clouds: torch.Tensor, idx: torch.Tensor, sub_pose: Optional[torch.Tensor] = None, yaw: int = 1, **kw):
    """``register_pairs`` on the candidates of ``revisit_search``: ``clouds`` (T, n, 3) float32 metric (``forward_trajectory(...,
    clouds=True)``), ``idx`` (Q, k) int32 with Q <= T -- query i is cloud i -- -> the pairs (i, idx[i, j]), formed on the device.  With
    ``sub_pose`` (T, 12) float64 every pair is seeded with the odometry's relative pose ``inv(sub_pose[idx[i, j]]) @ sub_pose[i]``, else
    with the identity; ``yaw`` > 1 multiplies the seed by ``yaw_seeds(yaw)``.  Returns ``(pose (Q, k, 12), fit (Q, k, 2), info (Q, k, 4),
    status (Q, k))``; a -1 of ``idx`` (and a NaN ``sub_pose``) is flagged EPC_STATUS_NO_PAIR.  No host read; ``kw`` goes to
    ``register_pairs``."""
    _check("register_pairs", "idx", idx, torch.int32, 2, clouds.device if torch.is_tensor(clouds) else None)
    Q, k = int(idx.shape[0]), int(idx.shape[1])
    dev = idx.device
    if not torch.is_tensor(clouds) or clouds.dim() != 3 or Q > int(clouds.shape[0]) or (
            sub_pose is not None and torch.is_tensor(sub_pose) and sub_pose.dim() == 2 and int(sub_pose.shape[0]) != int(clouds.shape[0])):
        raise L.EpcNetError(-1, "verify_revisits: expected clouds (T, n, 3), idx (Q, k) with Q <= T and sub_pose (T, 12)")
    pairs = _pairs_of(idx)
    seeds = None
    if sub_pose is not None:
        _check("register_pairs", "sub_pose", sub_pose, torch.float64, 2, dev, 12)
        m = sub_pose.reshape(-1, 3, 4)
        bottom = torch.tensor([0, 0, 0, 1], dtype=torch.float64, device=dev).expand(m.shape[0], 1, 4)
        inv = torch.cat([m[:, :, :3].transpose(1, 2), -(m[:, :, :3].transpose(1, 2) @ m[:, :, 3:])], 2)
        tgt = idx.reshape(-1).to(torch.int64).clamp(min=0, max=max(m.shape[0] - 1, 0))
        rel = inv[tgt] @ torch.cat([m, bottom], 1)[pairs[:, 0].to(torch.int64)]               # (Q k, 3, 4)
        seeds = yaw_seeds(yaw, rel.reshape(Q * k, 12))
    elif int(yaw) != 1:
        seeds = yaw_seeds(yaw, device=dev).unsqueeze(0).expand(Q * k, int(yaw), 12).contiguous()
    pose, fit, info, status = register_pairs(clouds, pairs, seeds, **kw)
    return pose.reshape(Q, k, 12), fit.reshape(Q, k, 2), info.reshape(Q, k, 4), status.reshape(Q, k)


def relax_trajectory(poses: torch.Tensor, pairs: torch.Tensor, rel: torch.Tensor, weights: torch.Tensor,
                     odo_weights: Tuple[float, float] = (1.0, 100.0), iterations: int = 4, cg_iterations: int = 64,
                     workspace: Optional[torch.Tensor] = None):
    """Loop closing (include/epcnet_trajectory.h): relaxes the pose graph of one trajectory -- the chain of odometry edges between
    consecutive rows of ``poses`` (T, 12) float64 ``[R | t]`` (``sub_pose``; the rows from the first non-finite one on are the NaN slots
    behind its end) plus the loops ``pairs`` (L, 2) int32 (source, target) with ``rel`` (L, 12) float64 source -> target (what
    ``register_pairs`` returns) and ``weights`` (L, 2) float64 (w_t, w_r) -- by ``iterations`` Gauss-Newton steps of ``cg_iterations``
    preconditioned CG iterations each, in chain-increment variables.  ``odo_weights``: (w_t, w_r) of every odometry edge.  Returns
    ``(poses_out (T, 12) float64, cost (iterations + 1,) float64, loop_chi2 (L,) float64, loop_status (L,) int32: 0 or
    EPC_STATUS_NO_EDGE, num_out (2,) int32: T_eff and the loops used)``; a loop with an index outside the trajectory (the -1 of
    ``revisit_search``), a NaN ``rel`` (a flagged pair) or two zero weights is skipped; with no loop used the poses come back bit for
    bit.  Bit for bit tests/relax_ref.py; only contiguous device tensors of the exact dtype are taken, float32 poses are refused, never
    converted; nothing is read back, the call is asynchronous and capturable in a graph.  ``workspace``: a uint8 device tensor of at
    least ``epcnet_trajectory_relax_workspace_bytes`` bytes to reuse (what a captured graph needs), else one is allocated."""
    L.require_gpu()
    who = "relax_trajectory"
    _check(who, "poses", poses, torch.float64, 2, None, 12)
    dev = poses.device
    _check(who, "pairs", pairs, torch.int32, 2, dev, 2)
    _check(who, "rel", rel, torch.float64, 2, dev, 12)
    _check(who, "weights", weights, torch.float64, 2, dev, 2)
    T, nl = int(poses.shape[0]), int(pairs.shape[0])
    if int(rel.shape[0]) != nl or int(weights.shape[0]) != nl:
        raise L.EpcNetError(-1, "relax_trajectory: rel must be (L, 12) and weights (L, 2) for pairs (L, 2), got %s and %s" % (
            tuple(rel.shape), tuple(weights.shape)))
    ws, own = _workspace(who, int(L.lib().epcnet_trajectory_relax_workspace_bytes(T, nl)), workspace, dev)
    iterations = int(iterations)
    poses_out = torch.empty((T, 12), dtype=torch.float64, device=dev)
    cost = torch.empty((max(iterations, 0) + 1,), dtype=torch.float64, device=dev)
    chi2 = torch.empty((nl,), dtype=torch.float64, device=dev)
    status = torch.empty((nl,), dtype=torch.int32, device=dev)
    num_out = torch.empty((2,), dtype=torch.int32, device=dev)
    arg = _arg(ws)
    L.run.epcnet_trajectory_relax(arg(poses), T, arg(pairs), arg(rel), arg(weights), nl, float(odo_weights[0]), float(odo_weights[1]),
                                  iterations, int(cg_iterations), arg(poses_out), cost, arg(chi2), arg(status), num_out, ws, ws.numel())
    if own:
        ws.record_stream(torch.cuda.current_stream(dev))
    return poses_out, cost, chi2, status, num_out


def close_loops(sub_pose: torch.Tensor, idx: torch.Tensor, pose: torch.Tensor, fit: torch.Tensor, st: torch.Tensor,
                min_overlap: float = 0.6, max_msr: float = 0.05, loop_weights: Tuple[float, float] = (1.0, 100.0), **kw):
    """``relax_trajectory`` on what ``verify_revisits`` returned: ``sub_pose`` (T, 12) float64, ``idx`` (Q, k) int32 the candidates of
    ``revisit_search``, ``pose`` (Q, k, 12), ``fit`` (Q, k, 2) and ``st`` (Q, k) the registration's results.  Query i is the SOURCE of
    its loops and ``idx[i, j]`` the target; a loop's weights are ``loop_weights`` where the pair is unflagged, its overlap ``fit[..., 1]``
    is at least ``min_overlap`` and its mean squared residual ``fit[..., 0]`` at most ``max_msr``, else (0, 0), which the relaxation
    skips.  Formed with torch on the device, outside the bit contract; no host read; ``kw`` goes to ``relax_trajectory``, whose
    result is returned (the loops in the row-major order of ``idx``)."""
    who = "relax_trajectory"
    _check(who, "idx", idx, torch.int32, 2, sub_pose.device if torch.is_tensor(sub_pose) else None)
    Q, k = int(idx.shape[0]), int(idx.shape[1])
    dev = idx.device
    _check(who, "pose", pose, torch.float64, 3, dev, 12)
    _check(who, "fit", fit, torch.float64, 3, dev, 2)
    _check(who, "st", st, torch.int32, 2, dev)
    if tuple(pose.shape[:2]) != (Q, k) or tuple(fit.shape[:2]) != (Q, k) or tuple(st.shape) != (Q, k):
        raise L.EpcNetError(-1, "close_loops: expected idx (Q, k), pose (Q, k, 12), fit (Q, k, 2) and st (Q, k)")
    good = (st == 0) & (fit[..., 1] >= float(min_overlap)) & (fit[..., 0] <= float(max_msr))
    w = torch.tensor([float(loop_weights[0]), float(loop_weights[1])], dtype=torch.float64, device=dev)
    weights = (good.reshape(Q * k, 1).to(torch.float64) * w.reshape(1, 2)).contiguous()
    return relax_trajectory(sub_pose, _pairs_of(idx), pose.reshape(Q * k, 12), weights, **kw)
