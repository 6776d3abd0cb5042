"""Inference engine: owns the packed (BN-folded, MFMA-ordered) weights and the workspace, and drives
``epc_net_forward`` of libepcnet_hip.so.  This is what ``forward(..., is_training=False)`` of the model
modules runs (reference: ``sess.run`` of ``models/epc-net.py:29-157`` / ``models/epc-net-l.py:29-102``).
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import torch

from . import lib as L
from .variables import VariableStore

ARCH_IDS = {"epc-net": L.EPC_ARCH_EPC_NET, "epc-net-l": L.EPC_ARCH_EPC_NET_L}

DEFAULT_PARAMS = {"CLUSTER_SIZE": 64, "FEATURE_OUTPUT_DIM": 256, "KNN": 20, "INPUT_DIM": 3, "GROUPS": 4}
# Arithmetic of the inference path when neither the engine nor params["PRECISION"] names one (include/epcnet.h:
# EPC_PRECISION_*).  "f32" = the reference's class of arithmetic (float32 graph, models/epc-net.py:24-26) on split
# half-precision MFMA; "fast" = the f16 + f6 path (either model): an explicit opt-in for checkpoints it has been validated on
# (tests/test_gpu_adversarial.py: it is wrong by 1e-2 on heavy-tailed weights while staying inside fp16's range, so
# nothing selects it automatically).
DEFAULT_PRECISION = "f32"
# EPC-Net-L (models/epc-net-l.py:29-102): batches of L_HALVES_FROM clouds or more run as L_HALF_BATCH-cloud passes on two HIP streams
L_HALVES_FROM = 256
L_HALF_BATCH = 128


def resolve_precision(params: Optional[dict], precision: Optional[str] = None) -> str:
    name = precision or (params or {}).get("PRECISION") or DEFAULT_PRECISION
    name = str(name).lower()
    if name not in ("f32", "fast"):
        raise ValueError("PRECISION must be 'f32' or 'fast', got %r" % (name,))
    return name


def make_cfg(arch: str, num_points: int, params: Optional[dict], micro_batch: int = 0,
             precision: Optional[str] = None) -> L.EpcCfg:
    p = dict(DEFAULT_PARAMS)
    p.update(params or {})
    if arch not in ARCH_IDS:
        raise ValueError("unknown ARCH %r" % arch)
    prec = resolve_precision(p, precision)
    return L.EpcCfg(arch=ARCH_IDS[arch], num_points=int(num_points), input_dim=int(p["INPUT_DIM"]),
                    knn=int(p["KNN"]), cluster_size=int(p["CLUSTER_SIZE"]), output_dim=int(p["FEATURE_OUTPUT_DIM"]),
                    groups=int(p.get("GROUPS", 4)), micro_batch=int(micro_batch), precision=L.PRECISION_IDS[prec])


class InferenceEngine:
    def __init__(self, arch: str, params: Optional[dict], store: VariableStore, outer: str = "query_triplets",
                 micro_batch: int = 0, backbone_scope: str = "fastdgcnn", in_flight: Optional[int] = None,
                 precision: Optional[str] = None):
        self.arch = arch
        self.precision = resolve_precision(params, precision)   # 'f32' | 'fast'
        self.resolved_precision: Optional[str] = None          # what the packed weights hold
        # passes kept in flight on separate HIP streams (submit / long calls).  Default: two in the `fast` arithmetic (+12 %),
        # ONE in the f32-equivalent one -- its kernels fill every CU's registers and LDS (the persistent block kernel the whole
        # chip): a second lane only delays the first (bench.py `overlapped`: 55.6 k against 57.5 k clouds/s)
        # EPC-Net-L, f32-equivalent: two lanes as well -- a batch of 256 clouds or more goes as 128-cloud halves in flight (the VALU-bound
        # kNN of one half beside the L1-bound blocks / the matrix-bound conv5 of the other: +3-4 %, the same bits; `_forward`).  EPC-Net-L,
        # `fast`: ONE lane -- the halves do not pay there (scripts/time_l_fast.py, two runs: -0.5 % and +0.6 % against one 256-cloud
        # pass, inside the run-to-run spread), the same bits either way
        if in_flight is None:
            in_flight = 2 if (arch == "epc-net") == (self.precision == "fast") else 1
        self.in_flight = max(1, min(int(in_flight), 8))
        self._lanes = None                                 # [(torch.cuda.Stream, workspace tensor or None, last event or None)]
        self._next_lane = 0
        self.backbone_scope = backbone_scope   # 'BACKBONE' for the KD student (models/kd_epc-net-l.py:44)
        self.params = dict(params or {})
        self.store = store
        self.outer = outer
        self.micro_batch = micro_batch
        self._packed: Optional[torch.Tensor] = None
        self._packed_key = None
        self._ws: Optional[torch.Tensor] = None
        self._last_cfg: Optional[L.EpcCfg] = None
        self._last_overlap = None                          # (cfg, lanes, bytes per lane slice, clouds) of a one-pass-per-lane overlapped call
        self._fallback: "Optional[InferenceEngine]" = None   # f32-equivalent engine for clouds the fast path flags

    # ------------------------------------------------------------------------------------------------------
    def _relative_tensors(self) -> Dict[str, torch.Tensor]:
        prefix = self.outer + "/" if self.outer else ""
        out = {}
        for name, t in self.store.vars.items():
            if prefix and not name.startswith(prefix):
                continue
            rel = name[len(prefix):]
            if self.backbone_scope != "fastdgcnn" and rel.startswith(self.backbone_scope + "/"):
                rel = "fastdgcnn/" + rel[len(self.backbone_scope) + 1:]   # the library looks variables up by the EPC-Net names
            out[rel] = t
        return out

    def cfg_for(self, num_points: int) -> L.EpcCfg:
        """The epc_cfg of a call on clouds of ``num_points`` points, in the precision the packed weights hold."""
        return make_cfg(self.arch, num_points, self.params, self.micro_batch, precision=self.precision)

    def packed(self, cfg: L.EpcCfg) -> torch.Tensor:
        # keyed on the version of THIS model's variables: a frozen teacher that shares the store with a student being
        # trained (kd_train.py:467-497) is not re-folded every step
        key = (self.store.version_of(self.outer), cfg.num_points, cfg.groups, cfg.knn, self.precision)
        if self._packed is not None and self._packed_key == key:
            cfg.precision = L.PRECISION_IDS[self.resolved_precision]
            return self._packed
        L.require_gpu()
        nbytes = L.lib().epc_net_packed_bytes(ctypes.byref(cfg))
        if nbytes == 0:
            raise L.EpcNetError(-1, "unsupported configuration (see include/epcnet.h: epc_cfg)")
        rel = self._relative_tensors()
        names = list(rel.keys())
        tensors = [rel[n] for n in names]
        for t in tensors:
            if not t.is_cuda:
                raise L.EpcNetError(-1, "variables must live on a ROCm device")
        c_names = (ctypes.c_char_p * len(names))(*[n.encode() for n in names])
        c_ptrs = (ctypes.c_void_p * len(names))(*[t.data_ptr() for t in tensors])
        buf = torch.empty(nbytes, dtype=torch.uint8, device=tensors[0].device)
        # (fast precision: EPC_ERANGE when a folded weight does not fit fp16 -- never a packed Inf)
        L.run.epc_net_pack_weights(ctypes.byref(cfg), c_names, c_ptrs, len(names), buf, nbytes)
        if self._packed is not None:
            # batches submitted on the engine's lanes may still be reading the previous buffer: keep it alive until their
            # streams have passed this point (the caching allocator would otherwise hand it out again)
            for lane in self._lanes or []:
                self._packed.record_stream(lane[0])
        self.resolved_precision = "fast" if cfg.precision == L.EPC_PRECISION_FAST else "f32"
        self._packed, self._packed_key = buf, key
        return buf

    def workspace(self, cfg: L.EpcCfg, num_clouds: int, device) -> torch.Tensor:
        need = L.lib().epc_net_workspace_bytes(ctypes.byref(cfg), num_clouds)
        if self._ws is None or self._ws.numel() < need or self._ws.device != device:
            self._ws = torch.empty(need, dtype=torch.uint8, device=device)
        return self._ws

    def forward(self, xyz: torch.Tensor, out: Optional[torch.Tensor] = None, profile: "Optional[StageProfile]" = None,
                check: Optional[bool] = None) -> torch.Tensor:
        """xyz (num_clouds, N, 3) float32 on the GPU -> (num_clouds, FEATURE_OUTPUT_DIM).
        ``profile``: record HIP events at the stage boundaries of this pass (same launches, same stream).
        ``check`` (fast precision only, default off): look at the result (this synchronises) and re-extract in the
        f32-equivalent arithmetic every cloud the kernels flagged (NaN descriptor: an activation left fp16's range, include/
        epcnet.h EPC_STATUS_FP16_RANGE -- e.g. the zero-padding clouds of evaluate.py:425-430).  A cloud that is still NaN
        afterwards has a NaN / Inf coordinate -- the reference returns NaN for it as well."""
        out = self._forward(xyz, out, profile)
        if check and self.resolved_precision == "fast":
            bad = torch.isnan(out).any(dim=1).nonzero().flatten()
            if bad.numel():
                if self._fallback is None:
                    self._fallback = InferenceEngine(self.arch, self.params, self.store, outer=self.outer,
                                                     micro_batch=self.micro_batch, backbone_scope=self.backbone_scope,
                                                     in_flight=1, precision="f32")
                out[bad] = self._fallback._forward(xyz.contiguous()[bad], None, None)
        return out

    def _forward(self, xyz: torch.Tensor, out: Optional[torch.Tensor], profile: "Optional[StageProfile]") -> torch.Tensor:
        if xyz.dim() != 3 or xyz.shape[-1] != 3:
            raise L.EpcNetError(-1, "expected (num_clouds, N, 3) points, got %s" % (tuple(xyz.shape),))
        if xyz.dtype != torch.float32:
            raise L.EpcNetError(-1, "points must be float32")
        L.require_gpu()
        xyz = xyz.contiguous()
        nc, n = int(xyz.shape[0]), int(xyz.shape[1])
        cfg = self.cfg_for(n)
        packed = self.packed(cfg)
        if out is None:
            out = torch.empty((nc, cfg.output_dim), dtype=torch.float32, device=xyz.device)
        if self.arch == "epc-net-l" and self.micro_batch == 0 and self.in_flight > 1 and profile is None and nc >= L_HALVES_FROM:
            cfg.micro_batch = L_HALF_BATCH          # (passes of 128 clouds dealt over the lanes: results do not depend on the pass size)
        mb = L.micro_batch_of(cfg, nc)
        if profile is None and self.in_flight > 1 and nc > mb:
            # several passes: deal them over this stream and the auxiliary lanes (epc_net_forward_overlapped)
            lanes = min(self.in_flight, (nc + mb - 1) // mb)
            need = L.lib().epc_net_workspace_bytes(ctypes.byref(cfg), nc) * lanes
            if self._ws is None or self._ws.numel() < need or self._ws.device != xyz.device:
                self._ws = torch.empty(need, dtype=torch.uint8, device=xyz.device)
            aux = [ln[0] for ln in self._get_lanes(xyz.device)[:lanes - 1]]
            arr = (ctypes.c_void_p * max(len(aux), 1))(*[a.cuda_stream for a in aux])
            # several lanes, several workspace slices: last_status() can answer only while no slice has been reused (one pass per lane)
            self._last_cfg = None
            self._last_overlap = (cfg, lanes, L.lib().epc_net_workspace_bytes(ctypes.byref(cfg), nc), nc) if (nc + mb - 1) // mb <= lanes else None
            L.check(L.lib().epc_net_forward_overlapped(ctypes.byref(cfg), packed.data_ptr(), L.ptr(xyz), nc, L.ptr(out),
                                                       self._ws.data_ptr(), self._ws.numel(), L.current_stream(), arr,
                                                       len(aux)))
            return out
        ws = self.workspace(cfg, max(nc, 1), xyz.device)
        self._last_cfg = cfg
        self._last_overlap = None
        L.check(L.lib().epc_net_forward_profiled(ctypes.byref(cfg), packed.data_ptr(), L.ptr(xyz), nc, L.ptr(out),
                                                 ws.data_ptr(), ws.numel(), L.current_stream(),
                                                 profile.handle if profile is not None else None))
        return out


    def forward_bank(self, bank, ids: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The descriptors of the records ``ids`` of an ``ops.CloudBank`` -> (len(ids), FEATURE_OUTPUT_DIM), bit-identical to
        ``forward(xyz[ids])`` on the clouds that were added (include/epcnet.h: epc_net_forward_bank): no upload, no sort, no kNN --
        the records hold them.  ``ids``: a contiguous int32 DEVICE tensor, read when the kernels run (repeats and any order allowed;
        a captured graph replays with whatever the buffer then holds).  An id outside the bank gives a NaN descriptor and the
        status word EPC_STATUS_NONFINITE_INPUT.  One stream, passes of the micro-batch; ``last_status`` answers for this call too."""
        if not torch.is_tensor(ids) or not ids.is_cuda or ids.dtype != torch.int32 or not ids.is_contiguous():
            raise L.EpcNetError(-1, "forward_bank: ids must be a contiguous int32 tensor on the ROCm device (no CPU fallback)")
        L.require_gpu()
        if len(bank) == 0:
            raise L.EpcNetError(-1, "forward_bank: the bank is empty")
        nc = int(ids.numel())
        cfg = self.cfg_for(bank.n)
        packed = self.packed(cfg)
        if out is None:
            out = torch.empty((nc, cfg.output_dim), dtype=torch.float32, device=ids.device)
        ws = self.workspace(cfg, max(nc, 1), ids.device)
        self._last_cfg = cfg
        self._last_overlap = None
        L.run.epc_net_forward_bank(ctypes.byref(cfg), packed, bank.records, len(bank), bank.n, bank.cap, ids, nc, L.ptr(out), ws,
                                   ws.numel())
        return out

    def forward_scans(self, points: torch.Tensor, offsets: torch.Tensor, num_points: int = 4096, normalize: bool = True,
                      out: Optional[torch.Tensor] = None, ground=None):
        """Descriptors of RAW scans: ``points`` (total, 3) float32 and ``offsets`` (B + 1,) int32 on the device (``ops.pack_scans``), any
        number of points per scan -> ``(descriptors (B, FEATURE_OUTPUT_DIM), status (B,) int32)``.  Runs ``ops.grid_downsample`` (to
        ``num_points`` points per cloud; include/epcnet.h: epc_grid_downsample) and then ``forward`` on the same stream, no host round
        trip in between -- bit-identical to ``forward(ops.grid_downsample(points, offsets, num_points, normalize)[0])``, and capturable
        in a graph (the offsets are read when the kernel runs).  ``status`` holds the down-sampler's words: a scan flagged
        EPC_STATUS_NO_GRID reaches the network as NaN rows, so its descriptor is NaN and ``last_status`` reports
        EPC_STATUS_NONFINITE_INPUT for it.

        ``ground=True``, or a dict of ``ops.remove_ground``'s keyword arguments, removes the ground plane of every scan first
        (include/epcnet_scans.h), on the same stream and into a copy of the rows: the networks were trained on clouds without their
        ground.  ``status`` is then the down-sampler's word ORed with the removal's (EPC_STATUS_NO_GROUND: no plane was found, the
        scan went on as it came).  ``None``, the default, is the path above unchanged."""
        return self._forward_scans(points, offsets, num_points, normalize, out, ground, False)[:2]

    def _forward_scans(self, points, offsets, num_points, normalize, out, ground, clouds):
        """``forward_scans`` -> (descriptors, status, metric): with ``clouds`` the rows that fed the network go through a second
        ``ops.grid_downsample(..., normalize=False)`` on the same stream -- (B, num_points, 3) float32 in the sensor's units, NaN rows where
        the scan has no grid --, else ``metric`` is None and nothing more is launched."""
        from . import ops
        if ground is None or ground is False:
            kept, st_ground = points, None
        else:
            if ground is not True and not isinstance(ground, dict):
                raise L.EpcNetError(-1, "forward_scans: `ground` is None, True or a dict of ops.remove_ground's arguments")
            kept, st_ground, _, _ = ops.remove_ground(points, offsets, **({} if ground is True else ground))
        xyz, status, _ = ops.grid_downsample(kept, offsets, num_points, normalize=normalize)
        desc = self.forward(xyz, out=out)
        metric = ops.grid_downsample(kept, offsets, num_points, normalize=False)[0] if clouds else None
        return desc, (status if st_ground is None else status | st_ground), metric

    def forward_trajectory(self, points: torch.Tensor, offsets: torch.Tensor, poses: torch.Tensor, along: Optional[torch.Tensor] = None,
                           num_points: int = 4096, normalize: bool = True, ground=None, submaps: Optional[dict] = None,
                           out: Optional[torch.Tensor] = None, clouds: bool = False):
        """Descriptors of POSED scans: ``points`` / ``offsets`` as ``forward_scans`` takes them, in the order the scans were taken,
        ``poses`` (S, 12) or (S, 3, 4) float64 on the device and, optionally, the travelled distance ``along`` (S,) float64 ->
        ``(descriptors (max_submaps, FEATURE_OUTPUT_DIM), status (max_submaps,) int32, sub_pose (max_submaps, 12) float64, num_out (2,)
        int32)``.  Runs ``ops.build_submaps`` (include/epcnet_submaps.h; ``submaps``: a dict of its keyword arguments -- length, spacing,
        the crop, the capacities) and then exactly what ``forward_scans`` does on the submaps, on the same stream with no host read in
        between: bit-identical to ``forward_scans(*ops.build_submaps(...)[:2], ...)`` and capturable in a graph.  ``ground`` is
        ``forward_scans``' argument: the plane is removed per SUBMAP, after the build, which is what the benchmark's preparation did
        (per scan, before the build, works too: call ``ops.remove_ground`` on the scans first).  ``status`` is the three stages' words ORed
        together: EPC_STATUS_NO_SUBMAP / EPC_STATUS_NO_ROOM of the build, EPC_STATUS_NO_GROUND, EPC_STATUS_NO_GRID; a slot that is no
        submap has no rows, hence no grid and a NaN descriptor.  ``num_out[0]`` says how many leading slots are submaps;
        ``sub_pose[:, [3, 7]]`` are their (x, y).  ``clouds=True`` appends the submaps' METRIC clouds (max_submaps, num_points, 3) float32 --
        a second ``ops.grid_downsample(..., normalize=False)`` of the same rows on the same stream, in the frame of ``sub_pose`` -- which is
        what ``retrieval.verify_revisits`` aligns; the default returns exactly the four above."""
        from . import ops
        if submaps is not None and not isinstance(submaps, dict):
            raise L.EpcNetError(-1, "forward_trajectory: `submaps` is None or a dict of ops.build_submaps' arguments")
        kw = dict(submaps or {})
        if "out" in kw or "return_along" in kw:
            raise L.EpcNetError(-1, "forward_trajectory: `submaps` holds build_submaps' parameters, not its `out` or `return_along`")
        sub_points, sub_offsets, st_build, sub_pose, _, num_out = ops.build_submaps(points, offsets, poses, along=along, **kw)
        desc, status, metric = self._forward_scans(sub_points, sub_offsets, num_points, normalize, out, ground, clouds)
        return (desc, status | st_build, sub_pose, num_out) + ((metric,) if clouds else ())

    def forward_stamped(self, points: torch.Tensor, offsets: torch.Tensor, scan_time: torch.Tensor, pose_time: torch.Tensor,
                        pose: torch.Tensor, point_dt: Optional[torch.Tensor] = None, max_gap: float = 0.5, num_points: int = 4096,
                        normalize: bool = True, ground=None, submaps: Optional[dict] = None, out: Optional[torch.Tensor] = None,
                        clouds: bool = False):
        """Descriptors of TIMESTAMPED scans and odometry on its own clock: ``points`` / ``offsets`` as ``forward_scans`` takes them, in
        the order the scans were taken, ``scan_time`` (S,) int64 ns, ``pose_time`` (P,) int64 ns with ``pose`` (P, 7) float64 ``tx ty tz
        qw qx qy qz`` and, for a spinning sensor, ``point_dt`` (total,) int32 ns per row -> ``(descriptors (max_submaps,
        FEATURE_OUTPUT_DIM), status (max_submaps,) int32, sub_pose (max_submaps, 12) float64, num_out (2,) int32, scan_status (S,)
        int32)``.  Runs ``ops.deskew_scans`` (include/epcnet_stamps.h), ``ops.travel_along`` on its poses, ``ops.build_submaps`` with that
        ``along`` and then exactly what ``forward_scans`` does on the submaps, on one stream with no host read in between: bit-identical
        to those calls made one by one, and capturable in a graph.  ``scan_status`` holds the de-skewer's words per SCAN
        (EPC_STATUS_NO_POSE, EPC_STATUS_PART_POSE); ``status`` the later stages' per submap, as ``forward_trajectory`` returns them.  A scan
        without a pose contributes NaN rows only; a submap whose reference scan has no pose ends as a NaN descriptor.  ``submaps`` holds
        ``build_submaps``' parameters, but not ``along``.  ``clouds=True`` appends the submaps' metric clouds, as ``forward_trajectory``
        does."""
        from . import ops
        if submaps is not None and not isinstance(submaps, dict):
            raise L.EpcNetError(-1, "forward_stamped: `submaps` is None or a dict of ops.build_submaps' arguments")
        kw = dict(submaps or {})
        if "out" in kw or "return_along" in kw or "along" in kw:
            raise L.EpcNetError(-1, "forward_stamped: `submaps` holds build_submaps' parameters, not its `out`, `along` or `return_along`")
        moved, scan_pose, scan_status = ops.deskew_scans(points, offsets, scan_time, pose_time, pose, point_dt=point_dt, max_gap=max_gap)
        along = ops.travel_along(scan_pose, scan_status)
        sub_points, sub_offsets, st_build, sub_pose, _, num_out = ops.build_submaps(points if moved is None else moved, offsets, scan_pose,
                                                                                    along=along, **kw)
        desc, status, metric = self._forward_scans(sub_points, sub_offsets, num_points, normalize, out, ground, clouds)
        return (desc, status | st_build, sub_pose, num_out, scan_status) + ((metric,) if clouds else ())

    def last_status(self, xyz_or_count) -> "list[int]":
        """Per-cloud EPC_STATUS_* words of the last pass of the most recent ``forward`` call on this engine's own
        workspace (include/epcnet.h: epc_net_last_status; synchronises the stream).  A non-zero word = that cloud's
        descriptor is NaN: bit 0 a NaN / Inf coordinate, bit 1 (fast precision) an activation outside fp16's range.
        Raises after a call that was dealt over several lanes (see below) -- never returns another call's words."""
        nc = int(xyz_or_count.shape[0]) if torch.is_tensor(xyz_or_count) else int(xyz_or_count)
        if nc <= 0:
            return []
        ov = getattr(self, "_last_overlap", None)
        if self._ws is not None and self._last_cfg is None and ov is not None and ov[3] == nc:
            # the last call went as one pass per lane (EPC-Net-L's two halves): every pass's words are still in its lane's slice
            cfg, lanes, slice_bytes, _ = ov
            mb = L.micro_batch_of(cfg, nc)
            words = []
            for p in range((nc + mb - 1) // mb):
                n_p = min(mb, nc - p * mb)
                arr = (ctypes.c_int32 * n_p)()
                L.run.epc_net_last_status(ctypes.byref(cfg), self._ws.data_ptr() + (p % lanes) * slice_bytes, n_p, arr)
                words += [int(v) for v in arr]
            return words
        if self._ws is None or self._last_cfg is None:
            # nothing ran yet, or the last call was dealt over the engine's lanes (num_clouds > micro_batch with in_flight > 1:
            # epc_net_forward_overlapped keeps one workspace slice per lane, so "the last pass's status words" do not exist in
            # one place): say so instead of returning stale words.  The NaN descriptor marks a flagged cloud in
            # every mode; for status words run the engine with in_flight=1.
            raise L.EpcNetError(-1, "last_status(): no single-workspace forward to report on (call forward() with "
                                    "num_clouds <= micro_batch or an engine built with in_flight=1)")
        mb = L.micro_batch_of(self._last_cfg, nc)
        last = nc % mb or mb
        arr = (ctypes.c_int32 * last)()
        L.run.epc_net_last_status(ctypes.byref(self._last_cfg), self._ws, nc, arr)
        return [int(v) for v in arr]

    # ---- throughput mode: independent batches in flight on the engine's own streams ---------------------------
    def _get_lanes(self, device):
        if self._lanes is None or self._lanes[0][0].device != device:
            self._lanes = [[torch.cuda.Stream(device=device), None, None] for _ in range(self.in_flight)]
        return self._lanes

    def submit(self, xyz: torch.Tensor, out: Optional[torch.Tensor] = None, profile: "Optional[StageProfile]" = None):
        """Asynchronous ``forward``: the batch runs on one of the engine's ``in_flight`` HIP streams (round-robin, own
        workspace each), ordered after everything already enqueued on the current stream.  Returns ``(out, event)``;
        ``out`` is valid once ``event`` has completed -- ``event.wait()`` orders the current stream after it,
        ``drain()`` after every submitted batch.  Batches submitted back to back overlap (the stages of a pass are
        bound by different units of the chip), which is where the throughput above a single stream comes from."""
        if xyz.dim() != 3 or xyz.shape[-1] != 3 or xyz.dtype != torch.float32:
            raise L.EpcNetError(-1, "expected float32 (num_clouds, N, 3) points, got %s %s" % (xyz.dtype, tuple(xyz.shape)))
        L.require_gpu()
        xyz = xyz.contiguous()
        nc, n = int(xyz.shape[0]), int(xyz.shape[1])
        cfg = self.cfg_for(n)
        packed = self.packed(cfg)
        if out is None:
            out = torch.empty((nc, cfg.output_dim), dtype=torch.float32, device=xyz.device)
        lanes = self._get_lanes(xyz.device)
        lane = lanes[self._next_lane % len(lanes)]
        self._next_lane += 1
        stream = lane[0]
        need = L.lib().epc_net_workspace_bytes(ctypes.byref(cfg), max(nc, 1))
        if lane[1] is None or lane[1].numel() < need:
            if lane[2] is not None:
                lane[2].synchronize()            # the lane's previous batch may still be using the old workspace
            lane[1] = torch.empty(need, dtype=torch.uint8, device=xyz.device)
        stream.wait_stream(torch.cuda.current_stream(xyz.device))
        xyz.record_stream(stream)
        out.record_stream(stream)
        packed.record_stream(stream)
        L.check(L.lib().epc_net_forward_profiled(ctypes.byref(cfg), packed.data_ptr(), L.ptr(xyz), nc, L.ptr(out),
                                                 lane[1].data_ptr(), lane[1].numel(), ctypes.c_void_p(stream.cuda_stream),
                                                 profile.handle if profile is not None else None))
        lane[2] = stream.record_event()
        return out, lane[2]

    def drain(self) -> None:
        """Order the current stream after every batch submitted so far."""
        for lane in self._lanes or []:
            if lane[2] is not None:
                lane[2].wait()


class StageProfile:
    """HIP-event stage timer (``epc_profile`` of include/epcnet.h)."""

    def __init__(self):
        h = ctypes.c_void_p()
        L.check(L.lib().epc_profile_create(ctypes.byref(h)))
        self.handle = h

    def elapsed_ms(self) -> Dict[str, float]:
        """Per-stage milliseconds; call after the stream is synchronised."""
        arr = (ctypes.c_float * L.EPC_NUM_STAGES)()
        L.check(L.lib().epc_profile_elapsed_ms(self.handle, arr))
        return {L.STAGE_NAMES[i]: float(arr[i]) for i in range(L.EPC_NUM_STAGES)}

    def __del__(self):
        try:
            if self.handle:
                L.lib().epc_profile_destroy(self.handle)
                self.handle = None
        except Exception:
            pass
