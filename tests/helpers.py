"""Test-side helpers: build a variable store from oracle weights, drive the stage entry points of the C ABI."""
import ctypes
import importlib
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import epcnet_oracle as O  # noqa: E402

PARAMS = {"CLUSTER_SIZE": 64, "FEATURE_OUTPUT_DIM": 256, "KNN": 20, "INPUT_DIM": 3, "GROUPS": 4}
OUTER = "query_triplets"


def pkg(name=""):
    return importlib.import_module("epc-net_amd" + ("." + name if name else ""))


GUARD = 4096    # bytes of poison on either side of every Guarded tensor


class Guarded:
    """A tensor of `shape` / `dtype` in the middle of a buffer of bytes 0xFF: `t` is the tensor to pass, `intact()` says whether the
    GUARD bytes in front of it and behind it still hold the poison, `untouched()` whether the tensor itself does too."""

    def __init__(self, shape, dtype, dev):
        self.nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.buf = torch.full((2 * GUARD + self.nbytes,), 0xFF, dtype=torch.uint8, device=dev)
        self.t = self.buf[GUARD:GUARD + self.nbytes].view(dtype).reshape(shape)

    def intact(self):
        return bool((self.buf[:GUARD] == 0xFF).all()) and bool((self.buf[GUARD + self.nbytes:] == 0xFF).all())

    def untouched(self):
        return bool((self.buf == 0xFF).all())


def make_store(arch, weights, device, params=None):
    """Variable store holding `weights` (oracle names, relative to OUTER) under the reference's full names."""
    V = pkg("variables")
    st = V.reset_default_store(device=device, seed=0)
    M = pkg("models." + arch)
    with V.variable_scope(OUTER):
        M.declare_variables(params or PARAMS, 4096)
    st.load_state_dict({OUTER + "/" + k: v for k, v in weights.items()}, strict=True)
    return st


def make_engine(arch, weights, device="cuda", micro_batch=0, precision=None, in_flight=None, params=None):
    """`precision`: None = the PRODUCT default (engine.py: 'f32', the f32-equivalent split arithmetic) / 'f32' / 'fast' (EPC-Net's
    f16 + f6 kernels, an explicit opt-in; EPC-Net-L ignores it).  Tests whose subject is the fast path pass 'fast'.
    `params`: the configuration (default PARAMS) -- the weights must have been drawn for it."""
    E = pkg("engine")
    st = make_store(arch, weights, device, params)
    return E.InferenceEngine(arch, params or PARAMS, st, outer=OUTER, micro_batch=micro_batch, precision=precision, in_flight=in_flight), st


def run_stages(eng, xyz):
    """Run the pipeline stage by stage through the C ABI, returning every intermediate as a torch tensor.
    EPC-Net's block chain runs on fp16 rows (x16 -> out16 / x_next16), EPC-Net-L's on f32 rows: `xs` / `cat` are
    returned in the dtype the stage wrote."""
    import stage_ref as R          # (the fragment decoders; it imports this module)
    L = pkg("lib")
    E = pkg("engine")
    lib = L.lib()
    nc, n, _ = xyz.shape
    cfg = eng.cfg_for(n)
    packed = eng.packed(cfg)
    f16 = eng.arch == "epc-net" and cfg.precision == L.EPC_PRECISION_FAST
    base = packed.data_ptr()
    off = lambda s: base + lib.epc_net_packed_offset(ctypes.byref(cfg), s)
    dev = xyz.device
    st = L.current_stream()
    M = nc * n
    out = {}
    status = torch.zeros((nc,), dtype=torch.int32, device=dev)
    idx = torch.empty((nc, n, L.EPC_KNN_CAP), dtype=torch.int32, device=dev)
    cnt = torch.empty((nc, n), dtype=torch.int32, device=dev)
    kth = torch.empty((nc, n), dtype=torch.float32, device=dev)
    L.check(lib.epc_knn_topk(xyz.data_ptr(), nc, n, L.EPC_KNN_CAP, idx.data_ptr(), cnt.data_ptr(), kth.data_ptr(), st))
    out.update(idx=idx, cnt=cnt, kth=kth)
    idx16 = idx.clamp(0, 32767).to(torch.int16)     # the pipeline's 2-byte list format (entries past cnt are never read)
    nblocks = 4 if eng.arch == "epc-net" else 2
    ccat = 64 * nblocks
    dt = torch.float16 if f16 else torch.float32
    xs = [torch.empty((nc, n, 64), dtype=dt, device=dev) for _ in range(nblocks + 1)]
    cat = torch.empty((nc, n, ccat), dtype=dt, device=dev)
    a32 = lambda t: None if f16 else t.data_ptr()
    a16 = lambda t: t.data_ptr() if f16 else None
    L.check(lib.epc_conv1_fwd(xyz.data_ptr(), off(0), M, a32(xs[0]), a16(xs[0]), st))
    for b in range(1, nblocks + 1):
        has_next = 1 if b < nblocks else 0
        # (lists: the int32 form for odd blocks, the pipeline's uint16 form for even ones -- both must give the same rows)
        u16 = (b % 2 == 0) and n <= 8192
        L.check(lib.epc_proxyconv_block_fwd(a32(xs[b - 1]), a16(xs[b - 1]), xyz.data_ptr(),
                                            (idx16 if u16 else idx).data_ptr(), 1 if u16 else 0,
                                            cnt.data_ptr(), kth.data_ptr(), L.EPC_KNN_CAP, off(b), has_next, nc, n,
                                            cfg.knn, a32(cat), a16(cat), ccat, 64 * (b - 1), a32(xs[b]), a16(xs[b]),
                                            status.data_ptr(), st))
    out.update(xs=xs, cat=cat)
    desc = torch.empty((nc, 256), dtype=torch.float32, device=dev)
    if eng.arch == "epc-net":
        rnorm = torch.empty((nc, n), dtype=torch.float32, device=dev)
        assign = torch.empty((nc, n, 64), dtype=torch.float32, device=dev)
        apart = torch.empty((nc, n // 32, 64), dtype=torch.float32, device=dev)
        vlad = torch.empty((nc, 1024, 64), dtype=torch.float32, device=dev)
        colss = torch.empty((nc, 32, 64), dtype=torch.float32, device=dev)
        if f16:
            featf = torch.empty((M // 32, 32, 2, 64, 8), dtype=torch.float16, device=dev)
            assignf = torch.empty((M // 32, 2, 2, 64, 8), dtype=torch.float16, device=dev)
            L.check(lib.epc_conv5_assign_fwd(cat.data_ptr(), 1, ccat, off(5), M, n, featf.data_ptr(), rnorm.data_ptr(),
                                             assign.data_ptr(), assignf.data_ptr(), apart.data_ptr(), status.data_ptr(), st))
            L.check(lib.epc_vlad_aggregate_fwd(featf.data_ptr(), assignf.data_ptr(), rnorm.data_ptr(), apart.data_ptr(),
                                               off(6), nc, n, vlad.data_ptr(), colss.data_ptr(), st))
            feat = R.decode_feat_f16(featf, M).reshape(nc, n, 1024)
            aprime = R.decode_assign_f16(assignf, M).reshape(nc, n, 64) * rnorm.reshape(nc, n, 1)   # assign * rnorm
        else:
            featf = torch.empty((M // 32, 32, 3, 64, 16), dtype=torch.uint8, device=dev)
            assignf = torch.empty((M // 32, 2, 2, 2, 64, 8), dtype=torch.bfloat16, device=dev)
            L.check(lib.epc_conv5_assign_f32_fwd(cat.data_ptr(), ccat, off(5), M, featf.data_ptr(), rnorm.data_ptr(),
                                                 assign.data_ptr(), assignf.data_ptr(), apart.data_ptr(), st))
            L.check(lib.epc_vlad_aggregate_f32_fwd(featf.data_ptr(), assignf.data_ptr(), rnorm.data_ptr(),
                                                   apart.data_ptr(), off(6), nc, n, vlad.data_ptr(), colss.data_ptr(), st))
            feat = R.decode_feat_b3(featf, M).reshape(nc, n, 1024)
            aprime = R.decode_assign_bf16x2(assignf, M).reshape(nc, n, 64) * rnorm.reshape(nc, n, 1)
        wsb = lib.epc_vlad_head_workspace_bytes(nc, cfg.groups)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        L.check(lib.epc_vlad_head_fwd(vlad.data_ptr(), colss.data_ptr(), off(6), cfg.groups, nc, desc.data_ptr(),
                                      status.data_ptr(), ws.data_ptr(), wsb, st))
        out.update(feat=feat, rnorm=rnorm, assign=assign, aprime=aprime, vlad=vlad, colss=colss, apart=apart)
    else:
        pooled = torch.empty((nc, 1024), dtype=torch.float32, device=dev)
        L.check(lib.epc_conv5_maxpool_fwd(cat.data_ptr(), ccat, off(5), nc, n, pooled.data_ptr(), st))
        L.check(lib.epc_fc_head_fwd(pooled.data_ptr(), off(6), nc, desc.data_ptr(), status.data_ptr(), st))
        out.update(pooled=pooled)
    out["desc"] = desc
    out["status"] = status
    torch.cuda.synchronize()
    return out


# ---- which launch form a call reached -------------------------------------------------------------------------------------------------
# The training step's kernels choose their form from the row count and the CU count (rows_tile_waves, epc_chain_parts, ...).  A test that
# exists for one form asserts that it reached it, so that a later change to a heuristic cannot quietly turn it into a duplicate.

def launched_kernels(fn):
    """Run fn() under torch.profiler; returns (fn's result, {device kernel name: launches})."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    names = {}
    for e in prof.events():
        if str(getattr(e, "device_type", "")).endswith("CUDA"):
            names[e.name] = names.get(e.name, 0) + 1
    return out, names


_ROWGEMM = (re.compile(r"hx_rowgemm_kernel<(\d+),(true|false),(unsignedshort|float),(\d+),(\d+),(true|false),(\d+)>"),
            re.compile(r"hx_rowgemm_kernelILi(\d+)ELb([01])E([tf])Li(\d+)ELi(\d+)ELb([01])ELi(\d+)E"))


def rowgemm_forms(names):
    """{(NT, XFORM, 'u16' | 'f32', P, KSC, BNB, NW): launches} of hx_rowgemm_kernel (csrc/train_head_common.h) among `names`, demangled or
    mangled; NW = 3 is the 96-row workgroup, 4 the 128-row one."""
    forms = {}
    for name, count in names.items():
        flat = name.replace(" ", "")
        for rx in _ROWGEMM:
            m = rx.search(flat)
            if m:
                nt, xf, ta, p, ksc, bnb, nw = m.groups()
                key = (int(nt), xf in ("true", "1"), "f32" if ta in ("float", "f") else "u16", int(p), int(ksc), bnb in ("true", "1"), int(nw))
                forms[key] = forms.get(key, 0) + count
                break
    return forms
