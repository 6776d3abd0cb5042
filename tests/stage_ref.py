"""What the stage-level tests share: the decoders of the fragment layouts of include/epcnet.h, float64 restatements of the
inference stages built from the oracle's own stage functions, poisoned output buffers, and the launch of one stage entry point
ALONE on inputs the test makes itself (tests/test_gpu_stage_forms.py; tests/test_stage_forms_cpu.py checks the decoders against
plain numpy encoders and the restatements against the oracle's taps, without a GPU)."""
import ctypes

import numpy as np
import torch

from helpers import O

CAP = 32           # EPC_KNN_CAP: list slots per point
TILE = 32          # points per tile of every inference kernel
BLK_WAVES = 12     # tiles per workgroup of the f32 block kernel (csrc/block.hip)
BLK16_WAVES = 16   # ... of the fp16 one


# ---- fragment decoders (torch, any device) -------------------------------------------------------------------------------------------
def decode_feat_f16(featf, M):
    """feat_frag of epc_conv5_assign_fwd, [tile g][chunk c][half s][lane l][q] fp16 -> feat (M, 1024) float32:
    feat[32g + (l&31)][32c + 16s + 8(q>>2) + 4(l>>5) + (q&3)]   (fp16: 11 significant bits)."""
    ff = featf.float().reshape(M // 32, 32, 2, 2, 32, 2, 4)        # (g, c, s, h, j, q>>2, q&3)
    return ff.permute(0, 4, 1, 2, 5, 3, 6).reshape(M, 1024)        # (g, j, c, s, q>>2, h, q&3) -> point-major


def decode_feat_b3(featf, M):
    """feat_frag of epc_conv5_assign_f32_fwd, uint8 [tile g][chunk c][piece][lane l][16 bytes] -> feat (M, 1024) float32.
    3-byte values: the 48 bytes of lane l of (tile g, chunk c) -- its three 16-byte pieces concatenated -- are 16 little-endian
    values; with li = l & 15, q = l >> 4, value 4t + r (t = 2g2 + p) -> feat[32g + 16p + li][32c + 16g2 + 4q + r]
    (conv5_f32.hip's 16x16x32 accumulator order)."""
    by = featf.reshape(M // 32, 32, 3, 64, 16).permute(0, 1, 3, 2, 4).reshape(M // 32, 32, 64, 16, 3).to(torch.int32)   # (g, c, l, value, byte)
    bits = (by[..., 0] << 8) | (by[..., 1] << 16) | (by[..., 2] << 24)
    ff = bits.view(torch.float32).reshape(M // 32, 32, 4, 16, 2, 2, 4)                       # (g, c, q, li, g2, p, r)
    return ff.permute(0, 5, 3, 1, 4, 2, 6).reshape(M, 1024)                                  # (g, p, li, c, g2, q, r)


def decode_assign_f16(assignf, M):
    """assign_frag of epc_conv5_assign_fwd, [tile g][t][s][lane l][q] fp16 of assign * 2^14 -> assign (M, 64) float32:
    a[32g + 16s + 8(l>>5) + q][32t + (l&31)]."""
    af = assignf.float().reshape(M // 32, 2, 2, 2, 32, 8) / 16384.0   # (g, t, s, h, j, q)
    return af.permute(0, 2, 3, 5, 1, 4).reshape(M, 64)


def decode_assign_bf16x2(assignf, M):
    """assign_frag of epc_conv5_assign_f32_fwd, [tile g][t][s][part][lane l][q] bf16 -> assign (M, 64) float32, hi + lo:
    a[32g + 16s + 8(l>>5) + q][32t + (l&31)]."""
    af = assignf.reshape(M // 32, 2, 2, 2, 64, 8).float().sum(3).reshape(M // 32, 2, 2, 2, 32, 8)   # (g, t, s, h, j, q)
    return af.permute(0, 2, 3, 5, 1, 4).reshape(M, 64)


# ---- float64 restatements (numpy; the oracle's own stage functions on a float64 State) -------------------------------------------------
def state64(weights):
    return O.State(weights, np.float64)


def rows_with_scales(rng, rows, cols, cloud_scale=None, n=None):
    """Random stage input: N(0, 1) rows, each multiplied by a power of two drawn uniformly from 2^-6 .. 2^6 (and cloud b's rows by
    cloud_scale[b], so that a row credited to the wrong cloud shows).  float32."""
    x = rng.randn(rows, cols) * np.exp2(rng.randint(-6, 7, size=(rows, 1)).astype(np.float64))
    if cloud_scale is not None:
        x = x * np.repeat(np.asarray(cloud_scale, dtype=np.float64), n)[:, None]
    return x.astype(np.float32)


def neighbour_sets(idx, cnt, a, kth):
    """(B, N, N) float64 0/1 matrix of the rows each point averages: the listed entries idx[b, i, :cnt] where cnt <= CAP, the oracle's
    mask a_ij >= kth_i (O.neg_sq_dist, float32) where the list overflows."""
    B, N = cnt.shape
    ovf = cnt > CAP
    W = np.zeros((B, N, N), dtype=np.float64)
    b, i, s = np.nonzero((np.arange(CAP)[None, None, :] < cnt[..., None]) & ~ovf[..., None])
    W[b, i, idx[b, i, s]] = 1.0
    W[ovf] = (a[ovf] >= kth[ovf][:, None]).astype(np.float64)
    return W


def block_ref(st, b, x, W, knn, has_next):
    """One ProxyConv block after its leading conv (the body of O.forward's loop): x (B, N, 64), W = neighbour_sets(...) ->
    (out, x_next or None)."""
    xm = O.neighbour_mean(x, mask=W, k=knn)
    t = xm - x
    t = O.conv1d(st, t, "fastdgcnn/conv%d_a" % b, False, None)
    t = O.conv1d(st, t, "fastdgcnn/conv%d_b" % b, False, None)
    out = t + xm
    return out, (O.conv1d(st, out, "fastdgcnn/conv%d" % (b + 1), False, None) if has_next else None)


def conv5_assign_ref(st, cat, n):
    """cat (M, 256) -> feat (M, 1024) un-normalised, rnorm (M), assign (M, 64), apart (M / 32, 64)."""
    feat = O.conv1d(st, cat, "fastdgcnn/conv5", False, None)
    rnorm = 1.0 / np.sqrt(np.maximum(np.sum(feat * feat, axis=1), O.L2_EPS))
    O._vlad_core(st, O.l2_normalize(feat, 1), n, False)
    assign = st.taps["vlad_assign"]
    return feat, rnorm, assign, assign.reshape(-1, TILE, 64).sum(1)


def aggregate_ref(featn, assign, a_sum, centres):
    """loupe.py:276-292 from the aggregate's own operands: featn (B, N, 1024) = feat * rnorm, assign (B, N, 64), a_sum (B, 64),
    centres (1024, 64) -> V (B, 1024, 64), colss (B, 32, 64) = the sums of V^2 over each chunk of 32 features."""
    V = np.matmul(np.transpose(featn, (0, 2, 1)), assign) - a_sum[:, None, :] * centres[None]
    return V, (V * V).reshape(V.shape[0], 32, 32, 64).sum(2)


def vlad_head_ref(st, V, groups):
    """O._vlad_core's and O.g_vlad_forward's tail + the final L2 (models/epc-net.py:153): V (B, 1024, 64) -> (B, 256)."""
    v = O.l2_normalize(V, 1)
    v = O.l2_normalize(v.reshape(-1, 65536), 1)
    v = np.matmul(v.reshape(-1, 65536 // groups), st.w["VLAD/hidden1_weights"])
    v = O.slim_batch_norm(st, v, "VLAD/bn", False, fused=True)
    v = v.reshape(-1, groups, v.shape[-1]).sum(-2)
    return O.l2_normalize(O.context_gating(st, v, False), 1)


def maxpool_ref(st, cat, nc, n):
    """cat (nc * n, 128) -> pooled (nc, 1024)."""
    return O.conv1d(st, cat.reshape(nc, n, -1), "fastdgcnn/conv5", False, None).max(axis=1)


def fc_head_ref(st, pooled):
    return O.l2_normalize(O.fully_connected(st, pooled, "VLAD/fc1", False, None), 1)


# ---- the inputs' conditions (block cases) ------------------------------------------------------------------------------------------------
def list_kinds(cnt, group):
    """From per-row counts (any shape, rows of a cloud consecutive, row count a multiple of `group`): the fractions of rows with exactly
    20 entries, with 21..CAP, and overflowing, and the fraction of `group`-row passes that mix overflowing and ordinary rows."""
    c = np.asarray(cnt).reshape(-1)
    ovf = (c > CAP).reshape(-1, group)
    mixed = ovf.any(1) & ~ovf.all(1)
    return float((c == 20).mean()), float(((c > 20) & (c <= CAP)).mean()), float((c > CAP).mean()), float(mixed.mean())


def smallest_persistent_nc(cus, n=96):
    """The smallest cloud count whose f32 block launch is one persistent workgroup per CU with a remainder in the tile partition:
    ceil(tiles / 12) > CUs and tiles % CUs != 0."""
    tiles_per = n // TILE
    nc = 1
    while not (-(-(nc * tiles_per) // BLK_WAVES) > cus and (nc * tiles_per) % cus != 0):
        nc += 1
    return nc


# ---- poisoned outputs --------------------------------------------------------------------------------------------------------------------
class Poisoned:
    """An output buffer of `shape` / `dtype` filled with bytes 0xFF (NaN in f32, fp16 and bf16) with `slack_rows` further rows (of the
    shape's last dimensions) behind it: `t` is the tensor to pass, `untouched()` says whether the slack still holds the poison."""

    def __init__(self, shape, dtype, dev, slack_rows=TILE):
        item = torch.empty((), dtype=dtype).element_size()
        self.nbytes = int(np.prod(shape)) * item
        row = int(np.prod(shape[1:])) * item
        self.buf = torch.full((self.nbytes + max(slack_rows * row, 4096),), 0xFF, dtype=torch.uint8, device=dev)
        self.t = self.buf[:self.nbytes].view(dtype).reshape(shape)

    def untouched(self):
        return bool((self.buf[self.nbytes:] == 0xFF).all())


def holds_poison(t):
    """Every byte of (a slice of) a Poisoned tensor is still 0xFF."""
    return bool((t.contiguous().view(torch.uint8) == 0xFF).all())


# ---- one stage entry point alone ---------------------------------------------------------------------------------------------------------
def stage_pack(L, eng, n):
    """(cfg, packed tensor -- keep it alive --, off(stage) -> device address) of an engine's packed weights."""
    cfg = eng.cfg_for(n)
    packed = eng.packed(cfg)
    base = packed.data_ptr()
    return cfg, packed, lambda s: base + L.lib().epc_net_packed_offset(ctypes.byref(cfg), s)


def knn_graph(L, xyz):
    nc, n, _ = xyz.shape
    idx = torch.zeros((nc, n, CAP), dtype=torch.int32, device=xyz.device)
    cnt = torch.zeros((nc, n), dtype=torch.int32, device=xyz.device)
    kth = torch.zeros((nc, n), dtype=torch.float32, device=xyz.device)
    L.run.epc_knn_topk(xyz, nc, n, CAP, idx, cnt, kth)
    return idx, cnt, kth


def launch_block(L, pack_addr, fast, x, xyz, idx, u16, cnt, kth, knn, has_next, out_off, ccat=256):
    """epc_proxyconv_block_fwd alone: x (nc, n, 64) f32 (fp16 on the fast path) -> the poisoned concat buffer (nc * n, ccat), the
    poisoned x_next (nc * n, 64) (passed whether has_next or not: without it the kernel must leave it alone), status."""
    nc, n, _ = x.shape
    dev = x.device
    dt = torch.float16 if fast else torch.float32
    assert x.dtype == dt
    cat = Poisoned((nc * n, ccat), dt, dev)
    nxt = Poisoned((nc * n, 64), dt, dev)
    status = torch.zeros((nc,), dtype=torch.int32, device=dev)
    lists = idx.clamp(0, 32767).to(torch.int16) if u16 else idx      # the pipeline's 2-byte list format
    a32 = lambda t: None if fast else t.data_ptr()
    a16 = lambda t: t.data_ptr() if fast else None
    L.check(L.lib().epc_proxyconv_block_fwd(a32(x), a16(x), xyz.data_ptr(), lists.data_ptr(), 1 if u16 else 0, cnt.data_ptr(),
                                            kth.data_ptr(), CAP, pack_addr, has_next, nc, n, knn, a32(cat.t), a16(cat.t), ccat, out_off,
                                            a32(nxt.t), a16(nxt.t), status.data_ptr(), L.current_stream()))
    torch.cuda.synchronize()
    return cat, nxt, status
