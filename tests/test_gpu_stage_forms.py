"""Every inference stage entry point ALONE, at the shapes where its launch changes form, against a float64 restatement of the same
stage fed the same stage input (tests/stage_ref.py; tests/test_stage_forms_cpu.py checks those restatements and the fragment decoders
without a GPU).  The whole-pipeline stage tests (test_stages_against_oracle) run three small clouds through 1 to 4 workgroups; the
descriptor-level tests average a few wrong rows, a dropped tile or a mis-added partial away.  Here:

  * the block kernels on neighbour lists of 20, 21..32 and more than 32 entries mixed inside every pass, on one workgroup, on a grid
    with a remainder in the f32 kernel's tile partition and a partly filled last fp16 workgroup, and (f32) on the persistent
    one-workgroup-per-CU launch with a remainder -- with 2-byte and 4-byte lists, with and without the next block's conv, into a
    slice of the concat buffer;
  * conv5 + assignment and then the VLAD aggregate, in both arithmetics, on one-tile clouds (empty second half, a second group of 8
    clouds), an odd tile count, and 72 tiles (the 8-wide pass over the a_sum partials);
  * conv5 + max-pool, f32 and fp16, with workgroups that straddle clouds whose maxima differ;
  * the VLAD head for GROUPS 1, 4 and 16 on 1 and 65 clouds (the hidden GEMM's third grid dimension), the fc head on 65.

Every output buffer is filled with bytes 0xFF (NaN) before the call and has slack behind it that must still hold them afterwards.
The input of a stage is random -- rows with a power-of-two scale each, spread over 2^-6 .. 2^6 -- not the previous stage's output; on
the fast path it is rounded to fp16 first and both sides get the rounded values.  The bars are those of test_stages_against_oracle
(tests/test_gpu_parity.py, tests/test_gpu_epc_net_l_fast.py): a stage alone on exact inputs cannot need more."""
import functools

import numpy as np
import pytest
import torch

import helpers as H
import stage_ref as R
from helpers import O

pytestmark = pytest.mark.gpu

BLOCK_SEED = 7     # (tests/test_stage_forms_cpu.py checks these clouds' lists with the oracle alone)
DESC_TOL = 1e-4    # descriptor L2 error of the heads (both run in f32)


def stage_tol(fast):
    """Relative to the tensor's largest magnitude: block rows, feat and the max-pool of the fast kernels 1e-3, every f32-equivalent
    stage 2e-5."""
    return 1e-3 if fast else 2e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X; there is no CPU fallback"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _weights(arch, groups=4):
    return O.seeded_weights(arch, 1, params=dict(H.PARAMS, GROUPS=groups))


def _engine(arch, dev, prec, groups=4):
    eng, _ = H.make_engine(arch, _weights(arch, groups), dev, precision=prec, params=dict(H.PARAMS, GROUPS=groups))
    return eng


def _f64(t):
    return t.detach().double().cpu().numpy()


def _rel(got, want):
    got = _f64(got) if torch.is_tensor(got) else got
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


def _with_slack(a, dtype, dev, rows=8 * R.TILE):
    """The rows `a` (numpy, 2-D) as a device tensor of `dtype` with `rows` rows of zeros behind it (a kernel's inactive waves)."""
    buf = torch.zeros((a.shape[0] + rows, a.shape[1]), dtype=dtype, device=dev)
    buf[:a.shape[0]] = torch.from_numpy(a).to(dev).to(dtype)
    return buf[:a.shape[0]]


# ---- ProxyConv block ---------------------------------------------------------------------------------------------------------------------
# (block b of EPC-Net, has_next, 2-byte lists, out_off): the first block with the next block's conv and epc_knn_topk's 4-byte lists, the
# last block without it and with the pipeline's 2-byte lists; both into the middle of the 256-column concat
BLOCK_FORMS = [(1, 1, False, 64), (4, 0, True, 128)]


def _block_case(dev, prec, nc, form, oracle_clouds):
    fast = prec == "fast"
    b, has_next, u16, out_off = form
    n = 96
    L = H.pkg("lib")
    eng = _engine("epc-net", dev, prec)
    cfg, packed, off = R.stage_pack(L, eng, n)
    assert eng.resolved_precision == prec
    pc = O.synthetic_clouds(nc, n, BLOCK_SEED, "repeat30")
    xyz = torch.from_numpy(pc).to(dev)
    idx, cnt, kth = R.knn_graph(L, xyz)
    torch.cuda.synchronize()
    idx_c, cnt_c, kth_c = idx.cpu().numpy(), cnt.cpu().numpy(), kth.cpu().numpy()
    # the graph is the oracle's
    kth_ref, lists = O.knn_lists(pc[oracle_clouds])
    for bi, c in enumerate(oracle_clouds):
        assert np.array_equal(kth_c[c], kth_ref[bi])
        for i in range(n):
            ref = lists[bi][i]
            assert cnt_c[c, i] == len(ref)
            m = min(len(ref), R.CAP)
            assert np.array_equal(idx_c[c, i, :m], ref[:m])
    # the input's condition, from the kernel's own counts
    plain, tail, ovf, mixed = R.list_kinds(cnt_c, 8 if fast else 4)
    assert min(plain, tail, ovf) >= 0.10 and mixed >= 0.25, (plain, tail, ovf, mixed)

    x_np = R.rows_with_scales(np.random.RandomState(100 * b + nc), nc * n, 64)
    x = _with_slack(x_np, torch.float16 if fast else torch.float32, dev).reshape(nc, n, 64)
    cat, nxt, status = R.launch_block(L, off(b), fast, x, xyz, idx, u16, cnt, kth, cfg.knn, has_next, out_off)

    W = R.neighbour_sets(idx_c, cnt_c, O.neg_sq_dist(pc), kth_c)
    out_ref, nxt_ref = R.block_ref(R.state64(_weights("epc-net")), b, _f64(x), W, cfg.knn, has_next)
    got = cat.t[:, out_off:out_off + 64]
    assert bool(torch.isfinite(got).all()), "rows of the concat slice were not written"
    e_out = _rel(got, out_ref.reshape(-1, 64))
    e_nxt = _rel(nxt.t, nxt_ref.reshape(-1, 64)) if has_next else 0.0
    print("block %s %d x %d, block %d, %s lists: out %.3e x_next %.3e (rows: 20 entries %.2f, 21..32 %.2f, overflow %.2f; mixed passes "
          "%.2f)" % (prec, nc, n, b, "2-byte" if u16 else "4-byte", e_out, e_nxt, plain, tail, ovf, mixed))
    assert e_out <= stage_tol(fast) and e_nxt <= stage_tol(fast)
    assert int(status.abs().sum()) == 0
    assert cat.untouched() and nxt.untouched(), "a write behind the last row"
    assert R.holds_poison(cat.t[:, :out_off]) and R.holds_poison(cat.t[:, out_off + 64:]), "a write outside the concat slice"
    if not has_next:
        assert R.holds_poison(nxt.t), "x_next written without has_next"


@pytest.mark.parametrize("form", BLOCK_FORMS, ids=["b1-next-i32", "b4-last-u16"])
@pytest.mark.parametrize("nc", [3, 50])
@pytest.mark.parametrize("prec", ["f32", "fast"])
def test_block_alone_on_lists_of_every_length(dev, prec, nc, form):
    """3 x 96: 9 tiles, one workgroup.  50 x 96: 150 tiles -- the f32 grid is 13 workgroups (11 tiles each, 7 of them one more; the XCD
    split of the 13 is 5 XCDs of two workgroups and 3 of one), the fp16 grid 10 workgroups of 16 tiles, the last with 6."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = nc * 3
    if prec == "f32":
        wgs = -(-tiles // R.BLK_WAVES)
        assert wgs <= cus, "a short-workgroup grid (no persistent launch)"
        assert (wgs, tiles % wgs, wgs & 7) == ((1, 0, 1) if nc == 3 else (13, 7, 5))
    else:
        assert (-(-tiles // R.BLK16_WAVES), tiles % R.BLK16_WAVES) == ((1, 9) if nc == 3 else (10, 6))
    _block_case(dev, prec, nc, form, list(range(nc)))


def test_f32_block_alone_on_the_persistent_launch_with_a_remainder(dev):
    """What every full-size pass runs: more than 12 * CUs tiles make the f32 launch one persistent workgroup per CU, each walking a
    balanced share of the tiles.  The smallest cloud count with a remainder in that partition (256 CUs: 1025 clouds of 96 points,
    3075 tiles = 12 per workgroup and 3 left over)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nc = R.smallest_persistent_nc(cus)
    tiles = 3 * nc
    assert -(-tiles // R.BLK_WAVES) > cus and tiles % cus != 0 and -(-tiles // R.BLK_WAVES) <= 4096 * cus
    _block_case(dev, "f32", nc, BLOCK_FORMS[0], list(range(8)) + list(range(nc // 2 - 4, nc // 2 + 4)) + list(range(nc - 8, nc)))


# ---- conv5 + assignment, then the aggregate ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc,n", [(9, 32), (3, 96), (2, 160), (2, 2304)])
@pytest.mark.parametrize("prec", ["f32", "fast"])
def test_conv5_assign_then_aggregate_alone(dev, prec, nc, n):
    """9 x 32: one tile per cloud (the aggregate's second half is empty), a second group of 8 clouds, idle aggregate workgroups.
    3 x 96: an odd tile count; 9 tiles, a partly active conv5 workgroup.  2 x 160: 5 tiles, halves of 3 and 2 -- the aggregate takes
    two tiles per turn of its loop, so at 3 tiles a half shortened by one tile still gets through; at 5 it does not.  2 x 2304: 72 tiles -- each aggregate wave's eighth of the
    a_sum partials is 9 tiles, one 8-wide pass and a tail of one.  Cloud b's rows are scaled by b + 1."""
    fast = prec == "fast"
    L = H.pkg("lib")
    lib = L.lib()
    eng = _engine("epc-net", dev, prec)
    cfg, packed, off = R.stage_pack(L, eng, n)
    assert eng.resolved_precision == prec
    M, tiles = nc * n, nc * n // 32
    assert (n // 32) % 2 == 1 or n // 32 >= 57
    w = _weights("epc-net")
    cat_np = R.rows_with_scales(np.random.RandomState(1000 * nc + n), M, 256, cloud_scale=np.arange(1, nc + 1), n=n)
    cat = _with_slack(cat_np, torch.float16 if fast else torch.float32, dev)
    featf = R.Poisoned((tiles, 32, 2, 64, 8), torch.float16, dev, 1) if fast else R.Poisoned((tiles, 32, 3, 64, 16), torch.uint8, dev, 1)
    assignf = (R.Poisoned((tiles, 2, 2, 64, 8), torch.float16, dev, 1) if fast else
               R.Poisoned((tiles, 2, 2, 2, 64, 8), torch.bfloat16, dev, 1))
    rnorm = R.Poisoned((M,), torch.float32, dev)
    assign = R.Poisoned((M, 64), torch.float32, dev)
    apart = R.Poisoned((tiles, 64), torch.float32, dev, 1)
    status = torch.zeros((nc,), dtype=torch.int32, device=dev)
    st = L.current_stream()
    if fast:
        L.check(lib.epc_conv5_assign_fwd(cat.data_ptr(), 1, 256, off(5), M, n, featf.t.data_ptr(), rnorm.t.data_ptr(),
                                         assign.t.data_ptr(), assignf.t.data_ptr(), apart.t.data_ptr(), status.data_ptr(), st))
    else:
        L.check(lib.epc_conv5_assign_f32_fwd(cat.data_ptr(), 256, off(5), M, featf.t.data_ptr(), rnorm.t.data_ptr(), assign.t.data_ptr(),
                                             assignf.t.data_ptr(), apart.t.data_ptr(), st))
    torch.cuda.synchronize()
    for name, p in (("feat", featf), ("assign fragments", assignf), ("rnorm", rnorm), ("assign", assign), ("apart", apart)):
        assert p.untouched(), "%s: a write behind the buffer" % name
    feat = R.decode_feat_f16(featf.t, M) if fast else R.decode_feat_b3(featf.t, M)
    afrag = R.decode_assign_f16(assignf.t, M) if fast else R.decode_assign_bf16x2(assignf.t, M)
    for name, t in (("feat", feat), ("assign fragments", afrag), ("rnorm", rnorm.t), ("assign", assign.t), ("apart", apart.t)):
        assert bool(torch.isfinite(t).all()), "%s: not every element was written" % name
    assert int(status.abs().sum()) == 0

    feat_ref, rnorm_ref, assign_ref, apart_ref = R.conv5_assign_ref(R.state64(w), _f64(cat), n)
    atol = 1e-4 if fast else 2e-5                    # assign
    ftol = 2.0 ** -11 if fast else 2.0 ** -16        # the fragments' format: fp16 / bf16 hi + lo of the f32 assignment
    e_feat = _rel(feat, feat_ref)
    # rnorm spans the 2^12 of the row scales, so it is compared per row: rnorm * |feat row| against 1.  The arithmetic of either conv5
    # is free of the row's scale (f32: a power-of-two scale per row; fast: the fp16 inputs are exact, accumulation is f32), so a row's
    # norm is as good relative to itself as feat is relative to its largest value on rows of one scale: the feat bar.
    e_rn = float(np.abs(_f64(rnorm.t) / rnorm_ref - 1.0).max())
    e_as = _rel(assign.t, assign_ref)
    e_fr_own = _rel(afrag, _f64(assign.t))
    e_fr = _rel(afrag, assign_ref)
    # a tile's partial is the sum of 32 assignments, each inside the assign bar
    e_ap = float(np.abs(_f64(apart.t) - apart_ref).max() / (32 * np.abs(assign_ref).max()))
    print("conv5 + assign %s %d x %d: feat %.3e rnorm %.3e assign %.3e fragments %.3e (of the kernel's own assign: %.3e) apart %.3e" % (
        prec, nc, n, e_feat, e_rn, e_as, e_fr, e_fr_own, e_ap))
    assert e_feat <= stage_tol(fast) and e_rn <= stage_tol(fast)
    assert e_as <= atol and e_fr_own <= ftol and e_fr <= atol + ftol and e_ap <= atol

    # the aggregate, from ITS inputs: the decoded feat, rnorm and assignment fragments, a_sum from apart
    V = R.Poisoned((nc, 1024, 64), torch.float32, dev, 1)
    colss = R.Poisoned((nc, 32, 64), torch.float32, dev, 1)
    fn = lib.epc_vlad_aggregate_fwd if fast else lib.epc_vlad_aggregate_f32_fwd
    L.check(fn(featf.t.data_ptr(), assignf.t.data_ptr(), rnorm.t.data_ptr(), apart.t.data_ptr(), off(6), nc, n, V.t.data_ptr(),
               colss.t.data_ptr(), st))
    torch.cuda.synchronize()
    assert V.untouched() and colss.untouched()
    assert bool(torch.isfinite(V.t).all()) and bool(torch.isfinite(colss.t).all())
    featn = (_f64(feat) * _f64(rnorm.t)[:, None]).reshape(nc, n, 1024)
    a_sum = _f64(apart.t).reshape(nc, n // 32, 64).sum(1)
    centres = w["VLAD/cluster_weights2"].astype(np.float64).reshape(1024, 64)
    V_ref, _ = R.aggregate_ref(featn, _f64(afrag).reshape(nc, n, 64), a_sum, centres)
    e_v = _rel(V.t, V_ref)
    e_v_cloud = max(_rel(V.t[b], V_ref[b]) for b in range(nc))
    colss_own = (_f64(V.t) ** 2).reshape(nc, 32, 32, 64).sum(2)
    e_c = _rel(colss.t, colss_own)
    print("aggregate %s %d x %d: vlad %.3e (worst cloud %.3e) column sums of squares %.3e" % (prec, nc, n, e_v, e_v_cloud, e_c))
    assert e_v <= (2.0 ** -11 if fast else 2e-5)
    assert e_c <= 1e-5


# ---- conv5 + max-pool --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc,n", [(5, 96), (3, 160), (3, 128)])
@pytest.mark.parametrize("prec", ["f32", "fast"])
def test_conv5_maxpool_alone(dev, prec, nc, n):
    """Workgroups of four 32-point tiles.  5 x 96: the first covers cloud 0's three tiles and cloud 1's first; 3 x 160: straddling
    workgroups (per-wave atomics to the wave's own cloud); 3 x 128: one-cloud workgroups (the maxima meet in LDS).  Cloud b's rows are
    scaled by b + 1, so the clouds' maxima differ and one sent to the wrong cloud shows; pooled is poisoned although the launcher
    clears it, because clearing it is part of what is under test."""
    fast = prec == "fast"
    L = H.pkg("lib")
    lib = L.lib()
    eng = _engine("epc-net-l", dev, prec)
    cfg, packed, off = R.stage_pack(L, eng, n)
    assert eng.resolved_precision == prec
    assert (n % 128 == 0) == (n == 128)
    M = nc * n
    cat_np = R.rows_with_scales(np.random.RandomState(1000 * nc + n), M, 128, cloud_scale=np.arange(1, nc + 1), n=n)
    cat = _with_slack(cat_np, torch.float16 if fast else torch.float32, dev)
    pooled = R.Poisoned((nc, 1024), torch.float32, dev, 1)
    fn = lib.epc_conv5_maxpool_f16_fwd if fast else lib.epc_conv5_maxpool_fwd
    L.check(fn(cat.data_ptr(), 128, off(5), nc, n, pooled.t.data_ptr(), L.current_stream()))
    torch.cuda.synchronize()
    assert pooled.untouched()
    assert bool(torch.isfinite(pooled.t).all())
    ref = R.maxpool_ref(R.state64(_weights("epc-net-l")), _f64(cat), nc, n)
    assert len({float(v) for v in ref.max(1)}) == nc
    err = _rel(pooled.t, ref)
    print("conv5 + max-pool %s %d x %d: %.3e" % (prec, nc, n, err))
    assert err <= stage_tol(fast)


# ---- heads -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", [1, 65])
@pytest.mark.parametrize("groups", [1, 4, 16])
def test_vlad_head_alone(dev, groups, nc):
    """Intra-normalisation, global norm, the grouped projection folded before the GEMM, BN, gating and L2 for the GROUPS the head
    dispatches on; 65 clouds give hidden_gemm_kernel a second 64-row group with clamped row pointers and zero masks.  V is random with a
    scale per (cloud, cluster) column; one flagged cloud must leave as NaN and disturb nobody."""
    L = H.pkg("lib")
    lib = L.lib()
    eng = _engine("epc-net", dev, "f32", groups)
    cfg, packed, off = R.stage_pack(L, eng, 32)
    assert cfg.groups == groups and (nc > 64) == (nc == 65)
    rng = np.random.RandomState(10 * groups + nc)
    V_np = (rng.randn(nc, 1024, 64) * np.exp2(rng.randint(-6, 7, size=(nc, 1, 64)).astype(np.float64))).astype(np.float32)
    colss_np = (V_np.astype(np.float64) ** 2).reshape(nc, 32, 32, 64).sum(2).astype(np.float32)
    V, colss = torch.from_numpy(V_np).to(dev), torch.from_numpy(colss_np).to(dev)
    flagged = 31 if nc > 1 else None
    status = torch.zeros((nc,), dtype=torch.int32, device=dev)
    if flagged is not None:
        status[flagged] = L.EPC_STATUS_FP16_RANGE
    out = R.Poisoned((nc, 256), torch.float32, dev)
    wsb = lib.epc_vlad_head_workspace_bytes(nc, groups)
    assert wsb > 0
    ws = R.Poisoned((wsb,), torch.uint8, dev)
    L.check(lib.epc_vlad_head_fwd(V.data_ptr(), colss.data_ptr(), off(6), groups, nc, out.t.data_ptr(), status.data_ptr(),
                                  ws.t.data_ptr(), wsb, L.current_stream()))
    torch.cuda.synchronize()
    assert out.untouched() and ws.untouched()
    ref = R.vlad_head_ref(R.state64(_weights("epc-net", groups)), V_np.astype(np.float64), groups)
    got = _f64(out.t)
    keep = np.arange(nc) != (-1 if flagged is None else flagged)
    if flagged is not None:
        assert np.isnan(got[flagged]).all()
    err = float(np.linalg.norm(got[keep] - ref[keep], axis=1).max())
    print("vlad head GROUPS=%d %d clouds: descriptor L2 error %.3e" % (groups, nc, err))
    assert err <= DESC_TOL


def test_fc_head_alone_on_65_clouds(dev):
    L = H.pkg("lib")
    eng = _engine("epc-net-l", dev, "f32")
    cfg, packed, off = R.stage_pack(L, eng, 32)
    nc, flagged = 65, 40
    pooled_np = np.abs(R.rows_with_scales(np.random.RandomState(65), nc, 1024))      # (a maximum of ReLU outputs: >= 0)
    pooled = torch.from_numpy(pooled_np).to(dev)
    status = torch.zeros((nc,), dtype=torch.int32, device=dev)
    status[flagged] = L.EPC_STATUS_NONFINITE_INPUT
    out = R.Poisoned((nc, 256), torch.float32, dev)
    L.check(L.lib().epc_fc_head_fwd(pooled.data_ptr(), off(6), nc, out.t.data_ptr(), status.data_ptr(), L.current_stream()))
    torch.cuda.synchronize()
    assert out.untouched()
    ref = R.fc_head_ref(R.state64(_weights("epc-net-l")), pooled_np.astype(np.float64))
    got = _f64(out.t)
    keep = np.arange(nc) != flagged
    assert np.isnan(got[flagged]).all()
    err = float(np.linalg.norm(got[keep] - ref[keep], axis=1).max())
    print("fc head %d clouds: descriptor L2 error %.3e" % (nc, err))
    assert err <= DESC_TOL
