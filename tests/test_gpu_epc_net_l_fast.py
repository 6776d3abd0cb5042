"""EPC-Net-L in EPC_PRECISION_FAST ("f16+f6": fp16 rows through conv1 and the two blocks, conv5 on fp16 activations against fp16
hi + MX-fp6 lo weights with the max over the points taken from the f32 accumulator, fc1 in f32) against the float32 oracle, and
what the fast path promises: EPC-Net's refusals (EPC_ERANGE at pack time; a NaN descriptor + EPC_STATUS_FP16_RANGE per cloud),
descriptors independent of the batch, the lanes and the run, and the KD student's scope.  The stage-by-stage runner lives here:
tests/helpers.run_stages drives EPC-Net-L's f32 stages only."""
import ctypes

import numpy as np
import pytest
import torch

import helpers as H
from helpers import O

# descriptor L2 error against the float32 oracle; relative max error of the stage taps block1, block2, maxpool
DESC_TOL = 1e-3
STAGE_TOL = 1e-3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X; there is no CPU fallback"
    return torch.device("cuda:0")


def _rel(a, b):
    a = a.float().cpu().numpy() if torch.is_tensor(a) else a
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _desc_err(got, ref):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    return float(np.linalg.norm(got - ref.reshape(got.shape[0], -1), axis=1).max())


def run_fast_stages(eng, xyz):
    """csrc/pipeline.hip's launch sequence for EPC-Net-L in EPC_PRECISION_FAST, stage by stage through the C ABI: Hilbert sort,
    kNN + conv1 (fp16 rows), the two fp16 blocks into the fp16 concat, epc_conv5_maxpool_f16_fwd, the fc head."""
    L = H.pkg("lib")
    lib = L.lib()
    nc, n, _ = xyz.shape
    cfg = eng.cfg_for(n)
    packed = eng.packed(cfg)
    assert cfg.precision == L.EPC_PRECISION_FAST
    off = lambda s: packed.data_ptr() + lib.epc_net_packed_offset(ctypes.byref(cfg), s)
    dev, st = xyz.device, L.current_stream()
    srt = torch.empty_like(xyz)
    perm = torch.empty((nc, n), dtype=torch.int32, device=dev)
    L.check(lib.epc_morton_sort(xyz.data_ptr(), nc, n, srt.data_ptr(), perm.data_ptr(), st))
    u16 = 1 if n <= 8192 else 0
    idx = torch.empty((nc, n, L.EPC_KNN_CAP), dtype=torch.int16 if u16 else torch.int32, device=dev)
    cnt = torch.empty((nc, n), dtype=torch.int32, device=dev)
    kth = torch.empty((nc, n), dtype=torch.float32, device=dev)
    status = torch.zeros((nc,), dtype=torch.int32, device=dev)
    xs = [torch.empty((nc, n, 64), dtype=torch.float16, device=dev) for _ in range(2)]
    cat = torch.empty((nc, n, 128), dtype=torch.float16, device=dev)
    L.check(lib.epc_knn_topk_conv1(srt.data_ptr(), nc, n, L.EPC_KNN_CAP, idx.data_ptr(), u16, cnt.data_ptr(), kth.data_ptr(), off(0),
                                   None, xs[0].data_ptr(), status.data_ptr(), st))
    x1 = xs[0].clone()
    for b in (1, 2):     # ping / pong as the pipeline uses them
        L.check(lib.epc_proxyconv_block_fwd(None, xs[(b - 1) & 1].data_ptr(), srt.data_ptr(), idx.data_ptr(), u16, cnt.data_ptr(),
                                            kth.data_ptr(), L.EPC_KNN_CAP, off(b), 1 if b == 1 else 0, nc, n, cfg.knn, None,
                                            cat.data_ptr(), 128, 64 * (b - 1), None, xs[b & 1].data_ptr(), status.data_ptr(), st))
    pooled = torch.empty((nc, 1024), dtype=torch.float32, device=dev)
    L.check(lib.epc_conv5_maxpool_f16_fwd(cat.data_ptr(), 128, off(5), nc, n, pooled.data_ptr(), st))
    desc = torch.empty((nc, 256), dtype=torch.float32, device=dev)
    L.check(lib.epc_fc_head_fwd(pooled.data_ptr(), off(6), nc, desc.data_ptr(), status.data_ptr(), st))
    torch.cuda.synchronize()
    return dict(sorted=srt, x1=x1, cat=cat, pooled=pooled, desc=desc, status=status)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n", [("uniform", 256), ("lidar", 512), ("dup", 128), ("zeros", 64)])
def test_stages_against_oracle(dev, kind, n):
    """Every stage boundary of the fast chain against the oracle's taps (the oracle runs on the Hilbert-sorted clouds, so that the
    per-point taps line up), and the pipeline's descriptor equal to this chain's bit for bit."""
    w = O.seeded_weights("epc-net-l", 1)
    eng, _ = H.make_engine("epc-net-l", w, dev, precision="fast")
    x = torch.from_numpy(O.synthetic_clouds(3, n, 5, kind)).to(dev)
    got = run_fast_stages(eng, x)
    ref, st = O.forward(got["sorted"].cpu().numpy()[:, None], w, arch="epc-net-l")
    assert int(got["status"].abs().sum()) == 0
    errs = {"conv1": _rel(got["x1"], st.taps["fastdgcnn/conv1"]), "block1": _rel(got["cat"][..., :64], st.taps["block1"]),
            "block2": _rel(got["cat"][..., 64:], st.taps["block2"]), "maxpool": _rel(got["pooled"], st.taps["maxpool"])}
    err = _desc_err(got["desc"], ref)
    print("EPC-Net-L fast %s n=%d: conv1 %.2e block1 %.2e block2 %.2e maxpool %.2e descriptor %.3e" % (
        kind, n, errs["conv1"], errs["block1"], errs["block2"], errs["maxpool"], err))
    assert errs["conv1"] <= 2.0 ** -11                 # one fp16 rounding of the f32 conv1 output
    for tap in ("block1", "block2", "maxpool"):
        assert errs[tap] <= STAGE_TOL, "%s: %.3e" % (tap, errs[tap])
    assert err <= DESC_TOL
    assert torch.equal(eng.forward(x), got["desc"])


@pytest.mark.gpu
def test_drop_in_forward_with_precision_fast(dev):
    """MODEL.forward(point_cloud, False, params=dict(PARAMS, PRECISION="fast")) at 1 x 3 x 4096: the key reaches the engine with no
    change to models/epc-net-l.py, and the engine reports the arithmetic that ran."""
    V, C = H.pkg("variables"), H.pkg("models._common")
    pc = O.synthetic_clouds(3, 4096, 11).reshape(1, 3, 4096, 3)
    w = O.seeded_weights("epc-net-l", 3)
    ref, _ = O.forward(pc, w, arch="epc-net-l")
    H.make_store("epc-net-l", w, dev)
    M = H.pkg("models.epc-net-l")
    params = dict(H.PARAMS, PRECISION="fast")
    with V.variable_scope(H.OUTER):
        x = M.placeholder_inputs(1, 3, 4096, 3)
        x.copy_(torch.from_numpy(pc))
        out = M.forward(x, False, bn_decay=None, params=params)
        eng = C.engine_for("epc-net-l", params)
    assert eng.resolved_precision == "fast"
    assert tuple(out.shape) == (1, 3, 256)
    out = out.cpu().numpy()
    assert np.allclose(np.linalg.norm(out, axis=-1), 1.0, atol=1e-5)
    err = float(np.linalg.norm(out - ref, axis=-1).max())
    print("EPC-Net-L fast full-size descriptor L2 error: %.3e" % err)
    assert err <= DESC_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("nc,n,kind,micro", [
    (3, 160, "lidar", 0),            # workgroups straddle clouds: per-wave atomics
    (2, 8192, "uniform", 1),
    (2, 32, "dup", 0),               # smallest legal cloud, inactive waves in the workgroup
    (1, 8192 + 64, "uniform", 0),    # streaming kNN, separate conv1 launch
])
def test_edge_shapes(dev, nc, n, kind, micro):
    pc = O.synthetic_clouds(nc, n, 17, kind)
    w = O.seeded_weights("epc-net-l", 6)
    _, lists = O.knn_lists(pc)
    ref, _ = O.forward(pc[:, None], w, arch="epc-net-l", formulation="lists", lists=lists)
    eng, _ = H.make_engine("epc-net-l", w, dev, micro_batch=micro, precision="fast")
    out = eng.forward(torch.from_numpy(pc).to(dev))
    assert bool(torch.isfinite(out).all())
    err = _desc_err(out, ref)
    print("EPC-Net-L fast edge shape %dx%d %s: descriptor L2 error %.3e" % (nc, n, kind, err))
    assert err <= DESC_TOL


@pytest.mark.gpu
def test_descriptor_does_not_depend_on_position_lanes_or_run(dev):
    """256 x 4096 as two 128-cloud halves in flight and as InferenceEngine.forward's default for the fast arithmetic (one lane, one
    256-cloud pass): a cloud gets the same bits alone, at other positions of the batch, on either form, and in a second run."""
    E = H.pkg("engine")
    w = O.seeded_weights("epc-net-l", 0)
    st = H.make_store("epc-net-l", w, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    x = torch.rand((256, 4096, 3), generator=g, device=dev) * 2 - 1
    eng = E.InferenceEngine("epc-net-l", H.PARAMS, st, outer=H.OUTER, precision="fast", in_flight=2)
    out = eng.forward(x).clone()
    assert bool(torch.isfinite(out).all()) and eng.last_status(256) == [0] * 256
    assert torch.equal(eng.forward(x), out)
    default = E.InferenceEngine("epc-net-l", H.PARAMS, st, outer=H.OUTER, precision="fast")
    assert default.in_flight == 1
    assert torch.equal(default.forward(x), out)
    for i in (0, 131, 255):
        assert torch.equal(eng.forward(x[i:i + 1])[0], out[i])
    rolled = eng.forward(torch.roll(x, shifts=37, dims=0))
    assert torch.equal(rolled[(131 + 37) % 256], out[131]) and torch.equal(rolled[36], out[255])


def test_export_exists_and_fast_workspace_holds_fp16_rows():
    """Host-side: the stage export is bound, and in FAST the ping / pong rows and the 128-channel concat take 2 bytes per value."""
    L, E = H.pkg("lib"), H.pkg("engine")
    assert "epc_conv5_maxpool_f16_fwd" in L.EXPORTS and hasattr(L.lib(), "epc_conv5_maxpool_f16_fwd")
    f32 = E.make_cfg("epc-net-l", 4096, H.PARAMS, precision="f32")
    fast = E.make_cfg("epc-net-l", 4096, H.PARAMS, precision="fast")
    ws32 = L.lib().epc_net_workspace_bytes(ctypes.byref(f32), 256)
    ws16 = L.lib().epc_net_workspace_bytes(ctypes.byref(fast), 256)
    assert ws32 - ws16 == 256 * 4096 * (64 + 64 + 128) * 2
    assert L.lib().epc_net_packed_bytes(ctypes.byref(f32)) == L.lib().epc_net_packed_bytes(ctypes.byref(fast))


@pytest.mark.gpu
def test_fast_descriptor_is_not_the_f32_one_but_within_the_bar(dev):
    w = O.seeded_weights("epc-net-l", 2)
    pc = O.synthetic_clouds(2, 1024, 4)
    ref, _ = O.forward(pc[:, None], w, arch="epc-net-l")
    x = torch.from_numpy(pc).to(dev)
    fast, _ = H.make_engine("epc-net-l", w, dev, precision="fast")
    f32, _ = H.make_engine("epc-net-l", w, dev, precision="f32")
    a, b = fast.forward(x), f32.forward(x)
    assert fast.resolved_precision == "fast" and f32.resolved_precision == "f32"
    assert not torch.equal(a, b)
    assert _desc_err(a, ref) <= DESC_TOL


@pytest.mark.gpu
def test_out_of_range_conv5_weights_are_refused_in_fast_and_packed_in_f32(dev):
    """A tiny conv5 moving variance.  BatchNorm's epsilon (1e-3) caps 1 / sqrt(var + eps) at 31.6, so the folded |W' * 256| passes
    65504 only together with a large gamma: EPC_ERANGE in FAST (never a packed Inf), a finite result in F32."""
    L = H.pkg("lib")
    w = O.seeded_weights("epc-net-l", 0)
    _, var = O.ema_names("fastdgcnn/conv5")
    w[var] = np.full_like(w[var], 1e-8)
    w["fastdgcnn/conv5/bn/gamma"] = np.full_like(w["fastdgcnn/conv5/bn/gamma"], 1000.0)
    pc = torch.from_numpy(O.synthetic_clouds(2, 256, 1)).to(dev)
    fast, _ = H.make_engine("epc-net-l", w, dev, precision="fast")
    with pytest.raises(L.EpcNetError) as ei:
        fast.forward(pc)
    assert ei.value.status == L.EPC_ERANGE and "EPC_PRECISION_F32" in str(ei.value)
    f32, _ = H.make_engine("epc-net-l", w, dev, precision="f32")
    assert bool(torch.isfinite(f32.forward(pc)).all())


@pytest.mark.gpu
def test_fp16_range_flag_nan_and_check_reextracts_in_f32(dev):
    """Coordinates scaled by 1e6 drive conv1 out of fp16: that cloud is flagged and NaN, the others are untouched; check=True
    returns the f32 engine's descriptor for it, bit for bit."""
    L = H.pkg("lib")
    w = O.seeded_weights("epc-net-l", 1)
    pc = O.synthetic_clouds(3, 512, 3)
    pc[1] *= 1e6
    ref, _ = O.forward(pc[[0, 2]][:, None], w, arch="epc-net-l")
    x = torch.from_numpy(pc).to(dev)
    fast, _ = H.make_engine("epc-net-l", w, dev, precision="fast")
    out = fast.forward(x, check=False).clone()
    assert fast.last_status(3) == [0, L.EPC_STATUS_FP16_RANGE, 0]
    assert bool(torch.isnan(out[1]).all()) and bool(torch.isfinite(out[[0, 2]]).all())
    assert _desc_err(out[[0, 2]], ref) <= DESC_TOL
    f32, _ = H.make_engine("epc-net-l", w, dev, precision="f32")
    want = f32.forward(x)
    got = fast.forward(x, check=True)
    assert torch.equal(got[1], want[1])
    assert torch.equal(got[0], out[0]) and torch.equal(got[2], out[2])


@pytest.mark.gpu
def test_nan_coordinate_still_sets_bit_0(dev):
    L = H.pkg("lib")
    w = O.seeded_weights("epc-net-l", 0)
    pc = O.synthetic_clouds(2, 256, 9)
    pc[0, 5, 1] = np.nan
    eng, _ = H.make_engine("epc-net-l", w, dev, precision="fast")
    out = eng.forward(torch.from_numpy(pc).to(dev))
    status = eng.last_status(2)
    assert status[0] & L.EPC_STATUS_NONFINITE_INPUT and status[1] == 0
    assert bool(torch.isnan(out[0]).all()) and bool(torch.isfinite(out[1]).all())


@pytest.mark.gpu
def test_kd_student_scope_gives_the_same_bits(dev):
    """models/kd_epc-net-l.py (backbone under BACKBONE) with PRECISION="fast" against the fastdgcnn-scoped engine on the same
    weights: the same descriptor bits."""
    V, C = H.pkg("variables"), H.pkg("models._common")
    KDL = H.pkg("models.kd_epc-net-l")
    w = O.seeded_weights("epc-net-l", 4)
    x = torch.from_numpy(O.synthetic_clouds(2, 1024, 8)).to(dev)
    params = dict(H.PARAMS, PRECISION="fast")
    plain, _ = H.make_engine("epc-net-l", w, dev, precision="fast")
    want = plain.forward(x)
    st = V.reset_default_store(device=dev, seed=0)
    with V.variable_scope(H.OUTER):
        KDL.declare_variables(params, 1024)
    st.load_state_dict({(H.OUTER + "/" + k).replace("/fastdgcnn/", "/BACKBONE/"): v for k, v in w.items()}, strict=True)
    with V.variable_scope(H.OUTER):
        got = KDL.descriptors(x.reshape(1, 2, 1024, 3), params)
        eng = C.engine_for("epc-net-l", params, backbone_scope="BACKBONE")
    assert eng.resolved_precision == "fast"
    assert torch.equal(got.reshape(2, -1), want)
