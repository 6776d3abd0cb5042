"""Inference from the records of a cloud bank (InferenceEngine.forward_bank, csrc/graph_bank.hip: epc_bank_gather_infer,
csrc/pipeline.hip: epc_net_forward_bank).  The bank changes where the sorted cloud and its graph come from, never what is computed
from them: forward_bank(bank, ids) is engine.forward(xyz[ids]) bit for bit, status words included.  EVERY comparison here is
torch.equal on the bit patterns (NaN descriptors must compare equal); the feature has no tolerance anywhere."""
import ctypes

import numpy as np
import pytest
import torch

import helpers as H
from helpers import O

pytestmark = pytest.mark.gpu
CAP = 32


@pytest.fixture
def dev():
    return torch.device("cuda:0")


def _hub_cloud(n, seed, m=68):
    """tests/test_gpu_cloud_bank.py: m points evenly on the unit sphere around a centre point that all of them list, the rest far away."""
    rng = np.random.RandomState(seed)
    k = np.arange(m) + 0.5
    phi, th = np.arccos(1 - 2 * k / m), np.pi * (1 + 5 ** 0.5) * k
    shell = np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], 1) * (1 + 1e-3 * rng.uniform(-1, 1, (m, 1)))
    rest = rng.uniform(-1, 1, (n - m - 1, 3)) + np.array([40.0, 0, 0])
    pc = np.concatenate([np.zeros((1, 3)), shell, rest], 0)
    return np.ascontiguousarray(pc[rng.permutation(n)][None], dtype=np.float32)


def _bank_clouds(n):
    """The ~40 clouds of tests/test_gpu_cloud_bank.py::_bank_clouds (ordinary ones and the hard kinds); at n = 4096 eight of them,
    among them duplicated points, a partially zero-padded cloud and a hub."""
    if n == 4096:
        parts = [O.synthetic_clouds(2, n, 1, "uniform"), O.synthetic_clouds(2, n, 2, "lidar"), O.synthetic_clouds(1, n, 4, "dup"),
                 O.synthetic_clouds(1, n, 6, "zeropad25"), O.synthetic_clouds(1, n, 7, "repeat30"), _hub_cloud(n, 8)]
    else:
        parts = [O.synthetic_clouds(12, n, 1, "uniform"), O.synthetic_clouds(10, n, 2, "lidar"), O.synthetic_clouds(4, n, 3, "lattice"),
                 O.synthetic_clouds(5, n, 4, "dup"), O.synthetic_clouds(2, n, 5, "zeros"), O.synthetic_clouds(3, n, 6, "zeropad25"),
                 O.synthetic_clouds(2, n, 7, "repeat30"), _hub_cloud(n, 8), _hub_cloud(n, 9)]
    return np.concatenate(parts, 0)


_CACHE = {}


def _data_and_bank(n, dev):
    """The clouds (caller order, unsorted) and the bank holding them; built once per size and left unchanged."""
    if n not in _CACHE:
        ops = H.pkg("ops")
        data = torch.from_numpy(_bank_clouds(n)).to(dev)
        bank = ops.CloudBank(n, int(data.shape[0]) + 2, dev)
        bank.add(data)
        _CACHE[n] = (data, bank)
    return _CACHE[n]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("n", [256, 4096])
@pytest.mark.parametrize("prec", ["f32", "fast"])
@pytest.mark.parametrize("arch", ["epc-net", "epc-net-l"])
def test_forward_bank_equals_forward(dev, arch, prec, n):
    ops = H.pkg("ops")
    data, bank = _data_and_bank(n, dev)
    M = int(data.shape[0])
    # the set really holds rows that take the exact scan (more than `cap` entries at the threshold)
    assert int((ops.KnnGraph(ops.morton_sort(data)).cnt > CAP).sum()) > 0
    w = O.seeded_weights(arch, 2)
    eng, _ = H.make_engine(arch, w, dev, precision=prec, in_flight=1)
    ref, _ = H.make_engine(arch, w, dev, precision=prec, in_flight=1)
    rng = np.random.RandomState(3)
    lists = [list(range(M)), [M - 1, 0, M - 1, 5, 5, 5, 2] + rng.permutation(M)[:6].tolist(), [3]]
    for ids in lists:
        t = torch.tensor(ids, dtype=torch.int32, device=dev)
        want = ref.forward(data[t.long()]).clone()
        want_status = ref.last_status(len(ids))
        got = eng.forward_bank(bank, t)
        assert got.shape == (len(ids), 256) and _same(got, want), (arch, prec, n, ids)
        assert eng.last_status(len(ids)) == want_status
    # into a reused `out`, over another batch's stale contents in the workspace and in `out`
    out = torch.empty((M, 256), dtype=torch.float32, device=dev)
    a = torch.arange(M, dtype=torch.int32, device=dev)
    eng.forward_bank(bank, a.flip(0).contiguous(), out=out)
    assert eng.forward_bank(bank, a, out=out) is out
    assert _same(out, ref.forward(data))
    if n == 256:
        # 70 ids at micro_batch 64: two passes, the second partial; the status words are those of the last pass
        eng64, _ = H.make_engine(arch, w, dev, micro_batch=64, precision=prec, in_flight=1)
        ref64, _ = H.make_engine(arch, w, dev, micro_batch=64, precision=prec, in_flight=1)
        t = torch.tensor(rng.randint(0, M, 70).tolist(), dtype=torch.int32, device=dev)
        want = ref64.forward(data[t.long()]).clone()
        assert _same(eng64.forward_bank(bank, t), want)
        st = eng64.last_status(70)
        assert len(st) == 6 and st == ref64.last_status(70)


def test_gather_equals_the_pipeline_stages(dev):
    """epc_bank_gather_infer leaves what the ordinary pipeline's sort and kNN leave: sorted, kth (as bits), cnt and the live slots of
    the 2-byte lists; the status words say "finite"."""
    ops, L = H.pkg("ops"), H.pkg("lib")
    n = 256
    data, bank = _data_and_bank(n, dev)
    M = int(data.shape[0])
    eng, _ = H.make_engine("epc-net-l", O.seeded_weights("epc-net-l", 2), dev)
    ids = torch.tensor([M - 1, 0, 7] + list(range(M)), dtype=torch.int32, device=dev)
    T = int(ids.numel())
    srt = ops.morton_sort(data[ids.long()])
    want = H.run_stages(eng, srt)
    xyz = torch.full((T, n, 3), 7.0, dtype=torch.float32, device=dev)
    kth = torch.full((T, n), 7.0, dtype=torch.float32, device=dev)
    cnt = torch.full((T, n), 7, dtype=torch.int32, device=dev)
    idx = torch.full((T, n, CAP), 7, dtype=torch.int16, device=dev)
    status = torch.full((T,), 7, dtype=torch.int32, device=dev)
    L.check(L.lib().epc_bank_gather_infer(bank.records.data_ptr(), len(bank), ids.data_ptr(), T, n, CAP, xyz.data_ptr(), kth.data_ptr(),
                                          cnt.data_ptr(), idx.data_ptr(), status.data_ptr(), L.current_stream()))
    assert torch.equal(xyz, srt)
    assert torch.equal(kth.view(torch.int32), want["kth"].view(torch.int32))
    assert torch.equal(cnt, want["cnt"])
    live = torch.arange(CAP, device=dev)[None, None, :] < want["cnt"].clamp(max=CAP)[:, :, None]
    assert int((want["cnt"] > CAP).sum()) > 0
    assert torch.equal((idx.to(torch.int32) & 0xffff)[live], want["idx"][live])
    assert int(status.abs().max()) == 0


def test_bad_ids_and_refusals(dev):
    """An id outside the bank: a NaN descriptor with EPC_STATUS_NONFINITE_INPUT in its slot, the other slots untouched, a following call
    clean.  Host ids and int64 ids are refused; a cfg for another cloud size gets EPC_EINVAL and nothing runs."""
    L = H.pkg("lib")
    n = 256
    data, bank = _data_and_bank(n, dev)
    M = len(bank)
    w = O.seeded_weights("epc-net", 2)
    eng, _ = H.make_engine("epc-net", w, dev, in_flight=1)
    good = torch.tensor([0, 1, 2, 3], dtype=torch.int32, device=dev)
    want = eng.forward_bank(bank, good).clone()
    assert eng.last_status(4) == [0, 0, 0, 0] and bool(torch.isfinite(want).all())
    got = eng.forward_bank(bank, torch.tensor([0, M, -1, 3], dtype=torch.int32, device=dev)).clone()
    assert eng.last_status(4) == [0, L.EPC_STATUS_NONFINITE_INPUT, L.EPC_STATUS_NONFINITE_INPUT, 0]
    assert bool(torch.isnan(got[1:3]).all())
    assert _same(got[0], want[0]) and _same(got[3], want[3])
    assert _same(eng.forward_bank(bank, good), want) and eng.last_status(4) == [0, 0, 0, 0]
    with pytest.raises(L.EpcNetError):
        eng.forward_bank(bank, good.cpu())
    with pytest.raises(L.EpcNetError):
        eng.forward_bank(bank, good.long())
    # the C entry with a cfg whose num_points is not the records'
    cfg = eng.cfg_for(2 * n)
    packed = eng.packed(cfg)
    need = L.lib().epc_net_workspace_bytes(ctypes.byref(cfg), 4)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.full((4, 256), 5.0, dtype=torch.float32, device=dev)
    rc = L.lib().epc_net_forward_bank(ctypes.byref(cfg), packed.data_ptr(), bank.records.data_ptr(), M, bank.n, bank.cap,
                                      good.data_ptr(), 4, out.data_ptr(), ws.data_ptr(), need, L.current_stream())
    assert rc == L.EPC_EINVAL
    cfg = eng.cfg_for(n)
    rc = L.lib().epc_net_forward_bank(ctypes.byref(cfg), eng.packed(cfg).data_ptr(), bank.records.data_ptr(), M, bank.n, 40,
                                      good.data_ptr(), 4, out.data_ptr(), ws.data_ptr(), need, L.current_stream())
    assert rc == L.EPC_EINVAL
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())


def test_fp16_range_refusal_is_the_same(dev):
    """tests/test_gpu_epc_net_l_fast.py: coordinates scaled by 1e6 drive conv1 out of fp16.  The standalone conv1 launch behind the
    gather flags the cloud exactly as the fused kNN + conv1 launch does: the same status words, the same NaN descriptor."""
    ops, L = H.pkg("ops"), H.pkg("lib")
    w = O.seeded_weights("epc-net-l", 1)
    pc = O.synthetic_clouds(3, 512, 3)
    pc[1] *= 1e6
    x = torch.from_numpy(pc).to(dev)
    bank = ops.CloudBank(512, 3, dev)
    bank.add(x)
    fast, _ = H.make_engine("epc-net-l", w, dev, precision="fast", in_flight=1)
    want = fast.forward(x).clone()
    assert fast.last_status(3) == [0, L.EPC_STATUS_FP16_RANGE, 0]
    got = fast.forward_bank(bank, torch.arange(3, dtype=torch.int32, device=dev))
    assert fast.last_status(3) == [0, L.EPC_STATUS_FP16_RANGE, 0]
    assert bool(torch.isnan(got[1]).all()) and _same(got, want)


def test_forward_bank_in_a_captured_graph(dev):
    """Captured with a static id buffer, replayed twice with other ids: each replay equals the eager call on those ids."""
    n = 256
    data, bank = _data_and_bank(n, dev)
    M = len(bank)
    eng, _ = H.make_engine("epc-net", O.seeded_weights("epc-net", 2), dev, in_flight=1)
    id_sets = [[0, 1, 2, 3, 4, 5], [M - 1, 9, 9, 30, 2, 17], [5, 4, 3, 2, 1, 0]]
    static_ids = torch.tensor(id_sets[0], dtype=torch.int32, device=dev)
    eager = [eng.forward_bank(bank, torch.tensor(s, dtype=torch.int32, device=dev)).clone() for s in id_sets]
    out = torch.empty((6, 256), dtype=torch.float32, device=dev)
    eng.forward_bank(bank, static_ids, out=out)               # (warm-up: weights packed, workspace allocated before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        eng.forward_bank(bank, static_ids, out=out)
    for s, want in zip(id_sets[1:], eager[1:]):
        static_ids.copy_(torch.tensor(s, dtype=torch.int32, device=dev))
        g.replay()
        torch.cuda.synchronize()
        assert _same(out, want), s
