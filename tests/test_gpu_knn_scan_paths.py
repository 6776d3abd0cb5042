"""The scan paths of the four-lane kNN kernel (knn_topk_quad_kernel) at the smallest clouds where they differ: a wave's warm-up
(its lanes' first 20 candidates go into the lists without the insertion network when the wave's own super-tile has at least three
tiles, and through the network otherwise), the carried threshold, the votes' compare masks and the one-exchange emit of pass 2.

Every case runs 4-byte lists (epc_knn_topk_form) and 2-byte lists with conv1 fused (epc_knn_topk_conv1_form) and holds the four-lane
form to the one-lane form bit for bit -- kth, cnt, every list slot up to the capacity, the status words, the conv1 rows -- and, for
n <= 160, to the oracle's lists as well.

    n      what it exercises
    20     a lane sees five candidates and no list ever fills
    32     one tile, one super-tile
    76-84  either side of the point where a lane's 20th candidate arrives and warm-up ends
    100    ragged last tile
    160    a full and a partial super-tile (the partial one warms up through the network)
    1056   33 tiles: a one-tile super-tile at the end, more than one 16-query group per wave

A cloud with a NaN coordinate: what the rows of the OTHER points of that cloud hold depends on the order in which the NaN comparisons
fail (tests/test_gpu_knn_forms.py), so of the poisoned cloud the test holds the status word and the poisoned point's own row (no
candidate passes: cnt 0, twenty slots padded with its own index); the other two clouds of the case are held bit for bit like any
other."""
import ctypes

import numpy as np
import pytest
import torch

import helpers as H
from helpers import O

pytestmark = pytest.mark.gpu

CLOUDS = 3
CAP = 32
SIZES = [20, 32, 76, 80, 84, 100, 160, 1056]
KINDS = ["uniform_sorted", "uniform", "dup", "identical", "zeros", "nan"]
NAN_CLOUD, NAN_POINT = 1, 17


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def conv1_pack(dev):
    """(engine, device address of the packed conv1 section): 3 -> 64 weights, the same at every cloud size."""
    lib = H.pkg("lib").lib()
    eng, _ = H.make_engine("epc-net", O.seeded_weights("epc-net", 0), dev)
    cfg = eng.cfg_for(1024)
    return eng, eng.packed(cfg).data_ptr() + lib.epc_net_packed_offset(ctypes.byref(cfg), 0)


def _cloud(kind, n, dev):
    if kind == "identical":
        pc = np.tile(np.array([0.25, -0.5, 0.75]), (CLOUDS, n, 1))
    else:
        pc = O.synthetic_clouds(CLOUDS, n, 11, {"uniform_sorted": "uniform", "nan": "uniform"}.get(kind, kind))
    x = torch.from_numpy(np.ascontiguousarray(pc, dtype=np.float32)).to(dev)
    if kind in ("uniform_sorted", "nan"):
        x = H.pkg("ops").morton_sort(x)
    if kind == "nan":
        x[NAN_CLOUD, NAN_POINT, 1] = float("nan")
    return x.contiguous()


def _run(xyz, n, form, pack):
    """-> (idx4, cnt4, kth4), (idx2, cnt2, kth2, x32, x16, status) as numpy arrays"""
    L = H.pkg("lib")
    lib = L.lib()
    dev = xyz.device
    st = L.current_stream()
    idx = torch.full((CLOUDS, n, CAP), -1, dtype=torch.int32, device=dev)
    cnt = torch.full((CLOUDS, n), -1, dtype=torch.int32, device=dev)
    kth = torch.zeros((CLOUDS, n), device=dev)
    L.check(lib.epc_knn_topk_form(xyz.data_ptr(), CLOUDS, n, CAP, idx.data_ptr(), cnt.data_ptr(), kth.data_ptr(), form, st))
    idx2 = torch.full((CLOUDS, n, CAP), -1, dtype=torch.int16, device=dev)
    cnt2 = torch.full((CLOUDS, n), -1, dtype=torch.int32, device=dev)
    kth2 = torch.zeros((CLOUDS, n), device=dev)
    x32 = torch.zeros((CLOUDS * n, 64), device=dev)
    x16 = torch.zeros((CLOUDS * n, 64), dtype=torch.float16, device=dev)
    status = torch.zeros((CLOUDS,), dtype=torch.int32, device=dev)
    L.check(lib.epc_knn_topk_conv1_form(xyz.data_ptr(), CLOUDS, n, CAP, idx2.data_ptr(), 1, cnt2.data_ptr(), kth2.data_ptr(), pack,
                                        x32.data_ptr(), x16.data_ptr(), status.data_ptr(), form, st))
    torch.cuda.synchronize()
    wide = [t.cpu().numpy() for t in (idx, cnt, kth)]
    narrow = [t.cpu().numpy() for t in (idx2, cnt2, kth2, x32, x16, status)]
    narrow[0] = narrow[0].astype(np.int64) & 0xFFFF
    return wide, narrow


def _same_lists(a, b, clouds):
    """kth, cnt and every list slot up to the capacity (slots past a row's count are never written: both hold the fill)"""
    ia, ca, ka = a[:3]
    ib, cb, kb = b[:3]
    assert np.array_equal(ka[clouds].view(np.uint32), kb[clouds].view(np.uint32))
    assert np.array_equal(ca[clouds], cb[clouds])
    assert np.array_equal(ia[clouds], ib[clouds])


def _oracle(pc, out, clouds):
    idx, cnt, kth = out[:3]
    kth_ref, lists = O.knn_lists(pc)
    for b in clouds:
        assert np.array_equal(kth[b], kth_ref[b])
        for i in range(pc.shape[1]):
            ref = lists[b][i]
            assert cnt[b, i] == len(ref), (b, i)
            m = min(len(ref), CAP)
            assert np.array_equal(idx[b, i, :m], ref[:m]), (b, i)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_four_lanes_against_one_lane_and_oracle(dev, conv1_pack, kind, n):
    _, pack = conv1_pack
    xyz = _cloud(kind, n, dev)
    one = _run(xyz, n, 0, pack)
    four = _run(xyz, n, 1, pack)
    clean = [b for b in range(CLOUDS) if not (kind == "nan" and b == NAN_CLOUD)]
    for a, b in zip(one, four):
        _same_lists(a, b, clean)
    # status words and conv1 rows (2-byte lists, conv1 fused)
    assert np.array_equal(one[1][5], four[1][5])
    assert np.array_equal(one[1][3], four[1][3], equal_nan=True) and np.array_equal(one[1][4], four[1][4], equal_nan=True)
    if kind == "nan":
        assert four[1][5][NAN_CLOUD] != 0 and not four[1][5][clean].any()
        for out in one + four:
            idx, cnt = out[0], out[1]
            assert cnt[NAN_CLOUD, NAN_POINT] == 0                                     # a short row ...
            assert np.array_equal(idx[NAN_CLOUD, NAN_POINT, :20], np.full(20, NAN_POINT))   # ... padded with the point's own index
    else:
        assert not four[1][5].any()
    if kind in ("identical", "zeros"):
        assert (four[0][1] == n).all() and (four[1][1] == n).all()                  # every distance ties: cnt = n (> cap from n = 76 on)
    if n <= 160:
        pc = xyz.cpu().numpy()
        for out in four:
            _oracle(pc, out, clean)
