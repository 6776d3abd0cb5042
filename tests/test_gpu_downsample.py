"""epc_grid_downsample on the device against its numpy restatement (tests/downsample_ref.py): every comparison is on bit patterns, there is
no tolerance anywhere -- the operation is integer arithmetic behind the quantisation.  Ragged batches with odd offsets, every branch of
the definition, the engine's raw-scan entry, a captured graph replayed on another batch, the refusals."""
import functools

import numpy as np
import pytest
import torch

import downsample_ref as R
import helpers as H
from helpers import O

pytestmark = pytest.mark.gpu

# (N, sizes of the scenes of the batch): the restatement returns status 0 for every one (tests/test_downsample_cpu.py); a 5-point scan
# in front makes every cloud start at an odd row (12-byte rows: no 16-byte alignment), and is itself a failed cloud beside good ones
SCENES = {32: (40, 200), 256: (1000, 3000), 1024: (9000,), 4096: (20000, 70000)}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _scene_batch(N):
    return tuple([R.scene(5, 99)] + [R.scene(M, M) for M in SCENES[N]])


@functools.lru_cache(maxsize=None)
def _reference(name, N, normalize):
    scans = _scene_batch(N) if name == "scene" else _branch_batch()
    return R.reference_batch(scans, N, normalize)


@functools.lru_cache(maxsize=None)
def _branch_batch():
    rng = np.random.default_rng(7)
    uniform = rng.uniform(-1, 1, (5000, 3)).astype(np.float32)
    on_max = np.concatenate([rng.uniform(0, 1, (1500, 3)), np.eye(3), np.ones((1, 3)), [[1, 1, 0], [0, 1, 1], [1, 0, 1]]]).astype(np.float32)
    clean = R.scene(3000, 11)
    # 10 % rows with a NaN / +Inf / -Inf coordinate sprinkled in
    bad = np.repeat(clean[:300], 1, axis=0).copy()
    bad[np.arange(300), rng.integers(0, 3, 300)] = rng.choice([np.nan, np.inf, -np.inf], 300)
    where = np.sort(rng.integers(0, 3001, 300))
    dirty = np.insert(clean, where, bad, axis=0)
    hundred = rng.uniform(-1, 1, (100, 3)).astype(np.float32)
    return (uniform, R.lattice(8), on_max, dirty, clean,
            R.scene(100, 1),                                   # M < N
            np.zeros((0, 3), np.float32),                      # M = 0
            np.tile(np.float32([[3.5, -2.0, 0.25]]), (300, 1)),  # all points identical
            np.tile(hundred, (30, 1)),                         # 100 distinct points: D(1024) < N
            R.scene(1000, 5))                                  # a good neighbour behind the failures


def _run(scans, N, normalize=True):
    ops = H.pkg("ops")
    points, offsets = ops.pack_scans(list(scans))
    xyz, status, info = ops.grid_downsample(points, offsets, N, normalize=normalize)
    assert xyz.is_cuda and status.is_cuda and info.is_cuda and status.dtype == torch.int32 and info.dtype == torch.int32
    return xyz.cpu(), status.cpu(), info.cpu()


def _check(got, want, what):
    xyz, status, info = got
    rx, rs, ri = (torch.from_numpy(a) for a in want)
    assert torch.equal(status, rs), (what, status.tolist(), rs.tolist())
    assert torch.equal(info, ri), (what, info.tolist(), ri.tolist())     # where a mismatch began: finite points, R*, D, last count
    for c in range(xyz.shape[0]):
        assert _same(xyz[c], rx[c]), (what, "cloud %d" % c, info[c].tolist(),
                                      "first differing row %d" % int((_bits(xyz[c]) != _bits(rx[c])).any(1).nonzero()[0]))


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("N", sorted(SCENES))
def test_scenes_equal_the_restatement(N, normalize):
    want = _reference("scene", N, normalize)
    assert want[1].tolist() == [4] + [0] * len(SCENES[N])
    _check(_run(_scene_batch(N), N, normalize), want, "scenes N=%d normalize=%s" % (N, normalize))


@pytest.mark.parametrize("normalize", [True, False])
def test_branches_in_one_batch(normalize):
    want = _reference("branch", 256, normalize)
    assert want[1].tolist() == [0, 0, 0, 0, 0, 4, 4, 4, 4, 0]
    assert want[2][0].tolist()[:3] == [5000, 7, 343] and want[2][1].tolist()[:3] == [512, 7, 343]
    got = _run(_branch_batch(), 256, normalize)
    _check(got, want, "branches normalize=%s" % normalize)
    xyz = got[0]
    assert _same(xyz[3], xyz[4])                                   # non-finite rows removed = never there
    for c in (5, 6, 7, 8):                                         # all-NaN rows, neighbours untouched (checked above)
        assert bool(torch.isnan(xyz[c]).all())


def test_lattice_ties_by_key_alone_and_too_many_cells():
    scans = (R.lattice(8), R.scene(5, 99))
    _check(_run(scans, 512), R.reference_batch(scans, 512), "lattice N=512")
    # D(R*) > 2N: status and the first two words as the restatement's; the third word says 2N + 1 (where the pass stops counting)
    scans = (R.split_clusters(), R.lattice(4))
    rx, rs, ri = R.reference_batch(scans, 32)
    assert rs.tolist() == [4, 0] and ri[0][2] > 64 and ri[1].tolist()[:3] == [64, 4, 64]           # the lattice: D = 2N exactly, kept
    ri[0][2] = 65
    _check(_run(scans, 32), (rx, rs, ri), "split clusters N=32")


def test_bad_offsets_fail_the_cloud_on_the_device():
    ops = H.pkg("ops")
    dev = torch.device("cuda")
    a, b = R.scene(200, 1), R.scene(300, 2)
    points = torch.from_numpy(np.concatenate([a, b])).to(dev)
    offsets = torch.tensor([0, 200, 150, 500], dtype=torch.int32, device=dev)      # cloud 1 runs backwards
    xyz, status, info = ops.grid_downsample(points, offsets, 32)
    assert status.tolist() == [0, 4, 0] and bool(torch.isnan(xyz[1]).all()) and info[1].tolist() == [0, 0, 0, 0]
    assert _same(xyz[0].cpu(), torch.from_numpy(R.grid_downsample_ref(a, 32)[0]))
    assert _same(xyz[2].cpu(), torch.from_numpy(R.grid_downsample_ref(np.concatenate([a, b])[150:500], 32)[0]))


def test_same_bits_twice():
    a = _run(_scene_batch(4096), 4096)
    b = _run(_scene_batch(4096), 4096)
    assert all(_same(x, y) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def _engine_scans():
    return (R.scene(1000, 21), R.scene(60, 22), R.scene(3000, 23), R.scene(777, 24))       # the second one has fewer than 256 points


@pytest.mark.parametrize("arch", ["epc-net-l", "epc-net"])
def test_engine_forward_scans(arch):
    ops = H.pkg("ops")
    L = H.pkg("lib")
    dev = torch.device("cuda")
    eng, _ = H.make_engine(arch, O.seeded_weights(arch, 0), dev, in_flight=1)
    points, offsets = ops.pack_scans(list(_engine_scans()))
    xyz, st_ds, _ = ops.grid_downsample(points, offsets, 256)
    want = eng.forward(xyz).clone()
    desc, status = eng.forward_scans(points, offsets, num_points=256)
    assert _same(desc, want) and _same(status, st_ds)
    assert status.tolist() == [0, L.EPC_STATUS_NO_GRID, 0, 0]
    assert bool(torch.isnan(desc[1]).all()) and bool(torch.isfinite(desc[[0, 2, 3]]).all())
    words = eng.last_status(4)
    assert words[1] & L.EPC_STATUS_NONFINITE_INPUT and words[0] == words[2] == words[3] == 0

    # captured on one stream, replayed after the buffers were overwritten with another batch of the same total
    other = (R.scene(2000, 31), R.scene(837, 32), R.scene(2000, 33))
    assert sum(len(s) for s in other) == sum(len(s) for s in _engine_scans())
    p2, o2 = ops.pack_scans(list(other) + [np.zeros((0, 3), np.float32)])            # four clouds again: the last one empty
    eager, eager_status = eng.forward_scans(p2, o2, num_points=256)
    eager, eager_status = eager.clone(), eager_status.clone()
    out = torch.empty((4, 256), dtype=torch.float32, device=dev)
    eng.forward_scans(points, offsets, num_points=256, out=out)        # (warm-up: weights packed, workspace allocated before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _, st_graph = eng.forward_scans(points, offsets, num_points=256, out=out)
    points.copy_(p2)
    offsets.copy_(o2)
    g.replay()
    torch.cuda.synchronize()
    assert _same(out, eager) and _same(st_graph, eager_status)
    assert eager_status.tolist() == [0, 0, 0, L.EPC_STATUS_NO_GRID]


def test_refusals_write_nothing():
    ops = H.pkg("ops")
    L = H.pkg("lib")
    dev = torch.device("cuda")
    points, offsets = ops.pack_scans([R.scene(200, 1)])
    for n in (48, 8192):
        out = torch.full((1, n, 3), 7.0, dtype=torch.float32, device=dev)
        with pytest.raises(L.EpcNetError):
            ops.grid_downsample(points, offsets, n, out=out)
        status = torch.full((1,), -7, dtype=torch.int32, device=dev)
        ws = torch.zeros(1024, dtype=torch.uint8, device=dev)
        with pytest.raises(L.EpcNetError):
            L.check(L.lib().epc_grid_downsample(points.data_ptr(), offsets.data_ptr(), 1, n, 1, out.data_ptr(), status.data_ptr(), None,
                                                ws.data_ptr(), ws.numel(), L.current_stream()))
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()) and status.item() == -7
    need = L.lib().epc_grid_downsample_workspace_bytes(1, 32)
    out = torch.full((1, 32, 3), 7.0, dtype=torch.float32, device=dev)
    status = torch.full((1,), -7, dtype=torch.int32, device=dev)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    with pytest.raises(L.EpcNetError):
        L.check(L.lib().epc_grid_downsample(points.data_ptr(), offsets.data_ptr(), 1, 32, 1, out.data_ptr(), status.data_ptr(), None,
                                            ws.data_ptr(), need - 1, L.current_stream()))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and status.item() == -7
    L.check(L.lib().epc_grid_downsample(points.data_ptr(), offsets.data_ptr(), 1, 32, 1, out.data_ptr(), status.data_ptr(), None,
                                        ws.data_ptr(), need, L.current_stream()))       # info may be NULL; the exact size is enough
    torch.cuda.synchronize()
    assert status.item() == 0 and _same(out[0].cpu(), torch.from_numpy(R.grid_downsample_ref(R.scene(200, 1), 32)[0]))
